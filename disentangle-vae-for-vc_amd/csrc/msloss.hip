// Modulation-spectrum and global-variance loss of the train step (ops.SmoothingPenaltyFn): the squared distance
// between the log modulation spectra, and between the log global variances, of rec_hat and of the input it reconstructs, its
// statistics and its gradient.  Part of elem.hip's translation unit (included at its end, behind modspec.hip, whose MsTile and
// ms_stage it uses; msl_dft2 is ms_dft on two tiles at once).
//
//   d_t = y_t - mean_t(y) over a window's D frames, Y_k = sum_t d_t e^{-2 pi i k t / D} (k = 1 .. H = D/2, t in index order)
//   P_k = |Y_k|^2, s_k = ln(P_k + eps_ms), Delta_k = s_k - s^x_k             eps_ms = D floor^2
//   m = mean, v = population variance over a row's T frames, g = ln(v + eps_gv), dg = g - g^x        eps_gv = floor^2
//
// Everything is float64 from the fp32 inputs to the one rounding at a store.  A workgroup owns MS_BINS = 16 bins of ONE row n
// (grid: N x ceil(C / 16)) and walks the row's W = T / D disjoint windows in order; y and its target x (row n of x1, or row
// n - Bh of x2) are staged side by side as centred float64 frames: two MsTiles, 37 KB of LDS (39 KB with the forward pass's
// sums), four workgroups to a CU.
//
// Forward, launch 1: thread <-> (bin, k) takes both DFTs and adds Delta^2 to its own sum (windows in order, then its items in
// order); the 256 sums go through a fixed tree; the 16 lanes of a bin take m and v of the row's T frames (lane j the frames j,
// j + 16, ... in index order, then the xor tree 8 .. 1).  The workgroup writes three float64 partials (sum Delta^2, sum dg^2,
// sum dg, the bins in order) and per (row, bin) m and 2 dg / (v + eps_gv) for the backward pass.  Launch 2: one workgroup adds
// the partials (thread r the workgroups r, r + 256, ... in index order from +0, then a fixed tree) and writes the statistics.
//
// Backward, ONE launch of the same grid: per window both DFTs again, q_k = Delta_k / (P_k + eps_ms) times (Re Y_k, Im Y_k) into
// LDS, then thread <-> (bin, t) adds its H terms in index order, the bin's mean comes off, the global-variance term is added
// and the element is stored: one writer per element of dy, no atomics, every order a function of (C, T, D) alone.

namespace {

constexpr int MSL_MAX_C = 65535;                       // grid.y = ceil(C / 16)
constexpr int MSL_ITEMS = MS_BINS * (MS_DMAX / 2) / MS_THREADS;      // (bin, k) items of a window per thread, at the most
static_assert(sizeof(double[MS_BINS][MS_DMAX / 2][2]) <= sizeof(MsTile::d), "the scaled coefficients reuse a tile's frames");

// mean and population variance of the T frames at p: lane j of a bin's 16 adds frames j, j + 16, ... in index order, then the
// xor tree over the 16; the mean first, the centred squares second.  Every lane of the wave calls it (`on`: the bin exists).
__device__ __forceinline__ void msl_gv(const float* __restrict__ p, int T, bool on, double& m, double& v) {
  const int j = threadIdx.x % MS_SEG;
  double a = 0.0;
  if (on) {
#pragma unroll 4
    for (int t = j; t < T; t += MS_SEG) a += (double)p[t];
  }
#pragma unroll
  for (int o = MS_SEG / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  m = a / (double)T;
  double q = 0.0;
  if (on) {
#pragma unroll 4
    for (int t = j; t < T; t += MS_SEG) {
      const double e = (double)p[t] - m;
      q += e * e;
    }
  }
#pragma unroll
  for (int o = MS_SEG / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  v = q / (double)T;
}

// ms_dft of both tiles in one walk (the same terms in the same order): one twiddle read serves both trajectories
__device__ __forceinline__ void msl_dft2(const MsTile& sy, const MsTile& sx, int b, int k, int D, double& re, double& im,
                                         double& rx, double& ix) {
  re = im = rx = ix = 0.0;
  int idx = 0;                                         // k t mod D
#pragma unroll 4
  for (int t = 0; t < D; ++t) {
    const double c = sy.tw[idx][0], s = sy.tw[idx][1];
    const double v = sy.d[b][t], u = sx.d[b][t];
    re += v * c;
    im -= v * s;
    rx += u * c;
    ix -= u * s;
    idx += k;
    if (idx >= D) idx -= D;
  }
}

__device__ __forceinline__ const float* msl_target(const float* __restrict__ x1, const float* __restrict__ x2, int n, int Bh,
                                                   int C, int c0, int T) {
  return n < Bh ? x1 + ((int64_t)n * C + c0) * T : x2 + ((int64_t)(n - Bh) * C + c0) * T;
}

// part [3][N tiles]: sum Delta^2, sum dg^2, sum dg of workgroup n tiles + tile; gm, gc [N][C]: m and 2 dg / (v + eps_gv)
__global__ void __launch_bounds__(MS_THREADS) msloss_rows_kernel(const float* __restrict__ y, const float* __restrict__ x1,
                                                                 const float* __restrict__ x2, int Bh, int C, int T, int D,
                                                                 double eps_ms, double eps_gv,
                                                                 const double* __restrict__ twiddle,
                                                                 double* __restrict__ part, double* __restrict__ gm,
                                                                 double* __restrict__ gc) {
  __shared__ MsTile sy, sx;
  __shared__ double red[MS_THREADS];
  __shared__ double dg[MS_BINS];
  const int tid = threadIdx.x, n = blockIdx.x, c0 = blockIdx.y * MS_BINS, nb = min(MS_BINS, C - c0), H = D / 2;
  const float* yp = y + ((int64_t)n * C + c0) * T;
  const float* xp = msl_target(x1, x2, n, Bh, C, c0, T);
  {
    const int b = tid / MS_SEG;
    const bool on = b < nb;
    double m, v, mx, vx;
    msl_gv(yp + (int64_t)(on ? b : 0) * T, T, on, m, v);
    msl_gv(xp + (int64_t)(on ? b : 0) * T, T, on, mx, vx);
    if (on && tid % MS_SEG == 0) {
      const double d = log(v + eps_gv) - log(vx + eps_gv);
      dg[b] = d;
      gm[(int64_t)n * C + c0 + b] = m;
      gc[(int64_t)n * C + c0 + b] = 2.0 * d / (v + eps_gv);
    }
  }
  double acc = 0.0;
  for (int w = 0; w < T / D; ++w) {
    ms_stage(yp + (int64_t)w * D, T, nb, D, twiddle, sy);
    ms_stage(xp + (int64_t)w * D, T, nb, D, twiddle, sx);
    for (int i = tid; i < nb * H; i += MS_THREADS) {
      const int b = i / H, k = i % H + 1;
      double re, im, rx, ix;
      msl_dft2(sy, sx, b, k, D, re, im, rx, ix);
      const double del = log(re * re + im * im + eps_ms) - log(rx * rx + ix * ix + eps_ms);
      acc += del * del;
    }
    __syncthreads();                                   // the next window overwrites the tiles
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = MS_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t nwg = (int64_t)gridDim.x * gridDim.y, wg = (int64_t)n * gridDim.y + blockIdx.y;
    double s2 = 0.0, s1 = 0.0;
    for (int b = 0; b < nb; ++b) {
      s2 += dg[b] * dg[b];
      s1 += dg[b];
    }
    part[wg] = red[0];
    part[nwg + wg] = s2;
    part[2 * nwg + wg] = s1;
  }
}

// stats = {L_ms, L_gv, msd_db, gv_ratio_db, penalty}; count_ms = N W C H, count_gv = N C
__global__ void __launch_bounds__(MS_THREADS) msloss_stats_kernel(const double* __restrict__ part, int64_t nwg,
                                                                  double count_ms, double count_gv,
                                                                  const float* __restrict__ weights,
                                                                  float* __restrict__ stats, float* __restrict__ penalty) {
  __shared__ double acc[MS_THREADS][3];
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int64_t r = tid; r < nwg; r += MS_THREADS) {
    a0 += part[r];
    a1 += part[nwg + r];
    a2 += part[2 * nwg + r];
  }
  acc[tid][0] = a0;
  acc[tid][1] = a1;
  acc[tid][2] = a2;
  __syncthreads();
  for (int o = MS_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 3; ++k) acc[tid][k] += acc[tid + o][k];
    __syncthreads();
  }
  if (tid == 0) {
    const double db = 4.3429448190325182765;           // 10 / ln 10
    const double lms = acc[0][0] / count_ms, lgv = acc[0][1] / count_gv;
    stats[0] = (float)lms;
    stats[1] = (float)lgv;
    stats[2] = (float)(db * sqrt(lms));
    stats[3] = (float)(db * (acc[0][2] / count_gv));
    const float pen = (float)((double)weights[0] * lms + (double)weights[1] * lgv);
    stats[4] = pen;
    if (penalty) penalty[0] = pen;
  }
}

// c_ms = 4 / (N W C H), c_gv = 2 / (T N C)
__global__ void __launch_bounds__(MS_THREADS) msloss_bwd_kernel(const float* __restrict__ y, const float* __restrict__ x1,
                                                                const float* __restrict__ x2, int Bh, int C, int T, int D,
                                                                double eps_ms, double c_ms, double c_gv,
                                                                const double* __restrict__ twiddle,
                                                                const float* __restrict__ weights,
                                                                const float* __restrict__ gscale,
                                                                const double* __restrict__ gm, const double* __restrict__ gc,
                                                                float* __restrict__ dy) {
  __shared__ MsTile sy, sx;
  __shared__ double gmean[MS_BINS], rm[MS_BINS], rc[MS_BINS];
  // q_k (Re Y_k, Im Y_k) take the place of y's frames once every DFT of the window is done: 37 KB of LDS, four workgroups a CU
  double(*Yc)[MS_DMAX / 2][2] = reinterpret_cast<double(*)[MS_DMAX / 2][2]>(&sy.d[0][0]);
  const int tid = threadIdx.x, n = blockIdx.x, c0 = blockIdx.y * MS_BINS, nb = min(MS_BINS, C - c0), H = D / 2;
  float* dp = dy + ((int64_t)n * C + c0) * T;
  const float w_ms = weights[0], w_gv = weights[1];
  if (w_ms == 0.f && w_gv == 0.f) {      // uniform: the feature only monitors, nothing of the inputs reaches a gradient
    for (int64_t i = tid; i < (int64_t)nb * T; i += MS_THREADS) dp[i] = 0.f;
    return;
  }
  const float* yp = y + ((int64_t)n * C + c0) * T;
  const float* xp = msl_target(x1, x2, n, Bh, C, c0, T);
  const double gs = gscale ? (double)gscale[0] : 1.0;
  const double a_ms = (double)w_ms * c_ms, a_gv = (double)w_gv * c_gv;
  if (tid < nb) {
    rm[tid] = gm[(int64_t)n * C + c0 + tid];
    rc[tid] = gc[(int64_t)n * C + c0 + tid];
  }
  for (int w = 0; w < T / D; ++w) {
    ms_stage(yp + (int64_t)w * D, T, nb, D, twiddle, sy);
    ms_stage(xp + (int64_t)w * D, T, nb, D, twiddle, sx);
    double qr[MSL_ITEMS], qi[MSL_ITEMS];
#pragma unroll
    for (int j = 0; j < MSL_ITEMS; ++j) {
      const int i = tid + j * MS_THREADS;
      if (i < nb * H) {
        double re, im, rx, ix;
        msl_dft2(sy, sx, i / H, i % H + 1, D, re, im, rx, ix);
        const double p = re * re + im * im + eps_ms;
        const double q = (log(p) - log(rx * rx + ix * ix + eps_ms)) / p;
        qr[j] = q * re;
        qi[j] = q * im;
      }
    }
    __syncthreads();                                   // every DFT has read its frames
#pragma unroll
    for (int j = 0; j < MSL_ITEMS; ++j) {
      const int i = tid + j * MS_THREADS;
      if (i < nb * H) {
        Yc[i / H][i % H][0] = qr[j];
        Yc[i / H][i % H][1] = qi[j];
      }
    }
    __syncthreads();
    // sum_k q_k (Re Y_k cos - Im Y_k sin)(2 pi k t / D), k in index order, into the target's tile (its frames are spent)
    for (int i = tid; i < nb * D; i += MS_THREADS) {
      const int b = i / D, t = i % D;
      double a = 0.0;
      int idx = t;                                     // k t mod D
#pragma unroll 4
      for (int k = 1; k <= H; ++k) {
        a += Yc[b][k - 1][0] * sy.tw[idx][0] - Yc[b][k - 1][1] * sy.tw[idx][1];
        idx += t;
        if (idx >= D) idx -= D;
      }
      sx.d[b][t] = a;
    }
    __syncthreads();
    {
      const int b = tid / MS_SEG, j = tid % MS_SEG;
      double a = 0.0;
      if (b < nb)
        for (int t = j; t < D; t += MS_SEG) a += sx.d[b][t];
#pragma unroll
      for (int o = MS_SEG / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (b < nb && j == 0) gmean[b] = a / (double)D;
    }
    __syncthreads();
    for (int i = tid; i < nb * D; i += MS_THREADS) {
      const int b = i / D, t = i % D;
      const int64_t at = (int64_t)b * T + (int64_t)w * D + t;
      const double v = gs * (a_ms * (sx.d[b][t] - gmean[b]) + a_gv * (rc[b] * ((double)yp[at] - rm[b])));
      const float r = (float)v;
      dp[at] = r == 0.f ? 0.f : r;                     // a constant trajectory: +0.0, never -0.0
    }
    __syncthreads();                                   // the next window overwrites the tiles
  }
}

inline bool msl_bad(const float* y, const float* x1, const float* x2, int Bh, int C, int T, int D, double floor,
                    const double* twiddle, const float* weights, const void* ws) {
  return !y || !x1 || !x2 || !twiddle || !weights || !ws || Bh < 1 || Bh > (1 << 30) - 1 || C < 1 || C > MSL_MAX_C ||
         D < DVAE_MODSPEC_DMIN || D > DVAE_MODSPEC_DMAX || (D & 1) || T < D || T % D != 0 || !(floor > 0.0) ||
         !(floor * floor > 0.0) || ms_misaligned(twiddle, 8) || ms_misaligned(ws, 8);
}

}  // namespace

DVAE_API int64_t dvae_msloss_ws_bytes(int N, int C) {
  if (N < 1 || C < 1 || C > MSL_MAX_C) return -1;
  return 8 * (3 * (int64_t)N * ((C + MS_BINS - 1) / MS_BINS) + 2 * (int64_t)N * C);
}

DVAE_API int dvae_msloss_fwd(const float* y, const float* x1, const float* x2, int Bh, int C, int T, int D, double floor,
                             const double* twiddle, const float* weights, float* stats, float* penalty, void* ws,
                             void* stream) {
  if (msl_bad(y, x1, x2, Bh, C, T, D, floor, twiddle, weights, ws) || !stats) return DVAE_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const int N = 2 * Bh, tiles = (C + MS_BINS - 1) / MS_BINS;
  const int64_t nwg = (int64_t)N * tiles;
  double* part = (double*)ws;
  double* gm = part + 3 * nwg;
  double* gc = gm + (int64_t)N * C;
  hipLaunchKernelGGL(msloss_rows_kernel, dim3((unsigned)N, (unsigned)tiles), dim3(MS_THREADS), 0, s, y, x1, x2, Bh, C, T, D,
                     (double)D * floor * floor, floor * floor, twiddle, part, gm, gc);
  const double count_gv = (double)N * (double)C;
  hipLaunchKernelGGL(msloss_stats_kernel, dim3(1), dim3(MS_THREADS), 0, s, (const double*)part, nwg,
                     count_gv * (double)(T / D) * (double)(D / 2), count_gv, weights, stats, penalty);
  return dvae_check_launch();
}

DVAE_API int dvae_msloss_bwd(const float* y, const float* x1, const float* x2, int Bh, int C, int T, int D, double floor,
                             const double* twiddle, const float* weights, const float* gscale, const void* ws, float* dy,
                             void* stream) {
  if (msl_bad(y, x1, x2, Bh, C, T, D, floor, twiddle, weights, ws) || !dy) return DVAE_EINVAL;
  const int N = 2 * Bh, tiles = (C + MS_BINS - 1) / MS_BINS;
  const int64_t nwg = (int64_t)N * tiles;
  const double* gm = (const double*)ws + 3 * nwg;
  const double* gc = gm + (int64_t)N * C;
  const double count_gv = (double)N * (double)C;
  hipLaunchKernelGGL(msloss_bwd_kernel, dim3((unsigned)N, (unsigned)tiles), dim3(MS_THREADS), 0, (hipStream_t)stream, y, x1,
                     x2, Bh, C, T, D, (double)D * floor * floor, 4.0 / (count_gv * (double)(T / D) * (double)(D / 2)),
                     2.0 / ((double)T * count_gv), twiddle, weights, gscale, gm, gc, dy);
  return dvae_check_launch();
}
