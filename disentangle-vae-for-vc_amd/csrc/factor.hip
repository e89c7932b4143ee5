// Total-correlation and shared-information penalty of the train step (ops.FactorPenaltyFn): the
// minibatch estimator of latents.hip on the N = 2 Bh rows of a step, its statistics and its gradient.  Part of probe.hip's
// translation unit (included at its end).
//
//   a_jd = -(ln(2 pi) / 2 + lv_jd / 2), h_jd = expf(-lv_jd) / 2            (the halvings are exact)
//   t_ijd = a_jd - h_jd (z_id - mu_jd)^2        dz = z - mu, q = dz * dz, t = fma(-h, q, a)
//   style_ij = sum_{d < S} t_ijd, content_ij = sum_{S <= d < D} t_ijd       lane d holds t_ijd, the 64 lanes by the xor tree
//                                                                           32 .. 1 (the other block's lanes and d >= D add +0)
//   joint_ij = style_ij + content_ij
//   L = M + logf(sum_j expf(x_j - M)), M the maximum of the x_j: the maximum comes off before every exponential, so a row
//   far from every column has M finite and 1 <= sum <= N.
//
// Forward, launch 1: one workgroup of four waves per row i.  Wave w takes the columns j = w, w + 4, ...: pass 1 finds the
// maximum of every t_i.d over its columns and leaves style_ij and content_ij in LDS, the four maxima are merged, pass 2
// recomputes t and adds expf(t - M_d) in column order; the four sums are added in wave order.  Then wave 0, 1, 2 take the
// style, content and joint LSE over the LDS rows: lane l the columns l, l + 64, ... in order, the lanes by the xor tree.
// Launch 2: one workgroup turns L [N, D + 3] and own_i = joint_ii into the five statistics in float64: thread r the rows
// r, r + 256, ... in order, then a fixed tree over the 256 threads.
//
// Backward, ONE launch of 2 N workgroups: workgroups 0 .. N - 1 own a row i and write dz[i, :], workgroups N .. 2 N - 1 own a
// column j and write dq_mu[j, :], dq_lv[j, :].  Each recomputes its N block sums into LDS as the forward pass did (the same
// code, the same bits) and then wave 0, lane d, adds its N terms in index order (one fma per term).  No N x N x D table is
// stored, there are no atomics, and every order is a function of (N, D, S) alone: two launches give the same bits.

namespace {

constexpr int FAC_WG = 256;
constexpr float FAC_HALF_LN_2PI = 0.91893853320467274178f;

__device__ __forceinline__ float fac_t(float z, float mu, float a, float h) {
  const float dz = z - mu;
  const float q = dz * dz;
  return __builtin_fmaf(-h, q, a);
}

__device__ __forceinline__ float fac_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float fac_wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// style / content sums of the pairs (fixed row, columns k = w, w + 4, ...) or (rows k, fixed column) into LDS.  `row_fixed`:
// zf is the row's z[d] and (mu, lv) are read per k; otherwise (muf, af, hf) are the column's and z is read per k.
__device__ __forceinline__ void fac_block_sums(const float* __restrict__ z, const float* __restrict__ mu,
                                               const float* __restrict__ lv, int N, int D, int S, bool row_fixed, int fixed,
                                               float* __restrict__ st, float* __restrict__ ct) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool in = lane < D;
  float zf = 0.f, muf = 0.f, af = 0.f, hf = 0.f;
  if (in) {
    if (row_fixed) {
      zf = z[(int64_t)fixed * D + lane];
    } else {
      muf = mu[(int64_t)fixed * D + lane];
      const float l = lv[(int64_t)fixed * D + lane];
      af = -(FAC_HALF_LN_2PI + 0.5f * l);
      hf = 0.5f * expf(-l);
    }
  }
  for (int k = w; k < N; k += 4) {
    float t = 0.f;
    if (in) {
      if (row_fixed) {
        const float l = lv[(int64_t)k * D + lane];
        t = fac_t(zf, mu[(int64_t)k * D + lane], -(FAC_HALF_LN_2PI + 0.5f * l), 0.5f * expf(-l));
      } else {
        t = fac_t(z[(int64_t)k * D + lane], muf, af, hf);
      }
    }
    const float s = fac_wave_sum(lane < S ? t : 0.f);
    const float c = fac_wave_sum(lane >= S ? t : 0.f);      // t = 0 at lane >= D
    if (lane == 0) {
      st[k] = s;
      ct[k] = c;
    }
  }
}

__global__ __launch_bounds__(FAC_WG) void factor_rows_kernel(const float* __restrict__ z, const float* __restrict__ mu,
                                                             const float* __restrict__ lv, int N, int D, int S,
                                                             float* __restrict__ L, float* __restrict__ own) {
#pragma clang fp contract(off)
  __shared__ float st[DVAE_FACTOR_MAX_N], ct[DVAE_FACTOR_MAX_N];
  __shared__ float xm[4][64], xs[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x;
  const bool in = lane < D;
  const float zi = in ? z[(int64_t)i * D + lane] : 0.f;
  // pass 1: the maximum of t_i.d over this wave's columns, and the block sums
  float m = -INFINITY;
  for (int j = w; j < N; j += 4) {
    float t = 0.f;
    if (in) {
      const float l = lv[(int64_t)j * D + lane];
      t = fac_t(zi, mu[(int64_t)j * D + lane], -(FAC_HALF_LN_2PI + 0.5f * l), 0.5f * expf(-l));
      m = fmaxf(m, t);
    }
    const float s = fac_wave_sum(lane < S ? t : 0.f);
    const float c = fac_wave_sum(lane >= S ? t : 0.f);
    if (lane == 0) {
      st[j] = s;
      ct[j] = c;
    }
  }
  xm[w][lane] = m;
  __syncthreads();
  m = fmaxf(fmaxf(xm[0][lane], xm[1][lane]), fmaxf(xm[2][lane], xm[3][lane]));      // -inf from a wave without columns
  // pass 2: sum_j expf(t - M) over this wave's columns in order
  float s = 0.f;
  if (in) {
    for (int j = w; j < N; j += 4) {
      const float l = lv[(int64_t)j * D + lane];
      const float t = fac_t(zi, mu[(int64_t)j * D + lane], -(FAC_HALF_LN_2PI + 0.5f * l), 0.5f * expf(-l));
      s = s + expf(t - m);
    }
  }
  xs[w][lane] = s;
  __syncthreads();
  float* Li = L + (int64_t)i * (D + 3);
  if (w == 3) {
    if (in) Li[lane] = m + logf(((xs[0][lane] + xs[1][lane]) + xs[2][lane]) + xs[3][lane]);
    if (lane == 0) own[i] = st[i] + ct[i];
  } else {
    // wave 0: style, 1: content, 2: joint
    float bm = -INFINITY;
    for (int j = lane; j < N; j += 64) {
      const float x = w == 0 ? st[j] : w == 1 ? ct[j] : st[j] + ct[j];
      bm = fmaxf(bm, x);
    }
    bm = fac_wave_max(bm);
    float bs = 0.f;
    for (int j = lane; j < N; j += 64) {
      const float x = w == 0 ? st[j] : w == 1 ? ct[j] : st[j] + ct[j];
      bs = bs + expf(x - bm);
    }
    bs = fac_wave_sum(bs);
    if (lane == 0) Li[D + w] = bm + logf(bs);
  }
}

__global__ __launch_bounds__(FAC_WG) void factor_stats_kernel(const float* __restrict__ L, const float* __restrict__ own,
                                                              const float* __restrict__ weights, int N, int D, int S,
                                                              double ln_n, float* __restrict__ stats,
                                                              float* __restrict__ penalty) {
  __shared__ double acc[FAC_WG][4];
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int r = tid; r < N; r += FAC_WG) {
    const float* Lr = L + (int64_t)r * (D + 3);
    double ms = 0.0, mc = 0.0;
    for (int d = 0; d < S; ++d) ms += (double)Lr[d] - ln_n;
    for (int d = S; d < D; ++d) mc += (double)Lr[d] - ln_n;
    const double ls = Lr[D], lc = Lr[D + 1], lj = Lr[D + 2];
    a0 += (ls - ln_n) - ms;
    a1 += (lc - ln_n) - mc;
    a2 += lj - ls - lc + ln_n;
    a3 += (double)own[r] - (lj - ln_n);
  }
  acc[tid][0] = a0;
  acc[tid][1] = a1;
  acc[tid][2] = a2;
  acc[tid][3] = a3;
  __syncthreads();
  for (int o = FAC_WG / 2; o >= 1; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 4; ++k) acc[tid][k] += acc[tid + o][k];
    __syncthreads();
  }
  if (tid == 0) {
    const double tcs = acc[0][0] / N, tcc = acc[0][1] / N, sh = acc[0][2] / N, mi = acc[0][3] / N;
    stats[0] = (float)tcs;
    stats[1] = (float)tcc;
    stats[2] = (float)sh;
    stats[3] = (float)mi;
    const float pen = (float)((double)weights[0] * (tcs + tcc) + (double)weights[1] * sh);
    stats[4] = pen;
    if (penalty) penalty[0] = pen;
  }
}

__global__ __launch_bounds__(FAC_WG) void factor_bwd_kernel(const float* __restrict__ z, const float* __restrict__ mu,
                                                            const float* __restrict__ lv, const float* __restrict__ L,
                                                            const float* __restrict__ weights,
                                                            const float* __restrict__ gscale, int N, int D, int S,
                                                            float inv_n, float* __restrict__ dz, float* __restrict__ dmu,
                                                            float* __restrict__ dlv) {
#pragma clang fp contract(off)
  __shared__ float st[DVAE_FACTOR_MAX_N], ct[DVAE_FACTOR_MAX_N];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool rows = (int)blockIdx.x < N;
  const int own = rows ? blockIdx.x : blockIdx.x - N;
  const bool in = lane < D;
  const float w_tc = weights[0], w_sh = weights[1];
  if (w_tc == 0.f && w_sh == 0.f) {      // uniform: the feature only monitors, nothing of the inputs reaches a gradient
    if (w == 0 && in) {
      if (rows) {
        dz[(int64_t)own * D + lane] = 0.f;
      } else {
        dmu[(int64_t)own * D + lane] = 0.f;
        dlv[(int64_t)own * D + lane] = 0.f;
      }
    }
    return;
  }
  fac_block_sums(z, mu, lv, N, D, S, rows, own, st, ct);
  __syncthreads();
  if (w != 0 || !in) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const float c_joint = w_sh * gs, c_block = (w_tc - w_sh) * gs, c_dim = -(w_tc * gs);
  const bool style = lane < S;
  const int64_t ldl = D + 3;
  if (rows) {
    const float zi = z[(int64_t)own * D + lane];
    const float* Li = L + own * ldl;
    const float Ld = Li[lane], Lb = Li[style ? D : D + 1], Lj = Li[D + 2];
    float acc = 0.f;
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
      const float m = mu[(int64_t)j * D + lane], l = lv[(int64_t)j * D + lane];
      const float h = 0.5f * expf(-l);
      const float t = fac_t(zi, m, -(FAC_HALF_LN_2PI + 0.5f * l), h);
      const float pj = expf((st[j] + ct[j]) - Lj), pb = expf((style ? st[j] : ct[j]) - Lb), pd = expf(t - Ld);
      const float g = ((c_joint * pj + c_block * pb) + c_dim * pd) * inv_n;
      const float r = (2.f * h) * (zi - m);
      acc = __builtin_fmaf(g, -r, acc);
    }
    dz[(int64_t)own * D + lane] = acc;
  } else {
    const float m = mu[(int64_t)own * D + lane], l = lv[(int64_t)own * D + lane];
    const float h = 0.5f * expf(-l), a = -(FAC_HALF_LN_2PI + 0.5f * l);
    float am = 0.f, al = 0.f;
#pragma unroll 4
    for (int i = 0; i < N; ++i) {
      const float zi = z[(int64_t)i * D + lane];
      const float* Li = L + i * ldl;
      const float Ld = Li[lane], Lb = Li[style ? D : D + 1], Lj = Li[D + 2];
      const float t = fac_t(zi, m, a, h);
      const float pj = expf((st[i] + ct[i]) - Lj), pb = expf((style ? st[i] : ct[i]) - Lb), pd = expf(t - Ld);
      const float g = ((c_joint * pj + c_block * pb) + c_dim * pd) * inv_n;
      const float df = zi - m;
      const float r = (2.f * h) * df;
      am = __builtin_fmaf(g, r, am);
      al = __builtin_fmaf(g, __builtin_fmaf(0.5f * r, df, -0.5f), al);
    }
    dmu[(int64_t)own * D + lane] = am;
    dlv[(int64_t)own * D + lane] = al;
  }
}

bool fac_shape_ok(int N, int D, int S) {
  return N >= 1 && N <= DVAE_FACTOR_MAX_N && S >= 1 && D - S >= 1 && D <= DVAE_LATENT_MAX_D;
}

}  // namespace

DVAE_API int64_t dvae_factor_ws_bytes(int N) { return N < 1 || N > DVAE_FACTOR_MAX_N ? -1 : (int64_t)N * 4; }

DVAE_API int dvae_factor_fwd(const float* z, const float* mu, const float* lv, int N, int D, int S, const float* weights,
                             float* L, float* stats, float* penalty, void* ws, void* stream) {
  if (!z || !mu || !lv || !weights || !L || !stats || !ws || !fac_shape_ok(N, D, S)) return DVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* own = (float*)ws;
  hipLaunchKernelGGL(factor_rows_kernel, dim3(N), dim3(FAC_WG), 0, s, z, mu, lv, N, D, S, L, own);
  hipLaunchKernelGGL(factor_stats_kernel, dim3(1), dim3(FAC_WG), 0, s, (const float*)L, (const float*)own, weights, N, D, S,
                     log((double)N), stats, penalty);
  return dvae_check_launch();
}

DVAE_API int dvae_factor_bwd(const float* z, const float* mu, const float* lv, const float* L, int N, int D, int S,
                             const float* weights, const float* gscale, float* dz, float* dmu, float* dlv, void* stream) {
  if (!z || !mu || !lv || !L || !weights || !dz || !dmu || !dlv || !fac_shape_ok(N, D, S)) return DVAE_EINVAL;
  hipLaunchKernelGGL(factor_bwd_kernel, dim3(2 * N), dim3(FAC_WG), 0, (hipStream_t)stream, z, mu, lv, L, weights, gscale, N, D,
                     S, 1.0f / (float)N, dz, dmu, dlv);
  return dvae_check_launch();
}
