// Latent map (python -m dvae_amd.latent_map): an exact, matrix-free t-SNE of N points x [N, D] and the
// nearest-neighbour search behind its 1-NN speaker agreement.  Part of probe.hip's translation unit (included at its end,
// after latents.hip).  No N x N table exists anywhere: every pass recomputes the squared distances
//
//   d_ij = sum_d (x_id - x_jd)^2        dz = x_id - x_jd, acc = fma(dz, dz, acc), d ascending from +0
//
// in the difference form, so d_ij and d_ji are the same bits and d_ij >= d2min_i = min_{j != i} d_ij holds exactly.
//
// The shape is dvae_latent_lse's.  A wave owns 64 rows, one per lane: the row's x [DP] and its running sums stay in
// registers.  The four waves of a workgroup share the rows and take the four quarters [w q, (w + 1) q), q = ceil(N / 4),
// of the columns in ascending order, each staging tiles of its own columns in LDS and reading them as broadcasts; the
// quarters' partial results go through LDS and are combined in wave order, ((w0 + w1) + w2) + w3.  The partition and every
// order are functions of (N, D) alone and there are no atomics: a row's bits depend neither on the other rows of the
// launch nor on the launch, and two launches give the same bits.

namespace {

constexpr int TS_WG = 256;
constexpr int TS_TILE_FLOATS = 1024;       // per wave: TJ = 1024 / DP columns of DP dimensions
constexpr float TS_ENTROPY_TOL = 1e-5f;    // scikit-learn's _binary_search_perplexity stops there
constexpr float TS_BETA_MAX = 0x1p100f;    // a precision that doubles for ever stays finite
constexpr float TS_MIN_GAIN = 0.01f;

// DP: D rounded up to 4, 8, 16, 32 or 64.  The dimensions D .. DP - 1 of a group of four that holds a real one carry
// x = 0 on both sides (fma(0, 0, acc) = acc); whole groups behind D are skipped.
template <int DP>
__device__ __forceinline__ float ts_dist(const float (&xr)[DP], const float* col, int D) {
#pragma clang fp contract(off)
  const f32x4* pc = reinterpret_cast<const f32x4*>(col);
  float acc = 0.f;
#pragma unroll
  for (int g = 0; g < DP / 4; ++g) {
    if (4 * g < D) {      // uniform
      const f32x4 v = pc[g];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dz = xr[4 * g + i] - v[i];
        acc = __builtin_fmaf(dz, dz, acc);
      }
    }
  }
  return acc;
}

// the columns of one wave: its quarter, and the tiles every wave of the workgroup walks (the same count for the four)
struct TsCols {
  int64_t begin, mine, ntiles;
};

template <int DP>
__device__ __forceinline__ TsCols ts_cols(int64_t N, int w) {
  constexpr int TJ = TS_TILE_FLOATS / DP;
  const int64_t q = (N + 3) / 4;
  TsCols c;
  c.begin = w * q;
  c.mine = N - w * q < q ? (N - w * q > 0 ? N - w * q : 0) : q;
  c.ntiles = (q + TJ - 1) / TJ;
  return c;
}

template <int DP>
__device__ __forceinline__ void ts_stage_x(float* tx, const float* __restrict__ x, int64_t ld, int D, int64_t c0, int cnt,
                                           int lane) {
  constexpr int TJ = TS_TILE_FLOATS / DP;
  for (int e = lane; e < TJ * DP; e += 64) {
    const int j = e / DP, d = e - j * DP;
    tx[e] = (j < cnt && d < D) ? x[(c0 + j) * ld + d] : 0.f;
  }
}

template <int DP>
__device__ __forceinline__ void ts_load_row(float (&xr)[DP], const float* __restrict__ x, int64_t ld, int D, int64_t r) {
  const float* xrow = x + r * ld;
#pragma unroll
  for (int d = 0; d < DP; ++d) xr[d] = d < D ? xrow[d] : 0.f;
}

// ---------------------------------------------------------------------------------------------------- nearest neighbour
template <int DP>
__global__ __launch_bounds__(TS_WG) void tsne_nn_kernel(const float* __restrict__ x, int64_t ld, int64_t N, int D,
                                                        const int* __restrict__ group, int64_t row0, int64_t nrows,
                                                        float* __restrict__ d2min, int* __restrict__ arg) {
  constexpr int TJ = TS_TILE_FLOATS / DP;
  __shared__ __attribute__((aligned(16))) float lds[4 * TS_TILE_FLOATS];
  __shared__ int lgrp[4 * TJ];
  __shared__ float pbest[4 * 64];
  __shared__ int parg[4 * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t rl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = rl < nrows;
  const int64_t r = row0 + (live ? rl : 0);
  const TsCols c = ts_cols<DP>(N, w);
  float xr[DP];
  ts_load_row<DP>(xr, x, ld, D, r);
  const int gi = group ? group[r] : 0;
  float best = INFINITY;
  int at = -1;
  float* tx = lds + w * TS_TILE_FLOATS;
  int* tg = lgrp + w * TJ;
  for (int64_t ti = 0; ti < c.ntiles; ++ti) {
    const int64_t t0 = ti * TJ;
    const int cnt = (int)(c.mine - t0 < TJ ? (c.mine - t0 > 0 ? c.mine - t0 : 0) : TJ);
    ts_stage_x<DP>(tx, x, ld, D, c.begin + t0, cnt, lane);
    if (group)
      for (int j = lane; j < cnt; j += 64) tg[j] = group[c.begin + t0 + j];
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const int64_t cj = c.begin + t0 + j;
      const float d = ts_dist<DP>(xr, tx + j * DP, D);
      const bool admissible = group ? tg[j] != gi : cj != r;
      if (admissible && d < best) {      // columns ascend: `<` keeps the lowest index of a tie
        best = d;
        at = (int)cj;
      }
    }
    __syncthreads();
  }
  pbest[w * 64 + lane] = best;
  parg[w * 64 + lane] = at;
  __syncthreads();
  if (w != 0 || !live) return;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (pbest[k * 64 + lane] < best) {      // the quarters ascend too
      best = pbest[k * 64 + lane];
      at = parg[k * 64 + lane];
    }
  d2min[r] = best;
  arg[r] = at;
}

// ------------------------------------------------------------------------------------------------- perplexity search
// Per row the precision b at which p_j ~ exp(-b d'_j), d'_j = max(d_ij - d2min_i, 0), j != i, has entropy ln perplexity:
//   S0 = sum exp(-b d'), S1 = sum d' exp(-b d'), lnz = ln S0, H = lnz + b S1 / S0
// b from 1, doubled or halved until bracketed, then bisected (van der Maaten's search, scikit-learn's tolerance).  Every
// wave carries the state of all 64 rows and combines the four quarters itself, in wave order: the four copies are the
// same bits, so the workgroup leaves the loop together.
template <int DP>
__global__ __launch_bounds__(TS_WG) void tsne_affinities_kernel(const float* __restrict__ x, int64_t ld, int64_t N, int D,
                                                                const float* __restrict__ d2min, float ln_perp,
                                                                int max_steps, int64_t row0, int64_t nrows,
                                                                float* __restrict__ beta, float* __restrict__ lnz,
                                                                float* __restrict__ entropy, int* __restrict__ steps) {
#pragma clang fp contract(off)
  constexpr int TJ = TS_TILE_FLOATS / DP;
  __shared__ __attribute__((aligned(16))) float lds[4 * TS_TILE_FLOATS];
  __shared__ float part[4 * 2 * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t rl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = rl < nrows;
  const int64_t r = row0 + (live ? rl : 0);
  const TsCols c = ts_cols<DP>(N, w);
  float xr[DP];
  ts_load_row<DP>(xr, x, ld, D, r);
  const float dmin = d2min[r];
  float b = 1.f, lo = -INFINITY, hi = INFINITY, o_lnz = 0.f, o_h = 0.f;
  int used = -1;
  bool done = !live;
  float* tx = lds + w * TS_TILE_FLOATS;
  for (int pass = 0; pass < max_steps; ++pass) {
    float s0 = 0.f, s1 = 0.f;
    for (int64_t ti = 0; ti < c.ntiles; ++ti) {
      const int64_t t0 = ti * TJ;
      const int cnt = (int)(c.mine - t0 < TJ ? (c.mine - t0 > 0 ? c.mine - t0 : 0) : TJ);
      ts_stage_x<DP>(tx, x, ld, D, c.begin + t0, cnt, lane);
      __syncthreads();
      for (int j = 0; j < cnt; ++j) {
        const float dp = fmaxf(ts_dist<DP>(xr, tx + j * DP, D) - dmin, 0.f);
        const float e = c.begin + t0 + j != r ? __expf(-b * dp) : 0.f;
        s0 += e;
        s1 = __builtin_fmaf(dp, e, s1);
      }
      __syncthreads();
    }
    part[(w * 2 + 0) * 64 + lane] = s0;
    part[(w * 2 + 1) * 64 + lane] = s1;
    __syncthreads();
    s0 = ((part[0 * 64 + lane] + part[2 * 64 + lane]) + part[4 * 64 + lane]) + part[6 * 64 + lane];
    s1 = ((part[1 * 64 + lane] + part[3 * 64 + lane]) + part[5 * 64 + lane]) + part[7 * 64 + lane];
    __syncthreads();
    if (!done) {
      o_lnz = logf(s0);
      o_h = __builtin_fmaf(b, s1 / s0, o_lnz);
      const float diff = o_h - ln_perp;
      if (fabsf(diff) <= TS_ENTROPY_TOL) {
        done = true;
        used = pass + 1;
      } else if (pass + 1 < max_steps) {      // the last iterate stays beside its lnz and entropy
        if (diff > 0.f) {
          lo = b;
          b = hi == INFINITY ? fminf(b * 2.f, TS_BETA_MAX) : (b + hi) * 0.5f;
        } else {
          hi = b;
          b = lo == -INFINITY ? b * 0.5f : (b + lo) * 0.5f;
        }
      }
    }
    if (__all(done)) break;
  }
  if (w != 0 || !live) return;
  beta[r] = b;
  lnz[r] = o_lnz;
  entropy[r] = o_h;
  steps[r] = used;
}

// ------------------------------------------------------------------------------------------------------------ forces
// One gradient evaluation.  Per pair (i, j), j != i:
//   p = (exp(fma(-b_i, d'_i, -lnz_i)) + exp(fma(-b_j, d'_j, -lnz_j))) * (1 / 2N)      d'_k = max(d_ij - d2min_k, 0)
//   q = fma(dy1, dy1, dy0 dy0), den = 1 + q, w = rcp(den)
// and the eight sums of a row: A (p w dy, 2), R (w w dy, 2), Z (w), and with KL: p ln p over p > 0, p ln w = -p log1p(q), p.
template <int DP, bool KL>
__global__ __launch_bounds__(TS_WG) void tsne_forces_kernel(const float* __restrict__ x, int64_t ld, int64_t N, int D,
                                                            const float* __restrict__ beta,
                                                            const float* __restrict__ d2min,
                                                            const float* __restrict__ lnz, const float* __restrict__ y,
                                                            float inv2n, int64_t row0, int64_t nrows,
                                                            float* __restrict__ rows) {
#pragma clang fp contract(off)
  constexpr int TJ = TS_TILE_FLOATS / DP;
  __shared__ __attribute__((aligned(16))) float lds[4 * TS_TILE_FLOATS];
  __shared__ float lcol[4 * 5 * TJ];
  __shared__ float part[4 * 8 * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t rl = (int64_t)blockIdx.x * 64 + lane;
  const bool live = rl < nrows;
  const int64_t r = row0 + (live ? rl : 0);
  const TsCols c = ts_cols<DP>(N, w);
  float xr[DP];
  ts_load_row<DP>(xr, x, ld, D, r);
  const float bi = beta[r], di = d2min[r], nli = -lnz[r], y0 = y[2 * r], y1 = y[2 * r + 1];
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  float* tx = lds + w * TS_TILE_FLOATS;
  float* tc = lcol + w * 5 * TJ;
  for (int64_t ti = 0; ti < c.ntiles; ++ti) {
    const int64_t t0 = ti * TJ;
    const int cnt = (int)(c.mine - t0 < TJ ? (c.mine - t0 > 0 ? c.mine - t0 : 0) : TJ);
    ts_stage_x<DP>(tx, x, ld, D, c.begin + t0, cnt, lane);
    for (int j = lane; j < cnt; j += 64) {
      const int64_t g = c.begin + t0 + j;
      tc[5 * j + 0] = beta[g];
      tc[5 * j + 1] = d2min[g];
      tc[5 * j + 2] = -lnz[g];
      tc[5 * j + 3] = y[2 * g];
      tc[5 * j + 4] = y[2 * g + 1];
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float d = ts_dist<DP>(xr, tx + j * DP, D);
      const float* cj = tc + 5 * j;
      const float ei = __expf(__builtin_fmaf(-bi, fmaxf(d - di, 0.f), nli));
      const float ej = __expf(__builtin_fmaf(-cj[0], fmaxf(d - cj[1], 0.f), cj[2]));
      const float p = c.begin + t0 + j != r ? (ei + ej) * inv2n : 0.f;
      const float dy0 = y0 - cj[3], dy1 = y1 - cj[4];
      const float q = __builtin_fmaf(dy1, dy1, dy0 * dy0);
      const float wq = __builtin_amdgcn_rcpf(1.f + q);
      const float pw = p * wq, w2 = wq * wq;
      s[0] = __builtin_fmaf(pw, dy0, s[0]);
      s[1] = __builtin_fmaf(pw, dy1, s[1]);
      s[2] = __builtin_fmaf(w2, dy0, s[2]);      // dy = 0 on the diagonal
      s[3] = __builtin_fmaf(w2, dy1, s[3]);
      s[4] += c.begin + t0 + j != r ? wq : 0.f;
      if constexpr (KL) {
        if (p > 0.f) s[5] = __builtin_fmaf(p, logf(p), s[5]);
        s[6] = __builtin_fmaf(p, -log1pf(q), s[6]);
        s[7] += p;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) part[(w * 8 + k) * 64 + lane] = s[k];
  __syncthreads();
  if (w != 0 || !live) return;
  float* o = rows + r * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    o[k] = ((part[k * 64 + lane] + part[(8 + k) * 64 + lane]) + part[(16 + k) * 64 + lane]) + part[(24 + k) * 64 + lane];
}

// ------------------------------------------------------------------------------------------------------------ update
// Every workgroup adds Z (and workgroup 0 the three KL sums) over the N rows itself, in float64 and in one order: thread t
// takes the rows t, t + 256, ... ascending, then the 256 partial sums are added in thread order.  Then scikit-learn's
// _gradient_descent rule on the workgroup's 256 rows.
__global__ __launch_bounds__(256) void tsne_update_kernel(const float* __restrict__ rows, int64_t N, float* __restrict__ y,
                                                          float* __restrict__ upd, float* __restrict__ gains, float lr,
                                                          float momentum, float ex, double* __restrict__ kl) {
#pragma clang fp contract(off)
  __shared__ double red[4 * 256];
  __shared__ double tot[4];
  const int t = threadIdx.x;
  const bool want = kl != nullptr && blockIdx.x == 0;      // uniform
  double z = 0.0, a = 0.0, b = 0.0, c = 0.0;
  for (int64_t i = t; i < N; i += 256) {
    z += (double)rows[8 * i + 4];
    if (want) {
      a += (double)rows[8 * i + 5];
      b += (double)rows[8 * i + 6];
      c += (double)rows[8 * i + 7];
    }
  }
  red[t] = z;
  red[256 + t] = a;
  red[512 + t] = b;
  red[768 + t] = c;
  __syncthreads();
  if (t < 4 && (t == 0 || want)) {
    double v = 0.0;
    for (int k = 0; k < 256; ++k) v += red[t * 256 + k];
    tot[t] = v;
  }
  __syncthreads();
  const double Z = tot[0];
  if (want && t == 0) *kl = tot[1] - tot[2] + log(Z) * tot[3];
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  if (i >= N) return;
  const float inv_z = (float)(1.0 / Z);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float g = 4.f * __builtin_fmaf(ex, rows[8 * i + k], -(rows[8 * i + 2 + k] * inv_z));
    const float u = upd[2 * i + k];
    float gn = gains[2 * i + k];
    gn = u * g < 0.f ? gn + 0.2f : gn * 0.8f;
    gn = fmaxf(gn, TS_MIN_GAIN);
    const float un = __builtin_fmaf(momentum, u, -(lr * (gn * g)));
    gains[2 * i + k] = gn;
    upd[2 * i + k] = un;
    y[2 * i + k] += un;
  }
}

bool ts_rows_ok(int64_t N, int D, int64_t ld, int64_t row0, int64_t nrows) {
  return N >= 1 && N <= INT_MAX && D >= 1 && D <= DVAE_LATENT_MAX_D && ld >= D && row0 >= 0 && nrows >= 0 &&
         row0 + nrows <= N;
}

}  // namespace

#define DVAE_TS_DISPATCH(LAUNCH) \
  do {                           \
    if (D <= 4) LAUNCH(4);       \
    else if (D <= 8) LAUNCH(8);  \
    else if (D <= 16) LAUNCH(16); \
    else if (D <= 32) LAUNCH(32); \
    else LAUNCH(64);             \
  } while (0)

DVAE_API int dvae_tsne_nn(const float* x, int64_t ld, int64_t N, int D, const int* group, int64_t row0, int64_t nrows,
                          float* d2min, int* arg, void* stream) {
  if (!x || !d2min || !arg || !ts_rows_ok(N, D, ld, row0, nrows)) return DVAE_EINVAL;
  if (nrows == 0) return DVAE_OK;
  const dim3 grid((unsigned)((nrows + 63) / 64)), block(TS_WG);
  hipStream_t s = (hipStream_t)stream;
#define DVAE_TS_NN(DP) hipLaunchKernelGGL(tsne_nn_kernel<DP>, grid, block, 0, s, x, ld, N, D, group, row0, nrows, d2min, arg)
  DVAE_TS_DISPATCH(DVAE_TS_NN);
#undef DVAE_TS_NN
  return dvae_check_launch();
}

DVAE_API int dvae_tsne_affinities(const float* x, int64_t ld, int64_t N, int D, const float* d2min, float perplexity,
                                  int max_steps, int64_t row0, int64_t nrows, float* beta, float* lnz, float* entropy,
                                  int* steps, void* stream) {
  if (!x || !d2min || !beta || !lnz || !entropy || !steps || !ts_rows_ok(N, D, ld, row0, nrows)) return DVAE_EINVAL;
  if (N < 2 || !(perplexity >= 1.f) || !(perplexity <= (float)(N - 1)) || max_steps < 1) return DVAE_EINVAL;
  if (nrows == 0) return DVAE_OK;
  const dim3 grid((unsigned)((nrows + 63) / 64)), block(TS_WG);
  hipStream_t s = (hipStream_t)stream;
  const float ln_perp = (float)log((double)perplexity);
#define DVAE_TS_AFF(DP)                                                                                              \
  hipLaunchKernelGGL(tsne_affinities_kernel<DP>, grid, block, 0, s, x, ld, N, D, d2min, ln_perp, max_steps, row0, nrows, \
                     beta, lnz, entropy, steps)
  DVAE_TS_DISPATCH(DVAE_TS_AFF);
#undef DVAE_TS_AFF
  return dvae_check_launch();
}

DVAE_API int dvae_tsne_forces(const float* x, int64_t ld, int64_t N, int D, const float* beta, const float* d2min,
                              const float* lnz, const float* y, int want_kl, int64_t row0, int64_t nrows, float* rows,
                              void* stream) {
  if (!x || !beta || !d2min || !lnz || !y || !rows || !ts_rows_ok(N, D, ld, row0, nrows)) return DVAE_EINVAL;
  if (want_kl != 0 && want_kl != 1) return DVAE_EINVAL;
  if (nrows == 0) return DVAE_OK;
  const dim3 grid((unsigned)((nrows + 63) / 64)), block(TS_WG);
  hipStream_t s = (hipStream_t)stream;
  const float inv2n = (float)(0.5 / (double)N);
#define DVAE_TS_FORCES(DP)                                                                                              \
  do {                                                                                                                  \
    if (want_kl)                                                                                                        \
      hipLaunchKernelGGL((tsne_forces_kernel<DP, true>), grid, block, 0, s, x, ld, N, D, beta, d2min, lnz, y, inv2n, row0, \
                         nrows, rows);                                                                                  \
    else                                                                                                                \
      hipLaunchKernelGGL((tsne_forces_kernel<DP, false>), grid, block, 0, s, x, ld, N, D, beta, d2min, lnz, y, inv2n,    \
                         row0, nrows, rows);                                                                            \
  } while (0)
  DVAE_TS_DISPATCH(DVAE_TS_FORCES);
#undef DVAE_TS_FORCES
  return dvae_check_launch();
}

DVAE_API int dvae_tsne_update(const float* rows, int64_t N, float* y, float* upd, float* gains, float lr, float momentum,
                              float exaggeration, double* kl, void* stream) {
  if (!rows || !y || !upd || !gains || N < 1 || N > INT_MAX || (((uintptr_t)kl) & 7)) return DVAE_EINVAL;
  if (!(lr > 0.f) || !(momentum >= 0.f) || !(exaggeration > 0.f)) return DVAE_EINVAL;
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, N, y,
                     upd, gains, lr, momentum, exaggeration, kl);
  return dvae_check_launch();
}

#undef DVAE_TS_DISPATCH
