// i-vector speaker embeddings (python -m dvae_amd.ivector): per-utterance Baum-Welch statistics under the
// UBM of §4.13, the posterior of the total-variability factor (a batch of small symmetric positive-definite solves, one
// utterance per workgroup, all on chip in float64) and the accumulators of the EM M-step.  Part of probe.hip's translation
// unit (included at its end): the posteriors come from gmm_stage / gmm_l / gmm_lse, THE functions of the E-step.
// No atomics anywhere; every sum has a fixed order.
namespace {

constexpr int IVEC_WG = 256;
constexpr int IVEC_KC = 16;             // components per thread of the A accumulator: S_u is read once per 16 of them
constexpr int IVEC_MIN_PER = 64;        // utterances of one accumulation group, at least
constexpr int IVEC_MAX_GROUPS = 8;      // ... and groups at most: the partition is a function of U alone

// One workgroup per segment; the E-step's tile loop over the segment's frames alone.  Thread j owns the outputs
// (k, c) = divmod(j + 256 p, D + 1), p < NP (c = 0: n_k; c = 1 + d: g_kd) and walks the frames in order, t ascending, terms
// formed in float64 from the fp32 gamma and x.  Then f_kd = (g_kd - n_k mu_kd) sqrt(prec_kd), three roundings.
template <int NP>
__global__ __launch_bounds__(GMM_WG) void gmm_utt_stats_kernel(const float* __restrict__ x, int64_t ldx, int col0, int D,
                                                               const int64_t* __restrict__ segs,
                                                               const float* __restrict__ a, const float* __restrict__ mu,
                                                               const float* __restrict__ prec, int K, int T,
                                                               double* __restrict__ n_out, double* __restrict__ f_out) {
  extern __shared__ __attribute__((aligned(16))) char gmm_lds[];
  const int tid = threadIdx.x;
  const int64_t sg = blockIdx.x, row0 = segs[2 * sg], N = segs[2 * sg + 1];
  const int D1 = D + 1, PT = K * D1;
  double* no = n_out + sg * K;
  double* fo = f_out + sg * (int64_t)K * D;
  if (N <= 0) {      // uniform
    for (int o = tid; o < PT; o += GMM_WG) {
      const int k = o / D1, c = o - k * D1;
      if (c == 0) no[k] = 0.0;
      else fo[k * D + c - 1] = 0.0;
    }
    return;
  }
  double* red = reinterpret_cast<double*>(gmm_lds);      // n_k, K <= 256 doubles
  float* fl = reinterpret_cast<float*>(gmm_lds + GMM_RED_BYTES);
  const GmmLds m = gmm_stage(fl, a, mu, prec, K, D);
  const int GS = T + 1, XS = gmm_xs_stride(D);
  float* g = fl + ((K * (8 * m.D4 + 1) + 3) & ~3);
  float* xs = g + K * GS;
  int gi[NP], xi[NP];
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int o = tid + GMM_WG * p, k = o < PT ? o / D1 : 0;
    gi[p] = k * GS;
    xi[p] = o < PT ? o - k * D1 : 0;
    acc[p] = 0.0;
  }
  __syncthreads();
  const float* xb = x + row0 * ldx + col0;
  for (int64_t t0 = 0; t0 < N; t0 += T) {
    const int cnt = (int)(N - t0 < T ? N - t0 : T);
    const int ft = tid & (T - 1), part = tid / T;
    float r[DVAE_GMM_MAX_DIM];
    if (ft < cnt) {
      gmm_load_row(xb + (t0 + ft) * ldx, D, r);
      for (int k = part; k < K; k += GMM_WG / T) g[k * GS + ft] = gmm_l(r, m, k);
    }
    __syncthreads();
    if (tid < cnt) {
      xs[tid * XS] = 1.f;
#pragma unroll
      for (int d = 0; d < DVAE_GMM_MAX_DIM; ++d)
        if (d < D) xs[tid * XS + 1 + d] = r[d];
      float* lcol = g + tid;
      float esum;
      (void)gmm_lse<true>(r, m, lcol, GS, esum);
      for (int k = 0; k < K; ++k) lcol[k * GS] = lcol[k * GS] / esum;
    }
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (tid + GMM_WG * p < PT) {
#pragma clang fp contract(off)
          const double term = (double)g[gi[p] + t] * (double)xs[t * XS + xi[p]];
          acc[p] += term;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int o = tid + GMM_WG * p;
    if (o < PT && xi[p] == 0) {
      red[o / D1] = acc[p];
      no[o / D1] = acc[p];
    }
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int o = tid + GMM_WG * p;
    if (o < PT && xi[p] > 0) {
#pragma clang fp contract(off)
      const int k = o / D1, d = xi[p] - 1;
      const double nm = red[k] * (double)mu[k * D + d];
      const double ctr = acc[p] - nm;
      fo[k * D + d] = ctr * sqrt((double)prec[k * D + d]);
    }
  }
}

// One workgroup per utterance.  LDS, float64: G [R][R + 1] (L's lower triangle, then its Cholesky factor), X [R][R + 1]
// (columns 0 .. R - 1 start as the identity and end as L^-1; column R starts as b and ends as w), n [K], the four partial
// sums of b and b itself.
//   L_ij (j <= i) = delta_ij + sum_c n_c P_c[i][j], c ascending, one fma per term from +0 (P's lower triangle is read)
//   b_r = ((p_0 + p_1) + p_2) + p_3, p_q = sum over rows q, q + 4, ... of T[row][r] f[row], one fma per term from +0
//   Cholesky by columns: thread i has s_i = L_ij - sum_{k<j} G_ik G_jk (k ascending, fma); G_jj = sqrt(s_j), G_ij = s_i / G_jj
//   thread c solves G y = X[:, c] (rows ascending, k ascending) and G^T x = y (rows descending, k ascending from i + 1):
//   every column is solved by one thread alone in the same order, so w does not depend on whether S is asked for
//   S_ij = X_ij + w_i w_j (not mirrored: symmetric within the inverse's bound, not bit for bit)
//   ll = 1/2 sum_i b_i w_i - sum_i ln G_ii, both i ascending from +0, by thread 0
__global__ __launch_bounds__(IVEC_WG) void ivec_posterior_kernel(const double* __restrict__ n, const double* __restrict__ f,
                                                                 const double* __restrict__ Tm,
                                                                 const double* __restrict__ P, int K, int D, int R,
                                                                 double* __restrict__ w, double* __restrict__ S,
                                                                 double* __restrict__ ll) {
  extern __shared__ __attribute__((aligned(16))) double ivec_lds[];
  const int tid = threadIdx.x, LD = R + 1, KD = K * D, RR = R * R;
  const int64_t u = blockIdx.x;
  double* G = ivec_lds;
  double* X = G + R * LD;
  double* sn = X + R * LD;
  double* bp = sn + K;        // [4][64]
  double* sb = bp + 256;      // [64]
  for (int k = tid; k < K; k += IVEC_WG) sn[k] = n[u * K + k];
  __syncthreads();
  for (int e = tid; e < RR; e += IVEC_WG) {
    const int i = e / R, j = e - i * R;
    if (j <= i) {
      const double* p = P + e;
      double acc = 0.0;
      for (int c = 0; c < K; ++c) acc = fma(sn[c], p[(int64_t)c * RR], acc);
      G[i * LD + j] = (i == j ? 1.0 : 0.0) + acc;
    }
    if (S) X[i * LD + j] = i == j ? 1.0 : 0.0;
  }
  {
    const int q = tid >> 6, r = tid & 63;
    if (r < R) {
      const double* fu = f + u * KD;
      double acc = 0.0;
      for (int row = q; row < KD; row += 4) acc = fma(Tm[(int64_t)row * R + r], fu[row], acc);
      bp[q * 64 + r] = acc;
    }
  }
  __syncthreads();
  if (tid < R) {
    const double b = ((bp[tid] + bp[64 + tid]) + bp[128 + tid]) + bp[192 + tid];
    sb[tid] = b;
    X[tid * LD + R] = b;
  }
  for (int j = 0; j < R; ++j) {
    double s = 0.0;
    if (tid >= j && tid < R) {
      s = G[tid * LD + j];
      for (int k = 0; k < j; ++k) s = fma(-G[tid * LD + k], G[j * LD + k], s);
      if (tid == j) G[j * LD + j] = sqrt(s);
    }
    __syncthreads();
    if (tid > j && tid < R) G[tid * LD + j] = s / G[j * LD + j];
    __syncthreads();
  }
  if (tid <= R && (S || tid == R)) {
    const int c = tid, i0 = c < R ? c : 0;      // an identity column is zero above its 1: y_i = 0 exactly for i < c
    for (int i = i0; i < R; ++i) {
      double s = X[i * LD + c];
      for (int k = i0; k < i; ++k) s = fma(-G[i * LD + k], X[k * LD + c], s);
      X[i * LD + c] = s / G[i * LD + i];
    }
    for (int i = R - 1; i >= 0; --i) {
      double s = X[i * LD + c];
      for (int k = i + 1; k < R; ++k) s = fma(-G[k * LD + i], X[k * LD + c], s);
      X[i * LD + c] = s / G[i * LD + i];
    }
  }
  __syncthreads();
  if (tid < R) w[u * R + tid] = X[tid * LD + R];
  if (S) {
    double* So = S + u * RR;
    for (int e = tid; e < RR; e += IVEC_WG) {
      const int i = e / R, j = e - i * R;
      So[e] = fma(X[i * LD + R], X[j * LD + R], X[i * LD + j]);
    }
  }
  if (ll && tid == 0) {
    double q = 0.0, lg = 0.0;
    for (int i = 0; i < R; ++i) q = fma(sb[i], X[i * LD + R], q);
    for (int i = 0; i < R; ++i) lg += log(G[i * LD + i]);
    ll[u] = 0.5 * q - lg;
  }
}

struct IvecPlan {
  int per, groups, a_ij, a_cb, a_items, c_items, s_items;
  int64_t E;
};

inline IvecPlan ivec_plan(int U, int K, int D, int R) {
  IvecPlan p;
  p.per = (U + IVEC_MAX_GROUPS - 1) / IVEC_MAX_GROUPS;
  if (p.per < IVEC_MIN_PER) p.per = IVEC_MIN_PER;
  p.groups = (U + p.per - 1) / p.per;
  p.a_ij = (R * R + IVEC_WG - 1) / IVEC_WG;
  p.a_cb = (K + IVEC_KC - 1) / IVEC_KC;
  p.a_items = p.a_ij * p.a_cb;
  p.c_items = (K * D * R + IVEC_WG - 1) / IVEC_WG;
  p.s_items = p.a_ij;
  p.E = (int64_t)K * R * R + (int64_t)K * D * R + (int64_t)R * R;
  return p;
}

// blockIdx.y is a group of `per` consecutive utterances, blockIdx.x an item: the first a_items own 256 elements (i, j) of
// 16 consecutive components of A, the next c_items 256 elements of C, the last s_items 256 of Ssum.  One thread per output
// element walks the group's utterances in order (terms formed in float64, one product and one addition each) and writes
// its sum to the group's slot of ws [groups][A | C | Ssum].
__global__ __launch_bounds__(IVEC_WG) void ivec_accumulate_kernel(const double* __restrict__ n, const double* __restrict__ f,
                                                                  const double* __restrict__ w,
                                                                  const double* __restrict__ S, int U, int K, int D, int R,
                                                                  int per, int a_ij, int a_items, int c_items,
                                                                  double* __restrict__ ws) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, item = blockIdx.x, RR = R * R, KD = K * D;
  const int u0 = blockIdx.y * per, u1 = u0 + per < U ? u0 + per : U;
  const int64_t E = (int64_t)K * RR + (int64_t)KD * R + RR;
  double* slot = ws + (int64_t)blockIdx.y * E;
  if (item < a_items) {
    const int cb = item / a_ij, e = (item - cb * a_ij) * IVEC_WG + tid, c0 = cb * IVEC_KC;
    if (e >= RR) return;
    double acc[IVEC_KC];
#pragma unroll
    for (int q = 0; q < IVEC_KC; ++q) acc[q] = 0.0;
    for (int u = u0; u < u1; ++u) {
      const double s = S[(int64_t)u * RR + e];
      const double* nu = n + (int64_t)u * K + c0;
#pragma unroll
      for (int q = 0; q < IVEC_KC; ++q)
        if (c0 + q < K) {      // uniform
          const double t = nu[q] * s;
          acc[q] += t;
        }
    }
#pragma unroll
    for (int q = 0; q < IVEC_KC; ++q)
      if (c0 + q < K) slot[(int64_t)(c0 + q) * RR + e] = acc[q];
  } else if (item < a_items + c_items) {
    const int64_t e = (int64_t)(item - a_items) * IVEC_WG + tid;
    if (e >= (int64_t)KD * R) return;
    const int row = (int)(e / R), r = (int)(e - (int64_t)row * R);
    double acc = 0.0;
    for (int u = u0; u < u1; ++u) {
      const double t = f[(int64_t)u * KD + row] * w[(int64_t)u * R + r];
      acc += t;
    }
    slot[(int64_t)K * RR + e] = acc;
  } else {
    const int e = (item - a_items - c_items) * IVEC_WG + tid;
    if (e >= RR) return;
    double acc = 0.0;
    for (int u = u0; u < u1; ++u) acc += S[(int64_t)u * RR + e];
    slot[(int64_t)K * RR + (int64_t)KD * R + e] = acc;
  }
}

__global__ __launch_bounds__(256) void ivec_fold_kernel(const double* __restrict__ ws, int groups, int64_t E, int64_t nA,
                                                        int64_t nC, double* __restrict__ A, double* __restrict__ C,
                                                        double* __restrict__ Ssum) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double s = ws[e];
  for (int g = 1; g < groups; ++g) s += ws[(int64_t)g * E + e];
  if (e < nA) A[e] = s;
  else if (e < nA + nC) C[e - nA] = s;
  else Ssum[e - nA - nC] = s;
}

bool ivec_shape_ok(int U, int K, int D, int R) {
  return U >= 1 && K >= 1 && K <= DVAE_GMM_MAX_K && D >= 1 && D <= DVAE_GMM_MAX_DIM && R >= 1 && R <= DVAE_IVEC_MAX_R;
}

}  // namespace

DVAE_API int dvae_gmm_utt_stats(const float* x, int64_t ldx, int col0, int D, const int64_t* segs, int nseg, const float* a,
                                const float* mu, const float* prec, int K, double* n, double* f, void* stream) {
  if (!x || !segs || !a || !mu || !prec || !n || !f || nseg < 1 || !gmm_shape_ok(K, D, col0, ldx)) return DVAE_EINVAL;
  if ((((uintptr_t)segs) | ((uintptr_t)n) | ((uintptr_t)f)) & 7) return DVAE_EINVAL;
  const int T = gmm_tile(K), need = (K * (D + 1) + GMM_WG - 1) / GMM_WG;
  const int lds = GMM_RED_BYTES + 4 * (gmm_model_floats(K, D) + K * (T + 1) + T * gmm_xs_stride(D));
  hipStream_t s = (hipStream_t)stream;
#define DVAE_UTT_LAUNCH(NP)                                                                                              \
  do {                                                                                                                   \
    (void)hipFuncSetAttribute((const void*)gmm_utt_stats_kernel<NP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);   \
    hipLaunchKernelGGL(gmm_utt_stats_kernel<NP>, dim3((unsigned)nseg), dim3(GMM_WG), lds, s, x, ldx, col0, D, segs, a,   \
                       mu, prec, K, T, n, f);                                                                            \
  } while (0)
  if (need <= 1) DVAE_UTT_LAUNCH(1);
  else if (need <= 2) DVAE_UTT_LAUNCH(2);
  else if (need <= 4) DVAE_UTT_LAUNCH(4);
  else if (need <= 8) DVAE_UTT_LAUNCH(8);
  else if (need <= 16) DVAE_UTT_LAUNCH(16);
  else DVAE_UTT_LAUNCH(33);      // K (D + 1) <= 256 * 33
#undef DVAE_UTT_LAUNCH
  return dvae_check_launch();
}

DVAE_API int dvae_ivec_posterior(const double* n, const double* f, const double* T, const double* P, int U, int K, int D,
                                 int R, double* w, double* S, double* ll, void* stream) {
  if (!n || !f || !T || !P || !w || !ivec_shape_ok(U, K, D, R)) return DVAE_EINVAL;
  if ((((uintptr_t)n) | ((uintptr_t)f) | ((uintptr_t)T) | ((uintptr_t)P) | ((uintptr_t)w) | ((uintptr_t)S) |
       ((uintptr_t)ll)) & 7)
    return DVAE_EINVAL;
  const int lds = 8 * (2 * R * (R + 1) + K + 256 + 64);
  (void)hipFuncSetAttribute((const void*)ivec_posterior_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(ivec_posterior_kernel, dim3((unsigned)U), dim3(IVEC_WG), lds, (hipStream_t)stream, n, f, T, P, K, D, R,
                     w, S, ll);
  return dvae_check_launch();
}

DVAE_API size_t dvae_ivec_ws_bytes(int U, int K, int D, int R) {
  if (!ivec_shape_ok(U, K, D, R)) return 0;
  const IvecPlan p = ivec_plan(U, K, D, R);
  return (size_t)p.groups * (size_t)p.E * sizeof(double);
}

DVAE_API int dvae_ivec_accumulate(const double* n, const double* f, const double* w, const double* S, int U, int K, int D,
                                  int R, void* ws, double* A, double* C, double* Ssum, void* stream) {
  if (!n || !f || !w || !S || !ws || !A || !C || !Ssum || !ivec_shape_ok(U, K, D, R)) return DVAE_EINVAL;
  if ((((uintptr_t)n) | ((uintptr_t)f) | ((uintptr_t)w) | ((uintptr_t)S) | ((uintptr_t)ws) | ((uintptr_t)A) |
       ((uintptr_t)C) | ((uintptr_t)Ssum)) & 7)
    return DVAE_EINVAL;
  const IvecPlan p = ivec_plan(U, K, D, R);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ivec_accumulate_kernel, dim3((unsigned)(p.a_items + p.c_items + p.s_items), (unsigned)p.groups),
                     dim3(IVEC_WG), 0, s, n, f, w, S, U, K, D, R, p.per, p.a_ij, p.a_items, p.c_items, (double*)ws);
  hipLaunchKernelGGL(ivec_fold_kernel, dim3((unsigned)((p.E + 255) / 256)), dim3(256), 0, s, (const double*)ws, p.groups,
                     p.E, (int64_t)K * R * R, (int64_t)K * D * R, A, C, Ssum);
  return dvae_check_launch();
}
