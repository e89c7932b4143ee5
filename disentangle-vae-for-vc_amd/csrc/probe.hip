// Speaker-identity probe of the latents (python -m dvae_amd.probe): fused softmax cross-entropy.
// The classifier's two Linear layers are the project's contractions (ops.LinearFn); what was missing on the device is the
// loss on its logits: log-sum-exp, the gradient of the logits, the arg-max and the batch sums.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

// One wavefront per row, four rows per workgroup.  Lane l holds the 16-byte pieces l, l + 64, ... of its row in registers
// (NJ of them: classes <= 256 * NJ), so the row is read ONCE; maximum, arg-max, sum of exponentials and the label's logit
// are reduced across the lanes by shuffles (no LDS, no barrier).  Every row is computed by one wave alone, in an order
// that depends on nothing but `classes`: its outputs do not depend on what else is in the batch.
// logits and dlogits may be the same buffer: a wave has its whole row in registers before it stores any of it, and no
// other wave touches that row (no __restrict__ on the two).
template <int NJ>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* logits, const int* __restrict__ labels,
                                                         float* dlogits, float* __restrict__ row_loss,
                                                         int* __restrict__ row_pred, int rows, int classes, int64_t ld,
                                                         float grad_scale) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;      // wave-uniform
  const float* x = logits + r * ld;
  const int label = labels[r];
  const bool counted = label >= 0 && label < classes;
  const float ninf = -INFINITY;
  f32x4 v[NJ];
  float m = ninf;
  int am = INT_MAX;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 4 * (j * 64 + lane);
    if (col < classes) {      // ld % 4 == 0 and classes <= ld: the whole piece lies inside the row
      v[j] = *reinterpret_cast<const f32x4*>(x + col);
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (col + k >= classes) v[j][k] = ninf;      // padding columns are never looked at
    } else {
      v[j] = f32x4{ninf, ninf, ninf, ninf};
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)      // columns ascend with (j, k): `>` keeps the lowest index of a tie
      if (v[j][k] > m) {
        m = v[j][k];
        am = col + k;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(am, o, 64);
    if (om > m || (om == m && oa < am)) {
      m = om;
      am = oa;
    }
  }
  float s = 0.f, xl = 0.f;      // sum of exp(x - max); x[label] - max (one lane has it, the others add zeros)
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 4 * (j * 64 + lane);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = v[j][k] - m;
      xl += (col + k == label && counted) ? d : 0.f;
      v[j][k] = expf(d);      // exp(-inf) = 0 on the masked columns
      s += v[j][k];
    }
  }
  s = wave_sum(s);
  xl = wave_sum(xl);
  if (lane == 0) {
    row_loss[r] = counted ? logf(s) - xl : 0.f;
    row_pred[r] = am == INT_MAX ? 0 : am;
  }
  if (!dlogits) return;
  float* g = dlogits + r * ld;
  const float inv = 1.f / s;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 4 * (j * 64 + lane);
    if (col >= ld) continue;
    f32x4 o = zero;
    if (counted && col < classes) {
#pragma unroll
      for (int k = 0; k < 4; ++k)      // v is 0 on the columns >= classes: they are written as zeros
        o[k] = grad_scale * (v[j][k] * inv - (col + k == label ? 1.f : 0.f));
    }
    *reinterpret_cast<f32x4*>(g + col) = o;
  }
  // the rest of the padding: the contractions behind read whole ld-wide rows
  for (int64_t col = 4 * ((int64_t)NJ * 64 + lane); col < ld; col += 256) *reinterpret_cast<f32x4*>(g + col) = zero;
}

// out = {sum of row_loss, counted rows, counted rows with row_pred == label, mean loss} over the counted rows: ONE
// workgroup, thread t adds rows t, t + 1024, ... in that order (float64), then a fixed tree: no atomics, the same bits in
// every run.
__global__ __launch_bounds__(1024) void softmax_ce_reduce_kernel(const float* __restrict__ row_loss,
                                                                 const int* __restrict__ row_pred,
                                                                 const int* __restrict__ labels, float* __restrict__ out,
                                                                 int rows, int classes) {
  double s = 0.0;
  int n = 0, k = 0;
  for (int64_t r = threadIdx.x; r < rows; r += 1024) {
    const int lab = labels[r];
    if (lab >= 0 && lab < classes) {
      s += (double)row_loss[r];
      n += 1;
      k += row_pred[r] == lab ? 1 : 0;
    }
  }
  s = wave_sum_d(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    k += __shfl_xor(k, o, 64);
  }
  __shared__ double ss[16];
  __shared__ int sn[16], sk[16];
  if ((threadIdx.x & 63) == 0) {
    ss[threadIdx.x >> 6] = s;
    sn[threadIdx.x >> 6] = n;
    sk[threadIdx.x >> 6] = k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ts = 0.0;
    int tn = 0, tk = 0;
    for (int w = 0; w < 16; ++w) {
      ts += ss[w];
      tn += sn[w];
      tk += sk[w];
    }
    out[0] = (float)ts;
    out[1] = (float)tn;
    out[2] = (float)tk;
    out[3] = tn > 0 ? (float)(ts / tn) : 0.f;
  }
}

__global__ __launch_bounds__(256) void scale_by_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                                       float* __restrict__ y, int64_t n4) {
  const float a = s[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    reinterpret_cast<f32x4*>(y)[i] = reinterpret_cast<const f32x4*>(x)[i] * a;
}

}  // namespace

DVAE_API int dvae_softmax_ce(const float* logits, const int* labels, float* dlogits, float* row_loss, int* row_pred,
                             float* out, int rows, int classes, int64_t ld, float grad_scale, void* stream) {
  if (!logits || !labels || !row_loss || !row_pred) return DVAE_EINVAL;
  if (rows < 1 || classes < 1 || classes > DVAE_CE_MAX_CLASSES || ld < classes || (ld & 3)) return DVAE_EINVAL;
  if ((((uintptr_t)logits) | ((uintptr_t)dlogits)) & 15) return DVAE_EINVAL;
  const dim3 grid((unsigned)(((int64_t)rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
#define DVAE_CE_LAUNCH(NJ)                                                                                              \
  hipLaunchKernelGGL(softmax_ce_kernel<NJ>, grid, block, 0, s, logits, labels, dlogits, row_loss, row_pred, rows, classes, \
                     ld, grad_scale)
  switch ((classes + 255) / 256) {
    case 1: DVAE_CE_LAUNCH(1); break;
    case 2: DVAE_CE_LAUNCH(2); break;
    case 3: DVAE_CE_LAUNCH(3); break;
    default: DVAE_CE_LAUNCH(4); break;
  }
#undef DVAE_CE_LAUNCH
  if (out)
    hipLaunchKernelGGL(softmax_ce_reduce_kernel, dim3(1), dim3(1024), 0, s, (const float*)row_loss, (const int*)row_pred,
                       labels, out, rows, classes);
  return dvae_check_launch();
}

DVAE_API int dvae_scale_by(const float* x, const float* scale, float* y, int64_t n, void* stream) {
  if (!x || !scale || !y || n < 4 || (n & 3) || ((((uintptr_t)x) | ((uintptr_t)y)) & 15)) return DVAE_EINVAL;
  const int64_t n4 = n / 4;
  const int64_t blocks = (n4 + 255) / 256;
  hipLaunchKernelGGL(scale_by_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream,
                     x, scale, y, n4);
  return dvae_check_launch();
}

// ------------------------------------------------------------------------------------------------------------------------
// GMM-UBM speaker verification of conversions (python -m dvae_amd.verify): the E-step of a diagonal
// Gaussian mixture (log-densities, log-sum-exp, posteriors, sufficient statistics) and the per-utterance likelihood.
namespace {

constexpr int GMM_WG = 256;
constexpr int GMM_MAX_WGS = 512;        // workgroups of an E-step: its partition is a function of (N, K, D) alone
constexpr int GMM_RED_BYTES = GMM_WG * 8;

// A model staged in LDS: mu, prec [K][D4] f32x4 (D padded to 4 D4 with mu = 0 and prec = 0; a frame's registers hold 0
// there too, so a padding term is fma(0 * 0, 0, q) = q to the bit), a [K].  Reads are broadcasts: every lane of a wave is
// at the same component.
struct GmmLds {
  const f32x4* mu;
  const f32x4* prec;
  const float* a;
  int K, D4;
};

inline int gmm_model_floats(int K, int D) { return (K * (8 * ((D + 3) / 4) + 1) + 3) & ~3; }
inline int gmm_tile(int K) { return K <= 64 ? 256 : K <= 128 ? 128 : 64; }      // frames per tile: K (T + 1) floats <= 65 KB
__host__ __device__ inline int gmm_xs_stride(int D) { return (D + 1) | 1; }        // {1, x_0 .. x_{D-1}}, an odd stride
inline void gmm_plan(int64_t N, int K, int64_t* tiles_per_wg, int* wgs) {
  const int64_t T = gmm_tile(K), tiles = (N + T - 1) / T;
  *tiles_per_wg = (tiles + GMM_MAX_WGS - 1) / GMM_MAX_WGS;
  *wgs = (int)((tiles + *tiles_per_wg - 1) / *tiles_per_wg);
}

__device__ __forceinline__ GmmLds gmm_stage(float* lds, const float* __restrict__ a, const float* __restrict__ mu,
                                            const float* __restrict__ prec, int K, int D) {
  const int D4 = (D + 3) / 4, DP = 4 * D4;
  float* smu = lds;
  float* sprec = smu + K * DP;
  float* sa = sprec + K * DP;
  for (int i = threadIdx.x; i < K * DP; i += GMM_WG) {
    const int k = i / DP, d = i - k * DP;
    smu[i] = d < D ? mu[k * D + d] : 0.f;
    sprec[i] = d < D ? prec[k * D + d] : 0.f;
  }
  for (int k = threadIdx.x; k < K; k += GMM_WG) sa[k] = a[k];
  return GmmLds{reinterpret_cast<const f32x4*>(smu), reinterpret_cast<const f32x4*>(sprec), sa, K, D4};
}

__device__ __forceinline__ void gmm_load_row(const float* __restrict__ x, int D, float (&r)[DVAE_GMM_MAX_DIM]) {
#pragma unroll
  for (int d = 0; d < DVAE_GMM_MAX_DIM; ++d) r[d] = d < D ? x[d] : 0.f;
}

// l_k = a_k - q_k / 2, q_k = sum_d (x_d - mu_kd)^2 prec_kd: d ascending, one fma per term (the halving is exact)
__device__ __forceinline__ float gmm_l(const float (&x)[DVAE_GMM_MAX_DIM], const GmmLds& m, int k) {
  const f32x4* mu = m.mu + k * m.D4;
  const f32x4* prec = m.prec + k * m.D4;
  float q = 0.f;
#pragma unroll
  for (int g = 0; g < DVAE_GMM_MAX_DIM / 4; ++g) {
    if (g < m.D4) {      // wave-uniform
      const f32x4 u = mu[g], p = prec[g];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = x[4 * g + i] - u[i];
        q = __builtin_fmaf(d * d, p[i], q);
      }
    }
  }
  return __builtin_fmaf(-0.5f, q, m.a[k]);
}

// lse = max_k l_k + ln sum_k exp(l_k - max), k ascending: THE function of both kernels.  LDS_L: the E-step has l_k in its
// LDS column (lcol[k * ls], written by gmm_l: the value is the same either way) and gets back there e_k = exp(l_k - max),
// with their sum in `s`, for the posteriors.
template <bool LDS_L>
__device__ __forceinline__ float gmm_lse(const float (&x)[DVAE_GMM_MAX_DIM], const GmmLds& m, float* lcol, int ls, float& s) {
  float mx = -INFINITY;
  for (int k = 0; k < m.K; ++k) mx = fmaxf(mx, LDS_L ? lcol[k * ls] : gmm_l(x, m, k));
  s = 0.f;
  for (int k = 0; k < m.K; ++k) {
    const float l = LDS_L ? lcol[k * ls] : gmm_l(x, m, k);
    const float e = expf(l - mx);
    if (LDS_L) lcol[k * ls] = e;
    s += e;
  }
  return mx + logf(s);
}

// One workgroup owns `tiles_per_wg` consecutive tiles of T frames.  Per tile: the 256 / T threads of frame t share its
// components (each with the row in registers) and write l into column t of the LDS tile g [K][T + 1]; thread t < T then
// turns the column into gamma and puts the row into xs [T][1 + D] behind a leading 1; then the roles change: thread j owns
// the outputs (k, c) = divmod(j + 256 p, D + 1), p < NP (c = 0: n_k; c = 1 + d: f_kd and s_kd) and walks the tile's frames
// in order, adding gamma * x and gamma * x^2 (terms formed in float64) to float64 accumulators it keeps across the
// workgroup's tiles.  The workgroup's sums go to its slot of ws; gmm_fold_kernel adds the slots in index order.
template <int NP>
__global__ __launch_bounds__(GMM_WG) void gmm_estep_kernel(const float* __restrict__ x, int64_t ldx, int col0, int64_t N,
                                                           int D, const float* __restrict__ a,
                                                           const float* __restrict__ mu, const float* __restrict__ prec,
                                                           int K, int T, int64_t tiles_per_wg, float* __restrict__ lse_out,
                                                           float* __restrict__ gamma_out, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char gmm_lds[];
  const int tid = threadIdx.x;
  double* red = reinterpret_cast<double*>(gmm_lds);
  float* fl = reinterpret_cast<float*>(gmm_lds + GMM_RED_BYTES);
  const GmmLds m = gmm_stage(fl, a, mu, prec, K, D);
  const int GS = T + 1, XS = gmm_xs_stride(D), D1 = D + 1, PT = K * D1;
  float* g = fl + ((K * (8 * m.D4 + 1) + 3) & ~3);
  float* xs = g + K * GS;
  int gi[NP], xi[NP];
  double acc1[NP], acc2[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int o = tid + GMM_WG * p, k = o < PT ? o / D1 : 0;
    gi[p] = k * GS;
    xi[p] = o < PT ? o - k * D1 : 0;
    acc1[p] = 0.0;
    acc2[p] = 0.0;
  }
  double lsum = 0.0;
  __syncthreads();
  for (int64_t ti = 0; ti < tiles_per_wg; ++ti) {
    const int64_t t0 = ((int64_t)blockIdx.x * tiles_per_wg + ti) * T;
    if (t0 >= N) break;      // uniform
    const int cnt = (int)(N - t0 < T ? N - t0 : T);
    const int ft = tid & (T - 1), part = tid / T;      // T is 64, 128 or 256: a wave has one `part`
    float r[DVAE_GMM_MAX_DIM];
    if (ft < cnt) {
      gmm_load_row(x + (t0 + ft) * ldx + col0, D, r);
      for (int k = part; k < K; k += GMM_WG / T) g[k * GS + ft] = gmm_l(r, m, k);
    }
    __syncthreads();
    if (tid < cnt) {      // part 0: ft == tid
      xs[tid * XS] = 1.f;
#pragma unroll
      for (int d = 0; d < DVAE_GMM_MAX_DIM; ++d)
        if (d < D) xs[tid * XS + 1 + d] = r[d];
      float* lcol = g + tid;
      float esum;
      const float lse = gmm_lse<true>(r, m, lcol, GS, esum);
      // gamma = exp(l - lse) formed as exp(l - max) / sum: a row adds up to 1 within K 2^-23 even where |lse| is 1e6 and
      // one ulp of lse is 0.06
      for (int k = 0; k < K; ++k) lcol[k * GS] = lcol[k * GS] / esum;
      if (lse_out) lse_out[t0 + tid] = lse;
      lsum += (double)lse;
    }
    __syncthreads();
    if (gamma_out) {      // [cnt, K] row-major: consecutive lanes, consecutive k
      float* go = gamma_out + t0 * K;
      for (int i = tid; i < cnt * K; i += GMM_WG) {
        const int t = i / K;
        go[i] = g[(i - t * K) * GS + t];
      }
    }
    for (int t = 0; t < cnt; ++t) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        if (tid + GMM_WG * p < PT) {
#pragma clang fp contract(off)
          const double gd = (double)g[gi[p] + t], xd = (double)xs[t * XS + xi[p]];
          const double t1 = gd * xd, t2 = gd * (xd * xd);
          acc1[p] += t1;
          acc2[p] += t2;
        }
      }
    }
    __syncthreads();
  }
  const int R = 1 + 2 * D;
  double* slot = ws + (int64_t)blockIdx.x * ((int64_t)K * R + 1);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int o = tid + GMM_WG * p;
    if (o < PT) {
      const int k = o / D1, c = o - k * D1;
      slot[(int64_t)k * R + c] = acc1[p];                 // n_k at 0, f_kd at 1 + d
      if (c > 0) slot[(int64_t)k * R + D + c] = acc2[p];  // s_kd at 1 + D + d
    }
  }
  red[tid] = lsum;
  __syncthreads();
  if (tid == 0) {
    double s = red[0];
    for (int i = 1; i < GMM_WG; ++i) s += red[i];
    slot[(int64_t)K * R] = s;
  }
}

__global__ __launch_bounds__(256) void gmm_fold_kernel(const double* __restrict__ ws, int wgs, int S,
                                                       double* __restrict__ stats) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S) return;
  double s = ws[e];
  for (int w = 1; w < wgs; ++w) s += ws[(int64_t)w * S + e];
  stats[e] = s;
}

// One workgroup per (segment, model): thread t adds the lse of frames t, t + 256, ... in that order (float64), then the
// xor tree of wave_sum_d and the four waves in order.
__global__ __launch_bounds__(GMM_WG) void gmm_score_kernel(const float* __restrict__ x, int64_t ldx, int col0, int D,
                                                           const int64_t* __restrict__ segs, const float* __restrict__ a,
                                                           const float* __restrict__ mu, const float* __restrict__ prec,
                                                           int K, int M, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char gmm_lds[];
  __shared__ double part[GMM_WG / 64];
  const int tid = threadIdx.x, mi = blockIdx.y;
  const int64_t sg = blockIdx.x, row0 = segs[2 * sg], cnt = segs[2 * sg + 1];
  if (cnt <= 0) {      // uniform
    if (tid == 0) out[sg * M + mi] = 0.0;
    return;
  }
  const GmmLds m = gmm_stage(reinterpret_cast<float*>(gmm_lds), a + (int64_t)mi * K, mu + (int64_t)mi * K * D,
                             prec + (int64_t)mi * K * D, K, D);
  __syncthreads();
  double acc = 0.0;
  for (int64_t t = tid; t < cnt; t += GMM_WG) {
    float r[DVAE_GMM_MAX_DIM];
    gmm_load_row(x + (row0 + t) * ldx + col0, D, r);
    float esum;
    acc += (double)gmm_lse<false>(r, m, nullptr, 0, esum);
  }
  acc = wave_sum_d(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) out[sg * M + mi] = ((part[0] + part[1]) + part[2]) + part[3];
}

bool gmm_shape_ok(int K, int D, int col0, int64_t ldx) {
  return K >= 1 && K <= DVAE_GMM_MAX_K && D >= 1 && D <= DVAE_GMM_MAX_DIM && col0 >= 0 && ldx >= (int64_t)col0 + D;
}

}  // namespace

DVAE_API size_t dvae_gmm_ws_bytes(int64_t N, int K, int D) {
  if (N < 1 || K < 1 || K > DVAE_GMM_MAX_K || D < 1 || D > DVAE_GMM_MAX_DIM) return 0;
  int64_t per;
  int wgs;
  gmm_plan(N, K, &per, &wgs);
  return (size_t)wgs * ((size_t)K * (1 + 2 * D) + 1) * sizeof(double);
}

DVAE_API int dvae_gmm_estep(const float* x, int64_t ldx, int col0, int64_t N, int D, const float* a, const float* mu,
                            const float* prec, int K, float* lse, float* gamma, void* ws, double* stats, void* stream) {
  if (!x || !a || !mu || !prec || !ws || !stats || N < 1 || !gmm_shape_ok(K, D, col0, ldx)) return DVAE_EINVAL;
  if ((((uintptr_t)ws) | ((uintptr_t)stats)) & 7) return DVAE_EINVAL;
  int64_t per;
  int wgs;
  gmm_plan(N, K, &per, &wgs);
  const int T = gmm_tile(K), S = K * (1 + 2 * D) + 1, need = (K * (D + 1) + GMM_WG - 1) / GMM_WG;
  const int lds = GMM_RED_BYTES + 4 * (gmm_model_floats(K, D) + K * (T + 1) + T * gmm_xs_stride(D));
  hipStream_t s = (hipStream_t)stream;
#define DVAE_GMM_LAUNCH(NP)                                                                                             \
  do {                                                                                                                  \
    (void)hipFuncSetAttribute((const void*)gmm_estep_kernel<NP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);      \
    hipLaunchKernelGGL(gmm_estep_kernel<NP>, dim3((unsigned)wgs), dim3(GMM_WG), lds, s, x, ldx, col0, N, D, a, mu, prec, \
                       K, T, per, lse, gamma, (double*)ws);                                                             \
  } while (0)
  if (need <= 1) DVAE_GMM_LAUNCH(1);
  else if (need <= 2) DVAE_GMM_LAUNCH(2);
  else if (need <= 4) DVAE_GMM_LAUNCH(4);
  else if (need <= 8) DVAE_GMM_LAUNCH(8);
  else if (need <= 16) DVAE_GMM_LAUNCH(16);
  else DVAE_GMM_LAUNCH(33);      // K (D + 1) <= 256 * 33
#undef DVAE_GMM_LAUNCH
  hipLaunchKernelGGL(gmm_fold_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, (const double*)ws, wgs, S, stats);
  return dvae_check_launch();
}

DVAE_API int dvae_gmm_score(const float* x, int64_t ldx, int col0, int D, const int64_t* segs, int nseg, const float* a,
                            const float* mu, const float* prec, int K, int M, double* out, void* stream) {
  if (!x || !segs || !a || !mu || !prec || !out || nseg < 1 || M < 1 || M > 65535 || !gmm_shape_ok(K, D, col0, ldx))
    return DVAE_EINVAL;
  if ((((uintptr_t)segs) | ((uintptr_t)out)) & 7) return DVAE_EINVAL;
  const int lds = 4 * gmm_model_floats(K, D);
  (void)hipFuncSetAttribute((const void*)gmm_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(gmm_score_kernel, dim3((unsigned)nseg, (unsigned)M), dim3(GMM_WG), lds, (hipStream_t)stream, x, ldx,
                     col0, D, segs, a, mu, prec, K, M, out);
  return dvae_check_launch();
}

#include "latents.hip"      // the latent report: part of this translation unit
#include "tsne.hip"         // the latent map: the same
#include "adversary.hip"    // the speaker adversary: the same
#include "factor.hip"       // the total-correlation / shared-information penalty: the same
#include "ivector.hip"      // i-vector speaker embeddings: the same
