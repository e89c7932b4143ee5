// Held-out validation (model/variational_base_vae.py: validate): the eight loss terms of loss_functionGVAE2
// (disentangled_vae.py:310-327) PER PAIR — the reference's test() (variational_base_vae.py:105-123) with its batch_size set
// to 1 — and their float64 sums per speaker over all batches of a pass.  Plain C++: no atomics, no inline assembly, every
// wait a __syncthreads; both launches give the same bits run after run.
#include "common.h"

namespace {

constexpr int VAL_WG = 256;

// x - r rounds once in fp32 (as loss_partial_kernel), |.| is exact, the sum is float64 from the first addition on
__device__ __forceinline__ double absdiff(float x, float r) { return (double)fabsf(x - r); }
// the KL term as kl_fwd_kernel / loss_final_kernel state it, fp32, widened before it is added
__device__ __forceinline__ double kl_term(float m, float l) { return (double)(1.f + l - m * m - expf(l)); }

// One workgroup per pair b.  v[0..3]: L1 of (x1, rec[b]), (x2, rec[Bh + b]), (x1, rec_hat[b]), (x2, rec_hat[Bh + b]);
// v[4..5]: sum of the KL terms of rows b and Bh + b of q_*; v[6]: of row b of s_*.  Per thread in index order, then the
// butterfly over the 64 lanes, then the four waves in order: a fixed tree.
template <bool VEC>
__global__ __launch_bounds__(VAL_WG) void pair_metrics_kernel(
    const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ rec,
    const float* __restrict__ rec_hat, const float* __restrict__ q_mu, const float* __restrict__ q_lv,
    const float* __restrict__ s_mu, const float* __restrict__ s_lv, float* __restrict__ out, int Bh, int64_t n_per, int D,
    int S, float mse_cof, float kl_cof) {
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* xa = x1 + (int64_t)b * n_per;
  const float* xb = x2 + (int64_t)b * n_per;
  const float* r[4] = {rec + (int64_t)b * n_per, rec + ((int64_t)Bh + b) * n_per, rec_hat + (int64_t)b * n_per,
                       rec_hat + ((int64_t)Bh + b) * n_per};
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if constexpr (VEC) {
    const int64_t n4 = n_per >> 2;
    for (int64_t i = tid; i < n4; i += VAL_WG) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xa + 4 * i), c = *reinterpret_cast<const f32x4*>(xb + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(r[k] + 4 * i);
        const f32x4 x = (k & 1) ? c : a;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[k] += absdiff(x[e], q[e]);
      }
    }
  } else {
    for (int64_t i = tid; i < n_per; i += VAL_WG) {
      const float a = xa[i], c = xb[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += absdiff((k & 1) ? c : a, r[k][i]);
    }
  }
  const float *m1 = q_mu + (int64_t)b * D, *l1 = q_lv + (int64_t)b * D;
  const float *m2 = q_mu + ((int64_t)Bh + b) * D, *l2 = q_lv + ((int64_t)Bh + b) * D;
  for (int i = tid; i < D; i += VAL_WG) {
    v[4] += kl_term(m1[i], l1[i]);
    v[5] += kl_term(m2[i], l2[i]);
  }
  const float *ms = s_mu + (int64_t)b * S, *ls = s_lv + (int64_t)b * S;
  for (int i = tid; i < S; i += VAL_WG) v[6] += kl_term(ms[i], ls[i]);

  __shared__ double red[7][VAL_WG / 64];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double d = wave_sum_d(v[k]);
    if ((tid & 63) == 0) red[k][tid >> 6] = d;
  }
  __syncthreads();
  if (tid == 0) {
    double t[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double tot = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
      t[k] = k < 4 ? tot : (k < 6 ? -0.5 * tot : -tot);
    }
    // the reference's operation order, in float64 from the unrounded sums: one rounding, at the store
    const double loss = (double)mse_cof * (((t[0] + t[1]) + t[2]) + t[3]) + (double)kl_cof * (t[4] + t[5]);
    float* o = out + (int64_t)b * 8;
    o[0] = (float)loss;
#pragma unroll
    for (int k = 0; k < 7; ++k) o[1 + k] = (float)t[k];
  }
}

// One workgroup per output row g (g == G: the total).  The rows are classified VAL_WG at a time into LDS (thread t looks at
// row p0 + t: its group and whether all K values are finite), then thread k < K walks the chunk in row order: sums[g][k] is a
// sequential float64 sum over p = 0 ... P - 1 that starts from what the buffer held.
__global__ __launch_bounds__(VAL_WG) void group_sum_kernel(const float* __restrict__ rows, const int* __restrict__ group,
                                                           int P, int K, int G, double* __restrict__ sums,
                                                           int64_t* __restrict__ counts, int64_t* __restrict__ bad) {
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ int s_group[VAL_WG];
  __shared__ unsigned char s_finite[VAL_WG];
  double acc = tid < K ? sums[(int64_t)g * K + tid] : 0.0;
  int64_t n_ok = 0, n_bad = 0;                  // thread 0 only
  for (int p0 = 0; p0 < P; p0 += VAL_WG) {
    const int np = min(VAL_WG, P - p0);
    if (tid < np) {
      const float* row = rows + (int64_t)(p0 + tid) * K;
      bool fin = true;
      for (int k = 0; k < K; ++k) fin = fin && isfinite(row[k]);
      s_group[tid] = group[p0 + tid];
      s_finite[tid] = fin ? 1 : 0;
    }
    __syncthreads();
    for (int q = 0; q < np; ++q) {
      const int gp = s_group[q];
      if (g != G && gp != g) continue;
      if (gp >= 0 && gp < G && s_finite[q]) {
        if (tid < K) acc += (double)rows[(int64_t)(p0 + q) * K + tid];
        if (tid == 0) ++n_ok;
      } else if (tid == 0) {
        ++n_bad;                                // g < G: gp == g, so in range and not finite; g == G: either kind
      }
    }
    __syncthreads();
  }
  if (tid < K) sums[(int64_t)g * K + tid] = acc;
  if (tid == 0) {
    counts[g] += n_ok;
    bad[g] += n_bad;
  }
}

}  // namespace

DVAE_API int dvae_pair_metrics(const float* x1, const float* x2, const float* rec, const float* rec_hat, const float* q_mu,
                               const float* q_lv, const float* s_mu, const float* s_lv, float* out, int Bh, int64_t n_per,
                               int D, int S, float mse_cof, float kl_cof, void* stream) {
  if (!x1 || !x2 || !rec || !rec_hat || !q_mu || !q_lv || !s_mu || !s_lv || !out) return DVAE_EINVAL;
  if (Bh < 1 || n_per < 1 || D < 1 || S < 1) return DVAE_EINVAL;
  const uintptr_t al = (uintptr_t)x1 | (uintptr_t)x2 | (uintptr_t)rec | (uintptr_t)rec_hat;
  if (al & 3) return DVAE_EINVAL;
  // rows start 16-byte aligned when the bases are and n_per is a multiple of 4 (rec + Bh * n_per included)
  const bool vec = !(al & 15) && !(n_per & 3);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(pair_metrics_kernel<true>, dim3(Bh), dim3(VAL_WG), 0, s, x1, x2, rec, rec_hat, q_mu, q_lv, s_mu, s_lv,
                       out, Bh, n_per, D, S, mse_cof, kl_cof);
  else
    hipLaunchKernelGGL(pair_metrics_kernel<false>, dim3(Bh), dim3(VAL_WG), 0, s, x1, x2, rec, rec_hat, q_mu, q_lv, s_mu,
                       s_lv, out, Bh, n_per, D, S, mse_cof, kl_cof);
  return dvae_check_launch();
}

DVAE_API int dvae_group_sum_f64(const float* rows, const int* group, int P, int K, int G, double* sums, int64_t* counts,
                                int64_t* bad, void* stream) {
  if (!rows || !group || !sums || !counts || !bad || P < 1 || K < 1 || K > VAL_WG || G < 1) return DVAE_EINVAL;
  if ((((uintptr_t)sums) | ((uintptr_t)counts) | ((uintptr_t)bad)) & 7) return DVAE_EINVAL;
  hipLaunchKernelGGL(group_sum_kernel, dim3(G + 1), dim3(VAL_WG), 0, (hipStream_t)stream, rows, group, P, K, G, sums, counts,
                     bad);
  return dvae_check_launch();
}
