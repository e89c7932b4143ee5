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
