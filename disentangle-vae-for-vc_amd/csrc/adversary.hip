// Speaker adversary on the content latent (dvae_amd/adversary.py): Linear(D, H) -> ReLU -> Linear(H, S) ->
// softmax cross-entropy on R rows, forward and backward, as TWO launches.  R = 128, D = 28, H = 256, S = 109 is some
// 10 MFLOP: what a step pays for is launches, not arithmetic.  Part of probe.hip's translation unit (included at its end).
//   adv_rows_kernel     one workgroup per row: everything a row owns (loss, arg-max, h, g2, g1, dx)
//   adv_params_kernel   one lane per element of (dw2, db2, dw1, db1): the sum over the rows in ascending order, stored;
//                       one more workgroup adds the four statistics
// No atomics; every sum has one owner and one order, which depends on (D, H, S) alone: a row's bits do not depend on the
// other rows, a parameter gradient's bits not on the other parameters, and two launches give the same bits.

namespace {

constexpr int ADV_WG = 512;                 // 8 waves
constexpr int ADV_NW = ADV_WG / 64;
constexpr int ADV_MAX_D = 64;               // DVAE_ADV_MAX_D
constexpr int ADV_MAX_H = 1024;             // DVAE_ADV_MAX_H

__device__ __forceinline__ bool adv_counted(int label, int S) { return label >= 0 && label < S; }

__global__ __launch_bounds__(ADV_WG) void adv_rows_kernel(
    const float* __restrict__ x, int64_t ldx, const int* __restrict__ labels, const float* __restrict__ w1, int ldw1,
    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
    const float* __restrict__ coef, float inv_rows, int D, int H, int S, float* __restrict__ row_loss,
    int* __restrict__ row_pred, float* __restrict__ h_out, float* __restrict__ g2_out, float* __restrict__ g1_out,
    float* __restrict__ dx, int64_t lddx, int dx_col0) {
  __shared__ float xs[ADV_MAX_D];
  __shared__ __attribute__((aligned(16))) float hs[ADV_MAX_H];
  __shared__ float ls[DVAE_CE_MAX_CLASSES];      // the logits, then g2
  __shared__ float g1s[ADV_MAX_H];
  __shared__ float part[ADV_NW][ADV_MAX_D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = blockIdx.x;
  const int label = labels[r];
  const bool counted = adv_counted(label, S);      // uniform: the workgroup has one row
  const float lam = coef[0];

  if (tid < ADV_MAX_D) xs[tid] = tid < D ? x[r * ldx + tid] : 0.f;
  __syncthreads();

  // h_j = relu(sum_d w1[j, d] x_d + b1_j): d ascending from +0, one fma per term, then the bias
  for (int j = tid; j < H; j += ADV_WG) {
    const f32x4* wr = reinterpret_cast<const f32x4*>(w1 + (int64_t)j * ldw1);
    float acc = 0.f;
    for (int p = 0; 4 * p < D; ++p) {
      const f32x4 w = wr[p];      // ldw1 % 4 == 0 and D <= ldw1: the whole piece lies inside the row
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * p + k < D) acc = __builtin_fmaf(w[k], xs[4 * p + k], acc);
    }
    const float pre = acc + b1[j];
    const float hj = pre > 0.f ? pre : 0.f;
    hs[j] = hj;
    h_out[r * H + j] = hj;
  }
  __syncthreads();

  // logit_c = sum_j w2[c, j] h_j + b2_c: a wave per class; lane l adds the 16-byte pieces l, l + 64, ... of the row in
  // ascending order (one fma per term, from +0), the lanes are added by the xor tree, then the bias
  const int np = H / 4;
#pragma unroll 4
  for (int c = wave; c < S; c += ADV_NW) {
    const f32x4* wr = reinterpret_cast<const f32x4*>(w2 + (int64_t)c * H);
    float acc = 0.f;
    for (int p = lane; p < np; p += 64) {
      const f32x4 w = wr[p], hv = reinterpret_cast<const f32x4*>(hs)[p];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc = __builtin_fmaf(w[k], hv[k], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) ls[c] = acc + b2[c];
  }
  __syncthreads();

  // the row's statistics, by every wave for itself (the same order, hence the same bits, in each): no barrier, no broadcast
  float m = -INFINITY;
  int am = INT_MAX;
  for (int c = lane; c < S; c += 64) {      // ascending per lane: `>` keeps the lowest index of a tie
    const float v = ls[c];
    if (v > m) {
      m = v;
      am = c;
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
  float s = 0.f;
  for (int c = lane; c < S; c += 64) s += expf(ls[c] - m);
  s = wave_sum(s);
  const float xl = counted ? ls[label] - m : 0.f;
  if (tid == 0) {
    row_loss[r] = counted ? logf(s) - xl : 0.f;
    row_pred[r] = am == INT_MAX ? 0 : am;
  }
  const float inv = 1.f / s;
  __syncthreads();      // every wave has read the logits: ls becomes g2

  // g2_c = inv_rows (softmax_c - onehot_c); an ignored row has no gradient
  for (int c = tid; c < S; c += ADV_WG) {
    float g = 0.f;
    if (counted) g = inv_rows * (expf(ls[c] - m) * inv - (c == label ? 1.f : 0.f));
    ls[c] = g;
    g2_out[r * S + c] = g;
  }
  __syncthreads();

  // g1_j = (h_j > 0) sum_c g2_c w2[c, j]: c ascending from +0, one fma per term
  for (int j = tid; j < H; j += ADV_WG) {
    float acc = 0.f;
    if (counted && hs[j] > 0.f)
      for (int c = 0; c < S; ++c) acc = __builtin_fmaf(ls[c], w2[(int64_t)c * H + j], acc);
    else
      acc = 0.f;
    g1s[j] = acc;
    g1_out[r * H + j] = acc;
  }
  __syncthreads();

  // dx_d = -lam sum_j g1_j w1[j, d]: wave q adds j in [q H / 8, (q + 1) H / 8) in ascending order, the eight sums are added
  // in wave order.  lam == 0 (the adversary only monitors) and an ignored row write +0.0 whatever the sums hold.
  const bool live = counted && lam != 0.f;
  if (live && lane < D) {
    const int j0 = wave * (H / ADV_NW), j1 = j0 + H / ADV_NW;
    float acc = 0.f;
    for (int j = j0; j < j1; ++j) acc = __builtin_fmaf(g1s[j], w1[(int64_t)j * ldw1 + lane], acc);
    part[wave][lane] = acc;
  }
  __syncthreads();
  for (int64_t c = tid; c < lddx; c += ADV_WG) {
    float v = 0.f;
    const int d = (int)(c - dx_col0);
    if (live && c >= dx_col0 && d < D) {
      float t = part[0][d];
#pragma unroll
      for (int q = 1; q < ADV_NW; ++q) t += part[q][d];
      v = -(lam * t);
    }
    dx[r * lddx + c] = v;
  }
}

// Element e of the concatenation dw2 [S, H] | db2 [S] | dw1 [H, ldw1] | db1 [H] belongs to lane e of the grid.  The rows
// are added in ascending order from +0, one fma per term; an ignored row is skipped (its g2 and g1 are zeros).  The
// workgroup behind the last element adds the statistics: rows staged in LDS, then thread 0 in row order, in float64.
__global__ __launch_bounds__(256) void adv_params_kernel(
    const float* __restrict__ x, int64_t ldx, const int* __restrict__ labels, const float* __restrict__ h,
    const float* __restrict__ g2, const float* __restrict__ g1, const float* __restrict__ row_loss,
    const int* __restrict__ row_pred, float inv_rows, int R, int D, int H, int S, float* __restrict__ dw1, int ldw1,
    float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2, float* __restrict__ out,
    unsigned grad_blocks) {
  if (blockIdx.x >= grad_blocks) {      // the statistics
    __shared__ float sl[256];
    __shared__ int sf[256];              // bit 0: counted, bit 1: row_pred == label
    double ts = 0.0;
    int tn = 0, tk = 0;
    for (int r0 = 0; r0 < R; r0 += 256) {
      const int rr = r0 + threadIdx.x;
      if (rr < R) {
        const int lab = labels[rr];
        const bool cnt = adv_counted(lab, S);
        sl[threadIdx.x] = cnt ? row_loss[rr] : 0.f;
        sf[threadIdx.x] = (cnt ? 1 : 0) | (cnt && row_pred[rr] == lab ? 2 : 0);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = R - r0 < 256 ? R - r0 : 256;
        for (int i = 0; i < n; ++i)
          if (sf[i] & 1) {
            ts += (double)sl[i];
            tn += 1;
            tk += sf[i] >> 1;
          }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      out[0] = (float)ts;
      out[1] = (float)tn;
      out[2] = (float)tk;
      out[3] = (float)(ts * (double)inv_rows);
    }
    return;
  }
  const int64_t n_w2 = (int64_t)S * H, n_w1 = (int64_t)H * ldw1;
  int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float acc = 0.f;
  if (e < n_w2) {
    const int c = (int)(e / H), j = (int)(e - (int64_t)c * H);
    for (int r = 0; r < R; ++r)
      if (adv_counted(labels[r], S)) acc = __builtin_fmaf(g2[(int64_t)r * S + c], h[(int64_t)r * H + j], acc);
    dw2[e] = acc;
    return;
  }
  e -= n_w2;
  if (e < S) {
    for (int r = 0; r < R; ++r)
      if (adv_counted(labels[r], S)) acc += g2[(int64_t)r * S + e];
    db2[e] = acc;
    return;
  }
  e -= S;
  if (e < n_w1) {
    const int j = (int)(e / ldw1), d = (int)(e - (int64_t)j * ldw1);
    if (d < D)      // a padding column keeps its zero
      for (int r = 0; r < R; ++r)
        if (adv_counted(labels[r], S)) acc = __builtin_fmaf(g1[(int64_t)r * H + j], x[(int64_t)r * ldx + d], acc);
    dw1[e] = acc;
    return;
  }
  e -= n_w1;
  if (e < H) {
    for (int r = 0; r < R; ++r)
      if (adv_counted(labels[r], S)) acc += g1[(int64_t)r * H + e];
    db1[e] = acc;
  }
}

bool adv_shape_ok(int R, int D, int H, int S, int64_t ldx, int ldw1) {
  return R >= 1 && D >= 1 && D <= ADV_MAX_D && H >= 64 && H <= ADV_MAX_H && H % 64 == 0 && S >= 1 &&
         S <= DVAE_CE_MAX_CLASSES && ldx >= D && ldw1 >= D && ldw1 % 4 == 0 && ldw1 <= ADV_MAX_D;
}

}  // namespace

static_assert(ADV_MAX_D == DVAE_ADV_MAX_D && ADV_MAX_H == DVAE_ADV_MAX_H, "include/dvae_hip.h");

DVAE_API int dvae_adv_rows(const float* x, int64_t ldx, const int* labels, const float* w1, int ldw1, const float* b1,
                           const float* w2, const float* b2, const float* coef, float inv_rows, int R, int D, int H, int S,
                           float* row_loss, int* row_pred, float* h, float* g2, float* g1, float* dx, int64_t lddx,
                           int dx_col0, void* stream) {
  if (!x || !labels || !w1 || !b1 || !w2 || !b2 || !coef || !row_loss || !row_pred || !h || !g2 || !g1 || !dx)
    return DVAE_EINVAL;
  if (!adv_shape_ok(R, D, H, S, ldx, ldw1) || dx_col0 < 0 || lddx < (int64_t)dx_col0 + D) return DVAE_EINVAL;
  if ((((uintptr_t)w1) | ((uintptr_t)w2)) & 15) return DVAE_EINVAL;
  hipLaunchKernelGGL(adv_rows_kernel, dim3((unsigned)R), dim3(ADV_WG), 0, (hipStream_t)stream, x, ldx, labels, w1, ldw1, b1,
                     w2, b2, coef, inv_rows, D, H, S, row_loss, row_pred, h, g2, g1, dx, lddx, dx_col0);
  return dvae_check_launch();
}

DVAE_API int dvae_adv_params(const float* x, int64_t ldx, const int* labels, const float* h, const float* g2,
                             const float* g1, const float* row_loss, const int* row_pred, float inv_rows, int R, int D,
                             int H, int S, float* dw1, int ldw1, float* db1, float* dw2, float* db2, float* out,
                             void* stream) {
  if (!x || !labels || !h || !g2 || !g1 || !row_loss || !row_pred || !out) return DVAE_EINVAL;
  if (!adv_shape_ok(R, D, H, S, ldx, ldw1)) return DVAE_EINVAL;
  const bool grads = dw1 && db1 && dw2 && db2;
  if (!grads && (dw1 || db1 || dw2 || db2)) return DVAE_EINVAL;      // all four, or none (evaluation: the statistics only)
  const int64_t n = (int64_t)S * H + S + (int64_t)H * ldw1 + H;
  const unsigned grad_blocks = grads ? (unsigned)((n + 255) / 256) : 0u;
  hipLaunchKernelGGL(adv_params_kernel, dim3(grad_blocks + 1), dim3(256), 0, (hipStream_t)stream, x, ldx, labels, h, g2, g1,
                     row_loss, row_pred, inv_rows, R, D, H, S, dw1, ldw1, db1, dw2, db2, out, grad_blocks);
  return dvae_check_launch();
}
