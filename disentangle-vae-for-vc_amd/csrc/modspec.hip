// Over-smoothing instruments of the conversion chain (include/dvae_hip.h, "modulation spectrum"): the global
// variance of packed mels, the modulation spectrum of windows cut by dvae_mel_to_windows, its exact float64 group sums and
// the modulation-spectrum postfilter.  Every accumulation is float64 in a fixed order, one writer per output element, no
// atomics, nothing passed between workgroups: a launch gives the same bits twice.
//
// Thread mapping of the two window kernels.  A workgroup owns MS_BINS = 16 bins of ONE window: it stages them once as centred
// float64 frames (16 KB at D = 128) beside the twiddle table (2 KB) and, in the filter, the 16 x D/2 filtered coefficients
// (16 KB) — 34 KB of LDS, four workgroups to a CU.  At C = 80 that is five workgroups a window, which fills the chip from
// about 50 windows on, where one workgroup per window (40 KB of fp32 frames) would need 256.  Forward: thread <-> (bin, k), t
// in index order; the D/2 threads of a bin read the same frame (a broadcast) and the twiddle at k t mod D.  Inverse: thread <->
// (bin, t), k in index order.
#include "common.h"  // (csrc/elem.hip includes this file at its end)

namespace {

constexpr int MS_BINS = 16;                            // bins of a window per workgroup
constexpr int MS_THREADS = 256;
constexpr int MS_DMAX = DVAE_MODSPEC_DMAX;
constexpr int MS_SEG = MS_THREADS / MS_BINS;           // threads that share a bin's meanstatic_assert(MS_SEG == 16 && MS_DMAX % 2 == 0 && MS_DMAX <= MS_THREADS, "16 lanes a bin, one thread a frame");

struct MsTile {
  double d[MS_BINS][MS_DMAX];                          // y_t - mean
  double tw[MS_DMAX][2];                               // cos, sin of 2 pi j / D
  double mean[MS_BINS];
};

// frames of bins [c0, c0 + nb) of one window (bin b at win + b ld) -> centred float64 frames in LDS.  mean: lane j of a bin's
// 16 adds frames j, j + 16, ... in index order, then a fixed xor tree over the 16 (they lie in one wave).
__device__ __forceinline__ void ms_stage(const float* __restrict__ win, int64_t ld, int nb, int D,
                                         const double* __restrict__ twiddle, MsTile& s) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nb * D; i += MS_THREADS) s.d[i / D][i % D] = (double)win[(i / D) * ld + i % D];
  for (int i = tid; i < 2 * D; i += MS_THREADS) s.tw[i >> 1][i & 1] = twiddle[i];
  __syncthreads();
  const int b = tid / MS_SEG, j = tid % MS_SEG;
  double a = 0.0;
  if (b < nb)
    for (int t = j; t < D; t += MS_SEG) a += s.d[b][t];
#pragma unroll
  for (int o = MS_SEG / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if (b < nb && j == 0) s.mean[b] = a / (double)D;
  __syncthreads();
  for (int i = tid; i < nb * D; i += MS_THREADS) s.d[i / D][i % D] -= s.mean[i / D];
  __syncthreads();
}

// Y_k = sum_t d_t e^{-2 pi i k t / D}, t in index order
__device__ __forceinline__ void ms_dft(const MsTile& s, int b, int k, int D, double& re, double& im) {
  re = 0.0;
  im = 0.0;
  int idx = 0;                                         // k t mod D
  for (int t = 0; t < D; ++t) {
    const double v = s.d[b][t];
    re += v * s.tw[idx][0];
    im -= v * s.tw[idx][1];
    idx += k;
    if (idx >= D) idx -= D;
  }
}

// rows[(w C + c)] = s_1 .. s_{D/2} | s_1^2 .. s_{D/2}^2 with s_k = fp32(ln max(|Y_k|^2, FLOOR)) and the square that of the
// stored value, taken in float64 and rounded once
__global__ void __launch_bounds__(MS_THREADS) modspec_windows_kernel(const float* __restrict__ windows, int C, int D,
                                                                     const double* __restrict__ twiddle,
                                                                     float* __restrict__ rows) {
  __shared__ MsTile s;
  const int w = blockIdx.x, c0 = blockIdx.y * MS_BINS, nb = min(MS_BINS, C - c0), H = D / 2;
  ms_stage(windows + ((int64_t)w * C + c0) * D, D, nb, D, twiddle, s);
  for (int i = threadIdx.x; i < nb * H; i += MS_THREADS) {
    const int b = i / H, k = i % H + 1;
    double re, im;
    ms_dft(s, b, k, D, re, im);
    const float sf = (float)log(fmax(re * re + im * im, DVAE_MODSPEC_FLOOR));
    float* row = rows + ((int64_t)w * C + c0 + b) * D;
    row[k - 1] = sf;
    row[H + k - 1] = (float)((double)sf * (double)sf);
  }
}

// the postfilter of one window tile: s -> s' -> the clamped log-gain -> Y'_k = Y_k e^gain (scaled by c_k / D here) -> y'
__global__ void __launch_bounds__(MS_THREADS) modspec_filter_kernel(const float* __restrict__ windows, int C, int D,
                                                                    const double* __restrict__ twiddle,
                                                                    const double* __restrict__ mu_n,
                                                                    const double* __restrict__ sigma_n,
                                                                    const double* __restrict__ mu_g,
                                                                    const double* __restrict__ sigma_g, double alpha,
                                                                    double max_log_gain, float* __restrict__ out) {
  __shared__ MsTile s;
  __shared__ double Y[MS_BINS][MS_DMAX / 2][2];
  const int w = blockIdx.x, c0 = blockIdx.y * MS_BINS, nb = min(MS_BINS, C - c0), H = D / 2;
  ms_stage(windows + ((int64_t)w * C + c0) * D, D, nb, D, twiddle, s);
  for (int i = threadIdx.x; i < nb * H; i += MS_THREADS) {
    const int b = i / H, k = i % H + 1;
    double re, im;
    ms_dft(s, b, k, D, re, im);
    const double sk = log(fmax(re * re + im * im, DVAE_MODSPEC_FLOOR));
    const int64_t q = (int64_t)(c0 + b) * H + (k - 1);
    const double r = fmax(sigma_n[q], DVAE_MODSPEC_SIGMA_MIN) / fmax(sigma_g[q], DVAE_MODSPEC_SIGMA_MIN);
    const double sp = (1.0 - alpha) * sk + alpha * (r * (sk - mu_g[q]) + mu_n[q]);
    const double lg = fmin(fmax(0.5 * (sp - sk), -max_log_gain), max_log_gain);
    const double g = exp(lg) * ((k == H ? 1.0 : 2.0) / (double)D);
    Y[b][k - 1][0] = re * g;
    Y[b][k - 1][1] = im * g;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb * D; i += MS_THREADS) {
    const int b = i / D, t = i % D;
    double acc = 0.0;
    int idx = t;                                       // k t mod D
    for (int k = 1; k <= H; ++k) {
      acc += Y[b][k - 1][0] * s.tw[idx][0] - Y[b][k - 1][1] * s.tw[idx][1];
      idx += t;
      if (idx >= D) idx -= D;
    }
    out[((int64_t)w * C + c0 + b) * D + t] = (float)(s.mean[b] + acc);
  }
}

__global__ void __launch_bounds__(256) ms_copy_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = in[i];
}

// One wave per (utterance, bin): lane l adds frames l, l + 64, ... in index order, then the xor tree over the wave; the mean
// first, the centred squares second.  An entry of the table that does not fit the buffer gives NaN and reads nothing.
__global__ void __launch_bounds__(256) mel_gv_kernel(const float* __restrict__ x, int64_t ld, const int* __restrict__ utt,
                                                     int C, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x, c = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= C) return;                                  // wave-uniform
  const int col0 = utt[4 * u], L = utt[4 * u + 1];
  double* o = out + ((int64_t)u * C + c) * 2;
  if (col0 < 0 || L < 1 || (int64_t)col0 + L > ld) {
    if (lane == 0) o[0] = o[1] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const float* p = x + (int64_t)c * ld + col0;
  double a = 0.0;
  for (int t = lane; t < L; t += 64) a += (double)p[t];
  const double m = wave_sum_d(a) / (double)L;
  double q = 0.0;
  for (int t = lane; t < L; t += 64) {
    const double e = (double)p[t] - m;
    q += e * e;
  }
  const double v = wave_sum_d(q) / (double)L;
  if (lane == 0) {
    o[0] = m;
    o[1] = v;
  }
}

// sums[g][c][j] = the float64 sum of rows[order[i] C + c][j] over i in [first[g], first[g + 1]), in that order from +0:
// workgroup (g, c), thread j.  Only the group's own rows are read; an index outside [0, nwin) is passed over.
__global__ void __launch_bounds__(MS_DMAX) ms_group_sum_kernel(const float* __restrict__ rows, const int* __restrict__ order,
                                                               int norder, const int* __restrict__ first, int nwin, int C,
                                                               int D, double* __restrict__ sums) {
  const int g = blockIdx.x, c = blockIdx.y, j = threadIdx.x;
  if (j >= D) return;
  const int a = max(first[g], 0), b = min(first[g + 1], norder);
  double acc = 0.0;
  for (int i = a; i < b; ++i) {
    const int w = order[i];
    if (w < 0 || w >= nwin) continue;
    acc += (double)rows[((int64_t)w * C + c) * D + j];
  }
  sums[((int64_t)g * C + c) * D + j] = acc;
}

inline bool ms_misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }
inline bool ms_bad_shape(int nwin, int C, int D) {
  return nwin < 1 || C < 1 || C > 65535 || D < DVAE_MODSPEC_DMIN || D > DVAE_MODSPEC_DMAX || (D & 1);
}

}  // namespace

DVAE_API int dvae_mel_gv(const float* x, int64_t ld, const int* utt_table, int nutt, int C, double* out, void* stream) {
  if (!x || !utt_table || !out || ld < 1 || nutt < 1 || C < 1 || C > 4 * 65535 || ms_misaligned(out, 8)) return DVAE_EINVAL;
  hipLaunchKernelGGL(mel_gv_kernel, dim3((unsigned)nutt, (unsigned)((C + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ld,
                     utt_table, C, out);
  return dvae_check_launch();
}

DVAE_API int dvae_modspec_windows(const float* windows, int nwin, int C, int D, const double* twiddle, float* rows,
                                  void* stream) {
  if (!windows || !twiddle || !rows || ms_bad_shape(nwin, C, D) || ms_misaligned(twiddle, 8)) return DVAE_EINVAL;
  hipLaunchKernelGGL(modspec_windows_kernel, dim3((unsigned)nwin, (unsigned)((C + MS_BINS - 1) / MS_BINS)), dim3(MS_THREADS),
                     0, (hipStream_t)stream, windows, C, D, twiddle, rows);
  return dvae_check_launch();
}

DVAE_API int dvae_modspec_group_sum(const float* rows, const int* order, int norder, const int* group_first, int G, int nwin,
                                    int C, int D, double* sums, void* stream) {
  if (!rows || !order || !group_first || !sums || norder < 1 || G < 1 || ms_bad_shape(nwin, C, D) || ms_misaligned(sums, 8))
    return DVAE_EINVAL;
  hipLaunchKernelGGL(ms_group_sum_kernel, dim3((unsigned)G, (unsigned)C), dim3(MS_DMAX), 0, (hipStream_t)stream, rows, order,
                     norder, group_first, nwin, C, D, sums);
  return dvae_check_launch();
}

DVAE_API int dvae_modspec_filter(const float* windows, int nwin, int C, int D, const double* twiddle, const double* mu_n,
                                 const double* sigma_n, const double* mu_g, const double* sigma_g, double alpha,
                                 double max_gain_db, float* out, void* stream) {
  if (!windows || !twiddle || !mu_n || !sigma_n || !mu_g || !sigma_g || !out || out == windows || ms_bad_shape(nwin, C, D) ||
      !(alpha >= 0.0 && alpha <= 1.0) || !(max_gain_db > 0.0) || ms_misaligned(twiddle, 8) || ms_misaligned(mu_n, 8) ||
      ms_misaligned(sigma_n, 8) || ms_misaligned(mu_g, 8) || ms_misaligned(sigma_g, 8))
    return DVAE_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  if (alpha == 0.0) {                                  // the input's bits
    const int64_t n = (int64_t)nwin * C * D;
    hipLaunchKernelGGL(ms_copy_kernel, dim3((unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, st,
                       windows, out, n);
    return dvae_check_launch();
  }
  hipLaunchKernelGGL(modspec_filter_kernel, dim3((unsigned)nwin, (unsigned)((C + MS_BINS - 1) / MS_BINS)), dim3(MS_THREADS),
                     0, st, windows, C, D, twiddle, mu_n, sigma_n, mu_g, sigma_g, alpha,
                     max_gain_db * 0.11512925464970228420, out);
  return dvae_check_launch();
}
