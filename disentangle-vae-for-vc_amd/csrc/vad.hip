// Energy-based silence trimming of the corpus tool (include/dvae_hip.h, "silence trimming"): the stage of
// preprocessing/encoder/audio.py:78-118 `trim_long_silences` between volume normalisation and the mel, on the packed batch
// of dvae_resample_batch / dvae_volume_normalize.  Three plain grids, one launch each for the whole batch: no atomics on
// floating point, one writer per output element, no word passed between workgroups.  Everything behind the window energy
// is integer logic, so an utterance's result depends on that utterance alone.
#include "common.h"  // (csrc/frontend.hip includes this file at its end)

namespace {

constexpr int VAD_WIN = DVAE_VAD_WINDOW;               // 30 ms at 16 kHz
constexpr int VAD_LANES = VAD_WIN / 8;                 // 60 of a wave's 64 lanes hold 8 consecutive samples each
constexpr int VAD_WAVES = 4;                           // windows per workgroup of the energy and the compaction grids
constexpr int VAD_BINS = DVAE_VAD_BINS;
constexpr int MK_THREADS = 256;                        // the mask kernel's chunk: one window per thread
static_assert(VAD_WIN % 8 == 0 && VAD_LANES <= 64 && VAD_WIN / 4 <= 128, "a wave64 covers one window");

// window gw of the map -> its segment and index; false where the map does not fit the segment table
__device__ __forceinline__ bool vad_window(const int64_t* __restrict__ wins, const int64_t* __restrict__ segs, int nseg,
                                           int64_t gw, int64_t& sg, int64_t& w, int64_t& out0) {
  sg = wins[2 * gw];
  w = wins[2 * gw + 1];
  if (sg < 0 || sg >= nseg || w < 0) return false;
  out0 = segs[6 * sg + 2];
  return w < segs[6 * sg + 3] / VAD_WIN;
}

// E_w = sum over the window's 480 samples of (y[i] - 0.97 y[i-1])^2 in float64 (y[-1] = 0 at the utterance's first sample,
// the predecessor crosses window borders): lane l < 60 its 8 samples in index order, then the xor tree over the wave.
// b_w = clamp(ilogb(E_w) + 80, 0, 95) from the exponent field (0 for zero and subnormals).
__global__ void __launch_bounds__(64 * VAD_WAVES) vad_energy_kernel(const float* __restrict__ y,
                                                                   const int64_t* __restrict__ segs, int nseg,
                                                                   const int64_t* __restrict__ wins, int64_t nwin,
                                                                   double* __restrict__ E, int* __restrict__ bins) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * VAD_WAVES + (threadIdx.x >> 6);
  if (gw >= nwin) return;                              // wave-uniform
  int64_t sg, w, out0;
  if (!vad_window(wins, segs, nseg, gw, sg, w, out0)) {
    if (lane == 0) {
      if (E) E[gw] = 0.0;
      bins[gw] = 0;
    }
    return;
  }
  const float* p = y + out0 + w * VAD_WIN;
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
  if (lane < VAD_LANES) {
    a = reinterpret_cast<const f32x4*>(p)[2 * lane];
    b = reinterpret_cast<const f32x4*>(p)[2 * lane + 1];
  }
  float prev = __shfl_up(b[3], 1, 64);
  if (lane == 0) prev = w > 0 ? p[-1] : 0.f;
  const float v[9] = {prev, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  double acc = 0.0;
  if (lane < VAD_LANES) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double d = (double)v[e + 1] - DVAE_VAD_PREEMPH * (double)v[e];
      acc += d * d;
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) {
    const uint64_t u = (uint64_t)__double_as_longlong(acc);
    const int ex = (int)((u >> 52) & 0x7ff);
    const int bin = ex == 0 ? 0 : min(max(ex - 1023 + DVAE_VAD_BIN_OFFSET, 0), VAD_BINS - 1);
    if (E) E[gw] = acc;
    bins[gw] = bin;
  }
}

// One workgroup per utterance: histogram of the bins -> b10, b90, t; then per chunk of MK_THREADS windows the flags, the
// 8-wide majority mask, its 7-wide dilation and the running count of kept windows.
__global__ void __launch_bounds__(MK_THREADS) vad_mask_kernel(const int64_t* __restrict__ segs,
                                                              const int64_t* __restrict__ win_first, int64_t nwin,
                                                              const int* __restrict__ bins, int* __restrict__ flags,
                                                              int* __restrict__ keep, int* __restrict__ dst,
                                                              int* __restrict__ t_out, int* __restrict__ K) {
  __shared__ int hist[VAD_BINS];
  __shared__ int fl[MK_THREADS + 13];                  // flags of windows [c0 - 6, c0 + MK_THREADS + 7)
  __shared__ int mk[MK_THREADS + 6];                   // mask of windows  [c0 - 3, c0 + MK_THREADS + 3)
  __shared__ int wave_tot[MK_THREADS / 64];
  __shared__ int t_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sg = blockIdx.x;
  const int64_t first = win_first[sg];
  int64_t W = segs[6 * sg + 3] / VAD_WIN;
  if (W < 0 || first < 0 || first + W > nwin) W = 0;   // a map that does not fit: nothing kept, nothing read
  const int* bs = bins + first;
  for (int i = tid; i < VAD_BINS; i += MK_THREADS) hist[i] = 0;
  __syncthreads();
  for (int64_t w = tid; w < W; w += MK_THREADS) atomicAdd(&hist[bs[w]], 1);   // integer adds: any order, one sum
  __syncthreads();
  if (tid == 0) {
    const int64_t n10 = (W + 9) / 10, n90 = (9 * W + 9) / 10;
    int b10 = -1, b90 = -1;
    int64_t c = 0;
    for (int b = 0; b < VAD_BINS; ++b) {
      c += hist[b];
      if (b10 < 0 && c >= n10) b10 = b;
      if (b90 < 0 && c >= n90) b90 = b;
    }
    t_s = max(DVAE_VAD_BIN_FLOOR, min(b10 + DVAE_VAD_BIN_ABOVE_P10, b90 - DVAE_VAD_BIN_BELOW_P90));
  }
  __syncthreads();
  const int t = t_s;
  int base = 0;                                        // kept windows before this chunk (the same in every thread)
  for (int64_t c0 = 0; c0 < W; c0 += MK_THREADS) {
    for (int i = tid; i < MK_THREADS + 13; i += MK_THREADS) {
      const int64_t w = c0 - 6 + i;
      fl[i] = (w >= 0 && w < W) ? (bs[w] >= t) : 0;
    }
    __syncthreads();
    for (int i = tid; i < MK_THREADS + 6; i += MK_THREADS) {
      const int64_t w = c0 - 3 + i;                    // flags of [w - 3, w + 4] are fl[i .. i + 7]
      int n = 0;
#pragma unroll
      for (int j = 0; j < DVAE_VAD_MA_WIDTH; ++j) n += fl[i + j];
      mk[i] = (w >= 0 && w < W) ? (2 * n > DVAE_VAD_MA_WIDTH) : 0;
    }
    __syncthreads();
    const int64_t w = c0 + tid;
    int kp = 0;
    if (w < W) {
#pragma unroll
      for (int j = 0; j <= DVAE_VAD_MAX_SILENCE; ++j) kp |= mk[tid + j];   // mask of [w - 3, w + 3]
    }
    const unsigned long long votes = __ballot(kp);
    if (lane == 0) wave_tot[wv] = __popcll(votes);
    __syncthreads();
    int before = base, total = 0;
#pragma unroll
    for (int i = 0; i < MK_THREADS / 64; ++i) {
      if (i < wv) before += wave_tot[i];
      total += wave_tot[i];
    }
    before += __popcll(votes & ((1ull << lane) - 1ull));
    if (w < W) {
      if (flags) flags[first + w] = fl[tid + 6];
      keep[first + w] = kp;
      dst[first + w] = before;
    }
    base += total;
    __syncthreads();                                   // fl, mk and wave_tot are rewritten by the next chunk
  }
  if (tid == 0) {
    if (t_out) t_out[sg] = t;
    K[sg] = base;
  }
}

// kept window -> out[out0 + 480 dst_w ..]: a wave per window, 120 16-byte loads and stores
__global__ void __launch_bounds__(64 * VAD_WAVES) vad_compact_kernel(const float* __restrict__ y, float* __restrict__ out,
                                                                    const int64_t* __restrict__ segs, int nseg,
                                                                    const int64_t* __restrict__ wins, int64_t nwin,
                                                                    const int* __restrict__ keep,
                                                                    const int* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * VAD_WAVES + (threadIdx.x >> 6);
  if (gw >= nwin) return;
  int64_t sg, w, out0;
  if (!vad_window(wins, segs, nseg, gw, sg, w, out0) || !keep[gw]) return;
  const int64_t d = dst[gw];
  if (d < 0 || d > w) return;                          // a kept window never moves up
  const f32x4* src = reinterpret_cast<const f32x4*>(y + out0 + w * VAD_WIN);
  f32x4* to = reinterpret_cast<f32x4*>(out + out0 + d * VAD_WIN);
  to[lane] = src[lane];
  if (lane + 64 < VAD_WIN / 4) to[lane + 64] = src[lane + 64];
}

inline bool misaligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) != 0; }

}  // namespace

DVAE_API int dvae_vad_trim(const float* y, float* out, const int64_t* segs_host, const int64_t* segs, int nseg,
                           const int64_t* wins, int64_t nwin, const int64_t* win_first, double* E, int* bins, int* flags,
                           int* keep, int* dst, int* t, int* K, void* stream) {
  if (nseg < 0 || nwin < 0) return DVAE_EINVAL;
  if (nseg == 0) return nwin == 0 ? DVAE_OK : DVAE_EINVAL;
  if (!y || !out || y == out || !segs_host || !segs || !win_first || !K || (nwin > 0 && (!wins || !bins || !keep || !dst)))
    return DVAE_EINVAL;
  if (misaligned(y, 16) || misaligned(out, 16) || misaligned(segs, 8) || misaligned(wins, 8) || misaligned(win_first, 8) ||
      misaligned(E, 8) || misaligned(bins, 4) || misaligned(flags, 4) || misaligned(keep, 4) || misaligned(dst, 4) ||
      misaligned(t, 4) || misaligned(K, 4))
    return DVAE_EINVAL;
  int64_t total = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t out0 = segs_host[6 * s + 2], n = segs_host[6 * s + 3];
    if (out0 < 0 || (out0 & 3) || n < 0) return DVAE_EINVAL;
    total += n / VAD_WIN;
  }
  if (total != nwin || (nwin + VAD_WAVES - 1) / VAD_WAVES > 0x7fffffff) return DVAE_EINVAL;
  const hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((nwin + VAD_WAVES - 1) / VAD_WAVES);
  int rc;
  if (nwin > 0) {
    ProfScope prof(DVAE_PROF_AUDIO, st, 0.0, 3);
    hipLaunchKernelGGL(vad_energy_kernel, dim3(grid), dim3(64 * VAD_WAVES), 0, st, y, segs, nseg, wins, nwin, E, bins);
    if ((rc = dvae_check_launch())) return rc;
  }
  {
    ProfScope prof(DVAE_PROF_AUDIO, st, 0.0, 4);
    hipLaunchKernelGGL(vad_mask_kernel, dim3((unsigned)nseg), dim3(MK_THREADS), 0, st, segs, win_first, nwin, bins, flags,
                       keep, dst, t, K);
    if ((rc = dvae_check_launch())) return rc;
  }
  if (nwin > 0) {
    ProfScope prof(DVAE_PROF_AUDIO, st, 0.0, 5);
    hipLaunchKernelGGL(vad_compact_kernel, dim3(grid), dim3(64 * VAD_WAVES), 0, st, y, out, segs, nseg, wins, nwin, keep,
                       dst);
    if ((rc = dvae_check_launch())) return rc;
  }
  return DVAE_OK;
}
