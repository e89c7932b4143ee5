// Mel front-end (reference preprocessing/utils.py:68-141): the HBM-bound pieces around the two
// contractions (windowed frames x DFT basis, magnitudes x mel basis), which run on the contraction kernel of gemm.hip.
#include "common.h"

namespace {

// frames[m][k] = win[k] * x[m*hop + k - left], zero outside the signal (lws pads fsize-hop samples on both sides and
// the tail up to a whole frame; utils.py:82-103).  One thread writes 4 consecutive k (16-byte stores).
__global__ void stft_frames_kernel(const float* __restrict__ wav, int64_t n, const float* __restrict__ win,
                                   float* __restrict__ frames, int M, int fsize, int hop, int left) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = fsize >> 2;
  if (idx >= (int64_t)M * per_row) return;
  const int m = (int)(idx / per_row), k = ((int)(idx - (int64_t)m * per_row)) << 2;
  const int64_t s = (int64_t)m * hop + k - left;
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = s + e;
    v[e] = (i >= 0 && i < n) ? wav[i] * win[k + e] : 0.f;
  }
  *reinterpret_cast<f32x4*>(frames + (int64_t)m * fsize + k) = v;
}

// reim[row][0..nbp) = Re, [nbp..2nbp) = Im  ->  mag[row][j] = sqrt(Re^2 + Im^2)
__global__ void stft_magnitude_kernel(const float* __restrict__ reim, float* __restrict__ mag, int64_t rows, int nbp) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nbp) return;
  const int64_t r = idx / nbp;
  const int j = (int)(idx - r * nbp);
  const float re = reim[r * 2 * nbp + j], im = reim[r * 2 * nbp + nbp + j];
  mag[idx] = sqrtf(re * re + im * im);
}

// out[c][col0 + m] = clip((20*log10(max(min_level, mel[m][c])) - ref_db - min_db) / -min_db, 0, 1)   (utils.py:127-137)
__global__ void mel_db_normalize_kernel(const float* __restrict__ mel, float* __restrict__ out, int M, int C,
                                        int64_t ld_out, int64_t col0, float min_level, float ref_db, float min_db) {
  __shared__ float tile[32][33];
  const int m0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 256 threads: 8 rows per pass
  for (int r = ty; r < 32; r += 8) {
    const int m = m0 + r, c = c0 + tx;
    tile[r][tx] = (m < M && c < C) ? mel[(int64_t)m * C + c] : 1.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, m = m0 + tx;
    if (c < C && m < M) {
      const float db = 20.f * log10f(fmaxf(min_level, tile[tx][r])) - ref_db;
      out[(int64_t)c * ld_out + col0 + m] = fminf(fmaxf((db - min_db) / -min_db, 0.f), 1.f);
    }
  }
}


// ---- Griffin-Lim inverse (mel -> linear magnitude -> waveform).  Every frame of every utterance of a batch is one row;
// only the overlap-add gather crosses rows, and it stays inside the utterance its segment-table entry describes.

// amp[col][c] = 10^((clip(mel[c][col], 0, 1) * -min_db + min_db + ref_db) / 20): the exact inverse of
// mel_db_normalize_kernel (above the clip), same 32 x 32 LDS transpose in the other direction
__global__ void mel_denormalize_kernel(const float* __restrict__ mel, float* __restrict__ amp, int L, int C,
                                       int64_t ld_in, float ref_db, float min_db) {
  __shared__ float tile[32][33];
  const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, l = l0 + tx;
    tile[r][tx] = (c < C && l < L) ? mel[(int64_t)c * ld_in + l] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int l = l0 + r, c = c0 + tx;
    if (l < L && c < C) {
      const float db = fminf(fmaxf(tile[tx][r], 0.f), 1.f) * -min_db + min_db + ref_db;
      amp[(int64_t)l * C + c] = exp10f(db * 0.05f);
    }
  }
}

// Projected gradient X <- max(0, X - step * M^T (M X - A)) on one frame per workgroup, all iterations on chip: the frame's
// bins live in registers (bin j = tid + PG_THREADS * i) and in LDS for the residual, the n_mels residuals in LDS.  M is
// read through its sparse form: residual f sums its bin range [lo, hi) in order, the gradient of bin j its (at most) two
// filters in slot order.  Fixed summation order, no atomics: bit-reproducible.
constexpr int PG_THREADS = 128, PG_PER = 8, PG_MAX_BINS = PG_THREADS * PG_PER, PG_MAX_MELS = 128;
__global__ void __launch_bounds__(PG_THREADS) mel_nnls_pg_kernel(const float* __restrict__ amp, float* __restrict__ x,
                                                                 int nbp, int C, const int* __restrict__ filt_range,
                                                                 const int* __restrict__ bin_filt,
                                                                 const float* __restrict__ bin_w, float step, int iters) {
  __shared__ float xs[PG_MAX_BINS];
  __shared__ float rs[PG_MAX_MELS];
  __shared__ int bf_s[PG_MAX_BINS][2];
  __shared__ float bw_s[PG_MAX_BINS][2];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  float xr[PG_PER], w0[PG_PER], w1[PG_PER];
  int f0[PG_PER], f1[PG_PER];
#pragma unroll
  for (int i = 0; i < PG_PER; ++i) {
    const int j = tid + PG_THREADS * i;
    const bool in = j < nbp;
    xr[i] = in ? x[row * nbp + j] : 0.f;
    f0[i] = in ? bin_filt[2 * j] : -1;
    f1[i] = in ? bin_filt[2 * j + 1] : -1;
    w0[i] = in ? bin_w[2 * j] : 0.f;
    w1[i] = in ? bin_w[2 * j + 1] : 0.f;
    if (in) {
      xs[j] = xr[i];
      bf_s[j][0] = f0[i];
      bf_s[j][1] = f1[i];
      bw_s[j][0] = w0[i];
      bw_s[j][1] = w1[i];
    }
  }
  int lo = 0, hi = 0;
  float a = 0.f;
  if (tid < C) {
    lo = filt_range[2 * tid];
    hi = filt_range[2 * tid + 1];
    a = amp[row * C + tid];
  }
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    if (tid < C) {
      float r = -a;
      for (int j = lo; j < hi; ++j) r += (bf_s[j][0] == tid ? bw_s[j][0] : bw_s[j][1]) * xs[j];
      rs[tid] = r;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PG_PER; ++i) {
      const int j = tid + PG_THREADS * i;
      if (j < nbp && f0[i] >= 0) {
        float g = w0[i] * rs[f0[i]];
        if (f1[i] >= 0) g += w1[i] * rs[f1[i]];
        xr[i] = fmaxf(0.f, xr[i] - step * g);
        xs[j] = xr[i];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < PG_PER; ++i) {
    const int j = tid + PG_THREADS * i;
    if (j < nbp) x[row * nbp + j] = xr[i];
  }
}

// reim = mag * (cos phase | sin phase), or (mag | 0) without a phase
__global__ void gl_init_kernel(const float* __restrict__ mag, const float* __restrict__ phase, float* __restrict__ reim,
                               int64_t rows, int nbp) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nbp) return;
  const int64_t r = idx / nbp;
  const int j = (int)(idx - r * nbp);
  const float s = mag[idx];
  float re = s, im = 0.f;
  if (phase) {
    float sn, cs;
    sincosf(phase[idx], &sn, &cs);
    re = s * cs;
    im = s * sn;
  }
  reim[r * 2 * nbp + j] = re;
  reim[r * 2 * nbp + nbp + j] = im;
}

// fast Griffin-Lim (Perraudin et al.; librosa.griffinlim): a = R - alpha R_prev, X = S a / |a| (X = S where |a| = 0)
__global__ void gl_phase_kernel(const float* __restrict__ reb, const float* __restrict__ prev, const float* __restrict__ mag,
                                float* __restrict__ reim, int64_t rows, int nbp, float alpha) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nbp) return;
  const int64_t r = idx / nbp;
  const int j = (int)(idx - r * nbp);
  const int64_t ire = r * 2 * nbp + j, iim = ire + nbp;
  float are = reb[ire], aim = reb[iim];
  if (prev) {
    are -= alpha * prev[ire];
    aim -= alpha * prev[iim];
  }
  const float s = mag[idx];
  const float a2 = are * are + aim * aim;
  float re = s, im = 0.f;
  if (a2 > 0.f) {
    const float inv = s / sqrtf(a2);
    re = are * inv;
    im = aim * inv;
  }
  reim[ire] = re;
  reim[iim] = im;
}

// segment table row: {row0, frames M, sample0, n} (int64 x 4)
__device__ __forceinline__ int find_segment(const int64_t* __restrict__ segs, int nseg, int64_t key, int col) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {             // last segment whose column `col` is <= key
    const int mid = (lo + hi + 1) >> 1;
    if (segs[4 * mid + col] <= key) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Overlap-add of the synthesis frames y[rows, fsize] of one utterance: s[t] = sum_m w[q] y[m][q], q = t + left - m*hop,
// over the (at most ceil(fsize/hop)) frames that cover padded position t + left, in increasing m; divided by the same sum
// of w[q]^2 when `norm` (a window whose squares do not overlap-add to 1).  Four consecutive samples per thread: P is a
// multiple of 4 and so is hop, hence all four share their frames.
__device__ __forceinline__ f32x4 ola4(const float* __restrict__ y, const float* __restrict__ win, int64_t row0, int M,
                                      int64_t P, int fsize, int hop, int norm) {
  const int64_t m_hi = min((int64_t)M - 1, P / hop);
  const int64_t m_lo = P >= fsize ? (P - fsize) / hop + 1 : 0;
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, e = {0.f, 0.f, 0.f, 0.f};
  for (int64_t m = m_lo; m <= m_hi; ++m) {
    const int q = (int)(P - m * hop);
    const f32x4 w = *reinterpret_cast<const f32x4*>(win + q);
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + (row0 + m) * fsize + q);
    s += w * v;
    if (norm) e += w * w;
  }
  if (norm) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = e[k] > 1e-20f ? s[k] / e[k] : 0.f;
  }
  return s;
}

// mode 0: out[rows, fsize] = the next analysis frames w[k] s[m*hop + k - left] (zero outside [0, n): the padding of
// stft_frames_kernel), without materialising s.  mode 1: out[sample0 + t] = s[t], t in [0, n).
__global__ void ola_gather_kernel(const float* __restrict__ y, const int64_t* __restrict__ segs, int nseg, int64_t rows,
                                  const float* __restrict__ win, float* __restrict__ out, int64_t out_len, int fsize,
                                  int hop, int mode, int norm) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int left = fsize - hop;
  if (mode == 0) {
    const int per_row = fsize >> 2;
    if (idx >= rows * per_row) return;
    const int64_t r = idx / per_row;
    const int k = ((int)(idx - r * per_row)) << 2;
    const int sg = find_segment(segs, nseg, r, 0);
    const int64_t row0 = segs[4 * sg], n = segs[4 * sg + 3];
    const int M = (int)segs[4 * sg + 1];
    const int64_t m = r - row0;
    const int64_t t = m * hop + k - left;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (m < M && t >= 0 && t < n) {
      const f32x4 s = ola4(y, win, row0, M, t + left, fsize, hop, norm);
      v = s * *reinterpret_cast<const f32x4*>(win + k);
    }
    *reinterpret_cast<f32x4*>(out + r * fsize + k) = v;
  } else {
    if (idx >= (out_len >> 2)) return;
    const int64_t i = idx << 2;
    const int sg = find_segment(segs, nseg, i, 2);
    const int64_t row0 = segs[4 * sg], sample0 = segs[4 * sg + 2], n = segs[4 * sg + 3];
    const int M = (int)segs[4 * sg + 1];
    const int64_t t = i - sample0;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t >= 0 && t < n) v = ola4(y, win, row0, M, t + left, fsize, hop, norm);
    *reinterpret_cast<f32x4*>(out + i) = v;
  }
}

}  // namespace

DVAE_API int dvae_stft_frames(const float* wav, int64_t n, const float* window, float* frames, int M, int fsize,
                              int hop, int left, void* stream) {
  if (!wav || !window || !frames || n < 1 || M < 1 || fsize < 4 || (fsize & 3) || hop < 1 || left < 0) return DVAE_EINVAL;
  const int64_t work = (int64_t)M * (fsize >> 2);
  hipLaunchKernelGGL(stft_frames_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     wav, n, window, frames, M, fsize, hop, left);
  return dvae_check_launch();
}

DVAE_API int dvae_stft_magnitude(const float* reim, float* mag, int64_t rows, int nbins_padded, void* stream) {
  if (!reim || !mag || rows < 1 || nbins_padded < 1) return DVAE_EINVAL;
  const int64_t work = rows * nbins_padded;
  hipLaunchKernelGGL(stft_magnitude_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reim, mag, rows, nbins_padded);
  return dvae_check_launch();
}

DVAE_API int dvae_mel_db_normalize(const float* mel, float* out, int M, int n_mels, int64_t ld_out, int64_t col0,
                                   float min_level, float ref_level_db, float min_level_db, void* stream) {
  if (!mel || !out || M < 1 || n_mels < 1 || ld_out < M || col0 < 0 || !(min_level > 0.f) || !(min_level_db < 0.f))
    return DVAE_EINVAL;
  dim3 grid((M + 31) / 32, (n_mels + 31) / 32);
  hipLaunchKernelGGL(mel_db_normalize_kernel, grid, dim3(256), 0, (hipStream_t)stream, mel, out, M, n_mels, ld_out,
                     col0, min_level, ref_level_db, min_level_db);
  return dvae_check_launch();
}

DVAE_API int dvae_mel_denormalize(const float* mel, float* amp, int L, int n_mels, int64_t ld_in, float ref_level_db,
                                  float min_level_db, void* stream) {
  if (!mel || !amp || L < 1 || n_mels < 1 || ld_in < L || !(min_level_db < 0.f)) return DVAE_EINVAL;
  dim3 grid((L + 31) / 32, (n_mels + 31) / 32);
  hipLaunchKernelGGL(mel_denormalize_kernel, grid, dim3(256), 0, (hipStream_t)stream, mel, amp, L, n_mels, ld_in,
                     ref_level_db, min_level_db);
  return dvae_check_launch();
}

DVAE_API int dvae_mel_nnls_pg(const float* amp, float* x, int64_t rows, int nbp, int n_mels, const int* filt_range,
                              const int* bin_filt, const float* bin_w, float step, int iters, void* stream) {
  if (!amp || !x || !filt_range || !bin_filt || !bin_w || rows < 1 || rows > 0x7fffffff || nbp < 1 ||
      nbp > PG_MAX_BINS || n_mels < 1 || n_mels > PG_MAX_MELS || iters < 0 || !(step > 0.f))
    return DVAE_EINVAL;
  if (iters == 0) return DVAE_OK;
  hipLaunchKernelGGL(mel_nnls_pg_kernel, dim3((unsigned)rows), dim3(PG_THREADS), 0, (hipStream_t)stream, amp, x, nbp,
                     n_mels, filt_range, bin_filt, bin_w, step, iters);
  return dvae_check_launch();
}

DVAE_API int dvae_gl_init(const float* mag, const float* phase, float* reim, int64_t rows, int nbp, void* stream) {
  if (!mag || !reim || rows < 1 || nbp < 1) return DVAE_EINVAL;
  const int64_t work = rows * nbp;
  hipLaunchKernelGGL(gl_init_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mag, phase,
                     reim, rows, nbp);
  return dvae_check_launch();
}

DVAE_API int dvae_gl_phase(const float* rebuilt, const float* prev, const float* mag, float* reim, int64_t rows, int nbp,
                           float momentum, void* stream) {
  if (!rebuilt || !mag || !reim || rows < 1 || nbp < 1 || !(momentum >= 0.f) || momentum >= 1e30f) return DVAE_EINVAL;
  const int64_t work = rows * nbp;
  hipLaunchKernelGGL(gl_phase_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rebuilt,
                     prev, mag, reim, rows, nbp, momentum / (1.f + momentum));
  return dvae_check_launch();
}

DVAE_API int dvae_gl_segment_table(const int* frames, int nseg, int fsize, int hop, int64_t* table) {
  if (!frames || !table || nseg < 1 || fsize < 4 || (fsize & 3) || hop < 4 || (hop & 3) || hop > fsize || fsize % hop)
    return DVAE_EINVAL;
  const int min_frames = fsize / hop;          // M frames <-> n = (M - fsize/hop + 1) * hop samples, n >= hop
  int64_t row0 = 0, sample0 = 0;
  for (int s = 0; s < nseg; ++s) {
    if (frames[s] < min_frames) return DVAE_EINVAL;
    const int64_t n = (int64_t)(frames[s] - min_frames + 1) * hop;
    table[4 * s] = row0;
    table[4 * s + 1] = frames[s];
    table[4 * s + 2] = sample0;
    table[4 * s + 3] = n;
    row0 += frames[s];
    sample0 += n;
  }
  return DVAE_OK;
}

DVAE_API int dvae_ola_gather(const float* y, const int64_t* segs, int nseg, int64_t rows, const float* window, float* out,
                             int64_t out_len, int fsize, int hop, int mode, int norm, void* stream) {
  if (!y || !segs || !window || !out || nseg < 1 || rows < 1 || fsize < 4 || (fsize & 3) || hop < 4 || (hop & 3) ||
      hop > fsize || (mode != 0 && mode != 1) || (mode == 1 && (out_len < 4 || (out_len & 3))) ||
      ((((uintptr_t)y) | ((uintptr_t)window) | ((uintptr_t)out)) & 15))
    return DVAE_EINVAL;
  const int64_t work = mode == 0 ? rows * (fsize >> 2) : (out_len >> 2);
  hipLaunchKernelGGL(ola_gather_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, segs,
                     nseg, rows, window, out, out_len, fsize, hop, mode, norm);
  return dvae_check_launch();
}
