// Mel front-end (reference preprocessing/utils.py:68-141): the HBM-bound pieces around the two
// contractions (windowed frames x DFT basis, magnitudes x mel basis), which run on the contraction kernel of gemm.hip.
#include "common.h"

namespace {

// reim[row][0..nbp) = Re, [nbp..2nbp) = Im  ->  mag[row][j] = sqrt(Re^2 + Im^2)
__global__ void stft_magnitude_kernel(const float* __restrict__ reim, float* __restrict__ mag, int64_t rows, int nbp) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nbp) return;
  const int64_t r = idx / nbp;
  const int j = (int)(idx - r * nbp);
  const float re = reim[r * 2 * nbp + j], im = reim[r * 2 * nbp + nbp + j];
  mag[idx] = sqrtf(re * re + im * im);
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


// ---- corpus preprocessing (preprocessing/encoder/audio.py:22-51 `preprocess_wav`): band-limited resampling (resampy
// kaiser_best), increase-only volume normalisation, and the framing / dB passes of the mel path on a PACKED batch
// (one launch per pass for the whole batch; an element's bits depend only on its own utterance).

// segment row {in0, n_in, out0, n_out, n_valid, filter} (int64 x 6), filter row {P, Q, taps, base, woff, -} (int64 x 6),
// tile row {segment, t0} (int64 x 2).  Output t < n_valid of a segment: m = floor(t Q / P), phase = t Q - m P,
// y[t] = sum_{c < taps} w[woff + phase*taps + c] * x[m - base + c] (x zero outside [0, n_in)); t >= n_valid: 0.
constexpr int RS_TILE = 256;                                 // DVAE_RESAMPLE_TILE
__global__ void __launch_bounds__(RS_TILE) resample_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const int64_t* __restrict__ segs,
                                                          const int64_t* __restrict__ filts,
                                                          const float* __restrict__ w,
                                                          const int64_t* __restrict__ tiles, int lds_cap) {
  extern __shared__ float xs[];
  const int tid = threadIdx.x;
  const int64_t sg = tiles[2 * blockIdx.x], t0 = tiles[2 * blockIdx.x + 1];
  const int64_t* s = segs + 6 * sg;
  const int64_t in0 = s[0], n_in = s[1], out0 = s[2], n_out = s[3], n_valid = s[4];
  const int64_t* f = filts + 6 * s[5];
  const int64_t P = f[0], Q = f[1], base = f[3], woff = f[4];
  const int taps = (int)f[2];
  const int64_t t_end = min(t0 + RS_TILE, n_valid);          // outputs [t0, t_end) run the filter
  if (t0 < t_end) {
    const int64_t lo = (t0 * Q) / P - base;                  // first input sample of the tile's span
    const int64_t hi = ((t_end - 1) * Q) / P - base + taps;  // one past the last
    const int64_t g0 = in0 + lo;                             // packed index of xs[shift]
    const int64_t a0 = g0 & ~(int64_t)3;                    // floor to a 16-byte boundary (g0 may be < 0)
    const int shift = (int)(g0 - a0);
    const int nld = min((int)(hi - lo) + shift, lds_cap);
    const int64_t s_lo = in0, s_hi = in0 + n_in;             // valid packed range of this segment
    for (int q = tid * 4; q < nld; q += RS_TILE * 4) {
      const int64_t g = a0 + q;
      f32x4 v;
      if (g >= s_lo && g + 3 < s_hi) {
        v = *reinterpret_cast<const f32x4*>(x + g);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (g + e >= s_lo && g + e < s_hi) ? x[g + e] : 0.f;
      }
      if (q + 3 < lds_cap) {
        *reinterpret_cast<f32x4*>(xs + q) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (q + e < lds_cap) xs[q + e] = v[e];
      }
    }
    __syncthreads();
    const int64_t t = t0 + tid;
    if (t < t_end) {
      const int64_t m = (t * Q) / P, ph = t * Q - m * P;
      const int j0 = (int)(m - base - lo) + shift;
      const float* __restrict__ wr = w + woff + ph * taps;
      float acc = 0.f;
      if (j0 >= 0 && j0 + taps <= lds_cap) {
        for (int c = 0; c < taps; ++c) acc = fmaf(wr[c], xs[j0 + c], acc);
      } else {
        acc = __builtin_nanf("");                            // the host's LDS bound was wrong: never silently
      }
      y[out0 + t] = acc;
    }
  }
  const int64_t t = t0 + tid;
  if (t >= n_valid && t < min(t0 + RS_TILE, n_out)) y[out0 + t] = 0.f;   // librosa fix=True pad
}

// volume: per tile of NV_TILE samples sum of squares in float64 (each thread its 8 samples in order, then a fixed tree)
constexpr int NV_THREADS = 256, NV_PER = 8, NV_TILE = NV_THREADS * NV_PER;
static_assert(NV_TILE == 2048 && RS_TILE == 256, "DVAE_VOLUME_TILE / DVAE_RESAMPLE_TILE of include/dvae_hip.h");
__global__ void __launch_bounds__(NV_THREADS) sumsq_tiles_kernel(const float* __restrict__ y,
                                                                const int64_t* __restrict__ segs,
                                                                const int64_t* __restrict__ tiles,
                                                                double* __restrict__ part) {
  __shared__ double red[NV_THREADS];
  const int tid = threadIdx.x;
  const int64_t sg = tiles[2 * blockIdx.x], t0 = tiles[2 * blockIdx.x + 1];
  const int64_t out0 = segs[6 * sg + 2], n_out = segs[6 * sg + 3];
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < NV_PER; ++e) {
    const int64_t t = t0 + (int64_t)tid * NV_PER + e;
    if (t < n_out) {
      const double v = (double)y[out0 + t];
      acc += v * v;
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int h = NV_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = red[0];
}

// one thread per segment: mean square from its tiles' partials (tile_first[s] .. tile_first[s+1]) in order, then the gain
// of normalize_volume (audio.py:121-127): change = target - 10 log10(ms); increase_only and change < 0 -> 1
__global__ void volume_finalize_kernel(const int64_t* __restrict__ segs, int nseg, const int64_t* __restrict__ tile_first,
                                       const double* __restrict__ part, double target_dbfs, int increase_only,
                                       double* __restrict__ ms_out, float* __restrict__ gain, int* __restrict__ silent) {
  const int sg = blockIdx.x * blockDim.x + threadIdx.x;
  if (sg >= nseg) return;
  double sum = 0.0;
  for (int64_t i = tile_first[sg]; i < tile_first[sg + 1]; ++i) sum += part[i];
  const int64_t n = segs[6 * sg + 3];
  const double ms = n > 0 ? sum / (double)n : 0.0;
  float g = 1.f;
  int sil = 0;
  if (!(ms > 0.0)) {
    sil = 1;                                     // the reference: 0 * 10^(inf) = NaN mel; here flagged, left as is
  } else {
    const double change = target_dbfs - 10.0 * log10(ms);
    if (!(increase_only && change < 0.0)) g = (float)pow(10.0, change / 20.0);
  }
  if (ms_out) ms_out[sg] = ms;
  gain[sg] = g;
  silent[sg] = sil;
}

__global__ void __launch_bounds__(NV_THREADS) volume_scale_kernel(float* __restrict__ y, const int64_t* __restrict__ segs,
                                                                 const int64_t* __restrict__ tiles,
                                                                 const float* __restrict__ gain) {
  const int64_t sg = tiles[2 * blockIdx.x], t0 = tiles[2 * blockIdx.x + 1];
  const float g = gain[sg];
  if (g == 1.f) return;
  const int64_t out0 = segs[6 * sg + 2], n_out = segs[6 * sg + 3];
#pragma unroll
  for (int e = 0; e < NV_PER; ++e) {
    const int64_t t = t0 + (int64_t)e * NV_THREADS + threadIdx.x;
    if (t < n_out) y[out0 + t] = y[out0 + t] * g;
  }
}

// frames[r][k] = win[k] * x[(r - row0)*hop + k - left], zero outside the signal x = wav[sample0, sample0 + n) (lws pads
// fsize-hop samples on both sides and the tail up to a whole frame; utils.py:82-103).  Row r belongs to segment
// {row0, M, sample0, n} of `segs` (the dvae_gl_segment_table layout); segs == nullptr: one utterance, {0, rows, 0,
// n_one}.  One thread writes 4 consecutive k (16-byte stores).
__global__ void stft_frames_kernel(const float* __restrict__ wav, const int64_t* __restrict__ segs, int nseg, int64_t n_one,
                                   int64_t rows, const float* __restrict__ win, float* __restrict__ frames, int fsize,
                                   int hop, int left) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = fsize >> 2;
  if (idx >= rows * per_row) return;
  const int64_t r = idx / per_row;
  const int k = ((int)(idx - r * per_row)) << 2;
  int64_t row0 = 0, sample0 = 0, n = n_one;
  if (segs) {
    const int sg = find_segment(segs, nseg, r, 0);
    row0 = segs[4 * sg];
    sample0 = segs[4 * sg + 2];
    n = segs[4 * sg + 3];
  }
  const int64_t s = (r - row0) * hop + k - left;
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = s + e;
    v[e] = (i >= 0 && i < n) ? wav[sample0 + i] * win[k + e] : 0.f;
  }
  *reinterpret_cast<f32x4*>(frames + r * fsize + k) = v;
}

// clip((20*log10(max(min_level, mel[m][c])) - ref_db - min_db) / -min_db, 0, 1) (utils.py:127-137), transposed through a
// 32 x 33 LDS tile: mel[rows, C] -> the utterances' [C, M] blocks back to back (segment {row0, M, ..} at C * row0);
// segs == nullptr: one utterance, out[c * ld_one + m] (the host adds col0 to `out`)
__global__ void mel_db_normalize_kernel(const float* __restrict__ mel, float* __restrict__ out,
                                        const int64_t* __restrict__ segs, int nseg, int64_t ld_one, int64_t rows, int C,
                                        float min_level, float ref_db, float min_db) {
  __shared__ float tile[32][33];
  const int64_t m0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 256 threads: 8 rows per pass
  for (int r = ty; r < 32; r += 8) {
    const int64_t m = m0 + r;
    const int c = c0 + tx;
    tile[r][tx] = (m < rows && c < C) ? mel[m * C + c] : 1.f;
  }
  __syncthreads();
  const int64_t m = m0 + tx;
  if (m >= rows) return;
  int64_t row0 = 0, ld = ld_one;
  if (segs) {
    const int sg = find_segment(segs, nseg, m, 0);
    row0 = segs[4 * sg];
    ld = segs[4 * sg + 1];
  }
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    if (c < C) {
      const float db = 20.f * log10f(fmaxf(min_level, tile[tx][r])) - ref_db;
      out[C * row0 + (int64_t)c * ld + (m - row0)] = fminf(fmaxf((db - min_db) / -min_db, 0.f), 1.f);
    }
  }
}


// ---- mel-cepstral distortion (evaluate.py; preprocessing/MCD_calculate.py:54-103): the passes around the three
// contractions of the feature pass (frames x DFT basis, logP x sp2mc matrix, P x lag basis) and the batched exact DTW.
// No atomics, one writer per output element, fixed orders: a pair's bits do not depend on the batch or the run.

// reim[row][0..nbp) = Re, [nbp..2nbp) = Im  ->  P = Re^2 + Im^2, logP = ln(max(P, floor)); bins j >= nb are 0 in both.
// One thread per 4 consecutive bins (16-byte loads and stores; nbp is a multiple of 4).
__global__ void log_power_kernel(const float* __restrict__ reim, float* __restrict__ pw, float* __restrict__ lp,
                                 int64_t rows, int nb, int nbp, float floor_) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = nbp >> 2;
  if (idx >= rows * per_row) return;
  const int64_t r = idx / per_row;
  const int j = ((int)(idx - r * per_row)) << 2;
  const f32x4 re = *reinterpret_cast<const f32x4*>(reim + r * 2 * nbp + j);
  const f32x4 im = *reinterpret_cast<const f32x4*>(reim + r * 2 * nbp + nbp + j);
  f32x4 p, l;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = j + e < nb;
    p[e] = in ? fmaf(re[e], re[e], im[e] * im[e]) : 0.f;
    l[e] = in ? logf(fmaxf(p[e], floor_)) : 0.f;
  }
  *reinterpret_cast<f32x4*>(pw + r * nbp + j) = p;
  *reinterpret_cast<f32x4*>(lp + r * nbp + j) = l;
}

// One workgroup per utterance {row0, M, ..}.  r[row][0] = r(0), r[row][1..nlag] = r(lag) (the lag-basis contraction),
// gain[1..nlag] = r_w(0) / r_w(lag).  peak = max_lag(r * gain) / r(0) (0 where r(0) = 0); voiced = r(0) > 0 and
// r(0) >= rel_min * max r(0) over the utterance and peak >= peak_min.  Then the voiced frames' first MCD_DIM coefficients of
// mc[row][0..ldm) go to feats[row0 + k][MCD_DIM] in time order (k = the frame's rank among the voiced ones, from a fixed
// 256-frame-chunk ballot scan), and count[utterance] = the number of voiced frames.
constexpr int VC_THREADS = 256, VC_WAVES = VC_THREADS / 64, MCD_DIM = 24;
__global__ void __launch_bounds__(VC_THREADS) voicing_compact_kernel(const float* __restrict__ r, int ldr, int nlag,
                                                                    const float* __restrict__ gain,
                                                                    const float* __restrict__ mc, int ldm,
                                                                    const int64_t* __restrict__ segs, float peak_min,
                                                                    float rel_min, float* __restrict__ peak,
                                                                    int* __restrict__ voiced, float* __restrict__ feats,
                                                                    int* __restrict__ count) {
  __shared__ float red[VC_WAVES];
  __shared__ float pk[VC_THREADS];
  __shared__ int wsum[VC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t row0 = segs[4 * blockIdx.x], M = segs[4 * blockIdx.x + 1];
  float m0 = 0.f;                                   // r(0) is a sum of non-negative terms
  for (int64_t f = tid; f < M; f += VC_THREADS) m0 = fmaxf(m0, r[(row0 + f) * ldr]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m0 = fmaxf(m0, __shfl_xor(m0, o));
  if (lane == 0) red[wid] = m0;
  __syncthreads();
  float mx = red[0];
#pragma unroll
  for (int w = 1; w < VC_WAVES; ++w) mx = fmaxf(mx, red[w]);
  const float thr = rel_min * mx;
  int base = 0;
  for (int64_t c0 = 0; c0 < M; c0 += VC_THREADS) {
    for (int q = 0; q < 64; ++q) {                  // wave wid: frames c0 + 64 wid + q, its lanes over the lags
      const int64_t f = c0 + 64 * wid + q;
      if (f >= M) break;
      const float* rr = r + (row0 + f) * ldr;
      float m = 0.f;
      for (int t = 1 + lane; t <= nlag; t += 64) m = fmaxf(m, rr[t] * gain[t]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      if (lane == 0) pk[64 * wid + q] = m;
    }
    __syncthreads();
    const int64_t f = c0 + tid;
    int v = 0;
    if (f < M) {
      const float r0 = r[(row0 + f) * ldr];
      const float p = r0 > 0.f ? pk[tid] / r0 : 0.f;
      v = (r0 > 0.f && r0 >= thr && p >= peak_min) ? 1 : 0;
      peak[row0 + f] = p;
      voiced[row0 + f] = v;
    }
    const unsigned long long mask = __ballot(v);
    const int rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wid] = __popcll(mask);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int w = 0; w < VC_WAVES; ++w) {
      off += w < wid ? wsum[w] : 0;
      tot += wsum[w];
    }
    if (v) {
      const float* src = mc + (row0 + f) * ldm;
      float* dst = feats + (row0 + off + rank) * MCD_DIM;
#pragma unroll
      for (int c = 0; c < MCD_DIM; c += 4)
        *reinterpret_cast<f32x4*>(dst + c) = *reinterpret_cast<const f32x4*>(src + c);
    }
    base += tot;
    __syncthreads();                                // pk / wsum are rewritten by the next chunk
  }
  if (tid == 0) count[blockIdx.x] = base;
}

// Exact DTW of one pair per workgroup, pair row {x_row0, nx, y_row0, ny} (int64) into the packed [., MCD_DIM] buffers.
// D(i,j) = d(i,j) + min(D(i-1,j), D(i,j-1), D(i-1,j-1)) with d the float64 euclidean distance of the fp32 rows; a tie goes
// to the first of the three in that order; the path length L rides along with D (L(0,0) = 1), so no traceback.
// Anti-diagonal sweep along the shorter sequence A (index a; the longer is B, index b = diagonal - a): thread t owns
// a = t + DTW_THREADS * s for slots s < ceil(na / DTW_THREADS).  Cell (a, b) reads (a-1, b) from the previous diagonal in
// LDS (double-buffered, one barrier per diagonal), (a, b-1) from its own register and (a-1, b-1) from the register that
// kept last diagonal's LDS read.  Feature rows come through L1 / L2 in 16-byte loads.
constexpr int DTW_THREADS = 256, DTW_SLOTS = 16, DTW_MAX_SHORT = DTW_THREADS * DTW_SLOTS;
static_assert(DTW_MAX_SHORT == 4096 && MCD_DIM == 24, "DVAE_DTW_MAX_SHORT / DVAE_MCD_DIM of include/dvae_hip.h");

__device__ __forceinline__ double dist_row(const float* __restrict__ p, const float* __restrict__ q) {
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < MCD_DIM; c += 4) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(p + c), v = *reinterpret_cast<const f32x4*>(q + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double t = (double)u[e] - (double)v[e];
      acc = fma(t, t, acc);
    }
  }
  return sqrt(acc);
}

//
// F0 (dvae_dtw_batch_f0): one more quantity rides along the same path the way the length does, the sum over the path's
// cells of (lfx[i] - lfy[j])^2 with lfx / lfy the per-row log-F0 (indexed like x / y).  The difference and its square are
// float64, the running sum is fp32 (ps: 32 KiB more LDS, 128 of the 160 KiB; a float64 payload would sit exactly at the
// limit), so it never enters a comparison: cost and length are the F0 = false kernel's bits.
template <bool F0>
__global__ void __launch_bounds__(DTW_THREADS) dtw_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const int64_t* __restrict__ pairs, double* __restrict__ cost,
                                                          int64_t* __restrict__ length, const float* __restrict__ lfx,
                                                          const float* __restrict__ lfy, double* __restrict__ sse) {
  __shared__ double cs[2][DTW_MAX_SHORT];
  __shared__ int ls[2][DTW_MAX_SHORT];
  __shared__ float ps[2][F0 ? DTW_MAX_SHORT : 1];
  const int tid = threadIdx.x;
  const int64_t* pr = pairs + 4 * blockIdx.x;
  const int64_t nx = pr[1], ny = pr[3];
  if (nx < 1 || ny < 1) {                           // a side without voiced frames: no score
    if (tid == 0) {
      cost[blockIdx.x] = __builtin_nan("");
      length[blockIdx.x] = 0;
      if constexpr (F0) sse[blockIdx.x] = __builtin_nan("");
    }
    return;
  }
  const bool swap = nx > ny;                        // A = the shorter side; a = i unless swapped (then a = j)
  const float* __restrict__ A = swap ? y + pr[2] * MCD_DIM : x + pr[0] * MCD_DIM;
  const float* __restrict__ B = swap ? x + pr[0] * MCD_DIM : y + pr[2] * MCD_DIM;
  const int na = (int)(swap ? ny : nx);
  const int64_t nb = swap ? nx : ny;
  const float* __restrict__ LA = F0 ? (swap ? lfy + pr[2] : lfx + pr[0]) : nullptr;
  const float* __restrict__ LB = F0 ? (swap ? lfx + pr[0] : lfy + pr[2]) : nullptr;
  const int S = (na + DTW_THREADS - 1) / DTW_THREADS;
  const double inf = __builtin_inf();
  double cl[DTW_SLOTS], cu[DTW_SLOTS];              // own cell of the previous diagonal; last diagonal's (a-1) read
  int ll[DTW_SLOTS], lu[DTW_SLOTS];
  float pl[F0 ? DTW_SLOTS : 1], pu[F0 ? DTW_SLOTS : 1];   // the payload of the same two cells
#pragma unroll
  for (int s = 0; s < DTW_SLOTS; ++s) {
    cl[s] = cu[s] = inf;
    ll[s] = lu[s] = 0;
    if constexpr (F0) pl[s] = pu[s] = 0.f;
  }
  const int64_t ndiag = (int64_t)na + nb - 1;
  for (int64_t dg = 0; dg < ndiag; ++dg) {
    const int cur = (int)(dg & 1);
#pragma unroll
    for (int s = 0; s < DTW_SLOTS; ++s) {
      const int a = tid + DTW_THREADS * s;
      const int64_t b = dg - a;
      if (s < S && a < na && b >= 0 && b < nb) {
        const double d = dist_row(A + (int64_t)a * MCD_DIM, B + b * MCD_DIM);
        double c = d;
        int l = 1;
        float e = 0.f, pp = 0.f;
        if constexpr (F0) {
          const double t = (double)LA[a] - (double)LB[b];
          e = (float)(t * t);
          pp = e;
        }
        if (a > 0 || b > 0) {
          double cup = inf, clf = b > 0 ? cl[s] : inf, cdg = (a > 0 && b > 0) ? cu[s] : inf;
          int lup = 0;
          float pup = 0.f;
          if (a > 0) {
            cup = cs[cur ^ 1][a - 1];
            lup = ls[cur ^ 1][a - 1];
            if constexpr (F0) pup = ps[cur ^ 1][a - 1];
          }
          // order (i-1, j), (i, j-1), (i-1, j-1): (a-1, b), (a, b-1) when a = i; (a, b-1), (a-1, b) when a = j
          double bc = swap ? clf : cup;
          int bl = swap ? ll[s] : lup;
          const double c2 = swap ? cup : clf;
          const int l2 = swap ? lup : ll[s];
          float bp = 0.f;
          if constexpr (F0) bp = swap ? pl[s] : pup;
          if (c2 < bc) {
            bc = c2;
            bl = l2;
            if constexpr (F0) bp = swap ? pup : pl[s];
          }
          if (cdg < bc) {
            bc = cdg;
            bl = lu[s];
            if constexpr (F0) bp = pu[s];
          }
          c = d + bc;
          l = bl + 1;
          cu[s] = cup;
          lu[s] = lup;
          if constexpr (F0) {
            pp = bp + e;
            pu[s] = pup;
          }
        }
        cs[cur][a] = c;
        ls[cur][a] = l;
        cl[s] = c;
        ll[s] = l;
        if constexpr (F0) {
          ps[cur][a] = pp;
          pl[s] = pp;
        }
      }
    }
    __syncthreads();
  }
  const int last = na - 1;                          // cell (na-1, nb-1): its owner's register
  if (tid == last % DTW_THREADS) {
#pragma unroll
    for (int s = 0; s < DTW_SLOTS; ++s) {
      if (s == last / DTW_THREADS) {
        cost[blockIdx.x] = cl[s];
        length[blockIdx.x] = ll[s];
        if constexpr (F0) sse[blockIdx.x] = (double)pl[s];
      }
    }
  }
}

// ---- F0 contour (evaluate.py; replaces pyworld.harvest of preprocessing/WORLD_processing.py:29-38): a
// Viterbi pass over the F0_STATES lags of the voicing autocorrelation, every maximal run of voiced frames on its own.
// One workgroup per utterance {row0, M, ..}; thread j < F0_STATES owns state j (lag lag_min + j).
//   s_k(j) = (double)r[k][1+j] * (double)gain[1+j] / (double)r[k][0] - oct[j]
//   D_k(j) = s_k(j) + max_i (D_{k-1}(i) - jump * |l2[j] - l2[i]|), the first maximal i on a tie; D = s at a run's first frame
// in float64 with contraction off (every operation rounds once, in the order written, as a numpy restatement does).  The
// previous frame's D (double-buffered) and l2 sit in LDS and are read as broadcasts: one barrier per frame.  The
// back-pointers, one byte per state, go to back[rows][F0_LD]; at a run's last frame the first arg-max of D starts the
// traceback, which reads them back F0_CHUNK frames at a time into LDS (coalesced), walks the chunk there (thread 0) and
// lets one thread per frame write lag, f0 (parabolic refinement of r * gain around the lag) and, at the frame's rank among
// the utterance's voiced frames (the row of feats that dvae_voicing_compact gave it), lf0v = ln f0.  No atomics, one
// writer per element, and a launch reads only its own utterance.
constexpr int F0_THREADS = 256, F0_STATES = 206, F0_LD = 208, F0_CHUNK = 256;
static_assert(F0_LD <= F0_THREADS && F0_STATES <= 256 && (F0_LD & 7) == 0 && F0_LD >= F0_STATES, "one byte per state");

__global__ void __launch_bounds__(F0_THREADS) f0_viterbi_kernel(const float* __restrict__ r, int ldr,
                                                                const float* __restrict__ gain,
                                                                const int* __restrict__ voiced,
                                                                const int64_t* __restrict__ segs,
                                                                const double* __restrict__ l2g,
                                                                const double* __restrict__ octg, double jump, double rate,
                                                                int lag_min, unsigned char* back, int* __restrict__ lag,
                                                                float* __restrict__ f0, float* __restrict__ lf0v) {
#pragma clang fp contract(off)
  __shared__ double Ds[2][F0_LD];
  __shared__ double l2s[F0_LD];
  __shared__ unsigned int bps[F0_CHUNK * F0_LD / 4];
  __shared__ int path[F0_CHUNK];
  const int tid = threadIdx.x;
  const bool own = tid < F0_STATES;
  const int j = own ? tid : F0_STATES - 1;          // the idle threads shadow the last state and write nothing
  const int64_t row0 = segs[4 * blockIdx.x], M = segs[4 * blockIdx.x + 1];
  const double l2j = l2g[j], octj = octg[j], gj = (double)gain[1 + j];
  if (tid < F0_LD) {
    l2s[tid] = own ? l2j : 0.0;
    if (!own) Ds[0][tid] = Ds[1][tid] = -__builtin_inf();
  }
  __syncthreads();
  const unsigned char* bpb = reinterpret_cast<const unsigned char*>(bps);
  int cur = 0, state = 0;
  int64_t run0 = -1, vbase = 0;                     // first frame of the open run; voiced frames before it
  int v_n = 0;
  float r_n = 0.f, r0_n = 1.f;
  if (M > 0) {
    v_n = voiced[row0];
    r_n = r[row0 * ldr + 1 + j];
    r0_n = r[row0 * ldr];
  }
  for (int64_t k = 0; k < M; ++k) {
    const int v = __builtin_amdgcn_readfirstlane(v_n);
    const float rk = r_n, r0k = r0_n;
    if (k + 1 < M) {                                // the next frame's loads fly under this frame's recurrence
      v_n = voiced[row0 + k + 1];
      r_n = r[(row0 + k + 1) * ldr + 1 + j];
      r0_n = r[(row0 + k + 1) * ldr];
    }
    if (v) {
      const double s = (double)rk * gj / (double)r0k - octj;
      double d = s;
      if (run0 < 0) {
        run0 = k;
      } else {
        const double* Dp = Ds[cur ^ 1];
        double best = -__builtin_inf();             // the pad states F0_STATES .. F0_LD-1 hold D = -inf and never win
        int bi = 0;
#pragma unroll 8
        for (int i = 0; i < F0_LD; ++i) {
          const double c = Dp[i] - jump * fabs(l2j - l2s[i]);
          const bool g = c > best;
          best = g ? c : best;
          bi = g ? i : bi;
        }
        d = s + best;
        if (own) back[(row0 + k) * F0_LD + j] = (unsigned char)bi;
      }
      if (own) Ds[cur][j] = d;
      cur ^= 1;
      __syncthreads();
    } else if (tid == 0) {
      lag[row0 + k] = 0;
      f0[row0 + k] = 0.f;
    }
    if (run0 >= 0 && (!v || k + 1 == M)) {          // the run run0 .. e is complete; its last D is Ds[cur ^ 1]
      const int64_t e = v ? k : k - 1;
      if (tid == 0) {
        const double* Df = Ds[cur ^ 1];
        double bm = Df[0];
        state = 0;
        for (int i = 1; i < F0_STATES; ++i) {
          if (Df[i] > bm) {
            bm = Df[i];
            state = i;
          }
        }
      }
      for (int64_t c1 = e; c1 >= run0; c1 -= F0_CHUNK) {
        const int64_t c0 = c1 - (F0_CHUNK - 1) > run0 ? c1 - (F0_CHUNK - 1) : run0;
        const int nf = (int)(c1 - c0 + 1);
        const unsigned int* src = reinterpret_cast<const unsigned int*>(back + (row0 + c0) * F0_LD);
        for (int w = tid; w < nf * (F0_LD / 4); w += F0_THREADS) bps[w] = src[w];
        __syncthreads();
        if (tid == 0) {
          for (int f = nf - 1; f >= 0; --f) {
            path[f] = state;
            if (c0 + f > run0) {                    // the run's first frame has no predecessor (its row of back is unwritten)
              const int p = bpb[f * F0_LD + state];
              state = p < F0_STATES ? p : F0_STATES - 1;
            }
          }
        }
        __syncthreads();
        if (tid < nf) {
          const int64_t fr = c0 + tid;
          const int st = path[tid];
          const float* rr = r + (row0 + fr) * ldr;
          double delta = 0.0;
          if (st > 0 && st < F0_STATES - 1) {
            const double qm = (double)rr[st] * (double)gain[st], q0 = (double)rr[1 + st] * (double)gain[1 + st],
                         qp = (double)rr[2 + st] * (double)gain[2 + st];
            const double den = qm - 2.0 * q0 + qp;
            if (den < 0.0) {
              delta = 0.5 * (qm - qp) / den;
              delta = delta > 0.5 ? 0.5 : (delta < -0.5 ? -0.5 : delta);
            }
          }
          const float fz = (float)(rate / ((double)(lag_min + st) + delta));
          lag[row0 + fr] = lag_min + st;
          f0[row0 + fr] = fz;
          lf0v[row0 + vbase + (fr - run0)] = (float)log((double)fz);
        }
        __syncthreads();                            // bps / path are rewritten by the next chunk
      }
      vbase += e - run0 + 1;
      run0 = -1;
    }
  }
}

}  // namespace

DVAE_API int dvae_stft_frames(const float* wav, int64_t n, const float* window, float* frames, int M, int fsize,
                              int hop, int left, void* stream) {
  if (!wav || !window || !frames || n < 1 || M < 1 || fsize < 4 || (fsize & 3) || hop < 1 || left < 0) return DVAE_EINVAL;
  const int64_t work = (int64_t)M * (fsize >> 2);
  hipLaunchKernelGGL(stft_frames_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     wav, (const int64_t*)nullptr, 0, n, (int64_t)M, window, frames, fsize, hop, left);
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
  if (!mel || !out || M < 1 || n_mels < 1 || col0 < 0 || ld_out < col0 + M || !(min_level > 0.f) || !(min_level_db < 0.f))
    return DVAE_EINVAL;
  dim3 grid((M + 31) / 32, (n_mels + 31) / 32);
  hipLaunchKernelGGL(mel_db_normalize_kernel, grid, dim3(256), 0, (hipStream_t)stream, mel, out + col0,
                     (const int64_t*)nullptr, 0, ld_out, (int64_t)M, n_mels, min_level, ref_level_db, min_level_db);
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


// ---- corpus preprocessing
DVAE_API int dvae_resample_segment_table(const int64_t* n_in, const int* filt, int nseg, const int64_t* filters, int nfilt,
                                         int tile, int64_t* table, int64_t* tiles, int64_t max_tiles) {
  if (!n_in || !filt || !filters || !table || nseg < 1 || nfilt < 1 || tile < 1) return DVAE_EINVAL;
  int64_t in0 = 0, out0 = 0, nt = 0;
  for (int s = 0; s < nseg; ++s) {
    const int f = filt[s];
    if (f < 0 || f >= nfilt || n_in[s] < 1) return DVAE_EINVAL;
    const int64_t P = filters[6 * f], Q = filters[6 * f + 1];
    if (P < 1 || Q < 1 || n_in[s] > ((int64_t)1 << 40) / (P > Q ? P : Q)) return DVAE_EINVAL;
    const int64_t n_valid = n_in[s] * P / Q;              // resampy: int(n * ratio)
    const int64_t n_out = (n_in[s] * P + Q - 1) / Q;      // librosa fix=True: ceil(n * ratio)
    if (n_valid < 1) return DVAE_EINVAL;                  // resampy raises
    int64_t* r = table + 6 * s;
    r[0] = in0;
    r[1] = n_in[s];
    r[2] = out0;
    r[3] = n_out;
    r[4] = n_valid;
    r[5] = f;
    for (int64_t t0 = 0; t0 < n_out; t0 += tile, ++nt) {
      if (tiles) {
        if (nt >= max_tiles) return DVAE_EINVAL;
        tiles[2 * nt] = s;
        tiles[2 * nt + 1] = t0;
      }
    }
    in0 += (n_in[s] + 3) & ~(int64_t)3;                   // every segment starts 16-byte aligned
    out0 += (n_out + 3) & ~(int64_t)3;
  }
  return (int)(nt > 0x7fffffff ? DVAE_EINVAL : nt);
}

DVAE_API int dvae_resample_lds_floats(int64_t P, int64_t Q, int taps) {
  if (P < 1 || Q < 1 || taps < 1) return DVAE_EINVAL;
  const int64_t span = ((int64_t)(RS_TILE - 1) * Q + P - 1) / P + 1 + taps + 4;
  const int64_t cap = (span + 3) & ~(int64_t)3;
  return cap * 4 > 64 * 1024 ? DVAE_EINVAL : (int)cap;
}

DVAE_API int dvae_resample_batch(const float* x, float* y, const int64_t* segs, const int64_t* filters, const float* weights,
                                 const int64_t* tiles, int ntiles, int lds_floats, void* stream) {
  if (!x || !y || !segs || !filters || !weights || !tiles || ntiles < 1 || lds_floats < 4 || (lds_floats & 3) ||
      lds_floats * 4 > 64 * 1024 || ((((uintptr_t)x) | ((uintptr_t)y)) & 15))
    return DVAE_EINVAL;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)ntiles), dim3(RS_TILE), (size_t)lds_floats * 4, (hipStream_t)stream,
                     x, y, segs, filters, weights, tiles, lds_floats);
  return dvae_check_launch();
}

DVAE_API int dvae_volume_normalize(float* y, const int64_t* segs, int nseg, const int64_t* tiles, int ntiles,
                                   const int64_t* tile_first, double* part, double target_dbfs, int increase_only,
                                   double* ms_out, float* gain, int* silent, void* stream) {
  if (!y || !segs || !tiles || !tile_first || !part || !gain || !silent || nseg < 1 || ntiles < 1 ||
      !(target_dbfs < 1e3 && target_dbfs > -1e3))
    return DVAE_EINVAL;
  int rc;
  {
    ProfScope prof(DVAE_PROF_AUDIO, (hipStream_t)stream, 0.0, 0);
    hipLaunchKernelGGL(sumsq_tiles_kernel, dim3((unsigned)ntiles), dim3(NV_THREADS), 0, (hipStream_t)stream, y, segs, tiles,
                       part);
    rc = dvae_check_launch();
  }
  if (rc) return rc;
  {
    ProfScope prof(DVAE_PROF_AUDIO, (hipStream_t)stream, 0.0, 1);
    hipLaunchKernelGGL(volume_finalize_kernel, dim3((unsigned)((nseg + 127) / 128)), dim3(128), 0, (hipStream_t)stream,
                       segs, nseg, tile_first, part, target_dbfs, increase_only, ms_out, gain, silent);
    rc = dvae_check_launch();
  }
  if (rc) return rc;
  ProfScope prof(DVAE_PROF_AUDIO, (hipStream_t)stream, 0.0, 2);
  hipLaunchKernelGGL(volume_scale_kernel, dim3((unsigned)ntiles), dim3(NV_THREADS), 0, (hipStream_t)stream, y, segs, tiles,
                     gain);
  return dvae_check_launch();
}

DVAE_API int dvae_stft_frames_seg(const float* wav, const int64_t* segs, int nseg, int64_t rows, const float* window,
                                  float* frames, int fsize, int hop, int left, void* stream) {
  if (!wav || !segs || !window || !frames || nseg < 1 || rows < 1 || fsize < 4 || (fsize & 3) || hop < 1 || left < 0 ||
      (((uintptr_t)frames) & 15))
    return DVAE_EINVAL;
  const int64_t work = rows * (fsize >> 2);
  hipLaunchKernelGGL(stft_frames_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     wav, segs, nseg, (int64_t)0, rows, window, frames, fsize, hop, left);
  return dvae_check_launch();
}

DVAE_API int dvae_mel_db_normalize_seg(const float* mel, float* out, const int64_t* segs, int nseg, int64_t rows,
                                       int n_mels, float min_level, float ref_level_db, float min_level_db, void* stream) {
  if (!mel || !out || !segs || nseg < 1 || rows < 1 || rows > ((int64_t)1 << 36) || n_mels < 1 || !(min_level > 0.f) ||
      !(min_level_db < 0.f))
    return DVAE_EINVAL;
  dim3 grid((unsigned)((rows + 31) / 32), (n_mels + 31) / 32);
  hipLaunchKernelGGL(mel_db_normalize_kernel, grid, dim3(256), 0, (hipStream_t)stream, mel, out, segs, nseg,
                     (int64_t)0, rows, n_mels, min_level, ref_level_db, min_level_db);
  return dvae_check_launch();
}


// ---- mel-cepstral distortion
DVAE_API int dvae_log_power(const float* reim, float* power, float* log_power, int64_t rows, int nb, int nbp, float floor_,
                            void* stream) {
  if (!reim || !power || !log_power || rows < 1 || nb < 1 || nbp < nb || (nbp & 3) || !(floor_ > 0.f) ||
      ((((uintptr_t)reim) | ((uintptr_t)power) | ((uintptr_t)log_power)) & 15))
    return DVAE_EINVAL;
  const int64_t work = rows * (nbp >> 2);
  hipLaunchKernelGGL(log_power_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reim,
                     power, log_power, rows, nb, nbp, floor_);
  return dvae_check_launch();
}

DVAE_API int dvae_voicing_compact(const float* r, int ldr, int nlag, const float* gain, const float* mc, int ldm,
                                  const int64_t* segs, int nseg, float peak_min, float rel_power_min, float* peak,
                                  int* voiced, float* feats, int* count, void* stream) {
  if (!r || !gain || !mc || !segs || !peak || !voiced || !feats || !count || nseg < 1 || nlag < 1 || ldr < nlag + 1 ||
      ldm < MCD_DIM || (ldm & 3) || !(peak_min >= 0.f) || !(rel_power_min >= 0.f) ||
      ((((uintptr_t)mc) | ((uintptr_t)feats)) & 15))
    return DVAE_EINVAL;
  hipLaunchKernelGGL(voicing_compact_kernel, dim3((unsigned)nseg), dim3(VC_THREADS), 0, (hipStream_t)stream, r, ldr, nlag,
                     gain, mc, ldm, segs, peak_min, rel_power_min, peak, voiced, feats, count);
  return dvae_check_launch();
}

// everything the DTW kernel relies on, from the host copy of the pair table, before any launch
static bool dtw_refuses(const int64_t* pairs_host, int npairs) {
  for (int p = 0; p < npairs; ++p) {
    const int64_t* q = pairs_host + 4 * p;
    if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || q[1] > ((int64_t)1 << 30) || q[3] > ((int64_t)1 << 30))
      return true;
    if (q[1] > 0 && q[3] > 0 && (q[1] < q[3] ? q[1] : q[3]) > DTW_MAX_SHORT) return true;
  }
  return false;
}

DVAE_API int dvae_dtw_batch(const float* x, const float* y, const int64_t* pairs, const int64_t* pairs_host, int npairs,
                            double* cost, int64_t* length, void* stream) {
  if (!x || !y || !pairs || !pairs_host || !cost || !length || npairs < 1 || ((((uintptr_t)x) | ((uintptr_t)y)) & 15))
    return DVAE_EINVAL;
  if (dtw_refuses(pairs_host, npairs)) return DVAE_EINVAL;
  hipLaunchKernelGGL(dtw_kernel<false>, dim3((unsigned)npairs), dim3(DTW_THREADS), 0, (hipStream_t)stream, x, y, pairs,
                     cost, length, (const float*)nullptr, (const float*)nullptr, (double*)nullptr);
  return dvae_check_launch();
}

DVAE_API int dvae_dtw_batch_f0(const float* x, const float* y, const float* lf0x, const float* lf0y, const int64_t* pairs,
                               const int64_t* pairs_host, int npairs, double* cost, int64_t* length, double* sse,
                               void* stream) {
  if (!x || !y || !lf0x || !lf0y || !pairs || !pairs_host || !cost || !length || !sse || npairs < 1 ||
      ((((uintptr_t)x) | ((uintptr_t)y)) & 15))
    return DVAE_EINVAL;
  if (dtw_refuses(pairs_host, npairs)) return DVAE_EINVAL;
  hipLaunchKernelGGL(dtw_kernel<true>, dim3((unsigned)npairs), dim3(DTW_THREADS), 0, (hipStream_t)stream, x, y, pairs,
                     cost, length, lf0x, lf0y, sse);
  return dvae_check_launch();
}

DVAE_API int dvae_f0_viterbi(const float* r, int ldr, int nlag, const float* gain, const int* voiced, const int64_t* segs,
                             int nseg, const double* l2, const double* oct, double jump_cost, double sample_rate,
                             int lag_min, unsigned char* back, int* lag, float* f0, float* lf0v, void* stream) {
  if (!r || !gain || !voiced || !segs || !l2 || !oct || !back || !lag || !f0 || !lf0v || nseg < 1 || nlag != F0_STATES ||
      ldr < nlag + 1 || lag_min < 1 || !(jump_cost >= 0.0) || !(sample_rate > 0.0) || (((uintptr_t)back) & 3))
    return DVAE_EINVAL;
  hipLaunchKernelGGL(f0_viterbi_kernel, dim3((unsigned)nseg), dim3(F0_THREADS), 0, (hipStream_t)stream, r, ldr, gain,
                     voiced, segs, l2, oct, jump_cost, sample_rate, lag_min, back, lag, f0, lf0v);
  return dvae_check_launch();
}

// ---- silence trimming: the kernels behind dvae_vad_trim, part of this translation unit
#include "vad.hip"
