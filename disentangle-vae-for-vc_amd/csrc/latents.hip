// Latent report (python -m dvae_amd.latents): the pairwise log-densities log q(z_id | x_j) of a corpus of
// posteriors and their log-sum-exps over j, per dimension, per block (style, content) and jointly.  Part of probe.hip's
// translation unit (included at its end).
//
//   t_ijd = a_jd - h_jd (z_id - mu_jd)^2        dz = z - mu, q = dz * dz, t = fma(-h, q, a): three roundings
//   style_ij = sum_{d < S} t_ijd, content_ij = sum_{S <= d < D} t_ijd   (d ascending from +0, one rounding per term)
//   joint_ij = style_ij + content_ij
//   L = m + ln s over a job's columns, (m, s) the running maximum and the sum of exp(. - m)
//
// A wave owns 64 rows, one per lane: z [D] and the D + 3 running (m, s) pairs stay in registers.  The four waves of a
// workgroup share the rows and take the four quarters [w q, (w + 1) q), q = ceil(ncols / 4), of the job's columns, each
// staging tiles of its own columns' (mu, a, h) in LDS and reading them as broadcasts; the quarters are merged through LDS
// in wave order, ((w0 + w1) + w2) + w3.  The partition and every order are functions of (ncols, D) alone, a row is
// computed by its lane from the tables only, and there are no atomics: a row's bits depend neither on the other rows of
// the job nor on the other jobs of the launch, and two launches give the same bits.
//
// The maximum comes off before every exponential: a column updates (m, s) by e = exp(min(m, t) - max(m, t)) and
// s = t > m ? s e + 1 : s + e.  From (m, s) = (-inf, 0) the first column gives e = exp(-inf) = 0 and s = 0 * 0 + 1 = 1:
// there is no inf - inf, and a row far from every column ends with a finite m and 1 <= s <= ncols.

namespace {

constexpr int LAT_WG = 256;
constexpr int LAT_TILE_FLOATS = 1024;      // per wave and table: TJ = 1024 / DP columns of DP dimensions
constexpr float LAT_HALF_LN_2PI = 0.91893853320467274178f;

__global__ __launch_bounds__(256) void latent_tables_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                            const float* __restrict__ eps, float* __restrict__ z,
                                                            float* __restrict__ a, float* __restrict__ h, int64_t N, int D,
                                                            int64_t ld) {
#pragma clang fp contract(off)
  const int64_t total = N * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / D, o = r * ld + (i - r * D);
    const float l = lv[o];
    z[o] = __builtin_fmaf(expf(0.5f * l), eps[o], mu[o]);      // 0.5 l is exact
    a[o] = -(LAT_HALF_LN_2PI + 0.5f * l);                      // one rounding (and the constant's)
    h[o] = 0.5f * expf(-l);                                    // the halving is exact
  }
}

__device__ __forceinline__ void lat_update(float& m, float& s, float t) {
  const float hi = fmaxf(m, t), lo = fminf(m, t);
  const float e = __expf(lo - hi);
  s = t > m ? __builtin_fmaf(s, e, 1.f) : s + e;
  m = hi;
}

// (m, s) <- (m, s) merged with (m2, s2); one of the two exponentials is exp(0) = 1
__device__ __forceinline__ void lat_merge(float& m, float& s, float m2, float s2) {
  const float hi = fmaxf(m, m2);
  const float p = s * __expf(m - hi);
  s = __builtin_fmaf(s2, __expf(m2 - hi), p);
  m = hi;
}

// DP: D rounded up to 4, 8, 16, 32 or 64.  The dimensions D .. DP - 1 of a group of four that holds a real one carry
// z = mu = a = h = 0 (t = 0: nothing is added to a block sum, their LSEs are never stored); whole groups behind D are
// skipped.
template <int DP>
__global__ __launch_bounds__(LAT_WG) void latent_lse_kernel(const float* __restrict__ z, const float* __restrict__ mu,
                                                            const float* __restrict__ a, const float* __restrict__ h,
                                                            int64_t ld, int D, int S, const int64_t* __restrict__ jobs,
                                                            int njobs, float* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
  constexpr int TJ = LAT_TILE_FLOATS / DP, G = DP / 4, NL = DP + 3;
  __shared__ __attribute__((aligned(16))) float lds[4 * 3 * LAT_TILE_FLOATS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // (job, row tile) of this workgroup: a prefix over the job table (uniform)
  int64_t b = blockIdx.x;
  int k = 0;
  for (; k < njobs; ++k) {
    const int64_t tiles = (jobs[5 * k + 1] + 63) / 64;
    if (b < tiles) break;
    b -= tiles;
  }
  if (k >= njobs) return;      // the grid is the sum of the tiles: not reached
  const int64_t row0 = jobs[5 * k], nrows = jobs[5 * k + 1], col0 = jobs[5 * k + 2], ncols = jobs[5 * k + 3],
                out0 = jobs[5 * k + 4];
  const int64_t r = b * 64 + lane;
  const bool live = r < nrows;
  const int64_t q = (ncols + 3) / 4;
  const int64_t c_begin = col0 + w * q;
  const int64_t mine = ncols - w * q < q ? (ncols - w * q > 0 ? ncols - w * q : 0) : q;      // columns of this wave
  const int64_t ntiles = (q + TJ - 1) / TJ;                                                   // the same for the four waves

  float zr[DP], m[NL], s[NL];
  const float* zrow = z + (row0 + (live ? r : 0)) * ld;
#pragma unroll
  for (int d = 0; d < DP; ++d) zr[d] = d < D ? zrow[d] : 0.f;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    m[i] = -INFINITY;
    s[i] = 0.f;
  }
  float* tmu = lds + w * 3 * LAT_TILE_FLOATS;
  float* ta = tmu + LAT_TILE_FLOATS;
  float* th = ta + LAT_TILE_FLOATS;
  for (int64_t ti = 0; ti < ntiles; ++ti) {
    const int64_t t0 = ti * TJ;
    const int cnt = (int)(mine - t0 < TJ ? (mine - t0 > 0 ? mine - t0 : 0) : TJ);
    for (int e = lane; e < TJ * DP; e += 64) {
      const int j = e / DP, d = e - j * DP;
      const bool in = j < cnt && d < D;
      const int64_t g = (c_begin + t0 + j) * ld + d;
      tmu[e] = in ? mu[g] : 0.f;
      ta[e] = in ? a[g] : 0.f;
      th[e] = in ? h[g] : 0.f;
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const f32x4* pm = reinterpret_cast<const f32x4*>(tmu + j * DP);
      const f32x4* pa = reinterpret_cast<const f32x4*>(ta + j * DP);
      const f32x4* ph = reinterpret_cast<const f32x4*>(th + j * DP);
      float st = 0.f, ct = 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (4 * g < D) {      // uniform
          const f32x4 vm = pm[g], va = pa[g], vh = ph[g];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int d = 4 * g + i;
            const float dz = zr[d] - vm[i];
            const float qq = dz * dz;
            const float t = __builtin_fmaf(-vh[i], qq, va[i]);
            st = __builtin_fmaf(d < S ? 1.f : 0.f, t, st);
            ct = __builtin_fmaf(d < S ? 0.f : 1.f, t, ct);      // t = 0 at d >= D
            lat_update(m[d], s[d], t);
          }
        }
      }
      lat_update(m[DP], s[DP], st);
      lat_update(m[DP + 1], s[DP + 1], ct);
      lat_update(m[DP + 2], s[DP + 2], st + ct);
    }
    __syncthreads();
  }
  // the quarters in wave order through LDS: [2 NL][64] floats, NL * 128 <= 8576 of the 12288
  float* xm = lds;
  float* xs = lds + NL * 64;
#pragma unroll 1
  for (int step = 0; step < 4; ++step) {
    if (w == step) {
      if (step > 0 && mine > 0) {
#pragma unroll
        for (int i = 0; i < NL; ++i) lat_merge(m[i], s[i], xm[i * 64 + lane], xs[i * 64 + lane]);
      } else if (step > 0) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          m[i] = xm[i * 64 + lane];
          s[i] = xs[i * 64 + lane];
        }
      }
      if (step < 3) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          xm[i * 64 + lane] = m[i];
          xs[i * 64 + lane] = s[i];
        }
      }
    }
    if (step < 3) __syncthreads();
  }
  if (w != 3 || !live) return;
  float* o = out + (out0 + r) * ldo;
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) o[d] = m[d] + logf(s[d]);
#pragma unroll
  for (int i = 0; i < 3; ++i) o[D + i] = m[DP + i] + logf(s[DP + i]);
}

}  // namespace

DVAE_API int dvae_latent_tables(const float* mu, const float* lv, const float* eps, float* z, float* a, float* h, int64_t N,
                                int D, int64_t ld, void* stream) {
  if (!mu || !lv || !eps || !z || !a || !h || N < 0 || D < 1 || D > DVAE_LATENT_MAX_D || ld < D) return DVAE_EINVAL;
  if (N == 0) return DVAE_OK;
  const int64_t blocks = (N * D + 255) / 256;
  hipLaunchKernelGGL(latent_tables_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0,
                     (hipStream_t)stream, mu, lv, eps, z, a, h, N, D, ld);
  return dvae_check_launch();
}

DVAE_API int dvae_latent_lse(const float* z, const float* mu, const float* a, const float* h, int64_t ld, int D, int S,
                             const int64_t* jobs, const int64_t* jobs_host, int njobs, float* out, int64_t ldo,
                             void* stream) {
  if (!z || !mu || !a || !h || !jobs || !jobs_host || !out || njobs < 1) return DVAE_EINVAL;
  if (D < 1 || D > DVAE_LATENT_MAX_D || S < 0 || S > D || ld < D || ldo < D + 3 || (((uintptr_t)jobs) & 7)) return DVAE_EINVAL;
  int64_t tiles = 0;
  for (int k = 0; k < njobs; ++k) {
    const int64_t* j = jobs_host + 5 * k;
    if (j[0] < 0 || j[1] < 0 || j[2] < 0 || j[3] < 1 || j[4] < 0) return DVAE_EINVAL;
    tiles += (j[1] + 63) / 64;
    if (tiles > INT_MAX) return DVAE_EINVAL;
  }
  if (tiles == 0) return DVAE_OK;      // nrows = 0 everywhere: nothing to do
  const dim3 grid((unsigned)tiles), block(LAT_WG);
  hipStream_t s = (hipStream_t)stream;
#define DVAE_LAT_LAUNCH(DP) \
  hipLaunchKernelGGL(latent_lse_kernel<DP>, grid, block, 0, s, z, mu, a, h, ld, D, S, jobs, njobs, out, ldo)
  if (D <= 4) DVAE_LAT_LAUNCH(4);
  else if (D <= 8) DVAE_LAT_LAUNCH(8);
  else if (D <= 16) DVAE_LAT_LAUNCH(16);
  else if (D <= 32) DVAE_LAT_LAUNCH(32);
  else DVAE_LAT_LAUNCH(64);
#undef DVAE_LAT_LAUNCH
  return dvae_check_launch();
}
