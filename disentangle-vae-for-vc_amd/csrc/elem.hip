// The HBM-bound and tiny kernels of the step: reparameterise + latent assembly, KL and L1 reductions
// (wavefront shuffle reductions, fp64 only for the final cross-workgroup sums), flat Adam, layout changes.
#include <type_traits>
#include "common.h"

int g_dvae_last_hip_error = 0;

DVAE_API int dvae_version(void) { return DVAE_ABI_VERSION; }
DVAE_API int dvae_last_hip_error(void) { return g_dvae_last_hip_error; }

namespace {

// ------------------------------------------------------------------ latent
__global__ void latent_fwd_kernel(const float* __restrict__ style, const float* __restrict__ content,
                                  const float* __restrict__ eps_c, const float* __restrict__ eps_s,
                                  float* __restrict__ z, float* __restrict__ q_mu, float* __restrict__ q_lv,
                                  float* __restrict__ s_mu, float* __restrict__ s_lv, int Bh, int S, int Cn) {
  const int D = S + Cn;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * Bh * D) return;
  const int n = idx / D, dcol = idx - n * D;
  const int b = n % Bh;
  if (dcol < S) {
    const float mu = 0.5f * (style[b * 2 * S + dcol] + style[(Bh + b) * 2 * S + dcol]);
    const float lv = 0.5f * (style[b * 2 * S + S + dcol] + style[(Bh + b) * 2 * S + S + dcol]);
    q_mu[idx] = mu;
    q_lv[idx] = lv;
    z[idx] = eps_s[b * S + dcol] * expf(0.5f * lv) + mu;
    if (n < Bh) {
      s_mu[b * S + dcol] = mu;
      s_lv[b * S + dcol] = lv;
    }
  } else {
    const int k = dcol - S;
    const float mu = content[n * 2 * Cn + k];
    const float lv = content[n * 2 * Cn + Cn + k];
    q_mu[idx] = mu;
    q_lv[idx] = lv;
    z[idx] = eps_c ? eps_c[n * Cn + k] * expf(0.5f * lv) + mu : mu;
  }
}

__global__ void latent_bwd_kernel(const float* __restrict__ style, const float* __restrict__ content,
                                  const float* __restrict__ eps_c, const float* __restrict__ eps_s,
                                  const float* __restrict__ dz, const float* __restrict__ dq_mu,
                                  const float* __restrict__ dq_lv, const float* __restrict__ ds_mu,
                                  const float* __restrict__ ds_lv, float* __restrict__ dstyle,
                                  float* __restrict__ dcontent, int Bh, int S, int Cn) {
  const int D = S + Cn;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * Bh * D) return;
  const int n = idx / D, dcol = idx - n * D;
  const int b = n % Bh;
  auto ld = [](const float* p, int i) { return p ? p[i] : 0.f; };
  if (dcol < S) {
    if (n >= Bh) {  // x2's style head is detached (disentangled_vae.py:257-258)
      dstyle[n * 2 * S + dcol] = 0.f;
      dstyle[n * 2 * S + S + dcol] = 0.f;
      return;
    }
    const int i1 = b * D + dcol, i2 = (Bh + b) * D + dcol;
    const float lv = 0.5f * (style[b * 2 * S + S + dcol] + style[(Bh + b) * 2 * S + S + dcol]);
    const float gz = ld(dz, i1) + ld(dz, i2);
    const float gmu = gz + ld(dq_mu, i1) + ld(dq_mu, i2) + ld(ds_mu, b * S + dcol);
    const float glv = gz * eps_s[b * S + dcol] * 0.5f * expf(0.5f * lv) + ld(dq_lv, i1) + ld(dq_lv, i2) +
                      ld(ds_lv, b * S + dcol);
    dstyle[b * 2 * S + dcol] = 0.5f * gmu;
    dstyle[b * 2 * S + S + dcol] = 0.5f * glv;
  } else {
    const int k = dcol - S;
    const float lv = content[n * 2 * Cn + Cn + k];
    const float gz = ld(dz, idx);
    dcontent[n * 2 * Cn + k] = gz + ld(dq_mu, idx);
    dcontent[n * 2 * Cn + Cn + k] =
        (eps_c ? gz * eps_c[n * Cn + k] * 0.5f * expf(0.5f * lv) : 0.f) + ld(dq_lv, idx);
  }
}

// ------------------------------------------------------------------ KL
__global__ __launch_bounds__(256) void kl_fwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                     float* __restrict__ out, int64_t n, float scale) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const float m = mu[i], l = lv[i];
    acc += (double)(1.f + l - m * m - expf(l));
  }
  acc = wave_sum_d(acc);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((red[0] + red[1] + red[2] + red[3]) * (double)scale);
}

__global__ void kl_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                              const float* __restrict__ gout, float* __restrict__ dmu, float* __restrict__ dlv,
                              int64_t n, float scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float g = gout[0] * scale;
  dmu[i] = g * (-2.f * mu[i]);
  dlv[i] = g * (1.f - expf(lv[i]));
}

// ------------------------------------------------------------------ L1
constexpr int L1_BLOCKS = 512;

__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         double* __restrict__ part, int64_t n) {
  const int64_t n4 = n >> 2;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + 4 * i);
    const f32x4 b = *reinterpret_cast<const f32x4*>(y + 4 * i);
    acc += fabsf(a[0] - b[0]) + fabsf(a[1] - b[1]) + fabsf(a[2] - b[2]) + fabsf(a[3] - b[3]);
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) acc += fabsf(x[i] - y[i]);
  double d = wave_sum_d((double)acc);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(64) void l1_final_kernel(const double* __restrict__ part, float* __restrict__ out,
                                                      int nparts, float scale) {
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 64) a += part[i];
  a = wave_sum_d(a);
  if (threadIdx.x == 0) out[0] = (float)(a * (double)scale);
}

__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                     const float* __restrict__ gout, float* __restrict__ dy,
                                                     int64_t n, float scale) {
  const float g = gout[0] * scale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = x[i] - y[i];
    dy[i] = d > 0.f ? -g : (d < 0.f ? g : 0.f);
  }
}

// ------------------------------------------------------------------ the whole loss_functionGVAE2 in two launches
// (disentangled_vae.py:310-327): four L1 sums / batch_size, two KL terms, the report-only style KL and the weighted
// total.  Round 1 spent 19 launches on it forward (4 x (partial + final), 3 KL, ~8 ATen scalar ops) and ~15 backward.
struct LossArgs {
  const float* x[2];        // x1, x2                      [n]
  const float* r[4];        // recon1, recon2, recon1_hat, recon2_hat   [n]
  const float* qmu[2];      // q_z1_mu, q_z2_mu            [nq]
  const float* qlv[2];
  const float* smu;         // z_style_mu, z_style_logvar  [ns]
  const float* slv;
  int64_t n;
  int nq, ns;
  float l1_scale, kl_scale, style_scale, mse_cof, kl_cof;
};

__global__ __launch_bounds__(256) void loss_partial_kernel(const LossArgs a, double* __restrict__ part) {
  const int64_t n4 = a.n >> 2;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(a.x[0] + 4 * i), x2 = *reinterpret_cast<const f32x4*>(a.x[1] + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(a.r[k] + 4 * i);
      const f32x4 x = (k & 1) ? x2 : x1;
      acc[k] += fabsf(x[0] - r[0]) + fabsf(x[1] - r[1]) + fabsf(x[2] - r[2]) + fabsf(x[3] - r[3]);
    }
  }
  if (blockIdx.x == 0)
    for (int64_t i = (n4 << 2) + threadIdx.x; i < a.n; i += 256)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += fabsf(a.x[k & 1][i] - a.r[k][i]);
  __shared__ double red[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = wave_sum_d((double)acc[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = d;
  }
  __syncthreads();
  if (threadIdx.x < 4)
    part[blockIdx.x * 4 + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// The scheduled form of the two kernels below (dvae_loss_fwd_sched / dvae_loss_bwd_sched): the two weights are read from
// device memory, so a captured step follows a KL warm-up without a new capture, and each latent dimension may spend
// free_bits[j] nats unpenalised.  SCHED = false is dvae_loss_fwd / dvae_loss_bwd: `s` is not looked at.
struct LossSched {
  const float* coef;        // [8]: [0] mse_cof, [1] the KL weight in effect
  const float* free_bits;   // [D] or null
  float* aux;               // [4 + 4 D], see include/dvae_hip.h (read-only in the backward kernel)
  int D;
};
constexpr int LOSS_MAX_D = DVAE_LOSS_MAX_D;

// out[8] = (LOSS, L1_x1, L1_x2, L1_x1hat, L1_x2hat, KL_z1, KL_z2, KL_style)
template <bool SCHED>
__global__ __launch_bounds__(256) void loss_final_kernel(const LossArgs a, const double* __restrict__ part, int nparts,
                                                         float* __restrict__ out, const LossSched s) {
  __shared__ double red[7][4];
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += 256)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += part[i * 4 + k];
  auto kl = [](float m, float l) { return (double)(1.f + l - m * m - expf(l)); };
  for (int i = threadIdx.x; i < a.nq; i += 256) {
    v[4] += kl(a.qmu[0][i], a.qlv[0][i]);
    v[5] += kl(a.qmu[1][i], a.qlv[1][i]);
  }
  for (int i = threadIdx.x; i < a.ns; i += 256) v[6] += kl(a.smu[i], a.slv[i]);
  // per-dimension batch-mean KL of the [rows, D] blocks: a thread owns a column and adds its rows in row order in float64
  // (consecutive threads read consecutive addresses), one rounding at the store; the order depends on the shapes alone
  __shared__ float kd[SCHED ? 2 * LOSS_MAX_D : 1];
  __shared__ float clamped[2];
  if constexpr (SCHED) {
    const int rows = a.nq / s.D;
    for (int j = threadIdx.x; j < s.D; j += 256)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        double c = 0.0;
        for (int i = 0; i < rows; ++i) c += kl(a.qmu[k][i * s.D + j], a.qlv[k][i * s.D + j]);
        const float m = (float)(c * (double)a.kl_scale);
        kd[k * LOSS_MAX_D + j] = m;
        s.aux[4 + k * s.D + j] = m;
        s.aux[4 + (2 + k) * s.D + j] = (!s.free_bits || m > s.free_bits[j]) ? 1.f : 0.f;     // the gate is strict
      }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double d = wave_sum_d(v[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = d;
  }
  __syncthreads();
  if constexpr (SCHED) {
    if (s.free_bits) {      // sum_j max(lambda_j, kl_dim[j]) in float64 in dimension order: one lane per half
      if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {
        const int k = threadIdx.x >> 6;
        double c = 0.0;
        int nfree = 0;
        for (int j = 0; j < s.D; ++j) {
          const float m = kd[k * LOSS_MAX_D + j], lam = s.free_bits[j];
          const bool on = m > lam;
          c += (double)(on ? m : lam);
          nfree += on ? 0 : 1;
        }
        clamped[k] = (float)c;
        s.aux[2 + k] = (float)nfree;
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    float t[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double tot = red[k][0] + red[k][1] + red[k][2] + red[k][3];
      t[k] = (float)(tot * (double)(k < 4 ? a.l1_scale : (k < 6 ? a.kl_scale : a.style_scale)));
      out[1 + k] = t[k];
    }
    // the reference's operation order: mse_cof * (((a + b) + c) + d) + kl_cof * (e + f), all in fp32
    if constexpr (SCHED) {
      // out[1..7] stay the raw terms; what enters LOSS is aux[0..1]: the terms themselves, or the clamped sums
      const float e = s.free_bits ? clamped[0] : t[4], f = s.free_bits ? clamped[1] : t[5];
      s.aux[0] = e;
      s.aux[1] = f;
      if (!s.free_bits) s.aux[2] = s.aux[3] = 0.f;
      // spelled out as the compiler contracts the expression of the other branch (one product, then one fused
      // multiply-add): with both weights in registers it would pair the two products and add, which rounds differently
      out[0] = __builtin_fmaf(s.coef[1], e + f, s.coef[0] * (((t[0] + t[1]) + t[2]) + t[3]));
    } else {
      out[0] = a.mse_cof * (((t[0] + t[1]) + t[2]) + t[3]) + a.kl_cof * (t[4] + t[5]);
    }
  }
}

// gradients w.r.t. the four reconstructions and the six latent statistics, given g[8] = dL/d(out[8])
template <bool SCHED>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const LossArgs a, const float* __restrict__ g, float* __restrict__ dr0,
                                                       float* __restrict__ dr1, float* __restrict__ dr2,
                                                       float* __restrict__ dr3, float* __restrict__ dqmu0,
                                                       float* __restrict__ dqlv0, float* __restrict__ dqmu1,
                                                       float* __restrict__ dqlv1, float* __restrict__ dsmu,
                                                       float* __restrict__ dslv, int l1_blocks, const LossSched s) {
  const float g0 = g[0];
  const float mse_cof = SCHED ? s.coef[0] : a.mse_cof, kl_cof = SCHED ? s.coef[1] : a.kl_cof;
  if ((int)blockIdx.x < l1_blocks) {
    float* dr[4] = {dr0, dr1, dr2, dr3};
    float w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (g0 * mse_cof + g[1 + k]) * a.l1_scale;
    const int64_t n4 = a.n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)l1_blocks * 256) {
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(a.x[0] + 4 * i), x2 = *reinterpret_cast<const f32x4*>(a.x[1] + 4 * i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!dr[k]) continue;
        const f32x4 r = *reinterpret_cast<const f32x4*>(a.r[k] + 4 * i);
        const f32x4 x = (k & 1) ? x2 : x1;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = x[e] - r[e];
          o[e] = d > 0.f ? -w[k] : (d < 0.f ? w[k] : 0.f);
        }
        *reinterpret_cast<f32x4*>(dr[k] + 4 * i) = o;
      }
    }
    if (blockIdx.x == 0)
      for (int64_t i = (n4 << 2) + threadIdx.x; i < a.n; i += 256)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!dr[k]) continue;
          const float d = a.x[k & 1][i] - a.r[k][i];
          dr[k][i] = d > 0.f ? -w[k] : (d < 0.f ? w[k] : 0.f);
        }
    return;
  }
  // latent statistics: one extra workgroup
  const float w1 = (g0 * kl_cof + g[5]) * a.kl_scale, w2 = (g0 * kl_cof + g[6]) * a.kl_scale, ws = g[7] * a.style_scale;
  if (SCHED && s.free_bits) {
    // a free dimension (gate 0) takes nothing from g[0]: what is left of its weight is the direct gradient of out[5 + k];
    // a penalised one has the weight of the ungated kernel, bit for bit
    const float f1 = g[5] * a.kl_scale, f2 = g[6] * a.kl_scale;
    const float* gate = s.aux + 4 + 2 * s.D;
    for (int i = threadIdx.x; i < a.nq; i += 256) {
      const int j = i % s.D;
      const float u1 = gate[j] != 0.f ? w1 : f1, u2 = gate[s.D + j] != 0.f ? w2 : f2;
      if (dqmu0) { dqmu0[i] = u1 * (-2.f * a.qmu[0][i]); dqlv0[i] = u1 * (1.f - expf(a.qlv[0][i])); }
      if (dqmu1) { dqmu1[i] = u2 * (-2.f * a.qmu[1][i]); dqlv1[i] = u2 * (1.f - expf(a.qlv[1][i])); }
    }
  } else {
    for (int i = threadIdx.x; i < a.nq; i += 256) {
      if (dqmu0) { dqmu0[i] = w1 * (-2.f * a.qmu[0][i]); dqlv0[i] = w1 * (1.f - expf(a.qlv[0][i])); }
      if (dqmu1) { dqmu1[i] = w2 * (-2.f * a.qmu[1][i]); dqlv1[i] = w2 * (1.f - expf(a.qlv[1][i])); }
    }
  }
  if (dsmu)
    for (int i = threadIdx.x; i < a.ns; i += 256) {
      dsmu[i] = ws * (-2.f * a.smu[i]);
      dslv[i] = ws * (1.f - expf(a.slv[i]));
    }
}

// ------------------------------------------------------------------ Adam
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                   float b1, float b2, float eps, float gs, float bc1, float bc2s) {
  // torch.optim.Adam (no amsgrad, no weight decay):
  //   m += (g-m)(1-b1) ; v = b2 v + (1-b2) g^2 ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
  const int64_t n4 = n >> 2;
  const float step_size = lr / bc1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 pp = *reinterpret_cast<f32x4*>(p + 4 * i);
    const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i);
    f32x4 mm = *reinterpret_cast<f32x4*>(m + 4 * i);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gg[k] * gs;
      mm[k] = mm[k] + (gr - mm[k]) * (1.f - b1);
      vv[k] = vv[k] * b2 + (1.f - b2) * gr * gr;
      pp[k] -= step_size * (mm[k] / (sqrtf(vv[k]) / bc2s + eps));
    }
    *reinterpret_cast<f32x4*>(p + 4 * i) = pp;
    *reinterpret_cast<f32x4*>(m + 4 * i) = mm;
    *reinterpret_cast<f32x4*>(v + 4 * i) = vv;
  }
  if (blockIdx.x == 0) {
    for (int64_t i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
      const float gr = g[i] * gs;
      const float mk = m[i] + (gr - m[i]) * (1.f - b1);
      const float vk = v[i] * b2 + (1.f - b2) * gr * gr;
      m[i] = mk;
      v[i] = vk;
      p[i] -= step_size * (mk / (sqrtf(vk) / bc2s + eps));
    }
  }
}

// Device-resident step counter, bias corrections, learning rate and gradient scale, so that a captured hipGraph replays a
// correct Adam step: state[0] = t (as float), state[1] = 1 - beta1^t, state[2] = sqrt(1 - beta2^t), state[4] = lr,
// state[5] = grad_scale.  `skip`: while *skip != 0 (sticky error word of the persistent LSTM launches) nothing is touched.
// CLIP (dvae_adam_flat_dev_clip): clip[3] stands in for state[5], and while clip[4] != 0 (this step's gradient is not finite,
// grad_clip_finalize_kernel) the step does not happen: no tick here, no write of p, m, v below
template <bool CLIP>
__global__ void adam_tick_kernel(float* __restrict__ state, float b1, float b2, const unsigned* __restrict__ skip,
                                 const float* __restrict__ clip) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    if (CLIP && clip[4] != 0.f) return;
    const double t = (double)state[0] + 1.0;
    state[0] = (float)t;
    state[1] = (float)(1.0 - pow((double)b1, t));
    state[2] = (float)sqrt(1.0 - pow((double)b2, t));
  }
}
struct AdamClear {
  int64_t lo[8], hi[8];
  int n;
};
template <int U, bool CLIP>
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                       float b1, float b2, float eps, const float* __restrict__ state,
                                                       const unsigned* __restrict__ skip, AdamClear clr,
                                                       const float* __restrict__ clip) {
  if (skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if (CLIP && clip[4] != 0.f) {
    // a gradient that is not finite: p, m, v keep their bits, but the clear ranges are still zeroed — the next backward
    // pass accumulates into them (store-first gradients are overwritten by it anyway)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
      bool c = false;
      for (int r = 0; r < clr.n; ++r) c |= (4 * i >= clr.lo[r]) & (4 * i < clr.hi[r]);
      if (c) *reinterpret_cast<f32x4*>(g + 4 * i) = z;
    }
    return;
  }
  const float bc1 = state[1], bc2s = state[2], lr = state[4], gs = CLIP ? clip[3] : state[5];
  const float step_size = lr / bc1;
  // U independent 16-byte accesses per tensor and thread per trip: 4 U loads in flight before the first use
  for (int64_t i0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x; i0 < n4; i0 += (int64_t)gridDim.x * (256 * U)) {
    f32x4 pp[U], gg[U], mm[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256 < n4 ? i0 + u * 256 : i0;      // clamped: the tail re-reads element i0, stores are guarded
      // streamed once per step: non-temporal accesses keep 2.7 GB of optimiser traffic from evicting the caches
      pp[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p + 4 * i));
      gg[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + 4 * i));
      mm[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m + 4 * i));
      vv[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v + 4 * i));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256;
      if (i >= n4) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gr = gg[u][k] * gs;
        mm[u][k] = mm[u][k] + (gr - mm[u][k]) * (1.f - b1);
        vv[u][k] = vv[u][k] * b2 + (1.f - b2) * gr * gr;
        pp[u][k] -= step_size * (mm[u][k] / (sqrtf(vv[u][k]) / bc2s + eps));
      }
      __builtin_nontemporal_store(pp[u], reinterpret_cast<f32x4*>(p + 4 * i));
      __builtin_nontemporal_store(mm[u], reinterpret_cast<f32x4*>(m + 4 * i));
      __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4*>(v + 4 * i));
      bool c = false;
      for (int r = 0; r < clr.n; ++r) c |= (4 * i >= clr.lo[r]) & (4 * i < clr.hi[r]);
      if (c) *reinterpret_cast<f32x4*>(g + 4 * i) = z;     // plain store: the next step's launches accumulate into it
    }
  }
}

// ------------------------------------------------------------------ gradient norm, clipping, non-finite guard
// torch.nn.utils.clip_grad_norm_ over the whole flat gradient, on the device: sum of squares (one pass over g, float64) ->
// finalize (norm, clip coefficient, the gradient scale Adam then reads, the non-finite flag) -> dvae_adam_flat_dev_clip.
// The square of a finite float32 is exact in a double and n * FLT_MAX^2 ~ 1e85 cannot overflow one, so "the sum is not
// finite" means exactly "some element is not finite": no flag pass.  No floating-point atomics: the grid and the order
// of every addition depend on n alone, so the norm has the same bits run after run.
constexpr int SUMSQ_U = 2;          // 16-byte loads in flight per thread and trip
constexpr int SUMSQ_CAP = 2048;     // workgroups at most = float64 partial sums in the workspace
inline int sumsq_blocks(int64_t n) {
  const int64_t n4 = n >> 2;
  int64_t b = (n4 + 256 * SUMSQ_U - 1) / (256 * SUMSQ_U);
  if (b < 1) b = 1;
  return (int)(b > SUMSQ_CAP ? SUMSQ_CAP : b);
}

template <int U>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, double* __restrict__ part,
                                                         int64_t n4) {
  double acc = 0.0;
  for (int64_t i0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x; i0 < n4; i0 += (int64_t)gridDim.x * (256 * U)) {
    f32x4 gg[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256 < n4 ? i0 + u * 256 : i0;      // clamped like adam_dev_kernel's: the tail is not added
      gg[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + 4 * i));      // streamed once
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * 256 >= n4) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)gg[u][k] * (double)gg[u][k];      // the product is exact
    }
  }
  acc = wave_sum_d(acc);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  clip: float[8]
//   [0] max_norm (host-written; +inf: measure and guard, never clip)   [1] norm   [2] coef   [3] eff = grad_scale * coef
//   [4] 1 while this step is to be skipped (gradient not finite and `guard`)   [5] skipped steps   [6] clipped steps
//   [7] 1 when this step's gradient is not finite, guarded or not
// float64 throughout, rounded once on each store.
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ part, int nparts,
                                                                 const float* __restrict__ state,
                                                                 float* __restrict__ clip,
                                                                 const unsigned* __restrict__ skip, int guard) {
  if (skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  // thread t adds the partials t, t + 256, ... in index order, then the waves' butterflies, then the four waves in order
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
  a = wave_sum_d(a);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sum = (red[0] + red[1]) + (red[2] + red[3]);
  const double gs = (double)state[5], max_norm = (double)clip[0];
  const bool bad = !(sum <= 1.7976931348623157e308);      // +inf or NaN
  const double norm = gs * sqrt(sum);                     // of the gradient Adam consumes (the average over ranks)
  const double ratio = max_norm / (norm + 1e-6);          // clip_grad_norm_, its 1e-6 included
  const double coef = ratio < 1.0 ? ratio : 1.0;          // a NaN ratio does not clip
  const bool skipped = bad && guard;
  clip[1] = (float)norm;                                  // above FLT_MAX: +inf, while eff below comes from the double
  clip[2] = (float)coef;
  clip[3] = (float)(gs * coef);                           // coef == 1: grad_scale, bit for bit
  clip[4] = skipped ? 1.f : 0.f;
  clip[7] = bad ? 1.f : 0.f;
  if (skipped) clip[5] += 1.f;
  else if (coef < 1.0) clip[6] += 1.f;
}

// ------------------------------------------------------------------ exponential moving average of the weights
// e <- e + w (p - e) after the Adam launch(es) of a full step, inside the same (captured) step: a tick that decides whether
// this step counts and what it weighs, then one sweep over the two flat buffers.  es: float[8]
//   [0] decay (host-written)   [1] k: updates applied so far   [2] w = 1 - d_k of the last update
//   [3] warm-up on/off (host-written)   [4] 1 while this step's update is applied, 0 while it is skipped   [5..7] never written
// A step is skipped on the conditions adam_tick_kernel<CLIP> skips on: the error word of the persistent LSTM launches, or
// clip[4] (the gradient was not finite) — the weights did not move, so the average must not move towards them either.
__global__ void ema_tick_kernel(float* __restrict__ es, const unsigned* __restrict__ skip, const float* __restrict__ clip) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if ((skip && __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) || (clip && clip[4] != 0.f)) {
      es[4] = 0.f;
      return;
    }
    const double k = (double)es[1] + 1.0;
    double d = (double)es[0];
    if (es[3] != 0.f) {
      const double ramp = (1.0 + k) / (10.0 + k);       // the first updates follow the weights, not the initial values
      d = ramp < d ? ramp : d;
    }
    es[1] = (float)k;
    es[2] = (float)(1.0 - d);                           // rounded once
    es[4] = 1.f;
  }
}

// Shaped like adam_dev_kernel: U independent 16-byte accesses per tensor and thread per trip, clamped tail, streamed once.
// 8 bytes read, 4 written per parameter; every element depends on its own index alone.
template <int U>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ e, const float* __restrict__ p, int64_t n4,
                                                         const float* __restrict__ es) {
  if (es[4] == 0.f) return;
  const float w = es[2];
  for (int64_t i0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x; i0 < n4; i0 += (int64_t)gridDim.x * (256 * U)) {
    f32x4 ee[U], pp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256 < n4 ? i0 + u * 256 : i0;
      ee[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(e + 4 * i));
      pp[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 4 * i));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256;
      if (i >= n4) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) ee[u][k] = fmaf(w, pp[u][k] - ee[u][k], ee[u][k]);
      __builtin_nontemporal_store(ee[u], reinterpret_cast<f32x4*>(e + 4 * i));
    }
  }
}

// a <-> b, exactly (bits are moved, never computed with)
template <int U>
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n4) {
  for (int64_t i0 = (int64_t)blockIdx.x * (256 * U) + threadIdx.x; i0 < n4; i0 += (int64_t)gridDim.x * (256 * U)) {
    f32x4 aa[U], bb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256 < n4 ? i0 + u * 256 : i0;
      aa[u] = *reinterpret_cast<const f32x4*>(a + 4 * i);
      bb[u] = *reinterpret_cast<const f32x4*>(b + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * 256;
      if (i >= n4) break;
      *reinterpret_cast<f32x4*>(a + 4 * i) = bb[u];
      *reinterpret_cast<f32x4*>(b + 4 * i) = aa[u];
    }
  }
}

// ------------------------------------------------------------------ layout
// X[t][g*Bh+b][c] = x_g[b][c][t] ; tile-transpose through LDS over (c,t) per segment
template <bool OB16>
__global__ __launch_bounds__(256) void mel_to_frames_kernel(const float* __restrict__ x1,
                                                            const float* __restrict__ x2, void* __restrict__ Xv,
                                                            int Bh, int C, int T, int N) {
  using out_t = typename std::conditional<OB16, __bf16, float>::type;
  out_t* __restrict__ X = reinterpret_cast<out_t*>(Xv);
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const float* __restrict__ src = (n < Bh ? x1 + (int64_t)n * C * T : x2 + (int64_t)(n - Bh) * C * T);
  const int c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, t = t0 + tx;
    tile[k][tx] = (c < C && t < T) ? src[(int64_t)c * T + t] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int t = t0 + k, c = c0 + tx;
    if (t < T && c < C) X[((int64_t)t * N + n) * C + c] = (out_t)tile[tx][k];
  }
}

// out[n][c][t] = X[t][n][c]
__global__ __launch_bounds__(256) void frames_to_mel_kernel(const float* __restrict__ X, float* __restrict__ out,
                                                            int N, int C, int T) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int c0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int t = t0 + k, c = c0 + tx;
    tile[k][tx] = (t < T && c < C) ? X[((int64_t)t * N + n) * C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, t = t0 + tx;
    if (c < C && t < T) out[((int64_t)n * C + c) * T + t] = tile[tx][k];
  }
}

__global__ __launch_bounds__(256) void permute_102_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                          int A, int B, int C4) {
  // in[a][b][c] -> out[b][a][c], float4 along c
  const int64_t total = (int64_t)A * B * C4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C4);
    const int64_t ab = i / C4;
    const int a = (int)(ab % A);
    const int b = (int)(ab / A);
    reinterpret_cast<f32x4*>(out)[i] = reinterpret_cast<const f32x4*>(in)[((int64_t)a * B + b) * C4 + c];
  }
}

// out[c] += sum_r X[r][c]: 64 column-quads x 4 row lanes per workgroup, 16-byte loads (1 KiB per wave per row)
template <bool XB16>
__global__ __launch_bounds__(256) void colsum_kernel(const void* __restrict__ Xv, float* __restrict__ o1,
                                                     float* __restrict__ o2, int R, int C, int64_t ld, int rows_pb) {
  using elem_t = typename std::conditional<XB16, __bf16, float>::type;
  const elem_t* __restrict__ X = reinterpret_cast<const elem_t*>(Xv);
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + cl) * 4;
  const int r0 = blockIdx.y * rows_pb, r1 = min(R, r0 + rows_pb);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (c + 3 < C) {
    // eight independent 16-byte loads in flight per thread (one dependent load per iteration left the kernel at
    // ~2 TB/s: too little memory-level parallelism for HBM latency)
    const elem_t* __restrict__ px = X + (int64_t)(r0 + rl) * ld + c;
    const int n = (r1 - r0 - rl + 3) >> 2;          // rows of this thread
    int i = 0;
    for (; i + 8 <= n; i += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ld4<XB16>(px + (int64_t)(i + u) * 4 * ld, 0);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; i < n; ++i) s += ld4<XB16>(px + (int64_t)i * 4 * ld, 0);
  } else if (c < C) {
    for (int r = r0 + rl; r < r1; r += 4)
      for (int k = 0; k < 4 && c + k < C; ++k) s[k] += (float)X[(int64_t)r * ld + c + k];
  }
  __shared__ f32x4 red[4][64];
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c + k >= C) break;
      const float tot = red[0][cl][k] + red[1][cl][k] + red[2][cl][k] + red[3][cl][k];
      atomicAdd(o1 + c + k, tot);
      if (o2) atomicAdd(o2 + c + k, tot);
    }
  }
}

__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R,
                                                        int C) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    tile[k][tx] = (r < R && c < C) ? in[(int64_t)r * C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, r = r0 + tx;
    if (c < C && r < R) out[(int64_t)c * R + r] = tile[tx][k];
  }
}

// dU = dZ * act'(Z)   (Linear + ReLU backward, disentangled_vae.py:211)
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* dz, const float* __restrict__ z, float* du,
                                                      int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    du[i] = dz[i] * act_grad_from_out(z[i], act);
}

__global__ __launch_bounds__(256) void act_fwd_kernel(float* y, int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = act_apply(y[i], act);
}

// W[co][ci][5] -> Wp[tap][co][ci]
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ W, float* __restrict__ Wp,
                                                        int64_t cc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cc; i += (int64_t)gridDim.x * 256) {
#pragma unroll
    for (int tap = 0; tap < 5; ++tap) Wp[tap * cc + i] = W[i * 5 + tap];
  }
}
// W[co][ci][5] -> Wpt[tap][ci][co]: the transposed pack the data-gradient contraction reads k-contiguously
// (32x32 tiles of the (co, ci) plane through LDS: coalesced on both sides up to the stride-5 gather)
__global__ __launch_bounds__(256) void conv_pack_t_kernel(const float* __restrict__ W, float* __restrict__ Wpt, int Cout,
                                                          int Cin) {
  __shared__ float tile[5][32][33];
  const int co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int co = co0 + r, ci = ci0 + tx;
    if (co < Cout && ci < Cin) {
      const float* src = W + ((int64_t)co * Cin + ci) * 5;
#pragma unroll
      for (int tap = 0; tap < 5; ++tap) tile[tap][r][tx] = src[tap];
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Cin && co < Cout) {
#pragma unroll
      for (int tap = 0; tap < 5; ++tap) Wpt[((int64_t)tap * Cin + ci) * Cout + co] = tile[tap][tx][r];
    }
  }
}
__global__ __launch_bounds__(256) void conv_unpack_add_kernel(const float* __restrict__ dWp, float* __restrict__ dW,
                                                              int64_t cc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cc; i += (int64_t)gridDim.x * 256) {
#pragma unroll
    for (int tap = 0; tap < 5; ++tap) dW[i * 5 + tap] += dWp[tap * cc + i];
  }
}

// ---- inference-side layout helpers (mel -> mel conversion, variational_base_vae.py:269-298, 335-348)
__global__ __launch_bounds__(256) void mel_to_chunks_kernel(const float* __restrict__ mel, float* __restrict__ out,
                                                            int C, int L, int T, int n) {
  const int64_t total = (int64_t)n * C * T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i % T);
    const int c = (int)((i / T) % C);
    const int k = (int)(i / ((int64_t)T * C));
    const int64_t src = (int64_t)k * T + t;
    out[i] = src < L ? mel[(int64_t)c * L + src] : 0.f;
  }
}
__global__ __launch_bounds__(256) void chunks_to_mel_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int n, int C, int T, float lo, float hi, int clamp) {
  const int64_t W = (int64_t)n * T, total = (int64_t)C * W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i / W);
    const int64_t col = i % W;
    float v = in[((col / T) * C + c) * T + col % T];
    if (clamp) v = fminf(fmaxf(v, lo), hi);
    out[i] = v;
  }
}
// z_src[k] = [mean_rows(src_style_mu) | src_content_mu[k]] ; z_conv[k] = [mean_rows(trg_style_mu) | src_content_mu[k]]
__global__ void conversion_latents_kernel(const float* __restrict__ ss, const float* __restrict__ sc,
                                          const float* __restrict__ ts, float* __restrict__ zs, float* __restrict__ zc,
                                          int n, int m, int S, int Cn) {
  const int D = S + Cn;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * D) return;
  const int k = idx / D, d = idx % D;
  if (d < S) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < n; ++r) a += ss[r * 2 * S + d];
    for (int r = 0; r < m; ++r) b += ts[r * 2 * S + d];
    zs[idx] = a / (float)n;
    zc[idx] = b / (float)m;
  } else {
    const float v = sc[k * 2 * Cn + (d - S)];
    zs[idx] = v;
    zc[idx] = v;
  }
}
// ---- whole-utterance conversion: overlapped windows of a packed batch of utterances
// utt[u] = {col0, L, win0, nwin}, win[w] = {utt, frame0} (utt < 0: a padding window); mels [C, ld], utterance u in columns
// [col0, col0 + L).  out[w][c][j] = mels[c][col0 + frame0 + j] while frame0 + j < L, else 0: bits moved, never computed with.
__global__ __launch_bounds__(256) void mel_to_windows_kernel(const float* __restrict__ mels, int64_t ld,
                                                             const int* __restrict__ utt, const int* __restrict__ win,
                                                             float* __restrict__ out, int nwin, int C, int T) {
  const int64_t total = (int64_t)nwin * C * T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % T);
    const int c = (int)((i / T) % C);
    const int w = (int)(i / ((int64_t)T * C));
    const int u = win[2 * w];
    float v = 0.f;
    if (u >= 0) {
      const int f = win[2 * w + 1] + j;
      if (f < utt[4 * u + 1]) v = mels[(int64_t)c * ld + utt[4 * u] + f];
    }
    out[i] = v;
  }
}
// z[w] = [fp32((1 - mix) mean_src + mix mean_trg) | content_mu[w]] with mean_g = sums[g][:S] / counts[g] in float64 (the sums
// and counts of dvae_group_sum_f64 over the style heads, K columns a row); a padding window (a group < 0) is a row of zeros.
__global__ __launch_bounds__(256) void window_latents_kernel(const float* __restrict__ content,
                                                             const double* __restrict__ sums,
                                                             const int64_t* __restrict__ counts,
                                                             const int* __restrict__ g_src, const int* __restrict__ g_trg,
                                                             double mix, float* __restrict__ z, int nwin, int S, int Cn,
                                                             int K) {
  const int D = S + Cn;
  const int64_t total = (int64_t)nwin * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int w = (int)(i / D), d = (int)(i % D);
    const int gs = g_src[w], gt = g_trg[w];
    float v = 0.f;
    if (gs >= 0 && gt >= 0) {
      if (d < S) {
        const double a = sums[(int64_t)gs * K + d] / (double)counts[gs];
        const double b = sums[(int64_t)gt * K + d] / (double)counts[gt];
        v = (float)((1.0 - mix) * a + mix * b);
      } else {
        v = content[(int64_t)w * 2 * Cn + (d - S)];
      }
    }
    z[i] = v;
  }
}
// The gather form of the cross-fade: one thread per element (c, q) of out [C, ld].  Column q belongs to the utterance u with
// col0 <= q < col0 + L (col0 increases with u: a bisection), t = q - col0; the windows of u are contiguous and their frame0
// increases, so those that cover t are a run that starts at the first one with frame0 > t - T (a second bisection).  One
// window in the run: its value's bits.  More: num = sum w[t - frame0] y, den = sum w[t - frame0] in float64 in window order,
// out = fp32(num / den).  A column that no utterance owns is not written.
__global__ __launch_bounds__(256) void windows_overlap_add_kernel(const float* __restrict__ y, const int* __restrict__ utt,
                                                                  const int* __restrict__ win, const float* __restrict__ wt,
                                                                  float* __restrict__ out, int64_t ld, int nutt, int C,
                                                                  int T, float lo, float hi, int clamp) {
  const int64_t total = (int64_t)C * ld;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i / ld);
    const int64_t q = i % ld;
    int a = 0, b = nutt;                       // the last utterance with col0 <= q
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (utt[4 * m] <= q) a = m; else b = m;
    }
    const int col0 = utt[4 * a], L = utt[4 * a + 1], win0 = utt[4 * a + 2], nw = utt[4 * a + 3];
    if (q < col0 || q >= (int64_t)col0 + L || nw < 1) continue;
    const int t = (int)(q - col0);
    int p = 0, e = nw;                         // the first window with frame0 > t - T
    while (p < e) {
      const int m = (p + e) >> 1;
      if (win[2 * (win0 + m) + 1] > t - T) e = m; else p = m + 1;
    }
    if (p >= nw || win[2 * (win0 + p) + 1] > t) continue;      // a frame no window covers: a broken plan, left unwritten
    const float* yc = y + (int64_t)c * T;
    const int64_t wstride = (int64_t)C * T;
    float v;
    if (p + 1 >= nw || win[2 * (win0 + p + 1) + 1] > t) {
      v = yc[(win0 + p) * wstride + (t - win[2 * (win0 + p) + 1])];
    } else {
      double num = 0.0, den = 0.0;
      for (int k = p; k < nw; ++k) {
        const int j = t - win[2 * (win0 + k) + 1];
        if (j < 0) break;
        const double wj = (double)wt[j];
        num += wj * (double)yc[(win0 + k) * wstride + j];
        den += wj;
      }
      v = (float)(num / den);
    }
    if (clamp) v = fminf(fmaxf(v, lo), hi);
    out[i] = v;
  }
}
__global__ __launch_bounds__(256) void mul_div_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ c, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = a[i] * (b[i] / c[i]);
}

// out[i][c][t] = mels[utt[i]][c][off[i] + t] if off[i] + t < len[utt[i]] else 0   (random crop / right zero pad of
// preprocessing/dataset.py:100-109 for a whole batch, from a device-resident padded store [n_utt, C, Lmax])
__global__ __launch_bounds__(256) void gather_crop_kernel(const float* __restrict__ mels, const int* __restrict__ lens,
                                                          const int* __restrict__ utt, const int* __restrict__ off,
                                                          float* __restrict__ out, int n, int C, int T, int Lmax) {
  const int64_t total = (int64_t)n * C * T;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int t = (int)(i % T);
    const int c = (int)((i / T) % C);
    const int k = (int)(i / ((int64_t)T * C));
    const int u = utt[k];
    const int src = off[k] + t;
    out[i] = (src < lens[u]) ? mels[((int64_t)u * C + c) * Lmax + src] : 0.f;
  }
}

inline int nblk(int64_t n, int per = 256, int cap = 2048) {
  int64_t b = (n + per - 1) / per;
  if (b < 1) b = 1;
  return (int)(b > cap ? cap : b);
}

}  // namespace

DVAE_API int dvae_latent_fwd(const float* style, const float* content, const float* eps_c, const float* eps_s,
                             float* z, float* q_mu, float* q_lv, float* s_mu, float* s_lv, int Bh, int S, int Cn,
                             void* stream) {
  if (!style || !content || !eps_s || !z || !q_mu || !q_lv || !s_mu || !s_lv || Bh < 1 || S < 1 || Cn < 1)
    return DVAE_EINVAL;
  const int total = 2 * Bh * (S + Cn);
  hipLaunchKernelGGL(latent_fwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, style, content,
                     eps_c, eps_s, z, q_mu, q_lv, s_mu, s_lv, Bh, S, Cn);
  return dvae_check_launch();
}

DVAE_API int dvae_latent_bwd(const float* style, const float* content, const float* eps_c, const float* eps_s,
                             const float* dz, const float* dq_mu, const float* dq_lv, const float* ds_mu,
                             const float* ds_lv, float* dstyle, float* dcontent, int Bh, int S, int Cn,
                             void* stream) {
  if (!style || !content || !eps_s || !dstyle || !dcontent || Bh < 1 || S < 1 || Cn < 1) return DVAE_EINVAL;
  const int total = 2 * Bh * (S + Cn);
  hipLaunchKernelGGL(latent_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, style, content,
                     eps_c, eps_s, dz, dq_mu, dq_lv, ds_mu, ds_lv, dstyle, dcontent, Bh, S, Cn);
  return dvae_check_launch();
}

DVAE_API int dvae_kl_fwd(const float* mu, const float* lv, float* out, int64_t n, float scale, void* stream) {
  if (!mu || !lv || !out || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(kl_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, mu, lv, out, n, scale);
  return dvae_check_launch();
}

DVAE_API int dvae_kl_bwd(const float* mu, const float* lv, const float* gout, float* dmu, float* dlv, int64_t n,
                         float scale, void* stream) {
  if (!mu || !lv || !gout || !dmu || !dlv || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(kl_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mu, lv,
                     gout, dmu, dlv, n, scale);
  return dvae_check_launch();
}

DVAE_API int64_t dvae_l1_ws_bytes(int64_t n) {
  (void)n;
  return (int64_t)L1_BLOCKS * sizeof(double);
}

DVAE_API int dvae_l1_sum_fwd(const float* x, const float* y, float* out, void* ws, int64_t n, float scale,
                             void* stream) {
  if (!x || !y || !out || !ws || n < 1) return DVAE_EINVAL;
  if ((((uintptr_t)x) | ((uintptr_t)y)) & 15) return DVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = nblk(n / 4 + 1, 256, L1_BLOCKS);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(blocks), dim3(256), 0, s, x, y, (double*)ws, n);
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, out, blocks, scale);
  return dvae_check_launch();
}

DVAE_API int dvae_l1_sum_bwd(const float* x, const float* y, const float* gout, float* dy, int64_t n, float scale,
                             void* stream) {
  if (!x || !y || !gout || !dy || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, x, y, gout, dy, n, scale);
  return dvae_check_launch();
}


namespace {
int fill_loss_args(LossArgs& a, const dvae_loss_desc_t* d) {
  if (!d || d->n < 1 || d->nq < 1 || d->ns < 1) return DVAE_EINVAL;
  const void* ps[] = {d->x1, d->x2, d->recon1, d->recon2, d->recon1_hat, d->recon2_hat, d->q1_mu, d->q1_lv, d->q2_mu, d->q2_lv,
                      d->s_mu, d->s_lv};
  for (const void* p : ps)
    if (!p) return DVAE_EINVAL;
  for (int i = 0; i < 6; ++i)
    if (((uintptr_t)ps[i]) & 15) return DVAE_EINVAL;
  a.x[0] = d->x1; a.x[1] = d->x2;
  a.r[0] = d->recon1; a.r[1] = d->recon2; a.r[2] = d->recon1_hat; a.r[3] = d->recon2_hat;
  a.qmu[0] = d->q1_mu; a.qlv[0] = d->q1_lv; a.qmu[1] = d->q2_mu; a.qlv[1] = d->q2_lv;
  a.smu = d->s_mu; a.slv = d->s_lv;
  a.n = d->n; a.nq = d->nq; a.ns = d->ns;
  a.l1_scale = d->l1_scale; a.kl_scale = d->kl_scale; a.style_scale = d->style_scale;
  a.mse_cof = d->mse_cof; a.kl_cof = d->kl_cof;
  return DVAE_OK;
}
}  // namespace

DVAE_API int64_t dvae_loss_ws_bytes(int64_t n) {
  (void)n;
  return (int64_t)L1_BLOCKS * 4 * sizeof(double);
}

DVAE_API int dvae_loss_fwd(const dvae_loss_desc_t* desc, float* out8, void* ws, void* stream) {
  LossArgs a;
  int rc = fill_loss_args(a, desc);
  if (rc) return rc;
  if (!out8 || !ws) return DVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = nblk(a.n / 4 + 1, 256, L1_BLOCKS);
  hipLaunchKernelGGL(loss_partial_kernel, dim3(blocks), dim3(256), 0, s, a, (double*)ws);
  hipLaunchKernelGGL(loss_final_kernel<false>, dim3(1), dim3(256), 0, s, a, (const double*)ws, blocks, out8, LossSched{});
  return dvae_check_launch();
}

DVAE_API int dvae_loss_bwd(const dvae_loss_desc_t* desc, const float* g8, float* d_recon1, float* d_recon2,
                           float* d_recon1_hat, float* d_recon2_hat, float* d_q1_mu, float* d_q1_lv, float* d_q2_mu,
                           float* d_q2_lv, float* d_s_mu, float* d_s_lv, void* stream) {
  LossArgs a;
  int rc = fill_loss_args(a, desc);
  if (rc) return rc;
  if (!g8 || (!d_q1_mu != !d_q1_lv) || (!d_q2_mu != !d_q2_lv) || (!d_s_mu != !d_s_lv)) return DVAE_EINVAL;
  const float* outs[] = {d_recon1, d_recon2, d_recon1_hat, d_recon2_hat};
  for (const float* p : outs)
    if (p && (((uintptr_t)p) & 15)) return DVAE_EINVAL;
  const int blocks = nblk(a.n / 4 + 1, 256, 1024);
  hipLaunchKernelGGL(loss_bwd_kernel<false>, dim3(blocks + 1), dim3(256), 0, (hipStream_t)stream, a, g8, d_recon1, d_recon2,
                     d_recon1_hat, d_recon2_hat, d_q1_mu, d_q1_lv, d_q2_mu, d_q2_lv, d_s_mu, d_s_lv, blocks, LossSched{});
  return dvae_check_launch();
}

namespace {
// the weights and the free bits of a scheduled call: null coef / aux, D out of range or not dividing nq, misaligned
int fill_loss_sched(LossSched& s, const LossArgs& a, const dvae_loss_sched_t* sc, const float* aux) {
  if (!sc || !sc->coef || !aux) return DVAE_EINVAL;
  if (sc->D < 1 || sc->D > DVAE_LOSS_MAX_D || a.nq % sc->D != 0) return DVAE_EINVAL;
  if ((((uintptr_t)sc->coef) | ((uintptr_t)aux) | ((uintptr_t)sc->free_bits)) & 3) return DVAE_EINVAL;
  s.coef = sc->coef; s.free_bits = sc->free_bits; s.aux = const_cast<float*>(aux); s.D = sc->D;
  return DVAE_OK;
}
}  // namespace

DVAE_API int dvae_loss_fwd_sched(const dvae_loss_desc_t* desc, const dvae_loss_sched_t* sched, float* out8, float* aux,
                                 void* ws, void* stream) {
  LossArgs a;
  LossSched sc;
  int rc = fill_loss_args(a, desc);
  if (rc) return rc;
  if (!out8 || !ws) return DVAE_EINVAL;
  if ((rc = fill_loss_sched(sc, a, sched, aux))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = nblk(a.n / 4 + 1, 256, L1_BLOCKS);
  hipLaunchKernelGGL(loss_partial_kernel, dim3(blocks), dim3(256), 0, s, a, (double*)ws);
  hipLaunchKernelGGL(loss_final_kernel<true>, dim3(1), dim3(256), 0, s, a, (const double*)ws, blocks, out8, sc);
  return dvae_check_launch();
}

DVAE_API int dvae_loss_bwd_sched(const dvae_loss_desc_t* desc, const dvae_loss_sched_t* sched, const float* aux,
                                 const float* g8, float* d_recon1, float* d_recon2, float* d_recon1_hat,
                                 float* d_recon2_hat, float* d_q1_mu, float* d_q1_lv, float* d_q2_mu, float* d_q2_lv,
                                 float* d_s_mu, float* d_s_lv, void* stream) {
  LossArgs a;
  LossSched sc;
  int rc = fill_loss_args(a, desc);
  if (rc) return rc;
  if (!g8 || (!d_q1_mu != !d_q1_lv) || (!d_q2_mu != !d_q2_lv) || (!d_s_mu != !d_s_lv)) return DVAE_EINVAL;
  const float* outs[] = {d_recon1, d_recon2, d_recon1_hat, d_recon2_hat};
  for (const float* p : outs)
    if (p && (((uintptr_t)p) & 15)) return DVAE_EINVAL;
  if ((rc = fill_loss_sched(sc, a, sched, aux))) return rc;
  const int blocks = nblk(a.n / 4 + 1, 256, 1024);
  hipLaunchKernelGGL(loss_bwd_kernel<true>, dim3(blocks + 1), dim3(256), 0, (hipStream_t)stream, a, g8, d_recon1, d_recon2,
                     d_recon1_hat, d_recon2_hat, d_q1_mu, d_q1_lv, d_q2_mu, d_q2_lv, d_s_mu, d_s_lv, blocks, sc);
  return dvae_check_launch();
}

DVAE_API int dvae_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                            float beta2, float eps, float grad_scale, int step, void* stream) {
  if (!p || !g || !m || !v || n < 1 || step < 1) return DVAE_EINVAL;
  if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return DVAE_EINVAL;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3(nblk(n / 4 + 1, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                     lr, beta1, beta2, eps, grad_scale, (float)bc1, (float)sqrt(bc2));
  return dvae_check_launch();
}

static int adam_flat_dev_launch(float* p, float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                                float* state, const unsigned* skip_if_nonzero, const dvae_ranges_t* clear, int tick,
                                const float* clip, void* stream) {
  if (!p || !g || !m || !v || !state || n < 4 || (n & 3)) return DVAE_EINVAL;
  if ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) return DVAE_EINVAL;
  AdamClear c{};
  if (clear) {
    if (clear->n < 0 || clear->n > 8) return DVAE_EINVAL;
    c.n = clear->n;
    for (int r = 0; r < c.n; ++r) {
      if (clear->lo[r] < 0 || clear->hi[r] > n || clear->lo[r] > clear->hi[r] || ((clear->lo[r] | clear->hi[r]) & 3))
        return DVAE_EINVAL;
      c.lo[r] = clear->lo[r];
      c.hi[r] = clear->hi[r];
    }
  }
  hipStream_t s = (hipStream_t)stream;
#ifndef DVAE_ADAM_U
#define DVAE_ADAM_U 2
#endif
  constexpr int U = DVAE_ADAM_U;
  const int64_t n4 = n >> 2;
  const dim3 grid(nblk((n4 + U - 1) / U, 256, 2048));
  if (clip) {
    if (tick) hipLaunchKernelGGL(adam_tick_kernel<true>, dim3(1), dim3(64), 0, s, state, beta1, beta2, skip_if_nonzero, clip);
    hipLaunchKernelGGL((adam_dev_kernel<U, true>), grid, dim3(256), 0, s, p, g, m, v, n4, beta1, beta2, eps, state,
                       skip_if_nonzero, c, clip);
  } else {
    if (tick) hipLaunchKernelGGL(adam_tick_kernel<false>, dim3(1), dim3(64), 0, s, state, beta1, beta2, skip_if_nonzero, clip);
    hipLaunchKernelGGL((adam_dev_kernel<U, false>), grid, dim3(256), 0, s, p, g, m, v, n4, beta1, beta2, eps, state,
                       skip_if_nonzero, c, clip);
  }
  return dvae_check_launch();
}

DVAE_API int dvae_adam_flat_dev(float* p, float* g, float* m, float* v, int64_t n, float beta1, float beta2, float eps,
                                float* state, const unsigned* skip_if_nonzero, const dvae_ranges_t* clear, int tick,
                                void* stream) {
  return adam_flat_dev_launch(p, g, m, v, n, beta1, beta2, eps, state, skip_if_nonzero, clear, tick, nullptr, stream);
}

DVAE_API int dvae_adam_flat_dev_clip(float* p, float* g, float* m, float* v, int64_t n, float beta1, float beta2,
                                     float eps, float* state, const unsigned* skip_if_nonzero,
                                     const dvae_ranges_t* clear, int tick, const float* clip, void* stream) {
  if (!clip) return DVAE_EINVAL;
  return adam_flat_dev_launch(p, g, m, v, n, beta1, beta2, eps, state, skip_if_nonzero, clear, tick, clip, stream);
}

DVAE_API int64_t dvae_grad_sumsq_ws_bytes(int64_t n) {
  if (n < 4 || (n & 3)) return 0;
  return (int64_t)sumsq_blocks(n) * sizeof(double);
}

DVAE_API int dvae_grad_sumsq(const float* g, int64_t n, void* ws, void* stream) {
  if (!g || !ws || n < 4 || (n & 3) || (((uintptr_t)g) & 15) || (((uintptr_t)ws) & 7)) return DVAE_EINVAL;
  hipLaunchKernelGGL(grad_sumsq_kernel<SUMSQ_U>, dim3(sumsq_blocks(n)), dim3(256), 0, (hipStream_t)stream, g,
                     reinterpret_cast<double*>(ws), n >> 2);
  return dvae_check_launch();
}

DVAE_API int dvae_grad_clip_finalize(const void* ws, int64_t n, const float* state, float* clip,
                                     const unsigned* skip_if_nonzero, int guard_nonfinite, void* stream) {
  if (!ws || !state || !clip || n < 4 || (n & 3) || (((uintptr_t)ws) & 7)) return DVAE_EINVAL;
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const double*>(ws), sumsq_blocks(n), state, clip, skip_if_nonzero,
                     guard_nonfinite ? 1 : 0);
  return dvae_check_launch();
}

constexpr int EMA_U = 2;          // 16-byte loads in flight per tensor, thread and trip (ema_update_kernel, swap_kernel)
static bool flat_pair_ok(const float* a, const float* b, int64_t n) {
  if (!a || !b || n < 4 || (n & 3) || ((((uintptr_t)a) | ((uintptr_t)b)) & 15)) return false;
  const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b;
  const uintptr_t hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
  return hi - lo >= (uintptr_t)n * sizeof(float);      // the two buffers do not overlap
}

DVAE_API int dvae_ema_tick(float* ema_state, const unsigned* skip_if_nonzero, const float* clip_or_null, void* stream) {
  if (!ema_state) return DVAE_EINVAL;
  hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ema_state, skip_if_nonzero, clip_or_null);
  return dvae_check_launch();
}

DVAE_API int dvae_ema_update(float* ema, const float* p, int64_t n, const float* ema_state, void* stream) {
  if (!ema_state || !flat_pair_ok(ema, p, n)) return DVAE_EINVAL;
  const int64_t n4 = n >> 2;
  hipLaunchKernelGGL(ema_update_kernel<EMA_U>, dim3(nblk((n4 + EMA_U - 1) / EMA_U, 256, 2048)), dim3(256), 0,
                     (hipStream_t)stream, ema, p, n4, ema_state);
  return dvae_check_launch();
}

DVAE_API int dvae_swap_f32(float* a, float* b, int64_t n, void* stream) {
  if (!flat_pair_ok(a, b, n)) return DVAE_EINVAL;
  const int64_t n4 = n >> 2;
  hipLaunchKernelGGL(swap_kernel<EMA_U>, dim3(nblk((n4 + EMA_U - 1) / EMA_U, 256, 2048)), dim3(256), 0,
                     (hipStream_t)stream, a, b, n4);
  return dvae_check_launch();
}

// x[0, n) = 0 with plain stores, in a launch of its own right in front of the launches that accumulate into x atomically
// (gradients: FlatAdam.zero_grad; split-k outputs of the Linear layers)
__global__ __launch_bounds__(256) void zero_kernel(float* __restrict__ x, int64_t n) {
  const int64_t n4 = n >> 2;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    *reinterpret_cast<f32x4*>(x + 4 * i) = z;
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) x[(n4 << 2) + threadIdx.x] = 0.f;
}
DVAE_API int dvae_zero_f32(float* x, int64_t n, void* stream) {
  if (!x || n < 1 || (((uintptr_t)x) & 15)) return DVAE_EINVAL;
  hipLaunchKernelGGL(zero_kernel, dim3(nblk(n / 4 + 1, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, n);
  return dvae_check_launch();
}

// out = a + b (+ c): the sum of the gradients that reach a tensor with several consumers (ops.FanoutFn)
__global__ __launch_bounds__(256) void sum_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  const float* __restrict__ c, float* __restrict__ out, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(a + 4 * i) + *reinterpret_cast<const f32x4*>(b + 4 * i);
    if (c) v += *reinterpret_cast<const f32x4*>(c + 4 * i);
    *reinterpret_cast<f32x4*>(out + 4 * i) = v;
  }
}
DVAE_API int dvae_sum_f32(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream) {
  if (!a || !b || !out || n < 4 || (n & 3)) return DVAE_EINVAL;
  if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)out)) & 15) return DVAE_EINVAL;
  hipLaunchKernelGGL(sum_kernel, dim3(nblk(n / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a, b, c, out, n >> 2);
  return dvae_check_launch();
}

DVAE_API int dvae_gather_crop(const float* mels, const int* lens, const int* utt, const int* off, float* out, int n,
                              int C, int T, int Lmax, void* stream) {
  if (!mels || !lens || !utt || !off || !out || n < 1 || C < 1 || T < 1 || Lmax < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(gather_crop_kernel, dim3(nblk((int64_t)n * C * T)), dim3(256), 0, (hipStream_t)stream, mels, lens,
                     utt, off, out, n, C, T, Lmax);
  return dvae_check_launch();
}

DVAE_API int dvae_mel_to_chunks(const float* mel, float* out, int C, int L, int T, int n, void* stream) {
  if (!mel || !out || C < 1 || L < 0 || T < 1 || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(mel_to_chunks_kernel, dim3(nblk((int64_t)n * C * T)), dim3(256), 0, (hipStream_t)stream, mel, out,
                     C, L, T, n);
  return dvae_check_launch();
}
DVAE_API int dvae_chunks_to_mel(const float* in, float* out, int n, int C, int T, float lo, float hi, int clamp,
                                void* stream) {
  if (!in || !out || n < 1 || C < 1 || T < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(chunks_to_mel_kernel, dim3(nblk((int64_t)n * C * T)), dim3(256), 0, (hipStream_t)stream, in, out,
                     n, C, T, lo, hi, clamp);
  return dvae_check_launch();
}
DVAE_API int dvae_conversion_latents(const float* src_style, const float* src_content, const float* trg_style,
                                     float* z_src, float* z_conv, int n, int m, int S, int Cn, void* stream) {
  if (!src_style || !src_content || !trg_style || !z_src || !z_conv || n < 1 || m < 1 || S < 1 || Cn < 1)
    return DVAE_EINVAL;
  const int total = n * (S + Cn);
  hipLaunchKernelGGL(conversion_latents_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, src_style,
                     src_content, trg_style, z_src, z_conv, n, m, S, Cn);
  return dvae_check_launch();
}
DVAE_API int dvae_mel_to_windows(const float* mels, int64_t ld, const int* utt_table, const int* win_table, float* out,
                                 int nwin, int C, int T, void* stream) {
  if (!mels || !utt_table || !win_table || !out || ld < 1 || nwin < 1 || C < 1 || T < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(mel_to_windows_kernel, dim3(nblk((int64_t)nwin * C * T)), dim3(256), 0, (hipStream_t)stream, mels, ld,
                     utt_table, win_table, out, nwin, C, T);
  return dvae_check_launch();
}
DVAE_API int dvae_window_latents(const float* content, const double* sums, const int64_t* counts, const int* g_src,
                                 const int* g_trg, double mix, float* z, int nwin, int S, int Cn, int K, void* stream) {
  if (!content || !sums || !counts || !g_src || !g_trg || !z || nwin < 1 || S < 1 || Cn < 1 || K < S) return DVAE_EINVAL;
  if (!(mix >= 0.0 && mix <= 1.0)) return DVAE_EINVAL;
  hipLaunchKernelGGL(window_latents_kernel, dim3(nblk((int64_t)nwin * (S + Cn))), dim3(256), 0, (hipStream_t)stream, content,
                     sums, counts, g_src, g_trg, mix, z, nwin, S, Cn, K);
  return dvae_check_launch();
}
DVAE_API int dvae_windows_overlap_add(const float* y, const int* utt_table, const int* win_table, const float* w, float* out,
                                      int64_t ld, int nutt, int C, int T, float lo, float hi, int clamp, void* stream) {
  if (!y || !utt_table || !win_table || !w || !out || ld < 1 || nutt < 1 || C < 1 || T < 1) return DVAE_EINVAL;
  if (clamp && !(lo <= hi)) return DVAE_EINVAL;
  hipLaunchKernelGGL(windows_overlap_add_kernel, dim3(nblk((int64_t)C * ld)), dim3(256), 0, (hipStream_t)stream, y, utt_table,
                     win_table, w, out, ld, nutt, C, T, lo, hi, clamp);
  return dvae_check_launch();
}
DVAE_API int dvae_mul_div(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream) {
  if (!a || !b || !c || !out || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(mul_div_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, a, b, c, out, n);
  return dvae_check_launch();
}

DVAE_API int dvae_mel_to_frames(const float* x1, const float* x2, void* X, int Bh, int C, int T, int out_bf16,
                                void* stream) {
  if (!x1 || !X || Bh < 1 || C < 1 || T < 1) return DVAE_EINVAL;
  const int N = x2 ? 2 * Bh : Bh;
  dim3 grid((T + 31) / 32, (C + 31) / 32, N);
  if (out_bf16) hipLaunchKernelGGL(mel_to_frames_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x1, x2, X, Bh, C, T, N);
  else hipLaunchKernelGGL(mel_to_frames_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x1, x2, X, Bh, C, T, N);
  return dvae_check_launch();
}

DVAE_API int dvae_frames_to_mel(const float* X, float* out, int N, int C, int T, void* stream) {
  if (!X || !out || N < 1 || C < 1 || T < 1) return DVAE_EINVAL;
  dim3 grid((T + 31) / 32, (C + 31) / 32, N);
  hipLaunchKernelGGL(frames_to_mel_kernel, grid, dim3(256), 0, (hipStream_t)stream, X, out, N, C, T);
  return dvae_check_launch();
}

DVAE_API int dvae_permute_102(const float* in, float* out, int A, int B, int C, void* stream) {
  if (!in || !out || A < 1 || B < 1 || C < 4 || (C & 3)) return DVAE_EINVAL;
  const int64_t total = (int64_t)A * B * (C / 4);
  hipLaunchKernelGGL(permute_102_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, in, out, A, B, C / 4);
  return dvae_check_launch();
}

DVAE_API int dvae_colsum_add(const void* X, float* out1, float* out2, int R, int C, int64_t ld, int x_bf16, void* stream) {
  if (!X || !out1 || R < 1 || C < 1) return DVAE_EINVAL;
  if ((ld & 3) || (((uintptr_t)X) & (x_bf16 ? 7 : 15))) return DVAE_EINVAL;
  // (fewer rows per workgroup for narrow matrices -- more workgroups -- was tried: the extra same-address atomics
  // cost more than the parallelism gains, 0.43 -> 1.0 ms per step)
  const int cb = (C + 255) / 256;
  // Rows per workgroup: every workgroup ends in one atomic per column, so few, long workgroups win (measured, us at
  // 128 / 256 / 512 / 1024 rows: [16384 x 512] fp32 18.0 / 9.6 / 8.3 / 10.6; [65536 x 512] bf16 57 / 35 / 23 / 22;
  // [16384 x 4096] fp32 54 / 52 / 48 / 41): 512, and 1024 once there are >= 512 workgroups even so
  int rows_pb = ((int64_t)R * cb >= (int64_t)512 * 1024) ? 1024 : 512;
  if (dvae_dev_knob("DVAE_COLSUM_ROWS", 0) > 0) rows_pb = dvae_dev_knob("DVAE_COLSUM_ROWS", 0);
  if (g_dvae_deterministic) rows_pb = R;      // one workgroup per column block walks all rows: one add per column
  dim3 grid(cb, (R + rows_pb - 1) / rows_pb);
  if (x_bf16) hipLaunchKernelGGL(colsum_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, X, out1, out2, R, C, ld, rows_pb);
  else hipLaunchKernelGGL(colsum_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, X, out1, out2, R, C, ld, rows_pb);
  return dvae_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// k-split without atomics (round 6): the partial products a contraction stored into slabs (dvae_gemm_f32_slabs ...) are
// added to the result in the FIXED order ks = 1, 2, ...: every element has one writer and one summation order, so the
// result is run-to-run bit-identical.  HBM-bound: (nslab + 2) * 4 bytes per element.
// v + slab 0 + slab 1 + ... in THAT order; eight 16-byte loads in flight per thread (the trip count is a run-time value: without
// the explicit window the loads of a thread go out one behind the other)
__device__ __forceinline__ f32x4 slab_add(f32x4 v, const float* __restrict__ p, int64_t stride, int nslab) {
  int k = 0;
  for (; k + 8 <= nslab; k += 8) {
    f32x4 w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const f32x4*>(p + (int64_t)(k + j) * stride);
#pragma unroll
    for (int j = 0; j < 8; ++j) v += w[j];
  }
  if (k + 4 <= nslab) {
    f32x4 w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const f32x4*>(p + (int64_t)(k + j) * stride);
#pragma unroll
    for (int j = 0; j < 4; ++j) v += w[j];
    k += 4;
  }
  for (; k < nslab; ++k) v += *reinterpret_cast<const f32x4*>(p + (int64_t)k * stride);
  return v;
}
__global__ __launch_bounds__(256) void slab_sum_kernel(float* __restrict__ C, const float* __restrict__ slab, int64_t stride,
                                                       int nslab, int64_t n4, int act, int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (accumulate) v = *reinterpret_cast<const f32x4*>(C + 4 * i);
    v = slab_add(v, slab + 4 * i, stride, nslab);
    if (act != DVAE_ACT_NONE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_apply(v[e], act);
    }
    *reinterpret_cast<f32x4*>(C + 4 * i) = v;
  }
}
// C[i] = act((accumulate ? C[i] : 0) + sum_k slab[k * slab_stride + i]), i < n (n, slab_stride multiples of 4; 16-byte aligned)
DVAE_API int dvae_slab_sum(float* C, const float* slab, int64_t slab_stride, int nslab, int64_t n, int act, int accumulate,
                           void* stream) {
  if (!C || n < 4 || (n & 3) || nslab < 0 || (nslab > 0 && (!slab || (slab_stride & 3) || (((uintptr_t)slab) & 15))) ||
      (((uintptr_t)C) & 15) || (nslab == 0 && !accumulate))
    return DVAE_EINVAL;
  if (nslab == 0 && act == DVAE_ACT_NONE) return DVAE_OK;
  hipLaunchKernelGGL(slab_sum_kernel, dim3(nblk(n / 4, 256, 2048)), dim3(256), 0, (hipStream_t)stream, C, slab, slab_stride,
                     nslab, n >> 2, act, accumulate);
  return dvae_check_launch();
}

// the same for MANY results in one launch (the weight gradients of a step, in front of the Adam launch or of a bucket's
// collective): entry e adds its nslab slabs to its n elements.  The table travels as a kernel argument (<= 64 entries).
struct SlabTable {
  dvae_slab_desc_t e[DVAE_SLAB_FOLD_MAX];
};
__global__ __launch_bounds__(256) void slab_fold_kernel(const SlabTable t) {
  const dvae_slab_desc_t d = t.e[blockIdx.y];
  const int64_t n4 = d.n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(d.c + 4 * i);
    v = slab_add(v, d.slab + 4 * i, d.slab_stride, d.nslab);
    *reinterpret_cast<f32x4*>(d.c + 4 * i) = v;
  }
}
DVAE_API int dvae_slab_fold(const dvae_slab_desc_t* descs, int n_entries, void* stream) {
  if (!descs || n_entries < 0) return DVAE_EINVAL;
  for (int base = 0; base < n_entries; base += DVAE_SLAB_FOLD_MAX) {
    SlabTable t{};
    const int m = n_entries - base < DVAE_SLAB_FOLD_MAX ? n_entries - base : DVAE_SLAB_FOLD_MAX;
    int64_t nmax = 0;
    for (int i = 0; i < m; ++i) {
      const dvae_slab_desc_t& d = descs[base + i];
      if (!d.c || !d.slab || d.n < 4 || (d.n & 3) || (d.slab_stride & 3) || d.nslab < 1 ||
          ((((uintptr_t)d.c) | ((uintptr_t)d.slab)) & 15))
        return DVAE_EINVAL;
      t.e[i] = d;
      nmax = d.n > nmax ? d.n : nmax;
    }
    hipLaunchKernelGGL(slab_fold_kernel, dim3(nblk(nmax / 4, 256, 512), m), dim3(256), 0, (hipStream_t)stream, t);
  }
  return dvae_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// Column sums WITHOUT atomics: every workgroup stores the partial sums of its row block, the LAST workgroup of a column
// block to arrive (a ticket counter per column block, agent-scope release / acquire around it) adds them up in row-block
// order and is the one writer of out[c].  ws: [column blocks] counters (zero when the call starts, left zero) + the partials.
template <bool XB16>
__global__ __launch_bounds__(256) void colsum_ws_kernel(const void* __restrict__ Xv, float* __restrict__ o1,
                                                        float* __restrict__ o2, int R, int C, int64_t ld, int rows_pb,
                                                        unsigned* __restrict__ cnt, float* __restrict__ part) {
  using elem_t = typename std::conditional<XB16, __bf16, float>::type;
  const elem_t* __restrict__ X = reinterpret_cast<const elem_t*>(Xv);
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + cl) * 4;
  const int r0 = blockIdx.y * rows_pb, r1 = min(R, r0 + rows_pb);
  const int Cp = gridDim.x * 256;                    // padded row length of the partials
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (c + 3 < C) {
    const elem_t* __restrict__ px = X + (int64_t)(r0 + rl) * ld + c;
    const int n = (r1 - r0 - rl + 3) >> 2;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ld4<XB16>(px + (int64_t)(i + u) * 4 * ld, 0);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; i < n; ++i) s += ld4<XB16>(px + (int64_t)i * 4 * ld, 0);
  } else if (c < C) {
    for (int r = r0 + rl; r < r1; r += 4)
      for (int k = 0; k < 4 && c + k < C; ++k) s[k] += (float)X[(int64_t)r * ld + c + k];
  }
  __shared__ f32x4 red[4][64];
  __shared__ int last;
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0) {
    const f32x4 tot = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
    *reinterpret_cast<f32x4*>(part + (int64_t)blockIdx.y * Cp + (blockIdx.x * 64 + cl) * 4) = tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned tk = __hip_atomic_fetch_add(cnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (tk == gridDim.y - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  // wave rl adds the row blocks rl, rl + 4, ... in that order, then the four waves' sums are combined in a fixed tree: the
  // same sum in every run
  f32x4 ps = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (unsigned b = rl; b < gridDim.y; b += 4)
    ps += *reinterpret_cast<const f32x4*>(part + (int64_t)b * Cp + (blockIdx.x * 64 + cl) * 4);
  red[rl][cl] = ps;
  __syncthreads();
  if (rl == 0 && c < C) {
    const f32x4 tot = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c + k >= C) break;
      o1[c + k] += tot[k];
      if (o2) o2[c + k] += tot[k];
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(cnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static inline int colsum_rows_pb(int R, int C) {
  const int cb = (C + 255) / 256;
  return ((int64_t)R * cb >= (int64_t)512 * 1024) ? 1024 : 512;
}
DVAE_API int64_t dvae_colsum_ws_bytes(int R, int C) {
  if (R < 1 || C < 1) return 0;
  const int cb = (C + 255) / 256, rows_pb = colsum_rows_pb(R, C);
  return 4096 + (int64_t)((R + rows_pb - 1) / rows_pb) * cb * 256 * 4;
}
// out1[c] (and out2[c]) += sum_r X[r][c], deterministic (see above).  ws: >= dvae_colsum_ws_bytes(R, C) bytes, 16-byte aligned,
// its first 4096 bytes ZERO before the first call (the counters; every call leaves them zero); one ws per stream in flight
DVAE_API int dvae_colsum_add_ws(const void* X, float* out1, float* out2, int R, int C, int64_t ld, int x_bf16, void* ws,
                                void* stream) {
  if (!X || !out1 || !ws || R < 1 || C < 1 || C > 256 * 1024) return DVAE_EINVAL;
  if ((ld & 3) || (((uintptr_t)X) & (x_bf16 ? 7 : 15)) || (((uintptr_t)ws) & 15)) return DVAE_EINVAL;
  const int cb = (C + 255) / 256, rows_pb = colsum_rows_pb(R, C);
  dim3 grid(cb, (R + rows_pb - 1) / rows_pb);
  unsigned* cnt = (unsigned*)ws;
  float* part = (float*)((char*)ws + 4096);
  if (x_bf16) hipLaunchKernelGGL(colsum_ws_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, X, out1, out2, R, C, ld, rows_pb, cnt, part);
  else hipLaunchKernelGGL(colsum_ws_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, X, out1, out2, R, C, ld, rows_pb, cnt, part);
  return dvae_check_launch();
}

DVAE_API int dvae_transpose(const float* in, float* out, int R, int C, void* stream) {
  if (!in || !out || R < 1 || C < 1) return DVAE_EINVAL;
  dim3 grid((C + 31) / 32, (R + 31) / 32);
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, out, R, C);
  return dvae_check_launch();
}

DVAE_API int dvae_act_bwd(const float* dZ, const float* Z, float* dU, int64_t n, int act, void* stream) {
  if (!dZ || !Z || !dU || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, dZ, Z, dU, n, act);
  return dvae_check_launch();
}

DVAE_API int dvae_act_fwd(float* Y, int64_t n, int act, void* stream) {
  if (!Y || n < 1) return DVAE_EINVAL;
  hipLaunchKernelGGL(act_fwd_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, Y, n, act);
  return dvae_check_launch();
}

DVAE_API int dvae_conv_pack_w(const float* W, float* Wp, int Cout, int Cin, void* stream) {
  if (!W || !Wp || Cout < 1 || Cin < 1) return DVAE_EINVAL;
  const int64_t cc = (int64_t)Cout * Cin;
  hipLaunchKernelGGL(conv_pack_kernel, dim3(nblk(cc)), dim3(256), 0, (hipStream_t)stream, W, Wp, cc);
  return dvae_check_launch();
}

DVAE_API int dvae_conv_pack_wt(const float* W, float* Wpt, int Cout, int Cin, void* stream) {
  if (!W || !Wpt || Cout < 1 || Cin < 1) return DVAE_EINVAL;
  dim3 grid((Cin + 31) / 32, (Cout + 31) / 32);
  hipLaunchKernelGGL(conv_pack_t_kernel, grid, dim3(256), 0, (hipStream_t)stream, W, Wpt, Cout, Cin);
  return dvae_check_launch();
}

DVAE_API int dvae_conv_unpack_add_w(const float* dWp, float* dW, int Cout, int Cin, void* stream) {
  if (!dWp || !dW || Cout < 1 || Cin < 1) return DVAE_EINVAL;
  const int64_t cc = (int64_t)Cout * Cin;
  hipLaunchKernelGGL(conv_unpack_add_kernel, dim3(nblk(cc)), dim3(256), 0, (hipStream_t)stream, dWp, dW, cc);
  return dvae_check_launch();
}

// ---- global variance, modulation spectrum and its postfilter: the kernels of modspec.hip, part of this translation unit
#include "modspec.hip"
#include "msloss.hip"       // the modulation-spectrum / global-variance loss of the train step: the same
