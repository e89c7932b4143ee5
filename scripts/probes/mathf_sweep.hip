// The device's log10f, logf, exp10f, sincosf, sqrtf and fp32 division (what the audio kernels of csrc/frontend.hip call)
// against float64 on the host, over the domains those kernels use:
//   log10f   2^24 log-spaced x in [1e-5, 1e4]  + the 2^17 floats around 1          (mel_db_normalize)
//   logf     2^24 log-spaced x in [1e-10, 1e8] + the 2^17 floats around 1          (log_power)
//   exp10f   2^24 evenly spaced x in [-4.2, 0.8]                                   (mel_denormalize)
//   sincosf  2^24 evenly spaced x in [-64, 64]                                     (gl_init)
//   sqrtf    every float in [1, 4): all 2^24 significands of either exponent parity (stft_magnitude, gl_phase)
//   a / b    2^25 pairs of pseudo-random full significands, exponents in [-20, 20]  (gl_phase, ola, voicing, normalize)
// Per function: worst |got - ref| / (2^-24 |ref|) ("rel"), and for the functions whose value passes through zero inside
// the domain worst |got - ref| / 2^-24 ("abs", sincosf: |value| <= 1) or / (2^-24 max(|ref|, 1)) ("mixed", the logarithms).
// tests/audio_ref.py takes its *_MEASURED constants from this program's output.
// Build with the library's flags: hipcc --offload-arch=gfx950 -O3 -std=c++17 mathf_sweep.hip -o mathf_sweep
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

enum { F_LOG10 = 0, F_LOG = 1, F_EXP10 = 2, F_SINCOS = 3, F_SQRT = 4, F_DIV = 5 };

__global__ __launch_bounds__(256) void k(int fn, const float* x, const float* y, float* t, float* u, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float r = 0.f, r2 = 0.f;
  switch (fn) {
    case F_LOG10: r = log10f(v); break;
    case F_LOG: r = logf(v); break;
    case F_EXP10: r = exp10f(v); break;
    case F_SINCOS: sincosf(v, &r, &r2); break;
    case F_SQRT: r = sqrtf(v); break;
    default: r = v / y[i]; break;
  }
  t[i] = r;
  u[i] = r2;
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

struct Worst {
  double w = 0.0, at = 0.0, at2 = 0.0;
  void see(double e, double a, double b = 0.0) {
    if (!(e <= w)) { w = e; at = a; at2 = b; }          // a NaN or an infinity from the device counts as the worst
  }
};

int main() {
  const int N = 1 << 24, NEAR = 1 << 16, NMAX = 2 * N;
  const double eps = std::ldexp(1.0, -24);
  std::vector<float> x(NMAX), y(NMAX), t(NMAX), u(NMAX);
  float *dx, *dy, *dt, *du;
  CK(hipMalloc(&dx, sizeof(float) * NMAX));
  CK(hipMalloc(&dy, sizeof(float) * NMAX));
  CK(hipMalloc(&dt, sizeof(float) * NMAX));
  CK(hipMalloc(&du, sizeof(float) * NMAX));
  for (int fn = F_LOG10; fn <= F_DIV; ++fn) {
    int n = N;
    if (fn == F_LOG10 || fn == F_LOG) {
      const double lo = fn == F_LOG10 ? -5.0 : -10.0, hi = fn == F_LOG10 ? 4.0 : 8.0;
      for (int i = 0; i < N; ++i) x[i] = (float)std::pow(10.0, lo + (hi - lo) * i / (N - 1));
      float up = 1.f, dn = 1.f;
      for (int i = 0; i < NEAR; ++i) {
        x[n++] = up;
        x[n++] = dn;
        up = std::nextafterf(up, 2.f);
        dn = std::nextafterf(dn, 0.f);
      }
    } else if (fn == F_EXP10) {
      for (int i = 0; i < N; ++i) x[i] = (float)(-4.2 + 5.0 * i / (N - 1));
    } else if (fn == F_SINCOS) {
      for (int i = 0; i < N; ++i) x[i] = (float)(-64.0 + 128.0 * i / (N - 1));
    } else if (fn == F_SQRT) {
      float v = 1.f;
      for (int i = 0; i < N; ++i) {
        x[i] = v;
        v = std::nextafterf(v, 8.f);
      }
    } else {
      n = NMAX;
      uint64_t s = 0x9E3779B97F4A7C15ull;
      auto rnd = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 32);
      };
      for (int i = 0; i < n; ++i) {
        const uint32_t a = rnd(), b = rnd(), c = rnd();
        x[i] = std::ldexp(1.f + (float)(a & 0x7fffff) * 0x1p-23f, (int)(c % 41u) - 20) * ((c & 0x10000) ? -1.f : 1.f);
        y[i] = std::ldexp(1.f + (float)(b & 0x7fffff) * 0x1p-23f, (int)((c >> 8) % 41u) - 20);
      }
    }
    CK(hipMemcpy(dx, x.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dy, y.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, fn, dx, dy, dt, du, n);
    CK(hipGetLastError());
    CK(hipMemcpy(t.data(), dt, sizeof(float) * n, hipMemcpyDeviceToHost));
    CK(hipMemcpy(u.data(), du, sizeof(float) * n, hipMemcpyDeviceToHost));
    Worst rel, alt;
    for (int i = 0; i < n; ++i) {
      const double v = (double)x[i];
      if (fn == F_LOG10 || fn == F_LOG) {
        const double r = fn == F_LOG10 ? std::log10(v) : std::log(v), e = std::fabs((double)t[i] - r);
        if (r != 0.0) rel.see(e / (eps * std::fabs(r)), v);
        else rel.see(e == 0.0 ? 0.0 : INFINITY, v);
        alt.see(e / (eps * std::fmax(std::fabs(r), 1.0)), v);
      } else if (fn == F_EXP10) {
        const double r = std::pow(10.0, v);
        rel.see(std::fabs((double)t[i] - r) / (eps * r), v);
      } else if (fn == F_SINCOS) {
        alt.see(std::fabs((double)t[i] - std::sin(v)) / eps, v);
        alt.see(std::fabs((double)u[i] - std::cos(v)) / eps, v);
        if (std::sin(v) != 0.0) rel.see(std::fabs((double)t[i] - std::sin(v)) / (eps * std::fabs(std::sin(v))), v);
        rel.see(std::fabs((double)u[i] - std::cos(v)) / (eps * std::fabs(std::cos(v))), v);
      } else if (fn == F_SQRT) {
        const double r = std::sqrt(v);
        rel.see(std::fabs((double)t[i] - r) / (eps * r), v);
      } else {
        const double r = v / (double)y[i];
        rel.see(std::fabs((double)t[i] - r) / (eps * std::fabs(r)), v, (double)y[i]);
      }
    }
    static const char* names[] = {"log10f", "logf", "exp10f", "sincosf", "sqrtf", "div"};
    static const char* alts[] = {"mixed", "mixed", "-", "abs", "-", "-"};
    printf("%s over %d points: worst rel = %.4f at x = %.9g (y = %.9g); worst %s = %.4f at x = %.9g\n", names[fn], n,
           rel.w, rel.at, rel.at2, alts[fn], alt.w, alt.at);
  }
  CK(hipFree(dx));
  CK(hipFree(dy));
  CK(hipFree(dt));
  CK(hipFree(du));
  return 0;
}
