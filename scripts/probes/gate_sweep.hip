// The LSTM gate functions of csrc/common.h (gate_sigmoid, gate_tanh: v_exp_f32 + v_rcp_f32) against float64 on the host:
// worst |err| / 2^-24 of each over 40 000 001 evenly spaced x in [-100, 100] and 2^23 log-spaced |x| in [1e-6, 100] of
// either sign (ABSOLUTE errors: both expressions cancel by design), and the worst RELATIVE error of gate_tanh below
// |x| = 1e-3.  tests/lstm_ref.py takes GATE_SIGMOID_MEASURED / GATE_TANH_MEASURED from this program's output (DESIGN.md
// section 5).  Also says whether every |x| >= 90 gave exactly 0 / 1 / +-1 and whether anything was not finite.
// Build with the library's flags: hipcc --offload-arch=gfx950 -O3 -std=c++17 gate_sweep.hip -o gate_sweep
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

// the two definitions of csrc/common.h, verbatim
__device__ __forceinline__ float gate_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float gate_tanh(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * x) + 1.f); }

__global__ __launch_bounds__(256) void k(const float* x, float* s, float* t, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    s[i] = gate_sigmoid(x[i]);
    t[i] = gate_tanh(x[i]);
  }
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main() {
  const int n_lin = 40000001, n_log = 1 << 23, n = n_lin + 2 * n_log;
  std::vector<float> x(n), s(n), t(n);
  for (int i = 0; i < n_lin; ++i) x[i] = (float)(-100.0 + 200.0 * i / (n_lin - 1));
  for (int i = 0; i < n_log; ++i) {
    const float v = (float)std::pow(10.0, -6.0 + 8.0 * i / (n_log - 1));
    x[n_lin + 2 * i] = v;
    x[n_lin + 2 * i + 1] = -v;
  }
  float *dx, *ds, *dt;
  CK(hipMalloc(&dx, sizeof(float) * n));
  CK(hipMalloc(&ds, sizeof(float) * n));
  CK(hipMalloc(&dt, sizeof(float) * n));
  CK(hipMemcpy(dx, x.data(), sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, dx, ds, dt, n);
  CK(hipGetLastError());
  CK(hipMemcpy(s.data(), ds, sizeof(float) * n, hipMemcpyDeviceToHost));
  CK(hipMemcpy(t.data(), dt, sizeof(float) * n, hipMemcpyDeviceToHost));
  const double eps = std::ldexp(1.0, -24);
  double ws = 0.0, wt = 0.0, as = 0.0, at = 0.0, wrel = 0.0, arel = 0.0;
  long notfinite = 0, inexact = 0;
  for (int i = 0; i < n; ++i) {
    const double xd = x[i];
    const double rs = 1.0 / (1.0 + std::exp(-xd)), rt = std::tanh(xd);
    if (!std::isfinite(s[i]) || !std::isfinite(t[i])) { ++notfinite; continue; }
    const double es = std::fabs((double)s[i] - rs), et = std::fabs((double)t[i] - rt);
    if (es > ws) { ws = es; as = xd; }
    if (et > wt) { wt = et; at = xd; }
    if (std::fabs(xd) < 1e-3 && rt != 0.0 && et / std::fabs(rt) > wrel) { wrel = et / std::fabs(rt); arel = xd; }
    if (std::fabs(xd) >= 90.0 && (s[i] != (xd > 0 ? 1.f : 0.f) || t[i] != (xd > 0 ? 1.f : -1.f))) ++inexact;
  }
  printf("gate_sigmoid over %d points: worst |err| / 2^-24 = %.4f at x = %.9g\n", n, ws / eps, as);
  printf("gate_tanh    over %d points: worst |err| / 2^-24 = %.4f at x = %.9g\n", n, wt / eps, at);
  printf("gate_tanh below |x| = 1e-3: worst |err| / |tanh x| = %.4g at x = %.9g\n", wrel, arel);
  printf("not finite: %ld; |x| >= 90 not exactly 0 / 1 / +-1: %ld; gate_tanh(0) = %.9g\n", notfinite, inexact,
         (double)t[(n_lin - 1) / 2]);          // x[(n_lin - 1) / 2] is exactly 0
  CK(hipFree(dx));
  CK(hipFree(ds));
  CK(hipFree(dt));
  return 0;
}
