// The device's expf (what the latent, KL and loss kernels of csrc/elem.hip call) against float64 exp on the host: worst
// |expf(x) - exp(x)| / (2^-24 exp(x)) over 40 000 001 evenly spaced x in [-87, 88] and 2^23 log-spaced |x| in
// [1e-6, 1] of either sign.  tests/elem_ref.py takes EXPF_MEASURED from this program's output.
// Build with the library's flags: hipcc --offload-arch=gfx950 -O3 -std=c++17 expf_sweep.hip -o expf_sweep
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ __launch_bounds__(256) void k(const float* x, float* t, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) t[i] = expf(x[i]);
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

int main() {
  const int n_lin = 40000001, n_log = 1 << 23, n = n_lin + 2 * n_log;
  std::vector<float> x(n), t(n);
  for (int i = 0; i < n_lin; ++i) x[i] = (float)(-87.0 + 175.0 * i / (n_lin - 1));
  for (int i = 0; i < n_log; ++i) {
    const float v = (float)std::pow(10.0, -6.0 + 6.0 * i / (n_log - 1));
    x[n_lin + 2 * i] = v;
    x[n_lin + 2 * i + 1] = -v;
  }
  float *dx, *dt;
  CK(hipMalloc(&dx, sizeof(float) * n));
  CK(hipMalloc(&dt, sizeof(float) * n));
  CK(hipMemcpy(dx, x.data(), sizeof(float) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dt, n);
  CK(hipGetLastError());
  CK(hipMemcpy(t.data(), dt, sizeof(float) * n, hipMemcpyDeviceToHost));
  double worst = 0.0, at = 0.0;
  for (int i = 0; i < n; ++i) {
    const double r = std::exp((double)x[i]), e = std::fabs((double)t[i] - r) / (std::ldexp(1.0, -24) * r);
    if (!(e <= worst)) { worst = e; at = x[i]; }      // a NaN or an infinity from the device counts as the worst
  }
  printf("expf over %d points: worst |err| / (2^-24 exp x) = %.4f at x = %.9g\n", n, worst, at);
  CK(hipFree(dx));
  CK(hipFree(dt));
  return 0;
}
