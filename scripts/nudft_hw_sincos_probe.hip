// Error of the gfx950 hardware sine / cosine (v_sin_f32 / v_cos_f32, argument in revolutions) against double
// precision, and of the NUDFT kernel's whole fp32 sincos_phase (range reduction + hardware pair + quadrant fix-up):
// the measurement behind the accuracy choice in pyxu_amd/csrc/nudft.hip.  Run from the repository
// root on an MI355X:
//
//   hipcc --offload-arch=gfx950 -O2 -o nudft_hw_sincos_probe scripts/nudft_hw_sincos_probe.hip && ./nudft_hw_sincos_probe
//
// Prints largest absolute errors in units of u = 2^-24: of the bare instructions over 2^26 arguments in [-1/2, 1/2]
// and in [-1/8, 1/8] revolutions, and of sincos_phase over 2^26 phases in [-P, P] for P = 4, 256, 3000, 10^5.
#include "../pyxu_amd/csrc/nudft.hip"

#include <cmath>
#include <cstdio>
#include <vector>

__host__ __device__ inline float arg_of(int i, int n, float half_width) {
  return half_width * (-1.0f + 2.0f * ((float)i / (float)(n - 1)));
}

// mode 0: the bare instructions on x revolutions; mode 1: sincos_phase on x radians
__global__ void probe(int mode, int n, float half_width, float* s, float* c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = arg_of(i, n, half_width);
  if (mode == 0) {
    s[i] = __builtin_amdgcn_sinf(x);
    c[i] = __builtin_amdgcn_cosf(x);
  } else {
    pxa::sincos_phase(x, s[i], c[i]);
  }
}

int main() {
  const int n = 1 << 26;
  float *ds, *dc;
  if (hipMalloc(&ds, n * sizeof(float)) != hipSuccess || hipMalloc(&dc, n * sizeof(float)) != hipSuccess) return 1;
  std::vector<float> s(n), c(n);
  const double two_pi = 6.283185307179586476925;
  const struct { int mode; float hw; } runs[] = {{0, 0.5f}, {0, 0.125f}, {1, 4.0f}, {1, 256.0f}, {1, 3000.0f}, {1, 1e5f}};
  for (const auto& r : runs) {
    hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, r.mode, n, r.hw, ds, dc);
    if (hipMemcpy(s.data(), ds, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    if (hipMemcpy(c.data(), dc, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    double es = 0, ec = 0;
    for (int i = 0; i < n; ++i) {
      const double x = (double)arg_of(i, n, r.hw) * (r.mode == 0 ? two_pi : 1.0);
      es = fmax(es, fabs((double)s[i] - sin(x)));
      ec = fmax(ec, fabs((double)c[i] - cos(x)));
    }
    printf("%s on [-%g, %g] %s: max abs err sin %.2f u, cos %.2f u (u = 2^-24, %d arguments)\n",
           r.mode == 0 ? "v_sin_f32 / v_cos_f32" : "sincos_phase", r.hw, r.hw, r.mode == 0 ? "revolutions" : "radians",
           es * 16777216.0, ec * 16777216.0, n);
  }
  (void)hipFree(ds);
  (void)hipFree(dc);
  return 0;
}
