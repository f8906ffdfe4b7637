// Accuracy of the device rsqrtf, as csrc/layernorm.hip compiles it (same flags as build.py), against 1 / sqrt in fp64: every
// fp32 mantissa of three pairs of binades — [2^-40, 2^-38) (eps = 1e-12 sits there), [1, 4) and [2^110, 2^112); the error
// pattern of x^-1/2 repeats every two binades.  Prints the worst relative error per range; tests/layernorm_reference.py
// takes its ε_rsqrt from this number (docs/experiment_log.md).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/probes/rsqrt_probe tools/probes/rsqrt_probe.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

// non-negative doubles order like their bit patterns
__global__ __launch_bounds__(256) void sweep(unsigned first_bits, unsigned count, unsigned long long* worst, unsigned* worst_at) {
  double w = 0.0;
  unsigned at = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
    const unsigned bits = first_bits + i;
    const float x = __builtin_bit_cast(float, bits);
    const double ref = 1.0 / sqrt((double)x);
    const double rel = fabs((double)rsqrtf(x) - ref) / ref;
    if (rel > w) { w = rel; at = bits; }
  }
  const unsigned long long wb = __builtin_bit_cast(unsigned long long, w);
  if (atomicMax(worst, wb) < wb) *worst_at = at;     // the argument is informative only (racy between equal maxima)
}

int main() {
  unsigned long long* worst;
  unsigned* worst_at;
  CHECK(hipMalloc(&worst, 8));
  CHECK(hipMalloc(&worst_at, 4));
  const int exps[3] = {-40, 0, 110};
  double all = 0.0;
  for (int k = 0; k < 3; ++k) {
    const unsigned first = (unsigned)(exps[k] + 127) << 23;
    CHECK(hipMemset(worst, 0, 8));
    CHECK(hipMemset(worst_at, 0, 4));
    hipLaunchKernelGGL(sweep, 2048, 256, 0, 0, first, 1u << 24, worst, worst_at);
    CHECK(hipGetLastError());
    unsigned long long wb;
    unsigned at;
    CHECK(hipMemcpy(&wb, worst, 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&at, worst_at, 4, hipMemcpyDeviceToHost));
    double w;
    float x;
    memcpy(&w, &wb, 8);
    memcpy(&x, &at, 4);
    printf("rsqrtf on [2^%d, 2^%d): worst relative error %.6e = %.4f * 2^-24 (near x = %.9g)\n", exps[k], exps[k] + 2, w, w * 16777216.0, (double)x);
    if (w > all) all = w;
  }
  printf("rsqrtf worst relative error overall %.6e\n", all);
  return 0;
}
