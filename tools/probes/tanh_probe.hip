// Accuracy of the device tanhf, as csrc/rowops.hip compiles it (same flags as build.py), against tanh in fp64: every
// bf16-representable argument in [-12, 12] (what the bf16 pooler feeds it) and 2^20 evenly spaced fp32 arguments over the same
// range (tanhf is 1 to the last bit from |x| = 9.02 on; the pooler pre-activations of the tests stay below 10).  Prints the
// worst relative error per set; tests/rowops_reference.py takes its ε_tanh from this number (docs/experiment_log.md).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/probes/tanh_probe tools/probes/tanh_probe.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

constexpr float RANGE = 12.0f;

// set 0: i is a bf16 bit pattern (the upper half of an fp32); set 1: i of `count` points evenly spaced over [-RANGE, RANGE]
__device__ __forceinline__ bool argument(int set, unsigned i, unsigned count, float* x) {
  if (set == 0) {
    *x = __builtin_bit_cast(float, i << 16);
    return fabsf(*x) <= RANGE;                       // false for NaN too
  }
  *x = (float)(-(double)RANGE + 2.0 * (double)RANGE * (double)i / (double)(count - 1));
  return true;
}

// non-negative doubles order like their bit patterns
__global__ __launch_bounds__(256) void sweep(int set, unsigned count, unsigned long long* worst, unsigned* worst_at, unsigned* used) {
  double w = 0.0;
  unsigned at = 0, n = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
    float x;
    if (!argument(set, i, count, &x)) continue;
    ++n;
    const double ref = tanh((double)x);
    if (ref == 0.0) continue;                        // tanhf(±0) = ±0 is checked by the tests, not as a relative error
    const double rel = fabs((double)tanhf(x) - ref) / fabs(ref);
    if (rel > w) { w = rel; at = __builtin_bit_cast(unsigned, x); }
  }
  atomicAdd(used, n);
  const unsigned long long wb = __builtin_bit_cast(unsigned long long, w);
  if (atomicMax(worst, wb) < wb) *worst_at = at;     // the argument is informative only (racy between equal maxima)
}

int main() {
  unsigned long long* worst;
  unsigned *worst_at, *used;
  CHECK(hipMalloc(&worst, 8));
  CHECK(hipMalloc(&worst_at, 4));
  CHECK(hipMalloc(&used, 4));
  const unsigned counts[2] = {1u << 16, 1u << 20};
  const char* names[2] = {"every bf16 value", "2^20 evenly spaced fp32 values"};
  double all = 0.0;
  for (int k = 0; k < 2; ++k) {
    CHECK(hipMemset(worst, 0, 8));
    CHECK(hipMemset(worst_at, 0, 4));
    CHECK(hipMemset(used, 0, 4));
    hipLaunchKernelGGL(sweep, 256, 256, 0, 0, k, counts[k], worst, worst_at, used);
    CHECK(hipGetLastError());
    unsigned long long wb;
    unsigned at, n;
    CHECK(hipMemcpy(&wb, worst, 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&at, worst_at, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&n, used, 4, hipMemcpyDeviceToHost));
    double w;
    float x;
    memcpy(&w, &wb, 8);
    memcpy(&x, &at, 4);
    printf("tanhf on [-12, 12], %s (%u arguments): worst relative error %.6e = %.4f * 2^-24 (near x = %.9g)\n", names[k], n, w,
           w * 16777216.0, (double)x);
    if (w > all) all = w;
  }
  printf("tanhf worst relative error overall %.6e = %.4f * 2^-24\n", all, all * 16777216.0);
  return 0;
}
