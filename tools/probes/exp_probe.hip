// Accuracy of the device functions the attention kernels build softmax from (csrc/attention*.hip, same flags as build.py), against
// fp64: __expf (fp32 kernels, the v1 bf16 kernels, the key-chunked path, head weights), __builtin_amdgcn_exp2f (v2 forward, v2 - v5
// backward), and the three that make lse and 1 / sum: __logf, __builtin_amdgcn_logf (log2) and __builtin_amdgcn_rcpf.
// Every fp32 mantissa of the arguments tests/test_attention_routes_gpu.py reaches: score - max and score - lse lie in (-64, 1)
// (exponents 2^-10 .. 2^6 negative, 2^-10 .. 1 positive; below 2^-10 both functions return 1 to within u), row sums in [1, 512).
// __expf(x) is exp2 of the fp32 product x log2(e), whose rounding alone is worth |x| u: the error is reported per unit of
// max(1, |x|), which is what tests/attention_reference.py multiplies it by (docs/experiment_log.md).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o tools/probes/exp_probe tools/probes/exp_probe.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

enum { F_EXPF = 0, F_EXP2 = 1, F_LOGF = 2, F_LOG2 = 3, F_RCP = 4 };

// exp of 0 must be exactly 1: the key-chunked forward multiplies by it at every key that is no new maximum
__global__ void at_zero(float zero, float* out) { out[0] = __expf(zero); out[1] = __builtin_amdgcn_exp2f(zero); }

// non-negative doubles order like their bit patterns
template <int F>
__global__ __launch_bounds__(256) void sweep(unsigned first_bits, unsigned count, unsigned long long* worst, unsigned* worst_at) {
  double w = 0.0;
  unsigned at = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
    const unsigned bits = first_bits + i;
    const float x = __builtin_bit_cast(float, bits);
    const double xd = (double)x, ax = fabs(xd) > 1.0 ? fabs(xd) : 1.0;
    double err;
    if (F == F_EXPF) { const double r = exp(xd); err = fabs((double)__expf(x) - r) / r / ax; }
    else if (F == F_EXP2) { const double r = exp2(xd); err = fabs((double)__builtin_amdgcn_exp2f(x) - r) / r / ax; }
    else if (F == F_LOGF) err = fabs((double)__logf(x) - log(xd));                          // absolute: it is added to the row maximum
    else if (F == F_LOG2) err = fabs((double)__builtin_amdgcn_logf(x) - log2(xd));
    else { const double r = 1.0 / xd; err = fabs((double)__builtin_amdgcn_rcpf(x) - r) / r; }
    if (err > w) { w = err; at = bits; }
  }
  const unsigned long long wb = __builtin_bit_cast(unsigned long long, w);
  if (atomicMax(worst, wb) < wb) *worst_at = at;     // the argument is informative only (racy between equal maxima)
}

static unsigned long long* worst;
static unsigned* worst_at;

// worst error of function f over the binades [2^e0, 2^e1) of sign `neg`
static double run(int f, int e0, int e1, bool neg, const char* name, const char* unit) {
  double all = 0.0;
  float all_at = 0.f;
  for (int e = e0; e < e1; ++e) {
    const unsigned first = ((unsigned)(e + 127) << 23) | (neg ? 0x80000000u : 0u);
    CHECK(hipMemset(worst, 0, 8));
    CHECK(hipMemset(worst_at, 0, 4));
    switch (f) {
      case F_EXPF: hipLaunchKernelGGL(sweep<F_EXPF>, 2048, 256, 0, 0, first, 1u << 23, worst, worst_at); break;
      case F_EXP2: hipLaunchKernelGGL(sweep<F_EXP2>, 2048, 256, 0, 0, first, 1u << 23, worst, worst_at); break;
      case F_LOGF: hipLaunchKernelGGL(sweep<F_LOGF>, 2048, 256, 0, 0, first, 1u << 23, worst, worst_at); break;
      case F_LOG2: hipLaunchKernelGGL(sweep<F_LOG2>, 2048, 256, 0, 0, first, 1u << 23, worst, worst_at); break;
      default: hipLaunchKernelGGL(sweep<F_RCP>, 2048, 256, 0, 0, first, 1u << 23, worst, worst_at); break;
    }
    CHECK(hipGetLastError());
    unsigned long long wb;
    unsigned at;
    CHECK(hipMemcpy(&wb, worst, 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&at, worst_at, 4, hipMemcpyDeviceToHost));
    double w;
    float x;
    memcpy(&w, &wb, 8);
    memcpy(&x, &at, 4);
    if (w > all) { all = w; all_at = x; }
  }
  printf("%-24s on %s[2^%d, 2^%d): worst %s %.6e = %.4f * 2^-24 (near x = %.9g)\n", name, neg ? "-" : "", e0, e1, unit, all,
         all * 16777216.0, (double)all_at);
  return all;
}

int main() {
  CHECK(hipMalloc(&worst, 8));
  CHECK(hipMalloc(&worst_at, 4));
  const char* rel = "relative error / max(1, |x|)";
  double e1 = run(F_EXPF, -10, 6, true, "__expf", rel);
  double e2 = run(F_EXPF, -10, 0, false, "__expf", rel);
  double e3 = run(F_EXP2, -10, 6, true, "__builtin_amdgcn_exp2f", rel);
  double e4 = run(F_EXP2, -10, 1, false, "__builtin_amdgcn_exp2f", rel);
  const double l1 = run(F_LOGF, 0, 9, false, "__logf", "absolute error");
  const double l2 = run(F_LOG2, 0, 9, false, "__builtin_amdgcn_logf", "absolute error");
  const double r = run(F_RCP, 0, 9, false, "__builtin_amdgcn_rcpf", "relative error");
  if (e2 > e1) e1 = e2;
  if (e4 > e3) e3 = e4;
  printf("exp worst overall: __expf %.6e, exp2 %.6e per max(1, |x|); log: __logf %.6e, log2 %.6e absolute; rcp %.6e relative\n", e1,
         e3, l1, l2, r);
  float* z;
  float zh[2];
  CHECK(hipMalloc(&z, 8));
  hipLaunchKernelGGL(at_zero, 1, 1, 0, 0, 0.0f, z);      // the argument arrives at run time: no constant folding
  CHECK(hipMemcpy(zh, z, 8, hipMemcpyDeviceToHost));
  printf("__expf(0) = %.9g (%s), exp2(0) = %.9g (%s)\n", (double)zh[0], zh[0] == 1.0f ? "exact" : "NOT exact", (double)zh[1], zh[1] == 1.0f ? "exact" : "NOT exact");
  return 0;
}
