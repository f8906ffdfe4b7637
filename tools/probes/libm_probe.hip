// Accuracy of the precise device functions the loss and optimiser kernels use (csrc/rowops.hip node_ce, csrc/contrastive.hip,
// csrc/optim.hip; same flags as build.py), against fp64: expf, logf, log1pf, sqrtf and the fp32 division.  These are the libm
// entry points, not the __expf / __logf intrinsics of exp_probe.hip and not rsqrtf (rsqrt_probe.hip).
// Every fp32 mantissa of the binades tests/test_loss_optim_gpu.py reaches:
//   expf    arguments l - max and the log-probabilities of node_ce (logits within +-30: (-64, 0]), -|x| of the contrastive pair
//           pass's log_sigmoid and -x of its sigmoid 1 / (1 + expf(-x)), |x| <= scale = 20, which is POSITIVE for the pairs with
//           x < 0: negative binades 2^-126 .. 2^6 (expf(-64) = 1.6e-28 is still a normal number), positive binades 2^-126 .. 2^5;
//           expf(0) exactly 1
//   logf    the two-class sum e0 + e1 in [1, 2]: binades 2^0 and 2^1 and the value 4; logf(1) exactly 0
//   log1pf  expf(-|x|) in (0, 1]: binades 2^-64 .. 2^0 and the value 1
//   sqrtf   Adam's second moment (1e-27 .. 1e6 and below: grad 1e-12 squared times 1 - beta2) and the squared row norms of the
//           contrastive loss (1e-6 .. 1e6): binades 2^-100 .. 2^30
//   a / b   b over every mantissa of three binades, a one of eight fixed mantissas (a quotient's relative error does not
//           depend on the exponents outside the subnormal range)
// Reported: worst relative error of each.  Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off
//   -o tools/probes/libm_probe tools/probes/libm_probe.hip        Run once, under a time limit (it takes a few seconds).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

enum { F_EXPF = 0, F_LOGF = 1, F_LOG1PF = 2, F_SQRTF = 3, F_DIV = 4 };

// arguments arrive at run time: no constant folding
__global__ void at_points(float zero, float one, float* out) {
  out[0] = expf(zero);
  out[1] = logf(one);
  out[2] = log1pf(zero);
  out[3] = sqrtf(zero);
  out[4] = log1pf(one);
}

// non-negative doubles order like their bit patterns
template <int F>
__global__ __launch_bounds__(256) void sweep(unsigned first_bits, unsigned count, float num, unsigned long long* worst, unsigned* worst_at) {
  double w = 0.0;
  unsigned at = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
    const unsigned bits = first_bits + i;
    const float x = __builtin_bit_cast(float, bits);
    const double xd = (double)x;
    double r, got;
    if (F == F_EXPF) { r = exp(xd); got = (double)expf(x); }
    else if (F == F_LOGF) { r = log(xd); got = (double)logf(x); }
    else if (F == F_LOG1PF) { r = log1p(xd); got = (double)log1pf(x); }
    else if (F == F_SQRTF) { r = sqrt(xd); got = (double)sqrtf(x); }
    else { r = (double)num / xd; got = (double)(num / x); }
    const double err = r != 0.0 ? fabs(got - r) / fabs(r) : (got != 0.0 ? 1.0 : 0.0);
    if (err > w) { w = err; at = bits; }
  }
  const unsigned long long wb = __builtin_bit_cast(unsigned long long, w);
  if (atomicMax(worst, wb) < wb) *worst_at = at;     // the argument is informative only (racy between equal maxima)
}

static unsigned long long* worst;
static unsigned* worst_at;

// worst relative error of function f over the binades [2^e0, 2^e1) of sign `neg`; `extra`: arguments past the last binade
static double run(int f, int e0, int e1, bool neg, const char* name, float num = 1.0f, unsigned extra = 0) {
  double all = 0.0;
  float all_at = 0.f;
  for (int e = e0; e < e1; ++e) {
    const unsigned first = ((unsigned)(e + 127) << 23) | (neg ? 0x80000000u : 0u);
    const unsigned count = (1u << 23) + (e == e1 - 1 ? extra : 0u);
    CHECK(hipMemset(worst, 0, 8));
    CHECK(hipMemset(worst_at, 0, 4));
    switch (f) {
      case F_EXPF: hipLaunchKernelGGL(sweep<F_EXPF>, 2048, 256, 0, 0, first, count, num, worst, worst_at); break;
      case F_LOGF: hipLaunchKernelGGL(sweep<F_LOGF>, 2048, 256, 0, 0, first, count, num, worst, worst_at); break;
      case F_LOG1PF: hipLaunchKernelGGL(sweep<F_LOG1PF>, 2048, 256, 0, 0, first, count, num, worst, worst_at); break;
      case F_SQRTF: hipLaunchKernelGGL(sweep<F_SQRTF>, 2048, 256, 0, 0, first, count, num, worst, worst_at); break;
      default: hipLaunchKernelGGL(sweep<F_DIV>, 2048, 256, 0, 0, first, count, num, worst, worst_at); break;
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
  printf("%-10s on %s[2^%d, 2^%d)%s: worst relative error %.6e = %.4f * 2^-24 (near x = %.9g)\n", name, neg ? "-" : "", e0, e1,
         extra ? " and the next value" : "", all, all * 16777216.0, (double)all_at);
  fflush(stdout);
  return all;
}

int main() {
  CHECK(hipMalloc(&worst, 8));
  CHECK(hipMalloc(&worst_at, 4));
  double ex = run(F_EXPF, -126, 6, true, "expf");
  const double exp_pos = run(F_EXPF, -126, 5, false, "expf");
  if (exp_pos > ex) ex = exp_pos;
  const double lg = run(F_LOGF, 0, 2, false, "logf", 1.0f, 1);
  const double l1 = run(F_LOG1PF, -64, 0, false, "log1pf", 1.0f, 1);
  const double sq = run(F_SQRTF, -100, 30, false, "sqrtf");
  const float nums[8] = {1.0f, 1.1f, 1.3333334f, 1.5f, 1.5707964f, 1.75f, 1.3591409f, 1.9999999f};
  const int bins[3] = {-30, 0, 20};
  double dv = 0.0, rc = 0.0;
  for (int k = 0; k < 8; ++k)
    for (int b = 0; b < 3; ++b) {
      char name[32];
      snprintf(name, sizeof name, "%.7g /", (double)nums[k]);
      const double d = run(F_DIV, bins[b], bins[b] + 1, false, name, nums[k]);
      if (d > dv) dv = d;
      if (k == 0 && d > rc) rc = d;
    }
  printf("worst relative errors: expf %.6e  logf %.6e  log1pf %.6e  sqrtf %.6e  1/x %.6e  a/b %.6e\n", ex, lg, l1, sq, rc, dv);
  float* z;
  float zh[5];
  CHECK(hipMalloc(&z, sizeof zh));
  hipLaunchKernelGGL(at_points, 1, 1, 0, 0, 0.0f, 1.0f, z);
  CHECK(hipMemcpy(zh, z, sizeof zh, hipMemcpyDeviceToHost));
  printf("expf(0) = %.9g (%s), logf(1) = %.9g (%s), log1pf(0) = %.9g (%s), sqrtf(0) = %.9g (%s), log1pf(1) = %.9g (fp32(ln 2) = %.9g)\n",
         (double)zh[0], zh[0] == 1.0f ? "exact" : "NOT exact", (double)zh[1], zh[1] == 0.0f ? "exact" : "NOT exact", (double)zh[2],
         zh[2] == 0.0f ? "exact" : "NOT exact", (double)zh[3], zh[3] == 0.0f ? "exact" : "NOT exact", (double)zh[4], (double)(float)log(2.0));
  return 0;
}
