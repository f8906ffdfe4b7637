// Label-smoothed / focal objective of the two-class node classifier (criterion node_cross_entropy with --label-smoothing
// or --focal-gamma): the weighted cross entropy of rowops.hip's node_ce_kernel with two more knobs, its plain weighted NLL
// beside it (the log's nll_loss, comparable between runs with different objectives), the same four counters and
// dL / d logits.  One small launch per micro-batch, one workgroup, like node_ce_kernel.
#include <cmath>

#include "common.hpp"

namespace mdt {

// fp16 round-trip (round to nearest even), as node_ce_kernel rounds the logits and the class weights
__device__ __forceinline__ float objective_round_f16(float v) { return (float)(_Float16)v; }

// A labelled row, y its target and o = 1 - y.  With fp16_loss the two logits and the two class weights are rounded to fp16
// first (what the reference's .type(torch.HalfTensor) does to them); everything after that is plain fp32 — there is no torch
// Half kernel to imitate for these objectives, so no intermediate half rounding and no half cascade.
//   lp = log_softmax(l),  q = exp(lp_y),  r = exp(lp_o) = 1 - q
//   nll  = -(w_y lp_y)
//   f    = expf(gamma lp_o)                      = (1 - q)^gamma without powf and without the cancellation of 1 - q; 1 at gamma = 0
//   loss = (1 - eps) (f nll) + (eps / 2) (nll - w_o lp_o)              the focal factor modulates the hard-target term only
//   with A = (1 - eps) (w_y (f (r - (gamma q) lp_y))), sw = w_0 + w_1  (f is differentiated, not detached):
//   dL / d l_o =  A + (eps / 2) (sw r - w_o)
//   dL / d l_y = -A + (eps / 2) (sw q - w_y)
// Predictions and counters follow node_ce_kernel's rule for the same fp16_loss (the half-rounded softmax, ties to index 0).
// Sums: thread t adds the rows t, t + 256, ... in that order, thread 0 then adds the 256 partial sums in thread order — a fixed
// order without float atomics, so two launches on the same inputs give the same bits.
template <typename T>
__global__ __launch_bounds__(256) void node_objective_kernel(int nlab, const T* logits, const int32_t* rows, const int32_t* targets,
                                                             float w_neg, float w_pos, int fp16_loss, float eps, float gamma,
                                                             float grad_scale, float* out, int32_t* counters, T* dlogits) {
  __shared__ float s_loss[256];
  __shared__ float s_nll[256];
  __shared__ int s_cnt[4][256];
  float wn = w_neg, wp = w_pos;
  if (fp16_loss) { wn = objective_round_f16(wn); wp = objective_round_f16(wp); }
  const float ome = 1.0f - eps, he = eps * 0.5f, sw = wn + wp;
  float loss = 0.f, nll_sum = 0.f;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int i = threadIdx.x; i < nlab; i += 256) {
    const int64_t row = rows[i];
    const int y = targets[i] != 0;
    float l0 = to_f32(logits[row * 2]), l1 = to_f32(logits[row * 2 + 1]);
    if (fp16_loss) { l0 = objective_round_f16(l0); l1 = objective_round_f16(l1); }
    const float m = fmaxf(l0, l1);
    const float a0 = l0 - m, a1 = l1 - m;
    const float e0 = expf(a0), e1 = expf(a1);
    const float ls = logf(e0 + e1);
    const float lp0 = a0 - ls, lp1 = a1 - ls;
    int pred;
    if (fp16_loss) {
      const float inv = 1.0f / (e0 + e1);
      pred = (objective_round_f16(e1 * inv) > objective_round_f16(e0 * inv)) ? 1 : 0;      // ties -> index 0 like torch.argmax
    } else {
      pred = (l1 > l0) ? 1 : 0;
    }
    const float lpy = y ? lp1 : lp0, lpo = y ? lp0 : lp1;
    const float wy = y ? wp : wn, wo = y ? wn : wp;
    const float nll = -(wy * lpy);
    const float f = expf(gamma * lpo);
    loss += ome * (f * nll) + he * (nll - wo * lpo);
    nll_sum += nll;
    c0 += (pred == y);
    c1 += (pred == y && pred == 1);
    c2 += (y == 1);
    c3 += (pred == 1);
    if (dlogits) {
      const float q = expf(lpy), r = expf(lpo);
      const float A = ome * (wy * (f * (r - (gamma * q) * lpy)));
      const float go = A + he * (sw * r - wo);
      const float gy = -A + he * (sw * q - wy);
      dlogits[row * 2 + y] = from_f32<T>(gy * grad_scale);
      dlogits[row * 2 + (1 - y)] = from_f32<T>(go * grad_scale);
    }
  }
  s_loss[threadIdx.x] = loss;
  s_nll[threadIdx.x] = nll_sum;
  s_cnt[0][threadIdx.x] = c0; s_cnt[1][threadIdx.x] = c1; s_cnt[2][threadIdx.x] = c2; s_cnt[3][threadIdx.x] = c3;
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f, N = 0.f;
    int t0 = 0, t1 = 0, t2 = 0, t3 = 0;
    for (int i = 0; i < 256; ++i) { L += s_loss[i]; N += s_nll[i]; t0 += s_cnt[0][i]; t1 += s_cnt[1][i]; t2 += s_cnt[2][i]; t3 += s_cnt[3][i]; }
    out[0] = L;
    out[1] = N;
    counters[0] = t0; counters[1] = t1; counters[2] = t2; counters[3] = t3;
  }
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_node_objective(void* stream, int dtype, int64_t M, int nlab, const void* logits, const int32_t* rows,
                                  const int32_t* targets, float w_neg, float w_pos, int fp16_loss, float label_smoothing,
                                  float focal_gamma, float grad_scale, float* out, int32_t* counters, void* dlogits) {
  MDT_CHECK_ARG(logits && out && counters, "node_objective: null pointer");
  MDT_CHECK_ARG(M >= 0 && nlab >= 0, "node_objective: negative M (%lld) or nlab (%d)", (long long)M, nlab);
  MDT_CHECK_ARG(nlab == 0 || (rows && targets), "node_objective: null rows / targets");
  // written so that a NaN fails them
  MDT_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 1.f, "node_objective: label_smoothing %g is not in [0, 1)", (double)label_smoothing);
  MDT_CHECK_ARG(focal_gamma >= 0.f && std::isfinite(focal_gamma), "node_objective: focal_gamma %g is not finite and >= 0", (double)focal_gamma);
  if (dtype != MDT_F32 && dtype != MDT_BF16) MDT_UNSUPPORTED("node_objective: dtype %d is neither MDT_F32 nor MDT_BF16", dtype);
  hipStream_t st = (hipStream_t)stream;
  if (dlogits && M > 0) {
    if (hipMemsetAsync(dlogits, 0, (size_t)M * 2 * dtype_size(dtype), st) != hipSuccess) {
      (void)hipGetLastError();
      set_error("node_objective: memset failed");
      return MDT_ERR_LAUNCH;
    }
  }
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<node_objective_kernel<T>>("node_objective", 1, 256, st, nlab, (const T*)logits, rows, targets, w_neg, w_pos, fp16_loss,
                                                  label_smoothing, focal_gamma, grad_scale, out, counters, (T*)dlogits);
  });
}
