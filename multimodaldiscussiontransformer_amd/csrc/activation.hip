// mdt_act_fwd: the FFN activation as a launch of its own, for the kinds the fc1 GEMM epilogue has no form for
// (fairseq utils.get_activation_fn: relu, gelu_accurate / gelu_fast, tanh, linear; the erf GELU too, so that this
// two-launch route can be held against the fused epilogue).  One pass over the pre-activation writes
//   h = act(pre) * s        what fc2 reads
//   u = act'(pre) * s       what the backward GEMM multiplies by (MDT_EPI_MULAUX)
// with s the activation-dropout scale of the element (counter r * N + c of the site, as mdt_dropout), 1 without dropout.
// Memory bound: one 16-byte load and two 16-byte stores per lane and step; arithmetic in fp32, one rounding per store.
#include "common.hpp"

namespace mdt {

// act_pair<KIND> (common.hpp): the five kinds, one element.
// Flat grid-stride walk over the rows * (N / VN) vectors of the matrix (VN = 1: the scalar path, any N, stride and
// alignment).  (r, cv) = (row, vector of the row) advances by the grid's stride without a division per step.
// h may be pre: a lane reads its vector before it writes it, and no other lane touches it.
template <typename T, int VN, int KIND>
__global__ __launch_bounds__(256) void act_fwd_kernel(int64_t rows, int N, const T* pre, int64_t ld_pre, T* h, int64_t ld_h,
                                                      T* u, int64_t ld_u, DropCfg d) {
  const int64_t nv = N / VN;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t sr = stride / nv, sc = stride % nv;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t r = i0 / nv, cv = i0 % nv;
  const bool drop = d.thresh != 0;
  for (; r < rows; r += sr, cv += sc) {
    if (cv >= nv) {
      cv -= nv;
      if (++r >= rows) break;
    }
    const int c = (int)cv * VN;
    float x[VN], s[VN], hv[VN], uv[VN];
    if constexpr (VN == 1) {
      x[0] = to_f32(pre[r * ld_pre + c]);
      s[0] = drop ? drop_scale(d, (uint64_t)r * N + c) : 1.0f;
    } else {
      const Vec<T> v = *(const Vec<T>*)(pre + r * ld_pre + c);
#pragma unroll
      for (int e = 0; e < VN; ++e) x[e] = v.get(e);
#pragma unroll
      for (int e = 0; e < VN; e += 2) {      // N is even here, so every vector starts on an even counter
        if (drop) drop_scale2(d, (uint64_t)r * N + c + e, s[e], s[e + 1]);
        else s[e] = s[e + 1] = 1.0f;
      }
    }
#pragma unroll
    for (int e = 0; e < VN; ++e) act_pair<KIND>(x[e], s[e], hv[e], uv[e]);
    if constexpr (VN == 1) {
      h[r * ld_h + c] = from_f32<T>(hv[0]);
      if (u) u[r * ld_u + c] = from_f32<T>(uv[0]);
    } else {
      Vec<T> ho, uo;
#pragma unroll
      for (int e = 0; e < VN; ++e) { ho.set(e, hv[e]); uo.set(e, uv[e]); }
      *(Vec<T>*)(h + r * ld_h + c) = ho;
      if (u) *(Vec<T>*)(u + r * ld_u + c) = uo;
    }
  }
}

template <typename T, int VN, int KIND>
static int launch_act(hipStream_t st, int64_t rows, int N, const void* pre, int64_t ld_pre, void* h, int64_t ld_h, void* u,
                      int64_t ld_u, const DropCfg& d) {
  // enough 256-thread workgroups for one step each, at most 8 per compute unit (every SIMD full); the loop does the rest
  const int64_t want = (rows * (N / VN) + 255) / 256, cap = (int64_t)device_cus() * 8;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  return launch_route<act_fwd_kernel<T, VN, KIND>>(VN == 1 ? "act_scalar" : "act_vec", dim3(grid), dim3(256), 0, st, rows, N,
                                                   (const T*)pre, ld_pre, (T*)h, ld_h, (T*)u, ld_u, d);
}

template <typename T, int VN, typename... Args>
static int launch_act_kind(int kind, Args... a) {
  switch (kind) {
    case MDT_ACT_GELU: return launch_act<T, VN, MDT_ACT_GELU>(a...);
    case MDT_ACT_RELU: return launch_act<T, VN, MDT_ACT_RELU>(a...);
    case MDT_ACT_GELU_ACCURATE: return launch_act<T, VN, MDT_ACT_GELU_ACCURATE>(a...);
    case MDT_ACT_TANH: return launch_act<T, VN, MDT_ACT_TANH>(a...);
    default: return launch_act<T, VN, MDT_ACT_LINEAR>(a...);
  }
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_act_fwd(void* stream, int dtype, int kind, int64_t rows, int N, const void* pre, int64_t ld_pre, void* h,
                           int64_t ld_h, void* u, int64_t ld_u, float drop_p, uint64_t drop_seed) {
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "mdt_act_fwd: dtype %d", dtype);
  MDT_CHECK_ARG(kind >= MDT_ACT_GELU && kind <= MDT_ACT_LINEAR, "mdt_act_fwd: kind %d", kind);
  MDT_CHECK_ARG(rows >= 0 && N >= 0, "mdt_act_fwd: rows=%lld N=%d", (long long)rows, N);
  if (rows == 0 || N == 0) return MDT_OK;
  MDT_CHECK_ARG(pre && h, "mdt_act_fwd: null pointer");
  MDT_CHECK_ARG(ld_pre >= N && ld_h >= N && (!u || ld_u >= N), "mdt_act_fwd: row stride below N=%d (ld_pre=%lld ld_h=%lld ld_u=%lld)", N,
                (long long)ld_pre, (long long)ld_h, (long long)ld_u);
  MDT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "mdt_act_fwd: p=%f", drop_p);
  MDT_CHECK_ARG(rows * N < DROP_MAX_ELEMS, "mdt_act_fwd: site of %lld elements (limit 2^33)", (long long)(rows * N));
  hipStream_t st = (hipStream_t)stream;
  const DropCfg d = make_drop(drop_p, drop_seed);
  const bool vec = vec16_ok(dtype, N, {ld_pre, ld_h, u ? ld_u : 0}, {pre, h, u});
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return vec ? launch_act_kind<T, Vec<T>::N>(kind, st, rows, N, pre, ld_pre, h, ld_h, u, ld_u, d)
               : launch_act_kind<T, 1>(kind, st, rows, N, pre, ld_pre, h, ld_h, u, ld_u, d);
  });
}
