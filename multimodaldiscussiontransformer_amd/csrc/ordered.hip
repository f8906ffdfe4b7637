// Ordered (bit-reproducible) gradient reductions: the kernels behind the deterministic mode.  Every float-atomic site of the
// backward pass has a form here, or in the file of the kernel it belongs to, that writes per-workgroup partials with plain
// stores and ends in ONE fixed-order reducer, sum_slices: the result is a function of the operands alone — not of timing,
// of the workgroup that ran first, or of another tenant on the card.
//   sum_slices_kernel         out = (accumulate ? out : 0) + (((ws[0] + ws[1]) + ws[2]) + ...)       one thread per element
//   row_segment_sum_kernel    embedding gradients from CSR segments, one thread per column           (mdt_row_segment_sum_f32)
//   attn_bias_hist_kernel     structural-bias histograms of a dense dS, one workgroup per (seq, h)   (mdt_attn_bias_grad_ordered)
// The ordered split-K GEMM, LayerNorm backward and column sums live beside their kernels (gemm.hip, gemm_wgrad.hip,
// layernorm.hip, elementwise.hip colsum_kernel<.., ORD>).
// The build runs with -ffp-contract=off: every add below is one fp32 rounding, no multiply is fused into it.
#include "common.hpp"

namespace mdt {

__global__ __launch_bounds__(256) void sum_slices_kernel(int64_t rows, int64_t cols, int slices, const float* __restrict__ ws,
                                                         int64_t ld_ws, int64_t slice_stride, float* __restrict__ out,
                                                         int64_t ldo, int accumulate) {
  const int64_t n = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols, c = i - r * cols;
    const float* w = ws + r * ld_ws + c;
    float s = w[0];
    for (int z = 1; z < slices; ++z) s += w[(int64_t)z * slice_stride];
    float* o = out + r * ldo + c;
    *o = (accumulate ? *o : 0.f) + s;       // the old value joins last
  }
}

int sum_slices_f32(hipStream_t st, int64_t rows, int64_t cols, int slices, const float* ws, int64_t ld_ws, int64_t slice_stride,
                   float* out, int64_t ldo, int accumulate) {
  if (rows <= 0 || cols <= 0) return MDT_OK;
  MDT_CHECK_ARG(slices >= 1 && ws && out, "sum_slices: no slices / null pointer");
  MDT_CHECK_ARG(ld_ws >= cols && ldo >= cols, "sum_slices: row stride shorter than a row");
  const int64_t blocks = (rows * cols + 255) / 256;
  hipLaunchKernelGGL(sum_slices_kernel, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, st, rows, cols, slices, ws, ld_ws,
                     slice_stride, out, ldo, accumulate);
  return check_launch("sum_slices");
}

// One thread per (segment, column).  Sources of a segment are taken in the order `order` lists them, in chunks of
// SEG_CHUNK: a chunk is summed left to right, the chunk sums are added left to right, the table's old value joins last.
constexpr int SEG_CHUNK = 64;
template <typename T>
__global__ __launch_bounds__(256) void row_segment_sum_kernel(int D, float* __restrict__ table, int64_t ldt,
                                                              const int32_t* __restrict__ seg_row, const int32_t* __restrict__ seg_off,
                                                              const int32_t* __restrict__ order, const T* __restrict__ src,
                                                              int64_t lds_, int64_t s_stride, int64_t s_off) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  const int seg = blockIdx.x;
  const int64_t t = seg_row[seg];
  const int o0 = seg_off[seg], o1 = seg_off[seg + 1];
  if (c >= D || t < 0 || o0 >= o1) return;
  float total = 0.f;
  for (int b = o0; b < o1; b += SEG_CHUNK) {
    const int e = b + SEG_CHUNK < o1 ? b + SEG_CHUNK : o1;
    float cs = to_f32(src[((int64_t)order[b] * s_stride + s_off) * lds_ + c]);
    for (int o = b + 1; o < e; ++o) cs += to_f32(src[((int64_t)order[o] * s_stride + s_off) * lds_ + c]);
    total = b == o0 ? cs : total + cs;
  }
  float* dst = table + t * ldt + c;
  *dst = *dst + total;
}

// One workgroup per (sequence, head): thread t owns elements t, t + 256, ... of the S x S matrix dS[seq, h] (row-major,
// element q * S + key) and adds them, in that order, to its private histogram hist[bin][t]; bins 0 .. num_spatial - 1 are
// the spatial_pos table rows (bin 0, the padding row, receives nothing), bin num_spatial the graph token (q == 0 or
// key == 0).  The 256 histograms are folded by halving: hist[.][t] += hist[.][t + 128], then + 64, ... + 1.
// ws[seq][bin][h] receives the fold.
// The workgroup has T = blockDim.x threads (attn_hist_threads: 256 while the histograms fit 96 KiB, else the largest power of
// two that does); read "256" above as T, "128" as T / 2.
__global__ __launch_bounds__(256) void attn_bias_hist_kernel(int S, int H, int num_spatial, const float* __restrict__ dS,
                                                             const int32_t* __restrict__ spatial_pos, float* __restrict__ ws) {
  extern __shared__ float hist[];          // [bins][T]
  const int bins = num_spatial + 1;
  const int T = blockDim.x;
  const int seq = blockIdx.x / H, h = blockIdx.x - seq * H;
  const int tid = threadIdx.x;
  for (int b = 0; b < bins; ++b) hist[b * T + tid] = 0.f;
  const float* d = dS + (int64_t)blockIdx.x * S * S;
  const int32_t* sp = spatial_pos + (int64_t)seq * (S - 1) * (S - 1);
  for (int e = tid; e < S * S; e += T) {
    const int q = e / S, key = e - q * S;
    int bin = num_spatial;
    if (q >= 1 && key >= 1) bin = sp[(q - 1) * (S - 1) + (key - 1)];
    if (bin > 0 && bin < bins) hist[bin * T + tid] += d[e];      // nn.Embedding(padding_idx=0): row 0 gets no gradient
  }
  for (int stride = T / 2; stride >= 1; stride >>= 1) {
    __syncthreads();
    for (int i = tid; i < bins * stride; i += T) {
      const int b = i / stride, t = i - b * stride;
      hist[b * T + t] += hist[b * T + t + stride];
    }
  }
  __syncthreads();
  for (int b = tid; b < bins; b += T) ws[((int64_t)seq * bins + b) * H + h] = hist[b * T];
}

// Threads (= private histograms) of a workgroup for num_spatial table rows: 256 for up to 95 rows, then 128 (191), 64 (383),
// 32 (767) — (num_spatial + 1) x T floats stay within 96 KiB; 0: more rows than that.
static int attn_hist_threads(int num_spatial) {
  for (int t = 256; t >= 32; t >>= 1)
    if ((size_t)(num_spatial + 1) * t * sizeof(float) <= 96 * 1024) return t;
  return 0;
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_sum_slices_f32(void* stream, int64_t rows, int64_t cols, int slices, const float* ws, int64_t ld_ws,
                                  int64_t slice_stride, float* out, int64_t ldo, int accumulate) {
  MDT_CHECK_ARG(rows >= 0 && cols >= 0, "sum_slices: negative shape");
  return sum_slices_f32((hipStream_t)stream, rows, cols, slices, ws, ld_ws, slice_stride, out, ldo, accumulate);
}

extern "C" int mdt_row_segment_sum_f32(void* stream, int dtype, int nseg, int D, float* table, int64_t ldt, const int32_t* seg_row,
                                       const int32_t* seg_off, const int32_t* order, const void* src, int64_t lds_,
                                       int64_t s_stride, int64_t s_off) {
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "mdt_row_segment_sum: dtype %d", dtype);
  if (nseg <= 0 || D <= 0) return MDT_OK;
  MDT_CHECK_ARG(table && seg_row && seg_off && order && src, "mdt_row_segment_sum: null pointer");
  MDT_CHECK_ARG((D + 255) / 256 <= 65535, "mdt_row_segment_sum: D=%d too wide", D);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nseg, (unsigned)((D + 255) / 256));
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<row_segment_sum_kernel<T>>("row_segment_sum", grid, 256, st, D, table, ldt, seg_row, seg_off, order, (const T*)src, lds_, s_stride, s_off);
  });
}

extern "C" size_t mdt_attn_bias_grad_ordered_workspace_bytes(int nseq, int H, int num_spatial) {
  if (nseq <= 0 || H <= 0 || num_spatial < 0) return 0;
  return (size_t)nseq * (size_t)(num_spatial + 1) * (size_t)H * sizeof(float);
}

extern "C" int mdt_attn_bias_grad_ordered(void* stream, int nseq, int S, int H, int num_spatial, const float* dS,
                                          const int32_t* spatial_pos, float* d_sp_table, float* d_virt, void* workspace,
                                          size_t workspace_bytes) {
  if (nseq <= 0 || (!d_sp_table && !d_virt)) return MDT_OK;
  MDT_CHECK_ARG(S >= 1 && H >= 1 && num_spatial >= 1 && dS && (spatial_pos || S == 1), "mdt_attn_bias_grad_ordered: bad shape / null pointer");
  const int bins = num_spatial + 1;
  const int threads = attn_hist_threads(num_spatial);
  if (!threads) MDT_UNSUPPORTED("mdt_attn_bias_grad_ordered: the histograms of %d table rows do not fit a workgroup's LDS (at most 767 rows)", num_spatial);
  const size_t lds = (size_t)bins * threads * sizeof(float);
  const size_t need = mdt_attn_bias_grad_ordered_workspace_bytes(nseq, H, num_spatial);
  MDT_CHECK_ARG(workspace && workspace_bytes >= need, "mdt_attn_bias_grad_ordered: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  if (int e = launch_route<attn_bias_hist_kernel>("bias_hist", dim3((unsigned)(nseq * H)), dim3((unsigned)threads), lds, st, S, H, num_spatial, dS, spatial_pos, (float*)workspace))
    return e;
  const float* ws = (const float*)workspace;
  const int64_t slice = (int64_t)bins * H;
  if (d_sp_table)
    if (int e = sum_slices_f32(st, num_spatial, H, nseq, ws, H, slice, d_sp_table, H, 1)) return e;
  if (d_virt)
    if (int e = sum_slices_f32(st, 1, H, nseq, ws + (int64_t)num_spatial * H, H, slice, d_virt, H, 1)) return e;
  return MDT_OK;
}
