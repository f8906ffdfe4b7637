// Memory-bound kernels that are neither a GEMM nor a one-wave-per-row mover: column sums (atomic and ordered), dropout and
// its keep mask, dtype casts and the 2-D transpose.  They lived in gemm.hip (and colsum's ordered form in ordered.hip) for
// no better reason than having been written there.  A file of their own rather than rowops.hip: rowops.hip is the family
// with one wavefront per row and no LDS; colsum reduces over rows through LDS, transpose2d works on 32 x 32 tiles, cast and
// dropout_mask are flat — only dropout walks rows, and it stays beside the mask kernel that shares its counters.
// Each scalar / vector pair is ONE kernel templated on VN (1: any width, stride and alignment; Vec<T>::N: 16-byte access),
// as act_fwd_kernel (activation.hip) is; the arithmetic order of either form is that of the other.
// The build runs with -ffp-contract=off: every add below is one fp32 rounding, no multiply is fused into it.
#include "common.hpp"

namespace mdt {

// Column sums of X[M, N] (each row weighted by row_weight[r] where given; every term w * x rounded before its add).
// Workgroup = 64 lanes x 4 row lanes; a lane owns VN consecutive columns; grid.x = column groups, grid.y = blocks of
// rows_per_block rows.  Row lane j adds rows j, j + 4, ... of the block in ascending order, the block's partial is
// ((lane 0 + lane 1) + lane 2) + lane 3.
//   ORD = false: the partial is added to out[col] with a float atomic (mdt_colsum)
//   ORD = true:  the partial is stored to out[block][col], a fixed tree (mdt_colsum_ordered: blocks of CS_BLOCK_ROWS rows,
//                folded by sum_slices in block order)
constexpr int CS_BLOCK_ROWS = 256;
template <typename T, int VN, bool ORD>
__global__ __launch_bounds__(256) void colsum_kernel(int64_t M, int64_t N, const T* X, int64_t ldx, float* out, int rows_per_block,
                                                     const int32_t* row_weight) {
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * VN;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < M) ? r0 + rows_per_block : M;
  float acc[VN];
#pragma unroll
  for (int e = 0; e < VN; ++e) acc[e] = 0.f;
  if (c < N)
    for (int64_t r = r0 + rl; r < r1; r += 4) {
      const float w = row_weight ? (float)row_weight[r] : 1.f;
      if constexpr (VN == 1) {
        acc[0] += w * to_f32(X[r * ldx + c]);
      } else {
        const Vec<T> v = *(const Vec<T>*)(X + r * ldx + c);
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[e] += w * v.get(e);
      }
    }
  __shared__ float red[4][64 * VN];
#pragma unroll
  for (int e = 0; e < VN; ++e) red[rl][lane * VN + e] = acc[e];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * VN; i += 256) {
    const int64_t col = (int64_t)blockIdx.x * 64 * VN + i;
    if (col < N) {
      const float s = red[0][i] + red[1][i] + red[2][i] + red[3][i];
      if constexpr (ORD) out[(int64_t)blockIdx.y * N + col] = s;
      else atomicAdd(out + col, s);
    }
  }
}

// y = x * keep / (1 - p): element (r, c) takes counter r * D + c of the site; one wave per row, grid-stride over rows.
// The vector form needs D even, so that every vector starts on an even counter and one hash serves two elements.
template <typename T, int VN>
__global__ __launch_bounds__(256) void dropout_kernel(int64_t rows, int D, const T* x, int64_t ldx, T* y, int64_t ldy, DropCfg d) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4)
    for (int c = lane * VN; c < D; c += 64 * VN) {
      if constexpr (VN == 1) {
        y[r * ldy + c] = from_f32<T>(to_f32(x[r * ldx + c]) * drop_scale(d, (uint64_t)r * D + c));
      } else {
        const Vec<T> v = *(const Vec<T>*)(x + r * ldx + c);
        Vec<T> o;
#pragma unroll
        for (int e = 0; e < VN; e += 2) {
          float s0, s1;
          drop_scale2(d, (uint64_t)r * D + c + e, s0, s1);
          o.set(e, v.get(e) * s0);
          o.set(e + 1, v.get(e + 1) * s1);
        }
        *(Vec<T>*)(y + r * ldy + c) = o;
      }
    }
}
__global__ void dropout_mask_kernel(int64_t n, DropCfg d, uint8_t* mask) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    mask[i] = drop_scale(d, (uint64_t)i) != 0.f;
}

template <typename TS, typename TD>
__global__ void cast_kernel(int64_t n, const TS* s, TD* d) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    d[i] = from_f32<TD>(to_f32(s[i]));
}

template <typename TS, typename TD>
__global__ __launch_bounds__(256) void transpose_kernel(int64_t rows, int64_t cols, const TS* s, int64_t lds_, TD* d,
                                                        int64_t ldd) {
  __shared__ float tile[32][33];
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8)
    if (r0 + i < rows && c0 + tx < cols) tile[i][tx] = to_f32(s[(r0 + i) * lds_ + c0 + tx]);
  __syncthreads();
  for (int i = ty; i < 32; i += 8)
    if (c0 + i < cols && r0 + tx < rows) d[(c0 + i) * ldd + r0 + tx] = from_f32<TD>(tile[tx][i]);
}

template <typename T, int VN, bool ORD>
static int launch_colsum(const char* name, hipStream_t st, dim3 grid, int64_t M, int64_t N, const void* X, int64_t ldx, float* out,
                         int rows_per_block, const int32_t* row_weight) {
  return launch_plain<colsum_kernel<T, VN, ORD>>(name, grid, 256, st, M, N, (const T*)X, ldx, out, rows_per_block, row_weight);
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_colsum(void* stream, int dtype, int64_t M, int64_t N, const void* X, int64_t ldx, float* out,
                          const int32_t* row_weight) {
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "mdt_colsum: dtype %d", dtype);
  if (M == 0 || N == 0) return MDT_OK;           // nothing to add (an empty X has no address)
  MDT_CHECK_ARG(X && out, "mdt_colsum: null pointer");
  note_float_atomic_launch();
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (vec16_ok(dtype, N, {ldx}, {X})) {
      constexpr int VN = Vec<T>::N;
      const unsigned gx = (unsigned)((N + 64 * VN - 1) / (64 * VN));
      int64_t chunks = 2048 / gx;
      if (chunks < 1) chunks = 1;
      int rows_per_block = (int)((M + chunks - 1) / chunks);
      if (rows_per_block < 32) rows_per_block = 32;
      const dim3 grid(gx, (unsigned)((M + rows_per_block - 1) / rows_per_block));
      return launch_colsum<T, VN, false>("colsum_vec", st, grid, M, N, X, ldx, out, rows_per_block, row_weight);
    }
    const int rows_per_block = 512;
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((M + rows_per_block - 1) / rows_per_block));
    return launch_colsum<T, 1, false>("colsum", st, grid, M, N, X, ldx, out, rows_per_block, row_weight);
  });
}

extern "C" size_t mdt_colsum_ordered_workspace_bytes(int64_t M, int64_t N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)((M + CS_BLOCK_ROWS - 1) / CS_BLOCK_ROWS) * (size_t)N * sizeof(float);
}

extern "C" int mdt_colsum_ordered(void* stream, int dtype, int64_t M, int64_t N, const void* X, int64_t ldx, float* out,
                                  const int32_t* row_weight, void* workspace, size_t workspace_bytes) {
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "mdt_colsum_ordered: dtype %d", dtype);
  if (M <= 0 || N <= 0) return MDT_OK;
  MDT_CHECK_ARG(X && out, "mdt_colsum_ordered: null pointer");
  const size_t need = mdt_colsum_ordered_workspace_bytes(M, N);
  MDT_CHECK_ARG(workspace && workspace_bytes >= need, "mdt_colsum_ordered: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int64_t blocks = (M + CS_BLOCK_ROWS - 1) / CS_BLOCK_ROWS;
  MDT_CHECK_ARG(blocks <= 65535, "mdt_colsum_ordered: %lld rows (limit %d)", (long long)M, 65535 * CS_BLOCK_ROWS);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)blocks);
  if (int e = with_dtype(dtype, [&](auto t) {
        return launch_colsum<typename decltype(t)::type, 1, true>("colsum_ordered", st, grid, M, N, X, ldx, (float*)workspace, CS_BLOCK_ROWS, row_weight);
      }))
    return e;
  return sum_slices_f32(st, 1, N, (int)blocks, (const float*)workspace, N, N, out, N, 1);
}

extern "C" int mdt_dropout(void* stream, int dtype, int64_t rows, int D, const void* x, int64_t ldx, void* y, int64_t ldy,
                           float p_, uint64_t seed) {
  if (rows == 0 || D == 0) return MDT_OK;
  MDT_CHECK_ARG(x && y && p_ >= 0.f && p_ < 1.f, "mdt_dropout: bad arguments (p=%f)", p_);
  hipStream_t st = (hipStream_t)stream;
  MDT_CHECK_ARG(rows * D < DROP_MAX_ELEMS, "mdt_dropout: site of %lld elements (limit 2^33)", (long long)(rows * D));
  const DropCfg d = make_drop(p_, seed);
  const unsigned grid = (unsigned)((rows + 3) / 4 > 8192 ? 8192 : (rows + 3) / 4);
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    if (vec16_ok(dtype, D, {ldx, ldy}, {x, y}))
      return launch_plain<dropout_kernel<T, Vec<T>::N>>("dropout_vec", grid, 256, st, rows, D, (const T*)x, ldx, (T*)y, ldy, d);
    return launch_plain<dropout_kernel<T, 1>>("dropout", grid, 256, st, rows, D, (const T*)x, ldx, (T*)y, ldy, d);
  });
}

extern "C" int mdt_dropout_mask(void* stream, int64_t n, float p_, uint64_t seed, uint8_t* mask) {
  if (n == 0) return MDT_OK;
  MDT_CHECK_ARG(mask && p_ >= 0.f && p_ < 1.f && n < DROP_MAX_ELEMS, "mdt_dropout_mask: bad arguments");
  return launch_plain<dropout_mask_kernel>("dropout_mask", (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256), 256,
                                           (hipStream_t)stream, n, make_drop(p_, seed), mask);
}

extern "C" int mdt_cast(void* stream, int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst) {
  if (n == 0) return MDT_OK;
  MDT_CHECK_ARG(src && dst, "mdt_cast: null pointer");
  const int grid = (int)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  return with_dtypes(src_dtype, dst_dtype, [&](auto s, auto d) {
    using TS = typename decltype(s)::type;
    using TD = typename decltype(d)::type;
    return launch_plain<cast_kernel<TS, TD>>("cast", grid, 256, (hipStream_t)stream, n, (const TS*)src, (TD*)dst);
  });
}

extern "C" int mdt_transpose2d(void* stream, int src_dtype, int dst_dtype, int64_t rows, int64_t cols, const void* src,
                               int64_t lds_, void* dst, int64_t ldd) {
  if (rows == 0 || cols == 0) return MDT_OK;
  MDT_CHECK_ARG(src && dst, "mdt_transpose2d: null pointer");
  if (src_dtype == MDT_BF16 && dst_dtype == MDT_F32) MDT_UNSUPPORTED("mdt_transpose2d: dtypes %d -> %d", src_dtype, dst_dtype);
  const dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32));
  return with_dtypes(src_dtype, dst_dtype, [&](auto s, auto d) {
    using TS = typename decltype(s)::type;
    using TD = typename decltype(d)::type;
    return launch_plain<transpose_kernel<TS, TD>>("transpose2d", grid, 256, (hipStream_t)stream, rows, cols, (const TS*)src, lds_, (TD*)dst, ldd);
  });
}
