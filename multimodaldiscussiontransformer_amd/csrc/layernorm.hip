// LayerNorm forward / backward: one wavefront per row, the row held in registers
// (two-pass mean / variance, no re-read), 16-byte vector loads, fp32 statistics.
// HBM-bound: algorithmic bytes = rows * D * sizeof(T) * 2 (fwd), * 3 (+ residual 4) (bwd).
// Replaces fairseq LayerNorm / HF nn.LayerNorm (modules/graphormer_graph_encoder_layer.py:
// 127-130,138-141; modules/multigraphormer_graph_encoder.py:400-403; HF BertLayer/ViTLayer).
//
// Layout of this file: the row arithmetic (ln_fwd_row; ln_bwd_row and ln_bwd_reduce_columns) works on the register-resident
// vectors of a row; the kernels around it are shells that differ in how a row's vectors get into and out of registers.
// One exception, measured: layernorm_bwd_rows_kernel keeps its own copy of ln_bwd_row's statements (see there).  The launch
// code below the kernels decides each question (vectors per lane, fp8 format, backward form) in one place and writes each
// kernel family's argument list once.
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace mdt {

// One row forward, from the vectors xv a lane holds of it (vector i starts at column (i * 64 + lane) * V::N; vectors past D
// are absent): mean, variance and rstd over the wave, mean[row] / rstd[row], and y = (x - mean) * rstd * gamma + beta stored
// to yr.  The one place this arithmetic is written: the plain and the embedding-fused forward agree bit for bit because both
// come through here.
// Q8 (bf16 only): y ALSO leaves as fp8 (1: e4m3, 2: e5m2) for the 8-bit GEMM that consumes it — qr = saturate(bf16(y) * qs),
// qmax = max(qmax, max |bf16(y)|), the bytes and the maximum mdt_fp8_quantize would make of y (fp8.hip), without its pass
template <int NV, int Q8, typename T, typename V>
__device__ __forceinline__ void ln_fwd_row(const V* xv, const V* gv, const V* bv, int lane, int D, float eps, int64_t row,
                                           T* yr, float* mean, float* rstd, uint8_t* qr, float qs, float& qmax) {
  constexpr int VN = V::N;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) {
#pragma unroll
      for (int j = 0; j < VN; ++j) s += xv[i].get(j);
    }
  }
  const float mu = wave_sum_dpp(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) {
#pragma unroll
      for (int j = 0; j < VN; ++j) { const float d = xv[i].get(j) - mu; q += d * d; }
    }
  }
  const float rs = rsqrtf(wave_sum_dpp(q) / (float)D + eps);
  if (lane == 0) { if (mean) mean[row] = mu; if (rstd) rstd[row] = rs; }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) {
      V o;
#pragma unroll
      for (int j = 0; j < VN; ++j) o.set(j, (xv[i].get(j) - mu) * rs * gv[i].get(j) + bv[i].get(j));
      *(V*)(yr + c) = o;
      if constexpr (Q8 != 0 && (VN == 8 || VN == 4)) {
        constexpr float FMAX = Q8 == 1 ? 448.0f : 57344.0f;
        // mirrors fp8.hip: a NaN / infinity passes through as NaN (the MFMA propagates it to the loss) and marks the running
        // maximum +inf, which fp8_scale_update leaves the scale alone for
        float qv[VN];
#pragma unroll
        for (int j = 0; j < VN; ++j) {
          const float r = o.get(j);                 // the ROUNDED output
          const bool bad = !(fabsf(r) <= 3.4028234663852886e38f);
          qmax = bad ? __builtin_inff() : fmaxf(qmax, fabsf(r));
          const float xq = r * qs;
          qv[j] = (xq != xq) ? xq : fminf(fmaxf(xq, -FMAX), FMAX);
        }
        int w[VN / 4];
#pragma unroll
        for (int k = 0; k < VN / 4; ++k) {
          w[k] = 0;
          if constexpr (Q8 == 1) {
            w[k] = __builtin_amdgcn_cvt_pk_fp8_f32(qv[4 * k], qv[4 * k + 1], w[k], false); w[k] = __builtin_amdgcn_cvt_pk_fp8_f32(qv[4 * k + 2], qv[4 * k + 3], w[k], true);
          } else {
            w[k] = __builtin_amdgcn_cvt_pk_bf8_f32(qv[4 * k], qv[4 * k + 1], w[k], false); w[k] = __builtin_amdgcn_cvt_pk_bf8_f32(qv[4 * k + 2], qv[4 * k + 3], w[k], true);
          }
        }
        if constexpr (VN == 8) *(int2*)(qr + c) = make_int2(w[0], w[1]);
        else *(int*)(qr + c) = w[0];
      }
    }
  }
}

// NV = number of 16-B vectors per lane: D = NV * 64 * Vec<T>::N exactly, or masked tail.
// A wave walks rows wid, wid + nwaves, ...; the next row is requested before the current one is reduced, so a wave keeps
// two rows (and an 8-workgroup CU 64 of them, ~100 KiB) in flight — with one row per wave and no look-ahead the kernel
// moved 4.1 TB/s, bounded by bytes in flight over the ~2 us of an HBM round trip.
// Q8: the fp8 copy of ln_fwd_row, q8 = saturate(bf16(y) * *q8_scale), *q8_amax = max(*q8_amax, max |bf16(y)|)
template <typename T, int NV, int Q8 = 0, typename V = Vec<T>>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(int64_t rows, int D, const T* __restrict__ x, int64_t ldx,
                                                            const T* __restrict__ gamma, const T* __restrict__ beta,
                                                            float eps, T* __restrict__ y, int64_t ldy,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            uint8_t* __restrict__ q8 = nullptr, int64_t ldq = 0,
                                                            const float* __restrict__ q8_scale = nullptr, float* __restrict__ q8_amax = nullptr) {
  constexpr int VN = V::N;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  float qmax = 0.f;
  const float qs = Q8 != 0 ? *q8_scale : 1.0f;
  __shared__ float s_qmax[4];
  if constexpr (Q8 != 0) {
    if (threadIdx.x < 4) s_qmax[threadIdx.x] = 0.f;
    __syncthreads();
  }
  if (row < rows) {
  V gv[NV], bv[NV], xv[NV], xn[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) {
      xv[i] = *(const V*)(x + row * ldx + c);
      gv[i] = *(const V*)(gamma + c);
      bv[i] = *(const V*)(beta + c);
    }
  }
  for (;;) {
    const int64_t next = row + nwaves;
    if (next < rows) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * VN;
        if (c < D) xn[i] = *(const V*)(x + next * ldx + c);
      }
    }
    ln_fwd_row<NV, Q8>(xv, gv, bv, lane, D, eps, row, y + row * ldy, mean, rstd, Q8 != 0 ? q8 + row * ldq : nullptr, qs, qmax);
    if (next >= rows) break;
    row = next;
#pragma unroll
    for (int i = 0; i < NV; ++i) xv[i] = xn[i];
  }
  }
  if constexpr (Q8 != 0) {          // one atomic per workgroup (non-negative floats order like their bit patterns)
    qmax = wave_max(qmax);
    if (lane == 0) s_qmax[threadIdx.x >> 6] = qmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float m = fmaxf(fmaxf(s_qmax[0], s_qmax[1]), fmaxf(s_qmax[2], s_qmax[3]));
      if (m > 0.f) atomicMax((int*)q8_amax, __float_as_int(m));
    }
  }
}

// BERT embeddings and their LayerNorm in one pass (HF BertEmbeddings as run by the truncated BertModel,
// modules/multigraphormer_graph_encoder.py:325-329): x = T(word[ids] + type[types] + pos[pos_ids]) — rounded to the storage type
// exactly as mdt_bert_embed_rows leaves it — then y = LayerNorm(x).  The summed row never makes the round trip through HBM between
// the two; it is written out (xs) only when a backward pass will read it.  One wave per row, the next row's three gathers in flight.
template <typename T, int NV, typename V = Vec<T>>
__global__ __launch_bounds__(256) void bert_embed_ln_rows_kernel(int64_t rows, int D, const int32_t* __restrict__ ids,
                                                                 const int32_t* __restrict__ types, const int32_t* __restrict__ pos_ids,
                                                                 const T* __restrict__ word, const T* __restrict__ pos,
                                                                 const T* __restrict__ typ, const T* __restrict__ gamma,
                                                                 const T* __restrict__ beta, float eps, T* __restrict__ xs, int64_t ldxs,
                                                                 T* __restrict__ y, int64_t ldy, float* __restrict__ mean,
                                                                 float* __restrict__ rstd) {
  constexpr int VN = V::N;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  V gv[NV], bv[NV], wv[NV], pv[NV], tv[NV], wn[NV], pn[NV], tn[NV];
  auto request = [&](int64_t r, V* w_, V* p_, V* t_) {
    const int64_t wi = ids[r], pi = pos_ids[r], ti = types[r];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * VN;
      if (c < D) {
        w_[i] = *(const V*)(word + wi * D + c);
        p_[i] = *(const V*)(pos + pi * D + c);
        t_[i] = *(const V*)(typ + ti * D + c);
      }
    }
  };
  request(row, wv, pv, tv);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) { gv[i] = *(const V*)(gamma + c); bv[i] = *(const V*)(beta + c); }
  }
  for (;;) {
    const int64_t next = row + nwaves;
    if (next < rows) request(next, wn, pn, tn);
    V xv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * VN;
      if (c < D) {
        xv[i] = bert_embed_vec(wv[i], tv[i], pv[i]);
        if (xs) *(V*)(xs + row * ldxs + c) = xv[i];
      }
    }
    float unused = 0.f;
    ln_fwd_row<NV, 0>(xv, gv, bv, lane, D, eps, row, y + row * ldy, mean, rstd, (uint8_t*)nullptr, 1.0f, unused);
    if (next >= rows) break;
    row = next;
#pragma unroll
    for (int i = 0; i < NV; ++i) { wv[i] = wn[i]; pv[i] = pn[i]; tv[i] = tn[i]; }
  }
}

// Backward.  What a lane accumulates over the rows its wave walks: per-column partial dgamma / dbeta and (CS) column sums of
// the tail output, one float per element of its NV vectors.
template <int NV, int VN, bool CS>
struct LnBwdPartials {
  float g[NV][VN], b[NV][VN], c[CS ? NV : 1][CS ? VN : 1];
  __device__ __forceinline__ void zero(int i) {
#pragma unroll
    for (int j = 0; j < VN; ++j) { g[i][j] = 0.f; b[i][j] = 0.f; if constexpr (CS) c[i][j] = 0.f; }
  }
};

// One row backward, from the vectors a lane holds of it (x, dy, the residual-path gradient av when has_add, gamma):
// the two row sums, the partials, dx and — when dropped — dxd, the gradient of the dense layer behind a hidden dropout.
// store(i, c, o, od) takes vector i (column c) of dx and dxd to memory; vectors past D are absent.
template <int NV, bool CS, typename V, typename Store>
__device__ __forceinline__ void ln_bwd_row(int64_t row, int D, int lane, const V* xv, const V* gy, const V* av, const V* gv,
                                           float mu, float rs, bool has_add, bool dropped, const DropCfg& drop,
                                           LnBwdPartials<NV, V::N, CS>& part, Store&& store) {
  constexpr int VN = V::N;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) {
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const float xh = (xv[i].get(j) - mu) * rs;
        const float g = gy[i].get(j);
        const float gg = g * gv[i].get(j);
        s1 += gg;
        s2 += gg * xh;
        part.g[i][j] += g * xh;
        part.b[i][j] += g;
      }
    }
  }
  const float m1 = wave_sum_dpp(s1) / (float)D, m2 = wave_sum_dpp(s2) / (float)D;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) {
      V o, od;
      float ds0 = 0.f, ds1 = 0.f;
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const float xh = (xv[i].get(j) - mu) * rs;
        float v = rs * (gy[i].get(j) * gv[i].get(j) - m1 - xh * m2);
        if (has_add) v += av[i].get(j);
        o.set(j, v);
        if (dropped) {
          if ((j & 1) == 0) drop_scale2(drop, (uint64_t)row * D + c + j, ds0, ds1);   // D and c are even
          v = o.get(j) * ((j & 1) ? ds1 : ds0);
          od.set(j, v);
          v = od.get(j);
        } else {
          v = o.get(j);
        }
        if constexpr (CS) part.c[i][j] += v;
      }
      store(i, c, o, od);
    }
  }
}

// The workgroup's four waves combine their partials through ONE [4 waves][W = NV * 64 * VN] LDS buffer used three times
// (dgamma, dbeta, column sums; 16 KiB at D = 768: the 48 KiB of three buffers held a CU to three workgroups) and issue one
// float atomic per column.  ORD (mdt_layernorm_bwd_ordered): the three pointers are [gridDim.x][D] workspace arrays and the
// workgroup STORES its partial row there instead; mdt_sum_slices_f32 then adds the workgroups in ascending order.
template <int NV, int VN, bool CS, bool ORD = false>
__device__ __forceinline__ void ln_bwd_reduce_columns(const LnBwdPartials<NV, VN, CS>& part, float* red, int lane, int wave, int D,
                                                      float* dgamma, float* dbeta, float* colsum) {
  if (!dgamma && !dbeta && !colsum) return;
  constexpr int W = NV * 64 * VN;
#pragma unroll
  for (int round = 0; round < (CS ? 3 : 2); ++round) {
    float* dst = round == 0 ? dgamma : round == 1 ? dbeta : colsum;
    if (round) __syncthreads();           // the previous round's readers are done
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const int c = (i * 64 + lane) * VN + j;
        red[wave * W + c] = round == 0 ? part.g[i][j] : round == 1 ? part.b[i][j] : part.c[CS ? i : 0][CS ? j : 0];
      }
    __syncthreads();
    if (dst)
      for (int c = threadIdx.x; c < D; c += 256) {
        const float v = red[c] + red[W + c] + red[2 * W + c] + red[3 * W + c];
        if constexpr (ORD) dst[(int64_t)blockIdx.x * D + c] = v;
        else atomicAdd(dst + c, v);
      }
  }
}

// The generic backward shell: each wave walks rows_per_wave consecutive rows (the next row's x / dy / residual-gradient
// vectors are requested before the current row is reduced) through 64-bit pointers, vectors past D masked.
template <typename T, int NV, bool TAIL, bool CS = TAIL, typename V = Vec<T>, bool ORD = false>   // TAIL: second (dropped) output and / or column sums; CS: the column sums
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(int64_t rows, int D, const T* __restrict__ dy, int64_t lddy,
                                                            const T* __restrict__ x, int64_t ldx,
                                                            const T* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const T* __restrict__ add,
                                                            int64_t ldadd, T* __restrict__ dx, int64_t lddx,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            int rows_per_wave, T* __restrict__ dxd, int64_t lddxd,
                                                            DropCfg drop, float* __restrict__ colsum) {
  constexpr int VN = V::N;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = (float*)smem_raw;  // [4 waves][NV*64*VN]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * rows_per_wave;
  const int64_t r1 = (r0 + rows_per_wave < rows) ? r0 + rows_per_wave : rows;
  LnBwdPartials<NV, VN, CS> part;
  V gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * VN;
    if (c < D) gv[i] = *(const V*)(gamma + c);
    part.zero(i);
  }
  V xv[NV], gy[NV], av[NV], xn[NV], gn[NV], an[NV];
  float mu = 0.f, rs = 0.f, mu_n = 0.f, rs_n = 0.f;
  if (r0 < r1) {
    mu = mean[r0]; rs = rstd[r0];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * VN;
      if (c < D) {
        xv[i] = *(const V*)(x + r0 * ldx + c);
        gy[i] = *(const V*)(dy + r0 * lddy + c);
        if (add) av[i] = *(const V*)(add + r0 * ldadd + c);
      }
    }
  }
  for (int64_t row = r0; row < r1; ++row) {
    if (row + 1 < r1) {
      mu_n = mean[row + 1]; rs_n = rstd[row + 1];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * VN;
        if (c < D) {
          xn[i] = *(const V*)(x + (row + 1) * ldx + c);
          gn[i] = *(const V*)(dy + (row + 1) * lddy + c);
          if (add) an[i] = *(const V*)(add + (row + 1) * ldadd + c);
        }
      }
    }
    ln_bwd_row<NV, CS>(row, D, lane, xv, gy, av, gv, mu, rs, add != nullptr, TAIL && dxd != nullptr, drop, part,
                              [&](int, int c, const V& o, const V& od) {
                                *(V*)(dx + row * lddx + c) = o;
                                if constexpr (TAIL) {
                                  if (dxd) *(V*)(dxd + row * lddxd + c) = od;
                                }
                              });
    mu = mu_n; rs = rs_n;
#pragma unroll
    for (int i = 0; i < NV; ++i) { xv[i] = xn[i]; gy[i] = gn[i]; av[i] = an[i]; }
  }
  ln_bwd_reduce_columns<NV, VN, CS, ORD>(part, red, lane, wave, D, dgamma, dbeta, colsum);
}

// The backward shell for bf16 rows of 256 * NV elements (768: every LayerNorm of mDT-base; 1024: mDT-large) with its addresses in SCALAR registers: a wave owns whole
// rows, so a row's byte offset is wave-uniform — each tensor is a buffer descriptor based at the wave's first row, the row offset
// goes into the instruction's SGPR operand, the vector's place in the row into its 12-bit immediate (0 / 512 / 1024), and ONE VGPR
// (lane * 8) serves every load and store of the kernel.  Same arithmetic in the same order as layernorm_bwd_kernel<bf16_t, 3, ...,
// VecH>: what changes is the register budget (no 64-bit address per tensor and row, no vectors for an absent residual gradient).
// That budget is why the row loop below repeats the statements of ln_bwd_row instead of calling it: through the call (its
// vectors handed over as pointers, with or without __restrict__, the flags as template arguments, the stores inside or outside)
// the compiler packs the row's operations differently and every instantiation with NV >= 2 takes 2 to 17 more VGPRs; six of
// them (NV 2: fff ftf ftt ttf ttt, NV 4: ftf) lose a wave of occupancy.  Edit the two together: the D = 768 test compares them bit for bit.
template <int NV, bool DROPPED, bool CS, bool ADD>
__global__ __launch_bounds__(256) void layernorm_bwd_rows_kernel(int64_t rows, const bf16_t* __restrict__ dy, int64_t lddy,
                                                                const bf16_t* __restrict__ x, int64_t ldx,
                                                                const bf16_t* __restrict__ gamma, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const bf16_t* __restrict__ add,
                                                                int64_t ldadd, bf16_t* __restrict__ dx, int64_t lddx,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                int rows_per_wave, bf16_t* __restrict__ dxd, int64_t lddxd,
                                                                DropCfg drop, float* __restrict__ colsum) {
  constexpr int D = 256 * NV, VN = 4;
  typedef VecH<bf16_t> V;
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* red = (float*)smem_raw;  // [4 waves][D]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * rows_per_wave;
  const int64_t r1 = (r0 + rows_per_wave < rows) ? r0 + rows_per_wave : rows;
  const int nrow = r0 < r1 ? (int)(r1 - r0) : 0;
  auto desc = [&](const void* p, int64_t ld) {
    const int64_t bytes = (int64_t)nrow * ld * 2;
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p + (nrow ? r0 * ld * 2 : 0)), 0,
                                             (unsigned)(p == nullptr ? 0 : bytes > 0xFFFFFFF0ll ? 0xFFFFFFF0ll : bytes), 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t rs_dy = desc(dy, lddy), rs_x = desc(x, ldx), rs_add = desc(ADD ? add : nullptr, ldadd),
                               rs_dx = desc(dx, lddx), rs_dxd = desc(DROPPED ? dxd : nullptr, lddxd);
  const int s_dy = (int)(lddy * 2), s_x = (int)(ldx * 2), s_add = (int)(ldadd * 2), s_dx = (int)(lddx * 2), s_dxd = (int)(lddxd * 2);
  const int voff = lane * 8;
  auto ld8 = [&](__amdgpu_buffer_rsrc_t rs, int i, int soff) {
    V v;
    v.v = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rs, voff + i * 512, soff, 0));
    return v;
  };
  auto st8 = [&](__amdgpu_buffer_rsrc_t rs, int i, int soff, const V& v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v.v), rs, voff + i * 512, soff, 0);
  };
  LnBwdPartials<NV, VN, CS> part;
  V gv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    gv[i] = *(const V*)(gamma + (i * 64 + lane) * VN);
    part.zero(i);
  }
  V xv[NV], gy[NV], av[ADD ? NV : 1], xn[NV], gn[NV], an[ADD ? NV : 1];
  float mu = 0.f, rs = 0.f, mu_n = 0.f, rs_n = 0.f;
  if (nrow) {
    mu = mean[r0]; rs = rstd[r0];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      xv[i] = ld8(rs_x, i, 0);
      gy[i] = ld8(rs_dy, i, 0);
      if constexpr (ADD) av[i] = ld8(rs_add, i, 0);
    }
  }
  for (int k = 0; k < nrow; ++k) {
    const int64_t row = r0 + k;
    if (k + 1 < nrow) {
      mu_n = mean[row + 1]; rs_n = rstd[row + 1];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        xn[i] = ld8(rs_x, i, (k + 1) * s_x);
        gn[i] = ld8(rs_dy, i, (k + 1) * s_dy);
        if constexpr (ADD) an[i] = ld8(rs_add, i, (k + 1) * s_add);
      }
    }
    // ln_bwd_row, operation for operation, written out: see above the kernel
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const float xh = (xv[i].get(j) - mu) * rs;
        const float g = gy[i].get(j);
        const float gg = g * gv[i].get(j);
        s1 += gg;
        s2 += gg * xh;
        part.g[i][j] += g * xh;
        part.b[i][j] += g;
      }
    }
    const float m1 = wave_sum_dpp(s1) / (float)D, m2 = wave_sum_dpp(s2) / (float)D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * VN;
      V o, od;
      float ds0 = 0.f, ds1 = 0.f;
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const float xh = (xv[i].get(j) - mu) * rs;
        float v = rs * (gy[i].get(j) * gv[i].get(j) - m1 - xh * m2);
        if constexpr (ADD) v += av[i].get(j);
        o.set(j, v);
        if constexpr (DROPPED) {
          if ((j & 1) == 0) drop_scale2(drop, (uint64_t)row * D + c + j, ds0, ds1);
          v = o.get(j) * ((j & 1) ? ds1 : ds0);
          od.set(j, v);
          v = od.get(j);
        } else {
          v = o.get(j);
        }
        if constexpr (CS) part.c[i][j] += v;
      }
      st8(rs_dx, i, k * s_dx, o);
      if constexpr (DROPPED) st8(rs_dxd, i, k * s_dxd, od);
    }
    mu = mu_n; rs = rs_n;
#pragma unroll
    for (int i = 0; i < NV; ++i) { xv[i] = xn[i]; gy[i] = gn[i]; if constexpr (ADD) av[i] = an[i]; }
  }
  ln_bwd_reduce_columns(part, red, lane, wave, D, dgamma, dbeta, colsum);
}

// ---- launch: every choice made once, every argument list written once
// Runtime value -> template argument: f(std::integral_constant<int, v>) for the v among Vs that equals value; false if none does.
template <int... Vs, typename F>
static bool ln_pick(int value, F&& f) {
  return ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// How a lane holds a row of D elements: f(NV, V) with NV vectors of type V per lane.  bf16 rows of 768 are three 8-byte
// vectors, every lane busy (VecH); all else is ceil(D / (64 * Vec<T>::N)) 16-byte vectors, the last ones masked.
// false: no kernel is instantiated for that many vectors per lane.
template <typename T> static int ln_vectors_per_lane(int D) { return (D + 64 * Vec<T>::N - 1) / (64 * Vec<T>::N); }
template <typename T, typename F>
static bool ln_row_layout(int D, F&& f) {
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (D == 768) { f(std::integral_constant<int, 3>{}, VecH<T>{}); return true; }
  }
  return ln_pick<1, 2, 3, 4, 6, 8>(ln_vectors_per_lane<T>(D), [&](auto nv) { f(nv, Vec<T>{}); });
}

// Forward grids: 8 resident workgroups per CU (32 waves, two rows in flight each); short inputs get one row per wave
static unsigned ln_fwd_grid(int64_t rows) {
  const int64_t wgs = (rows + 3) / 4;
  return (unsigned)(wgs < 2048 ? wgs : 2048);
}

// The one launch: the arguments are converted to the kernel's own parameter types (the C ABI hands tensors over as void*)
template <typename... P, typename... A>
static void ln_launch(void (*kernel)(P...), unsigned grid, size_t lds, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, grid, 256, lds, st, (P)args...);
}

template <typename T>
static int ln_fwd_dispatch(hipStream_t st, int64_t rows, int D, const void* x, int64_t ldx, const void* gamma,
                           const void* beta, float eps, void* y, int64_t ldy, float* mean, float* rstd, void* q8 = nullptr,
                           int64_t ldq = 0, int q8_fmt = 0, const float* q8_scale = nullptr, float* q8_amax = nullptr) {
  const bool ok = ln_row_layout<T>(D, [&](auto nv, auto vec) {
    auto launch = [&](auto q8_form) {
      ln_launch(layernorm_fwd_kernel<T, decltype(nv)::value, decltype(q8_form)::value, decltype(vec)>, ln_fwd_grid(rows), 0, st,
                rows, D, x, ldx, gamma, beta, eps, y, ldy, mean, rstd, q8, ldq, q8_scale, q8_amax);
    };
    // the fp8 copy exists for bf16 rows only (mdt_layernorm_fwd_q8 lets nothing else through): 1 = e4m3, 2 = e5m2
    if constexpr (std::is_same<T, bf16_t>::value) ln_pick<0, 1, 2>(q8 ? (q8_fmt == 0 ? 1 : 2) : 0, launch);
    else launch(std::integral_constant<int, 0>{});
  });
  if (!ok) MDT_UNSUPPORTED("layernorm: D=%d not supported (vectors per lane %d)", D, ln_vectors_per_lane<T>(D));
  if (int e = check_launch("layernorm_fwd")) return e;
  set_last_route(q8 ? "ln_fwd_q8" : "ln_fwd");
  return MDT_OK;
}

template <typename T>
static int embed_ln_dispatch(hipStream_t st, int64_t rows, int D, const int32_t* ids, const int32_t* types, const int32_t* pos_ids,
                             const void* word, const void* pos, const void* typ, const void* gamma, const void* beta, float eps,
                             void* xs, int64_t ldxs, void* y, int64_t ldy, float* mean, float* rstd) {
  const bool ok = ln_row_layout<T>(D, [&](auto nv, auto vec) {
    ln_launch(bert_embed_ln_rows_kernel<T, decltype(nv)::value, decltype(vec)>, ln_fwd_grid(rows), 0, st,
              rows, D, ids, types, pos_ids, word, pos, typ, gamma, beta, eps, xs, ldxs, y, ldy, mean, rstd);
  });
  if (!ok) MDT_UNSUPPORTED("bert_embed_ln_rows: D=%d not supported (vectors per lane %d)", D, ln_vectors_per_lane<T>(D));
  return check_launch("bert_embed_ln_rows");
}

template <typename T>
static int ln_bwd_dispatch(hipStream_t st, int64_t rows, int D, const void* dy, int64_t lddy, const void* x, int64_t ldx,
                           const void* gamma, const float* mean, const float* rstd, const void* add, int64_t ldadd,
                           void* dx, int64_t lddx, float* dgamma, float* dbeta, void* dxd, int64_t lddxd, DropCfg drop,
                           float* colsum) {
  // ~2048 workgroups x 4 waves, at least 4 rows per wave so the column atomics stay few
  const int64_t want = switches().ln_bwd_wgs > 0 ? switches().ln_bwd_wgs : 2048;
  int rpw = (int)((rows + want * 4 - 1) / (want * 4));
  if (rpw < 4) rpw = 4;
  const unsigned grid = (unsigned)((rows + 4 * rpw - 1) / (4 * rpw));
  // both kernels end in the same parameters; lead is (rows) or (rows, D); LDS: [4 waves][row as the lanes hold it] floats
  auto launch = [&](auto kernel, int row_elems, auto... lead) {
    ln_launch(kernel, grid, (size_t)(4 * row_elems * 4), st, lead..., dy, lddy, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx,
              dgamma, dbeta, rpw, dxd, lddxd, drop, colsum);
  };
  // the form: which optional tensors take part (bit 2: the dropped copy, bit 1: the column sums, bit 0: the residual gradient)
  const int form = (dxd ? 4 : 0) | (colsum ? 2 : 0) | (add ? 1 : 0);
  bool ok = false;
  const char* route = "ln_generic";
  ln_pick<0, 1, 2, 3, 4, 5, 6, 7>(form, [&](auto f) {
    constexpr bool DROPPED = (decltype(f)::value & 4) != 0, CS = (decltype(f)::value & 2) != 0, ADD = (decltype(f)::value & 1) != 0;
    if constexpr (std::is_same<T, bf16_t>::value) {
      // row offsets inside a wave's block of rows are 32-bit scalars: rows_per_wave * row stride stays far below 2^31
      const int64_t ldmax = std::max(std::max(lddy, ldx), std::max(std::max(ldadd, lddx), lddxd));
      if ((D == 768 || D == 1024 || D == 512 || D == 256) && !switches().ln_generic && (int64_t)rpw * ldmax * 2 < (1ll << 31)) {
        route = "ln_rows";
        ok = ln_pick<1, 2, 3, 4>(D / 256, [&](auto nv) {
          launch(layernorm_bwd_rows_kernel<decltype(nv)::value, DROPPED, CS, ADD>, D, rows);
        });
        return;
      }
    }
    ok = ln_row_layout<T>(D, [&](auto nv, auto vec) {
      constexpr int NV = decltype(nv)::value;
      launch(layernorm_bwd_kernel<T, NV, DROPPED || CS, CS, decltype(vec)>, NV * 64 * decltype(vec)::N, rows, D);
    });
  });
  if (!ok) MDT_UNSUPPORTED("layernorm: D=%d not supported (vectors per lane %d)", D, ln_vectors_per_lane<T>(D));
  if (int e = check_launch("layernorm_bwd")) return e;
  set_last_route(route);
  return MDT_OK;
}

// Ordered form: the generic kernel (its row arithmetic, so dx / dxd keep their bits) with the per-workgroup partials stored to
// the workspace [3][workgroups][D] (dgamma, dbeta, column sums).  The grid is a function of `rows` alone.
static void ln_bwd_ordered_grid(int64_t rows, int& rpw, unsigned& grid) {
  rpw = (int)((rows + 2048 * 4 - 1) / (2048 * 4));
  if (rpw < 4) rpw = 4;
  grid = (unsigned)((rows + 4 * rpw - 1) / (4 * rpw));
}

template <typename T>
static int ln_bwd_ordered_dispatch(hipStream_t st, int64_t rows, int D, const void* dy, int64_t lddy, const void* x, int64_t ldx,
                                   const void* gamma, const float* mean, const float* rstd, const void* add, int64_t ldadd,
                                   void* dx, int64_t lddx, float* pg, float* pb, void* dxd, int64_t lddxd, DropCfg drop, float* pc) {
  int rpw;
  unsigned grid;
  ln_bwd_ordered_grid(rows, rpw, grid);
  const bool ok = ln_row_layout<T>(D, [&](auto nv, auto vec) {
    constexpr int NV = decltype(nv)::value;
    ln_launch(layernorm_bwd_kernel<T, NV, true, true, decltype(vec), true>, grid, (size_t)(4 * NV * 64 * decltype(vec)::N * 4), st,
              rows, D, dy, lddy, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, pg, pb, rpw, dxd, lddxd, drop, pc);
  });
  if (!ok) MDT_UNSUPPORTED("layernorm: D=%d not supported (vectors per lane %d)", D, ln_vectors_per_lane<T>(D));
  if (int e = check_launch("layernorm_bwd_ordered")) return e;
  set_last_route("ln_generic");
  return MDT_OK;
}

}  // namespace mdt

using namespace mdt;

static int ln_check(int dtype, int D, int64_t ld0, int64_t ld1, const void* p0, const void* p1) {
  const int vn = dtype == MDT_BF16 ? 8 : 4;
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "layernorm: bad dtype %d", dtype);
  MDT_CHECK_ARG(D > 0 && D % vn == 0, "layernorm: D=%d must be a multiple of %d", D, vn);
  MDT_CHECK_ARG(ld0 % vn == 0 && ld1 % vn == 0, "layernorm: row strides must be multiples of %d elements", vn);
  MDT_CHECK_ARG((((uintptr_t)p0 | (uintptr_t)p1) & 15) == 0, "layernorm: pointers must be 16-byte aligned");
  return MDT_OK;
}

extern "C" int mdt_layernorm_fwd(void* stream, int dtype, int64_t rows, int D, const void* x, int64_t ldx,
                                 const void* gamma, const void* beta, float eps, void* y, int64_t ldy, float* mean,
                                 float* rstd) {
  if (rows == 0) return MDT_OK;
  MDT_CHECK_ARG(x && y && gamma && beta, "layernorm_fwd: null pointer");
  if (int e = ln_check(dtype, D, ldx, ldy, x, y)) return e;
  MDT_CHECK_ARG((((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, "layernorm_fwd: gamma/beta must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    return ln_fwd_dispatch<typename decltype(t)::type>(st, rows, D, x, ldx, gamma, beta, eps, y, ldy, mean, rstd);
  });
}

extern "C" int mdt_layernorm_fwd_q8(void* stream, int dtype, int64_t rows, int D, const void* x, int64_t ldx,
                                    const void* gamma, const void* beta, float eps, void* y, int64_t ldy, float* mean,
                                    float* rstd, void* q8_out, int64_t ld_q8, int q8_format, const float* q8_scale, float* q8_amax) {
  if (!q8_out) return mdt_layernorm_fwd(stream, dtype, rows, D, x, ldx, gamma, beta, eps, y, ldy, mean, rstd);
  if (rows == 0) return MDT_OK;
  MDT_CHECK_ARG(x && y && gamma && beta, "layernorm_fwd_q8: null pointer");
  MDT_CHECK_ARG(dtype == MDT_BF16, "layernorm_fwd_q8: the fp8 copy exists for bf16 rows only (dtype %d)", dtype);
  MDT_CHECK_ARG(q8_format == 0 || q8_format == 1, "layernorm_fwd_q8: q8_format %d (0 = e4m3, 1 = e5m2)", q8_format);
  MDT_CHECK_ARG(q8_scale && q8_amax && ld_q8 >= D && ld_q8 % 8 == 0 && ((uintptr_t)q8_out & 7) == 0,
                "layernorm_fwd_q8: the fp8 copy needs its scale, its maximum slot and 8-byte aligned rows of at least D bytes");
  if (int e = ln_check(dtype, D, ldx, ldy, x, y)) return e;
  MDT_CHECK_ARG((((uintptr_t)gamma | (uintptr_t)beta) & 15) == 0, "layernorm_fwd_q8: gamma/beta must be 16-byte aligned");
  return ln_fwd_dispatch<bf16_t>((hipStream_t)stream, rows, D, x, ldx, gamma, beta, eps, y, ldy, mean, rstd, q8_out, ld_q8, q8_format, q8_scale, q8_amax);
}

extern "C" int mdt_bert_embed_ln_rows(void* stream, int dtype, int64_t rows, const int32_t* ids, const int32_t* types,
                                      const int32_t* pos_ids, const void* word, const void* pos, const void* type, int D,
                                      const void* gamma, const void* beta, float eps, void* xs, int64_t ldxs, void* y, int64_t ldy,
                                      float* mean, float* rstd) {
  if (rows == 0) return MDT_OK;
  MDT_CHECK_ARG(ids && types && pos_ids && word && pos && type && gamma && beta && y, "bert_embed_ln_rows: null pointer");
  if (int e = ln_check(dtype, D, xs ? ldxs : ldy, ldy, xs ? xs : y, y)) return e;
  MDT_CHECK_ARG((((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)word | (uintptr_t)pos | (uintptr_t)type) & 15) == 0,
                "bert_embed_ln_rows: tables, gamma and beta must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    return embed_ln_dispatch<typename decltype(t)::type>(st, rows, D, ids, types, pos_ids, word, pos, type, gamma, beta, eps, xs, ldxs, y, ldy, mean, rstd);
  });
}

extern "C" int mdt_layernorm_bwd(void* stream, int dtype, int64_t rows, int D, const void* dy, int64_t lddy,
                                 const void* x, int64_t ldx, const void* gamma, const float* mean, const float* rstd,
                                 const void* add, int64_t ldadd, void* dx, int64_t lddx, float* dgamma, float* dbeta,
                                 void* dxd, int64_t lddxd, float drop_p, uint64_t drop_seed, float* colsum) {
  if (rows == 0) return MDT_OK;
  MDT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "layernorm_bwd: dropout p=%f out of [0,1)", drop_p);
  MDT_CHECK_ARG(!dxd || rows * D < DROP_MAX_ELEMS, "layernorm_bwd: dropout site of %lld elements (limit 2^33)", (long long)(rows * D));
  const DropCfg drop = make_drop(dxd ? drop_p : 0.f, drop_seed);
  MDT_CHECK_ARG(dy && x && gamma && mean && rstd && dx, "layernorm_bwd: null pointer");
  if (int e = ln_check(dtype, D, lddy, ldx, dy, x)) return e;
  if (int e = ln_check(dtype, D, lddx, add ? ldadd : lddx, dx, add ? add : dx)) return e;
  if (dgamma || dbeta || colsum) note_float_atomic_launch();
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    return ln_bwd_dispatch<typename decltype(t)::type>(st, rows, D, dy, lddy, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, dgamma, dbeta, dxd, lddxd, drop, colsum);
  });
}

extern "C" size_t mdt_layernorm_bwd_ordered_workspace_bytes(int64_t rows, int D) {
  if (rows <= 0 || D <= 0) return 0;
  int rpw;
  unsigned grid;
  ln_bwd_ordered_grid(rows, rpw, grid);
  return (size_t)3 * grid * (size_t)D * sizeof(float);
}

extern "C" int mdt_layernorm_bwd_ordered(void* stream, int dtype, int64_t rows, int D, const void* dy, int64_t lddy,
                                         const void* x, int64_t ldx, const void* gamma, const float* mean, const float* rstd,
                                         const void* add, int64_t ldadd, void* dx, int64_t lddx, float* dgamma, float* dbeta,
                                         void* dxd, int64_t lddxd, float drop_p, uint64_t drop_seed, float* colsum,
                                         void* workspace, size_t workspace_bytes) {
  if (rows == 0) return MDT_OK;
  MDT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "layernorm_bwd_ordered: dropout p=%f out of [0,1)", drop_p);
  MDT_CHECK_ARG(!dxd || rows * D < DROP_MAX_ELEMS, "layernorm_bwd_ordered: dropout site of %lld elements (limit 2^33)", (long long)(rows * D));
  const DropCfg drop = make_drop(dxd ? drop_p : 0.f, drop_seed);
  MDT_CHECK_ARG(dy && x && gamma && mean && rstd && dx, "layernorm_bwd_ordered: null pointer");
  if (int e = ln_check(dtype, D, lddy, ldx, dy, x)) return e;
  if (int e = ln_check(dtype, D, lddx, add ? ldadd : lddx, dx, add ? add : dx)) return e;
  const size_t need = mdt_layernorm_bwd_ordered_workspace_bytes(rows, D);
  MDT_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
                "layernorm_bwd_ordered: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes, need);
  int rpw;
  unsigned grid;
  ln_bwd_ordered_grid(rows, rpw, grid);
  const int64_t slice = (int64_t)grid * D;
  float* pg = dgamma ? (float*)workspace : nullptr;
  float* pb = dbeta ? (float*)workspace + slice : nullptr;
  float* pc = colsum ? (float*)workspace + 2 * slice : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const int e = with_dtype(dtype, [&](auto t) {
    return ln_bwd_ordered_dispatch<typename decltype(t)::type>(st, rows, D, dy, lddy, x, ldx, gamma, mean, rstd, add, ldadd, dx, lddx, pg, pb, dxd, lddxd, drop, pc);
  });
  if (e) return e;
  // workgroup w's partial row is slice w: rows = 1, cols = D, slice stride D
  if (pg) if (int e2 = sum_slices_f32(st, 1, D, (int)grid, pg, D, D, dgamma, D, 1)) return e2;
  if (pb) if (int e2 = sum_slices_f32(st, 1, D, (int)grid, pb, D, D, dbeta, D, 1)) return e2;
  if (pc) if (int e2 = sum_slices_f32(st, 1, D, (int)grid, pc, D, D, colsum, D, 1)) return e2;
  return MDT_OK;
}
