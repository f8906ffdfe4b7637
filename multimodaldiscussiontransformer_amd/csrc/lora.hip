// Low-rank adapter (LoRA) products on the fused QKV projection: three skinny GEMMs with one dimension n = |targets| * rank of
// 8 ... 192 over ~10^5 token rows.  They replace the PEFT-style eager sequence around an adapted nn.Linear
//     t = x @ A.T;  y = base(x) + scale * (t @ B.T)          and autograd's  dB = t.T @ dy,  dt = dy @ B,  dA = dt.T @ x,  dx += dt @ A
// (the reference project has no adapters and hence no counterpart).  All three are memory-bound: the big operand ([R, D]) is
// read once from global memory straight into MFMA fragments (down, up_add) or through one LDS image (wgrad); nothing is staged
// through HBM and nothing is transposed in memory.
//   lora_down_bf16_kernel     T^T = W X^T: both operands k-contiguous, 16-byte loads are the fragments; a lane ends up with four
//                             consecutive T columns of one token (one 8-byte store)
//   lora_up_add_bf16_kernel   Y^T += W^T T^T: a wave keeps the W fragments of its 64 columns in registers for all its rows; the
//                             tile rows are interleaved so that a lane owns 16 consecutive Y columns (two 16-byte read-modify-writes).
//                             Its epilogue is a template parameter: the plain add (QKV, dx), and for the adapters of the dense layers
//                             whose GEMMs end in fused epilogues the add under a dropout mask (o, fc2), the add times the saved
//                             activation derivative (fc2's input gradient) and the add in front of the activation (fc1: h and u)
//   lora_wgrad_bf16_kernel    dW = T^T X: both operands run along the token axis — 32-token stages of T and X in row-major LDS
//                             images, fragments by ds_read_b64_tr_b16 (the situation of gemm_wgrad.hip).  A workgroup owns
//                             (slab of LORA_SLAB token rows, column tile) and stores its fp32 partial [n, tile] with plain stores;
//                             sum_slices_f32 adds the slabs in ascending order, dW's old value last: no float atomics, the
//                             result is a function of the operands and R alone.
// Adapter-input dropout (PEFT's lora_dropout: y = base(x) + s B A dropout(x)): the mask is a template parameter of down and
// wgrad.  It is made in registers from (seed, counter r W + c) — r the row of the operand as passed, W its logical width, not its
// row stride: the counters of mdt_dropout_mask(R W) — and a dropped element of X is replaced by +0 on its way into the MFMA
// fragment (down) or the LDS image (wgrad); 1 / (1 - p) joins alpha as one fp32 factor on the host.  No dropped copy of X exists.
// bf16 arithmetic: v_mfma_f32_16x16x32_bf16, fp32 accumulators; n = 8 (or the last 8 of n = 24, ...) is half a 16-row tile fed
// with zeros.  The fp32 forms are plain loops, one thread per output element: the parity path, not a hot path.
#include "common.hpp"

namespace mdt {

constexpr int LORA_SLAB = 1024;        // token rows per wgrad slab (mdt_lora_wgrad_slab_rows)
constexpr int LORA_LDT = 208;          // T stage image: 416-byte rows, 8 consecutive rows start on 8 different 32-byte bank groups

// ------------------------------------------------------------------------------------------------ down
// A operand = W (rows: the n index), B operand = X (columns: tokens): lane l loads W[t*16 + (l&15)][k0 + 8(l>>4) ..+8] and
// X[row + (l&15)][the same k].  Accumulator: column l&15 = token, rows 4(l>>4) + reg = four consecutive n indices.
//
// The 8 elements of a 16-byte chunk whose first dropout counter is idx_even (even): a dropped one becomes +0 by a select, so
// the kept ones stay exact bf16 and a non-finite value at a dropped position goes no further.
__device__ __forceinline__ bf16x8 lora_mask8(const DropCfg& d, uint64_t idx_even, bf16x8 x) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    float s0, s1;
    drop_scale2(d, idx_even + j, s0, s1);
    x[j] = s0 != 0.f ? x[j] : (bf16_t)0.f;
    x[j + 1] = s1 != 0.f ? x[j + 1] : (bf16_t)0.f;
  }
  return x;
}

// MASK: X is dropped with the counters r K + k of site d (alpha then carries 1 / (1 - p)); d is not read otherwise.
template <int NT, int MT, bool MASK = false>
__global__ __launch_bounds__(256) void lora_down_bf16_kernel(int64_t R, int n, int K, const bf16_t* __restrict__ X, int64_t ldx,
                                                             const bf16_t* __restrict__ W, int64_t ldw, bf16_t* __restrict__ T,
                                                             int64_t ldt, float alpha, DropCfg d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * MT);
  if (row0 >= R) return;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const bf16_t* xp[MT];
  bool xok[MT];
  uint64_t xc[MT];                             // MASK: the counter of the lane's first element at k0 = 0 (K is even: so is xc)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int64_t r = row0 + m * 16 + i;
    xok[m] = r < R;
    xp[m] = X + (xok[m] ? r : 0) * ldx + g * 8;
    xc[m] = (uint64_t)(xok[m] ? r : 0) * K + g * 8;
  }
  const bf16_t* wp[NT];
  bool wok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int wr = t * 16 + i;
    wok[t] = wr < n;
    wp[t] = W + (int64_t)(wok[t] ? wr : 0) * ldw + g * 8;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    const bool kok = k0 + g * 8 < K;           // K is a multiple of 8: a lane's chunk is inside or outside as a whole
    bf16x8 xf[MT], wf[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) xf[m] = (xok[m] && kok) ? *(const bf16x8*)(xp[m] + k0) : zero;
#pragma unroll
    for (int t = 0; t < NT; ++t) wf[t] = (wok[t] && kok) ? *(const bf16x8*)(wp[t] + k0) : zero;
    if constexpr (MASK) {
#pragma unroll
      for (int m = 0; m < MT; ++m) xf[m] = lora_mask8(d, xc[m] + k0, xf[m]);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[m][t] = mfma_bf16(wf[t], xf[m], acc[m][t]);
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int64_t r = row0 + m * 16 + i;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + 4 * g;            // n is a multiple of 8: c < n implies c + 4 <= n
      if (r < R && c < n) {
        const bf16x4 o = {(bf16_t)(alpha * acc[m][t][0]), (bf16_t)(alpha * acc[m][t][1]), (bf16_t)(alpha * acc[m][t][2]),
                          (bf16_t)(alpha * acc[m][t][3])};
        *(bf16x4*)(T + r * ldt + c) = o;
      }
    }
  }
}

template <typename T, bool MASK = false>
__global__ __launch_bounds__(256) void lora_down_plain_kernel(int64_t R, int n, int K, const T* __restrict__ X, int64_t ldx,
                                                              const T* __restrict__ W, int64_t ldw, T* __restrict__ Tm, int64_t ldt,
                                                              float alpha, DropCfg d) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= R * n) return;
  const int64_t r = e / n;
  const int i = (int)(e - r * n);
  const T* x = X + r * ldx;
  const T* w = W + (int64_t)i * ldw;
  float s = 0.f;
  for (int k = 0; k < K; ++k) {
    float xv = to_f32(x[k]);
    if constexpr (MASK) xv = drop_scale(d, (uint64_t)r * K + k) != 0.f ? xv : 0.f;
    s += xv * to_f32(w[k]);
  }
  Tm[r * ldt + i] = from_f32<T>(alpha * s);
}

// ------------------------------------------------------------------------------------------------ up_add
// A operand = W^T (rows: Y columns), B operand = T^T (columns: tokens).  A wave owns the 64 columns cb ... cb + 63 for all rows
// of its workgroup.  Row i of tile t is column cb + (i >> 2) * 16 + t * 4 + (i & 3), so that the accumulators of lane group g
// over the four tiles are the 16 consecutive columns cb + 16 g ... + 15 of token l & 15.
//
// Epilogues (EPI): what happens to p = (T W)[r, c] once it is in the accumulator.  Y is always read in its type, the arithmetic is
// fp32, every stored element is rounded once.
//   UP_ADD    Y = Y + alpha p                                        (mdt_lora_up_add)
//   UP_DROP   Y = Y + (alpha s) p, s the dropout scale of counter r N + c; a dropped element keeps its bits   (..._up_add_drop)
//   UP_MUL    Y = Y + (alpha p) aux                                  (mdt_lora_up_add_mul)
//   UP_MULDROP  Y = Y + (alpha s p) aux, s as in UP_DROP: a dropped element keeps its bits          (..._up_add_mul_drop)
//   UP_ACT+k  v = Y + alpha p (Y: the pre-activation, only read);  h = act_k(v) s,  u = act_k'(v) s, act_pair<k> (mdt_lora_up_act)
enum { UP_ADD = 0, UP_DROP = 1, UP_MUL = 2, UP_MULDROP = 3, UP_ACT = 4 };
template <typename T>
struct UpEpi {
  const T* aux;        // UP_MUL, UP_MULDROP
  int64_t ld_aux;
  T* h;                // UP_ACT: h may be Y; u may be null
  int64_t ld_h;
  T* u;
  int64_t ld_u;
  DropCfg d;           // UP_DROP, UP_MULDROP, UP_ACT (thresh 0: no dropout, every scale 1)
};
// one element: o0 = the new Y (UP_ACT: h), o1 = u.  y: Y's old value, s: the dropout scale, a: aux
template <int EPI>
__device__ __forceinline__ void up_elem(float p, float y, float alpha, float s, float a, float& o0, float& o1) {
  if constexpr (EPI == UP_ADD) o0 = __builtin_fmaf(alpha, p, y);
  else if constexpr (EPI == UP_DROP) o0 = __builtin_fmaf(alpha * s, p, y);
  else if constexpr (EPI == UP_MUL) o0 = __builtin_fmaf(alpha * p, a, y);
  else if constexpr (EPI == UP_MULDROP) o0 = __builtin_fmaf((alpha * s) * p, a, y);
  else act_pair<EPI - UP_ACT>(__builtin_fmaf(alpha, p, y), s, o0, o1);
}

template <int KS, int EPI = UP_ADD>
__global__ __launch_bounds__(256) void lora_up_add_bf16_kernel(int64_t R, int n, int N, const bf16_t* __restrict__ T, int64_t ldt,
                                                               const bf16_t* __restrict__ W, int64_t ldw, bf16_t* __restrict__ Y,
                                                               int64_t ldy, float alpha, int rows_per_wg, UpEpi<bf16_t> E) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int cb = (blockIdx.x * 4 + wave) * 64;
  if (cb >= N) return;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 wf[KS][4];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = cb + (i >> 2) * 16 + t * 4 + (i & 3);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = ks * 32 + 8 * g + j;
        wf[ks][t][j] = (k < n && c < N) ? W[(int64_t)k * ldw + c] : (bf16_t)0.f;
      }
    }
  const int64_t r_begin = (int64_t)blockIdx.y * rows_per_wg;
  const int64_t r_end = r_begin + rows_per_wg < R ? r_begin + rows_per_wg : R;
  const int c0 = cb + 16 * g;                  // N is a multiple of 16: the lane's 16 columns are inside or outside as a whole
  for (int64_t r0 = r_begin; r0 < r_end; r0 += 16) {
    const int64_t r = r0 + i;
    const bool ok = r < r_end;
    bf16x8 tf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) tf[ks] = (ok && ks * 32 + 8 * g < n) ? *(const bf16x8*)(T + r * ldt + ks * 32 + 8 * g) : zero;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = mfma_bf16(wf[ks][t], tf[ks], acc[t]);
    if (ok && c0 < N) {
      bf16_t* y = Y + r * ldy + c0;
      bf16x8 y0 = *(const bf16x8*)y, y1 = *(const bf16x8*)(y + 8);
      if constexpr (EPI == UP_ADD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          y0[j] = (bf16_t)__builtin_fmaf(alpha, acc[j >> 2][j & 3], (float)y0[j]);
          y1[j] = (bf16_t)__builtin_fmaf(alpha, acc[2 + (j >> 2)][j & 3], (float)y1[j]);
        }
        *(bf16x8*)y = y0;
        *(bf16x8*)(y + 8) = y1;
      } else {
        // column c0 + j of the row is acc[j >> 2][j & 3], j = 0 ... 15; its dropout counter r N + c0 + j (c0 and N are multiples
        // of 16: every pair starts on an even counter)
        float s[16];
        const bool drop = EPI != UP_MUL && E.d.thresh != 0;
        constexpr bool keeps = EPI == UP_DROP || EPI == UP_MULDROP;      // a dropped element keeps its bits
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
          if (drop) drop_scale2(E.d, (uint64_t)r * N + c0 + j, s[j], s[j + 1]);
          else s[j] = s[j + 1] = 1.0f;
        }
        bf16x8 a0 = zero, a1 = zero, u0, u1;
        if constexpr (EPI == UP_MUL || EPI == UP_MULDROP) {
          const bf16_t* a = E.aux + r * E.ld_aux + c0;
          a0 = *(const bf16x8*)a;
          a1 = *(const bf16x8*)(a + 8);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float o, v = 0.f;
          up_elem<EPI>(acc[j >> 2][j & 3], (float)y0[j], alpha, s[j], (float)a0[j], o, v);
          if (!keeps || s[j] != 0.f) y0[j] = (bf16_t)o;
          u0[j] = (bf16_t)v;
          up_elem<EPI>(acc[2 + (j >> 2)][j & 3], (float)y1[j], alpha, s[8 + j], (float)a1[j], o, v);
          if (!keeps || s[8 + j] != 0.f) y1[j] = (bf16_t)o;
          u1[j] = (bf16_t)v;
        }
        // h may be Y itself: this lane has read its 16 elements, and no other lane touches them
        bf16_t* out = (EPI < UP_ACT || E.h == Y) ? y : E.h + r * E.ld_h + c0;
        *(bf16x8*)out = y0;
        *(bf16x8*)(out + 8) = y1;
        if constexpr (EPI >= UP_ACT) {
          if (E.u) {
            bf16_t* up = E.u + r * E.ld_u + c0;
            *(bf16x8*)up = u0;
            *(bf16x8*)(up + 8) = u1;
          }
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void lora_up_add_plain_kernel(int64_t R, int n, int N, const T* __restrict__ Tm, int64_t ldt,
                                                                const T* __restrict__ W, int64_t ldw, T* __restrict__ Y, int64_t ldy,
                                                                float alpha) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= R * N) return;
  const int64_t r = e / N;
  const int c = (int)(e - r * N);
  const T* t = Tm + r * ldt;
  float s = 0.f;
  for (int k = 0; k < n; ++k) s += to_f32(t[k]) * to_f32(W[(int64_t)k * ldw + c]);
  T* y = Y + r * ldy + c;
  *y = from_f32<T>(__builtin_fmaf(alpha, s, to_f32(*y)));
}

// the other epilogues, one thread per element (Y is not __restrict__: h may be Y)
template <typename T, int EPI>
__global__ __launch_bounds__(256) void lora_up_epi_plain_kernel(int64_t R, int n, int N, const T* __restrict__ Tm, int64_t ldt,
                                                                const T* __restrict__ W, int64_t ldw, T* Y, int64_t ldy, float alpha,
                                                                UpEpi<T> E) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= R * N) return;
  const int64_t r = e / N;
  const int c = (int)(e - r * N);
  const T* t = Tm + r * ldt;
  float p = 0.f;
  for (int k = 0; k < n; ++k) p += to_f32(t[k]) * to_f32(W[(int64_t)k * ldw + c]);
  const float s = (EPI != UP_MUL && E.d.thresh != 0) ? drop_scale(E.d, (uint64_t)e) : 1.0f;
  const float a = (EPI == UP_MUL || EPI == UP_MULDROP) ? to_f32(E.aux[r * E.ld_aux + c]) : 0.f;
  float o, v = 0.f;
  up_elem<EPI>(p, to_f32(Y[r * ldy + c]), alpha, s, a, o, v);
  if constexpr (EPI >= UP_ACT) {
    E.h[r * E.ld_h + c] = from_f32<T>(o);
    if (E.u) E.u[r * E.ld_u + c] = from_f32<T>(v);
  } else if ((EPI != UP_DROP && EPI != UP_MULDROP) || s != 0.f) {
    Y[r * ldy + c] = from_f32<T>(o);
  }
}

// ------------------------------------------------------------------------------------------------ wgrad
// Fragment of a row-major LDS image img[token][column] for tokens 0 ... 31 and columns c0 ... c0 + 15: element j of lane l is
// img[8 (l >> 4) + j][c0 + (l & 15)] — the A operand (rows: columns of the image) and the B operand alike (attention.hip frag_km).
__device__ __forceinline__ bf16x8 lora_frag_tr(const bf16_t* img, int ld, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const bf16_t* a = img + (g * 8 + q) * ld + c0 + pp * 4;
  const bf16x4 lo = lds_read_tr16(a);
  const bf16x4 hi = lds_read_tr16(a + 4 * ld);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// NT: 16-row tiles of n; CTW: 16-column tiles per wave — a workgroup covers CW = 64 CTW columns.  The stage images hold 32 tokens;
// the next stage's global loads are in flight while the MFMAs of this one run.  MASK: X is dropped with the counters r N + c of
// site d on its way from the load registers into the stage image (alpha then carries 1 / (1 - p)); d is not read otherwise.
template <int NT, int CTW, bool MASK = false>
__global__ __launch_bounds__(256) void lora_wgrad_bf16_kernel(int64_t R, int n, int N, const bf16_t* __restrict__ T, int64_t ldt,
                                                              const bf16_t* __restrict__ X, int64_t ldx, float* __restrict__ ws,
                                                              float alpha, DropCfg d) {
  constexpr int CW = CTW * 64;
  constexpr int LDX = CW + 16;                 // 544 / 288 / 160-byte rows: 8 consecutive rows start on 8 different 32-byte bank groups
  constexpr int XCH = CW / 8;                  // 16-byte chunks per X stage row
  constexpr int TCH = NT * 2;                  // and per T stage row
  constexpr int XU = CTW;                      // X chunks per thread: 32 * XCH / 256
  constexpr int TU = (32 * TCH + 255) / 256;   // T chunks per thread (the last round may be partial)
  __shared__ __attribute__((aligned(16))) bf16_t sx[32 * LDX];
  __shared__ __attribute__((aligned(16))) bf16_t st[32 * LORA_LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cb = blockIdx.x * CW;
  const int64_t slab = blockIdx.y;
  const int64_t r_begin = slab * LORA_SLAB;
  const int64_t r_end = r_begin + LORA_SLAB < R ? r_begin + LORA_SLAB : R;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8 xr[XU], tr[TU];
  auto load = [&](int64_t r0) {
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int id = tid + u * 256, row = id / XCH, c = cb + (id % XCH) * 8;
      const int64_t r = r0 + row;
      xr[u] = (r < r_end && c < N) ? *(const bf16x8*)(X + r * ldx + c) : zero;
    }
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int id = tid + u * 256, row = id / TCH, c = (id % TCH) * 8;
      const int64_t r = r0 + row;
      tr[u] = (id < 32 * TCH && r < r_end && c < n) ? *(const bf16x8*)(T + r * ldt + c) : zero;
    }
  };
  auto stage = [&](int64_t r0) {               // r0: the first row of what load() left in xr / tr
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      const int id = tid + u * 256;
      // rows past r_end and columns past N hold zeros already; c is a multiple of 8 and N of 16: the first counter is even
      if constexpr (MASK) xr[u] = lora_mask8(d, (uint64_t)(r0 + id / XCH) * N + cb + (id % XCH) * 8, xr[u]);
      *(bf16x8*)(sx + (id / XCH) * LDX + (id % XCH) * 8) = xr[u];
    }
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int id = tid + u * 256;
      if (id < 32 * TCH) *(bf16x8*)(st + (id / TCH) * LORA_LDT + (id % TCH) * 8) = tr[u];
    }
  };
  f32x4 acc[NT][CTW];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < CTW; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int wc = wave * CTW * 16;              // the wave's first column inside the workgroup's tile
  load(r_begin);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += 32) {
    __syncthreads();                           // everybody has read the previous stage
    stage(r0);
    __syncthreads();
    if (r0 + 32 < r_end) load(r0 + 32);
    if (cb + wc < N) {
      bf16x8 af[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) af[t] = lora_frag_tr(st, LORA_LDT, t * 16, lane);
#pragma unroll
      for (int c = 0; c < CTW; ++c) {
        const bf16x8 bf = lora_frag_tr(sx, LDX, wc + c * 16, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][c] = mfma_bf16(af[t], bf, acc[t][c]);
      }
    }
  }
  float* out = ws + slab * (int64_t)n * N;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < CTW; ++c) {
      const int col = cb + wc + c * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = t * 16 + 4 * (lane >> 4) + reg;
        if (row < n && col < N) out[(int64_t)row * N + col] = alpha * acc[t][c][reg];
      }
    }
}

// one thread per (n index, column) of a slab: token rows in ascending order
template <typename T, bool MASK = false>
__global__ __launch_bounds__(256) void lora_wgrad_plain_kernel(int64_t R, int n, int N, const T* __restrict__ Tm, int64_t ldt,
                                                               const T* __restrict__ X, int64_t ldx, float* __restrict__ ws,
                                                               float alpha, DropCfg d) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n * N) return;
  const int i = e / N, c = e - i * N;
  const int64_t slab = blockIdx.y;
  const int64_t r_begin = slab * LORA_SLAB;
  const int64_t r_end = r_begin + LORA_SLAB < R ? r_begin + LORA_SLAB : R;
  float s = 0.f;
  for (int64_t r = r_begin; r < r_end; ++r) {
    float xv = to_f32(X[r * ldx + c]);
    if constexpr (MASK) xv = drop_scale(d, (uint64_t)r * N + c) != 0.f ? xv : 0.f;
    s += to_f32(Tm[r * ldt + i]) * xv;
  }
  ws[slab * (int64_t)n * N + e] = alpha * s;
}

// ------------------------------------------------------------------------------------------------ host
// The contract the three entry points share: n a multiple of 8 in 8 ... 192, the wide dimension a multiple of 16, bf16 rows and
// bases on 16-byte boundaries (fp32: 4-byte), row strides at least the width.
struct LoraOperand {
  const char* name;
  const void* p;
  int64_t ld;
  int64_t width;
  int elem;            // bytes per element
};
static int lora_check(const char* fn, int dtype, int64_t R, int n, int wide, const char* wide_name,
                      std::initializer_list<LoraOperand> ops) {
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "%s: dtype %d is neither MDT_F32 nor MDT_BF16", fn, dtype);
  MDT_CHECK_ARG(R >= 0, "%s: R=%lld is negative", fn, (long long)R);
  MDT_CHECK_ARG(n >= 8 && n <= 192 && n % 8 == 0, "%s: n=%d is not a multiple of 8 in 8 ... 192", fn, n);
  MDT_CHECK_ARG(wide >= 16 && wide % 16 == 0, "%s: %s=%d is not a positive multiple of 16", fn, wide_name, wide);
  if (R == 0) return MDT_OK;            // a no-op: an empty tensor has no base to check
  for (const LoraOperand& o : ops) {
    MDT_CHECK_ARG(o.p != nullptr, "%s: %s is a null pointer", fn, o.name);
    MDT_CHECK_ARG(o.ld >= o.width, "%s: row stride of %s (%lld) is shorter than its rows (%lld)", fn, o.name, (long long)o.ld,
                  (long long)o.width);
    const int align = o.elem == 2 ? 16 : 4;
    MDT_CHECK_ARG(((uintptr_t)o.p % align) == 0 && (o.ld * o.elem) % align == 0,
                  "%s: %s (base %p, row stride %lld elements) is not on %d-byte boundaries", fn, o.name, o.p, (long long)o.ld, align);
  }
  return MDT_OK;
}

template <int NT, bool MASK>
static int lora_down_launch(hipStream_t st, int64_t R, int n, int K, const bf16_t* X, int64_t ldx, const bf16_t* W, int64_t ldw,
                            bf16_t* T, int64_t ldt, float alpha, const DropCfg& d) {
  constexpr int MT = NT > 8 ? 1 : 2;
  const int64_t blocks = (R + 64 * MT - 1) / (64 * MT);
  return launch_route<lora_down_bf16_kernel<NT, MT, MASK>>(MASK ? "lora_down_drop" : "lora_down", dim3((unsigned)blocks), dim3(256), 0,
                                                            st, R, n, K, X, ldx, W, ldw, T, ldt, alpha, d);
}

template <int KS, int EPI = UP_ADD>
static int lora_up_launch(hipStream_t st, int64_t R, int n, int N, const bf16_t* T, int64_t ldt, const bf16_t* W, int64_t ldw,
                          bf16_t* Y, int64_t ldy, float alpha, const char* route = "lora_up", const UpEpi<bf16_t>& E = {}) {
  const int rows_per_wg = 256;
  const dim3 grid((unsigned)((N + 255) / 256), (unsigned)((R + rows_per_wg - 1) / rows_per_wg));
  return launch_route<lora_up_add_bf16_kernel<KS, EPI>>(route, grid, dim3(256), 0, st, R, n, N, T, ldt, W, ldw, Y, ldy, alpha,
                                                        rows_per_wg, E);
}

// One of the epilogue forms of up_add (EPI != UP_ADD) in either dtype, after the entry point's checks.  ``route``: the bf16 name.
template <int EPI>
static int lora_up_epi(hipStream_t st, int dtype, const char* route, const char* route_f32, int64_t R, int n, int N, const void* T,
                       int64_t ldt, const void* W, int64_t ldw, void* Y, int64_t ldy, float alpha, const void* aux, int64_t ld_aux,
                       void* h, int64_t ld_h, void* u, int64_t ld_u, const DropCfg& d) {
  if (dtype == MDT_F32) {
    const UpEpi<float> E{(const float*)aux, ld_aux, (float*)h, ld_h, (float*)u, ld_u, d};
    const int64_t blocks = (R * N + 255) / 256;
    return launch_route<lora_up_epi_plain_kernel<float, EPI>>(route_f32, dim3((unsigned)blocks), dim3(256), 0, st, R, n, N, (const float*)T,
                                                              ldt, (const float*)W, ldw, (float*)Y, ldy, alpha, E);
  }
  const UpEpi<bf16_t> E{(const bf16_t*)aux, ld_aux, (bf16_t*)h, ld_h, (bf16_t*)u, ld_u, d};
  const bf16_t *t = (const bf16_t*)T, *w = (const bf16_t*)W;
  bf16_t* y = (bf16_t*)Y;
  const int ks = (n + 31) / 32;
  if (ks <= 1) return lora_up_launch<1, EPI>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha, route, E);
  if (ks <= 2) return lora_up_launch<2, EPI>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha, route, E);
  if (ks <= 3) return lora_up_launch<3, EPI>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha, route, E);
  if (ks <= 4) return lora_up_launch<4, EPI>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha, route, E);
  return lora_up_launch<6, EPI>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha, route, E);
}

template <int NT, int CTW, bool MASK>
static int lora_wgrad_launch(hipStream_t st, int64_t R, int n, int N, int64_t slabs, const bf16_t* T, int64_t ldt, const bf16_t* X,
                             int64_t ldx, float* ws, float alpha, const DropCfg& d) {
  const dim3 grid((unsigned)((N + CTW * 64 - 1) / (CTW * 64)), (unsigned)slabs);
  return launch_route<lora_wgrad_bf16_kernel<NT, CTW, MASK>>(MASK ? "lora_wgrad_drop" : "lora_wgrad", grid, dim3(256), 0, st, R, n, N,
                                                              T, ldt, X, ldx, ws, alpha, d);
}

// what the entry points with a dropout site check on top of lora_check (W: the logical width of the masked operand)
static int lora_drop_check(const char* fn, int64_t R, int N, float drop_p) {
  MDT_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p=%f is not in [0, 1)", fn, drop_p);
  MDT_CHECK_ARG(R * N < DROP_MAX_ELEMS, "%s: dropout site of %lld elements (R=%lld, N=%d; limit 2^33)", fn, (long long)(R * N),
                (long long)R, N);
  return MDT_OK;
}

constexpr int64_t LORA_MAX_ROWS = (int64_t)65535 * 256;     // grid.y of up_add (256 rows) and of wgrad (LORA_SLAB rows)

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_lora_wgrad_slab_rows(void) { return LORA_SLAB; }

// mdt_lora_down (MASK false: drop_p and drop_seed are not looked at) and mdt_lora_down_drop
template <bool MASK>
static int lora_down_any(const char* fn, void* stream, int dtype, int64_t R, int n, int K, const void* X, int64_t ldx, const void* W,
                         int64_t ldw, void* T, int64_t ldt, float alpha, float drop_p, uint64_t drop_seed) {
  const int es = (int)dtype_size(dtype);
  if (int e = lora_check(fn, dtype, R, n, K, "K", {{"X", X, ldx, K, es}, {"W", W, ldw, K, es}, {"T", T, ldt, n, es}})) return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "%s: R=%lld exceeds %lld rows", fn, (long long)R, (long long)LORA_MAX_ROWS);
  DropCfg d{0, 0, 1.0f};
  if constexpr (MASK) {
    if (int e = lora_drop_check(fn, R, K, drop_p)) return e;
    d = make_drop(drop_p, drop_seed);
    alpha *= d.inv_keep;                         // one fp32 factor fl(alpha / (1 - p)), applied where alpha is
  }
  if (R == 0) return MDT_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MDT_F32) {
    const int64_t blocks = (R * n + 255) / 256;
    return launch_route<lora_down_plain_kernel<float, MASK>>(MASK ? "lora_down_drop_f32" : "lora_down_f32", dim3((unsigned)blocks),
                                                              dim3(256), 0, st, R, n, K, (const float*)X, ldx, (const float*)W, ldw,
                                                              (float*)T, ldt, alpha, d);
  }
  const bf16_t *x = (const bf16_t*)X, *w = (const bf16_t*)W;
  bf16_t* t = (bf16_t*)T;
  const int nt = (n + 15) / 16;
  if (nt <= 1) return lora_down_launch<1, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
  if (nt <= 2) return lora_down_launch<2, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
  if (nt <= 3) return lora_down_launch<3, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
  if (nt <= 4) return lora_down_launch<4, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
  if (nt <= 6) return lora_down_launch<6, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
  if (nt <= 8) return lora_down_launch<8, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
  return lora_down_launch<12, MASK>(st, R, n, K, x, ldx, w, ldw, t, ldt, alpha, d);
}

extern "C" int mdt_lora_down(void* stream, int dtype, int64_t R, int n, int K, const void* X, int64_t ldx, const void* W,
                             int64_t ldw, void* T, int64_t ldt, float alpha) {
  return lora_down_any<false>("mdt_lora_down", stream, dtype, R, n, K, X, ldx, W, ldw, T, ldt, alpha, 0.f, 0);
}

extern "C" int mdt_lora_down_drop(void* stream, int dtype, int64_t R, int n, int K, const void* X, int64_t ldx, const void* W,
                                  int64_t ldw, void* T, int64_t ldt, float alpha, float drop_p, uint64_t drop_seed) {
  return lora_down_any<true>("mdt_lora_down_drop", stream, dtype, R, n, K, X, ldx, W, ldw, T, ldt, alpha, drop_p, drop_seed);
}

extern "C" int mdt_lora_up_add(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* W,
                               int64_t ldw, void* Y, int64_t ldy, float alpha) {
  const int es = (int)dtype_size(dtype);
  if (int e = lora_check("mdt_lora_up_add", dtype, R, n, N, "N", {{"T", T, ldt, n, es}, {"W", W, ldw, N, es}, {"Y", Y, ldy, N, es}}))
    return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "mdt_lora_up_add: R=%lld exceeds %lld rows", (long long)R, (long long)LORA_MAX_ROWS);
  if (R == 0) return MDT_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MDT_F32) {
    const int64_t blocks = (R * N + 255) / 256;
    return launch_route<lora_up_add_plain_kernel<float>>("lora_up_f32", dim3((unsigned)blocks), dim3(256), 0, st, R, n, N, (const float*)T,
                                                          ldt, (const float*)W, ldw, (float*)Y, ldy, alpha);
  }
  const bf16_t *t = (const bf16_t*)T, *w = (const bf16_t*)W;
  bf16_t* y = (bf16_t*)Y;
  const int ks = (n + 31) / 32;
  if (ks <= 1) return lora_up_launch<1>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha);
  if (ks <= 2) return lora_up_launch<2>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha);
  if (ks <= 3) return lora_up_launch<3>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha);
  if (ks <= 4) return lora_up_launch<4>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha);
  return lora_up_launch<6>(st, R, n, N, t, ldt, w, ldw, y, ldy, alpha);
}

extern "C" int mdt_lora_up_add_drop(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* W,
                                    int64_t ldw, void* Y, int64_t ldy, float alpha, float drop_p, uint64_t drop_seed) {
  const char* fn = "mdt_lora_up_add_drop";
  const int es = (int)dtype_size(dtype);
  if (int e = lora_check(fn, dtype, R, n, N, "N", {{"T", T, ldt, n, es}, {"W", W, ldw, N, es}, {"Y", Y, ldy, N, es}})) return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "%s: R=%lld exceeds %lld rows", fn, (long long)R, (long long)LORA_MAX_ROWS);
  if (int e = lora_drop_check(fn, R, N, drop_p)) return e;
  if (R == 0) return MDT_OK;
  return lora_up_epi<UP_DROP>((hipStream_t)stream, dtype, "lora_up_drop", "lora_up_drop_f32", R, n, N, T, ldt, W, ldw, Y, ldy, alpha,
                              nullptr, 0, nullptr, 0, nullptr, 0, make_drop(drop_p, drop_seed));
}

extern "C" int mdt_lora_up_add_mul(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* W,
                                   int64_t ldw, void* Y, int64_t ldy, const void* aux, int64_t ld_aux, float alpha) {
  const char* fn = "mdt_lora_up_add_mul";
  const int es = (int)dtype_size(dtype);
  if (int e = lora_check(fn, dtype, R, n, N, "N",
                         {{"T", T, ldt, n, es}, {"W", W, ldw, N, es}, {"Y", Y, ldy, N, es}, {"aux", aux, ld_aux, N, es}}))
    return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "%s: R=%lld exceeds %lld rows", fn, (long long)R, (long long)LORA_MAX_ROWS);
  if (R == 0) return MDT_OK;
  return lora_up_epi<UP_MUL>((hipStream_t)stream, dtype, "lora_up_mul", "lora_up_mul_f32", R, n, N, T, ldt, W, ldw, Y, ldy, alpha, aux,
                             ld_aux, nullptr, 0, nullptr, 0, DropCfg{0, 0, 1.0f});
}

extern "C" int mdt_lora_up_add_mul_drop(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* W,
                                        int64_t ldw, void* Y, int64_t ldy, const void* aux, int64_t ld_aux, float alpha, float drop_p,
                                        uint64_t drop_seed) {
  const char* fn = "mdt_lora_up_add_mul_drop";
  const int es = (int)dtype_size(dtype);
  if (int e = lora_check(fn, dtype, R, n, N, "N",
                         {{"T", T, ldt, n, es}, {"W", W, ldw, N, es}, {"Y", Y, ldy, N, es}, {"aux", aux, ld_aux, N, es}}))
    return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "%s: R=%lld exceeds %lld rows", fn, (long long)R, (long long)LORA_MAX_ROWS);
  if (int e = lora_drop_check(fn, R, N, drop_p)) return e;
  if (R == 0) return MDT_OK;
  return lora_up_epi<UP_MULDROP>((hipStream_t)stream, dtype, "lora_up_mul_drop", "lora_up_mul_drop_f32", R, n, N, T, ldt, W, ldw, Y, ldy,
                                 alpha, aux, ld_aux, nullptr, 0, nullptr, 0, make_drop(drop_p, drop_seed));
}

extern "C" int mdt_lora_up_act(void* stream, int dtype, int kind, int64_t R, int n, int N, const void* T, int64_t ldt, const void* W,
                               int64_t ldw, const void* pre, int64_t ld_pre, void* h, int64_t ld_h, void* u, int64_t ld_u, float alpha,
                               float drop_p, uint64_t drop_seed) {
  const char* fn = "mdt_lora_up_act";
  const int es = (int)dtype_size(dtype);
  MDT_CHECK_ARG(kind >= MDT_ACT_GELU && kind <= MDT_ACT_LINEAR, "%s: kind %d is not an activation (0 ... 4)", fn, kind);
  if (int e = lora_check(fn, dtype, R, n, N, "N",
                         {{"T", T, ldt, n, es}, {"W", W, ldw, N, es}, {"pre", pre, ld_pre, N, es}, {"h", h, ld_h, N, es}}))
    return e;
  if (u)
    if (int e = lora_check(fn, dtype, R, n, N, "N", {{"u", u, ld_u, N, es}})) return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "%s: R=%lld exceeds %lld rows", fn, (long long)R, (long long)LORA_MAX_ROWS);
  if (int e = lora_drop_check(fn, R, N, drop_p)) return e;
  if (R == 0) return MDT_OK;
  hipStream_t st = (hipStream_t)stream;
  const DropCfg d = make_drop(drop_p, drop_seed);
  void* y = const_cast<void*>(pre);        // the kernel's Y operand: only read by this epilogue (written only where h is pre)
#define MDT_UP_ACT(K) \
  case K: return lora_up_epi<UP_ACT + K>(st, dtype, "lora_up_act", "lora_up_act_f32", R, n, N, T, ldt, W, ldw, y, ld_pre, alpha, nullptr, 0, h, ld_h, u, ld_u, d)
  switch (kind) {
    MDT_UP_ACT(MDT_ACT_GELU);
    MDT_UP_ACT(MDT_ACT_RELU);
    MDT_UP_ACT(MDT_ACT_GELU_ACCURATE);
    MDT_UP_ACT(MDT_ACT_TANH);
    default: MDT_UP_ACT(MDT_ACT_LINEAR);
  }
#undef MDT_UP_ACT
}

extern "C" size_t mdt_lora_wgrad_workspace_bytes(int64_t R, int n, int N) {
  if (R <= 0 || n <= 0 || N <= 0) return 0;
  const int64_t slabs = (R + LORA_SLAB - 1) / LORA_SLAB;
  return (size_t)slabs * (size_t)n * (size_t)N * sizeof(float);
}

// mdt_lora_wgrad (MASK false: drop_p and drop_seed are not looked at) and mdt_lora_wgrad_drop
template <bool MASK>
static int lora_wgrad_any(const char* fn, void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* X,
                          int64_t ldx, float* dW, int64_t lddw, float alpha, float drop_p, uint64_t drop_seed, void* workspace,
                          size_t workspace_bytes) {
  const int es = (int)dtype_size(dtype);
  if (int e = lora_check(fn, dtype, R, n, N, "N", {{"T", T, ldt, n, es}, {"X", X, ldx, N, es}, {"dW", dW, lddw, N, 4}})) return e;
  MDT_CHECK_ARG(R <= LORA_MAX_ROWS, "%s: R=%lld exceeds %lld rows", fn, (long long)R, (long long)LORA_MAX_ROWS);
  DropCfg d{0, 0, 1.0f};
  if constexpr (MASK) {
    if (int e = lora_drop_check(fn, R, N, drop_p)) return e;
    d = make_drop(drop_p, drop_seed);
    alpha *= d.inv_keep;
  }
  if (R == 0) return MDT_OK;
  const size_t need = mdt_lora_wgrad_workspace_bytes(R, n, N);
  MDT_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", fn, workspace ? workspace_bytes : (size_t)0, need);
  MDT_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace %p is not 16-byte aligned", fn, workspace);
  hipStream_t st = (hipStream_t)stream;
  const int64_t slabs = (R + LORA_SLAB - 1) / LORA_SLAB;
  float* ws = (float*)workspace;
  int e;
  if (dtype == MDT_F32) {
    const dim3 grid((unsigned)((n * N + 255) / 256), (unsigned)slabs);
    e = launch_route<lora_wgrad_plain_kernel<float, MASK>>(MASK ? "lora_wgrad_drop_f32" : "lora_wgrad_f32", grid, dim3(256), 0, st, R, n, N,
                                                            (const float*)T, ldt, (const float*)X, ldx, ws, alpha, d);
  } else {
    const bf16_t *t = (const bf16_t*)T, *x = (const bf16_t*)X;
    const int nt = (n + 15) / 16;
    if (nt <= 1) e = lora_wgrad_launch<1, 4, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
    else if (nt <= 2) e = lora_wgrad_launch<2, 4, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
    else if (nt <= 3) e = lora_wgrad_launch<3, 4, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
    else if (nt <= 4) e = lora_wgrad_launch<4, 4, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
    else if (nt <= 6) e = lora_wgrad_launch<6, 2, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
    else if (nt <= 8) e = lora_wgrad_launch<8, 2, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
    else e = lora_wgrad_launch<12, 1, MASK>(st, R, n, N, slabs, t, ldt, x, ldx, ws, alpha, d);
  }
  if (e) return e;
  // ascending slab order, dW's old value last
  return sum_slices_f32(st, n, N, (int)slabs, ws, N, (int64_t)n * N, dW, lddw, 1);
}

extern "C" int mdt_lora_wgrad(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* X,
                              int64_t ldx, float* dW, int64_t lddw, float alpha, void* workspace, size_t workspace_bytes) {
  return lora_wgrad_any<false>("mdt_lora_wgrad", stream, dtype, R, n, N, T, ldt, X, ldx, dW, lddw, alpha, 0.f, 0, workspace,
                               workspace_bytes);
}

extern "C" int mdt_lora_wgrad_drop(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt, const void* X,
                                   int64_t ldx, float* dW, int64_t lddw, float alpha, float drop_p, uint64_t drop_seed, void* workspace,
                                   size_t workspace_bytes) {
  return lora_wgrad_any<true>("mdt_lora_wgrad_drop", stream, dtype, R, n, N, T, ldt, X, ldx, dW, lddw, alpha, drop_p, drop_seed,
                              workspace, workspace_bytes);
}
