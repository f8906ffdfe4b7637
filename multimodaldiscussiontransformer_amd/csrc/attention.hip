// Fused self-attention for the three token spaces of mDT (comment text S = nb+L, image
// patches S = nb+P, discussion-tree graph S = N+1): scores, structural / padding bias,
// fp32 softmax and P@V in one kernel; backward recomputes P from the saved log-sum-exp.
//
// One workgroup (4 waves) per (sequence, head); sequences are short (S <= 256), so the
// whole key range of a 16-query tile lives in MFMA accumulators (NT tiles of 16 keys)
// and softmax is a single exact pass — no online rescaling.
//   bf16: v_mfma_f32_16x16x32_bf16; K / V (fwd), then K,V / Q,dO (bwd) staged in LDS
//         (head_dim 64 / 96 / 128: rows padded by 16 B; head_dim 16: 32-B rows, and the upper half of
//         the K = 32 contraction over the head is fed zeros); k-major operands (V in P@V, K in dS@K, dO / Q in the
//         key-tile pass) are fetched with ds_read_b64_tr_b16.
//   fp32: v_mfma_f32_16x16x4_f32 straight from global memory (parity path, exact fp32).
// The Graphormer structural bias (modules/graphormer_layers.py:86-110) is evaluated on
// the fly from int32 spatial_pos + the [num_spatial, H] table and never materialised;
// its gradient is reduced in an LDS histogram and leaves with one atomic per bin.
//
// Replaces modules/multihead_attention.py:139-202 and the eager attention inside HF
// BertLayer / ViTLayer (call sites modules/multi_graphormer_fusion_layer.py:94-96,138-146).
#include <type_traits>

#include <stdlib.h>

#include "attention_common.hpp"

namespace mdt {

template <typename T> struct MM;
template <> struct MM<float> {
  static constexpr int KS = 4;
  typedef float frag;
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return mfma_f32(a, b, c); }
};
template <> struct MM<bf16_t> {
  static constexpr int KS = 32;
  typedef bf16x8 frag;
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return mfma_bf16(a, b, c); }
};

// Row-major [rows][ld] operand.  fp32: global memory, row index clamped to rows-1
// (padded positions re-read the last real row: finite, and always masked).  bf16: an LDS
// image (zero-filled padding) or global memory for the wave-private 16-row tiles.
template <typename T> struct Src {
  const T* p;
  int64_t ld;
  int rows;
};

// fragment of a 16 x KS block whose rows are the MFMA row (A) or column (B) index and
// whose k runs along the contiguous axis:  element(rc, k) = p[rc*ld + k]
// KW (bf16): the k columns that exist from k0 on, 32 or 16 (a 16-wide head).  With 16, lanes 32-63 hold k = 16 .. 31:
// columns of the next head or the next row, which they never read — they re-read chunk lane >> 4 & 1 of their own row;
// the fragment from global memory becomes zeros there, the LDS one keeps the (finite) values it re-read: every
// contraction over a head pairs one of each.
template <typename T, bool LDS, int KW = 32>
__device__ __forceinline__ typename MM<T>::frag frag_kc(const Src<T>& s, int rc0, int k0, int lane) {
  int rc = rc0 + (lane & 15);
  if (rc > s.rows - 1) rc = s.rows - 1;
  if constexpr (std::is_same<T, float>::value) {
    return s.p[rc * s.ld + k0 + (lane >> 4)];
  } else {
    static_assert(KW == 32 || KW == 16, "a whole K = 32 step, or half of one");
    const int g = lane >> 4;
    const bf16_t* a = s.p + rc * s.ld + k0 + 8 * (KW == 32 ? g : g & 1);
    if constexpr (LDS) return *(const __attribute__((address_space(3))) bf16x8*)LDS_PTR(a);
    else if constexpr (KW == 32) return *(const bf16x8*)a;
    else {
      const bf16x8 v = *(const bf16x8*)a;      // every lane loads (its own row): the zeros are a select, not a lane mask
      return g < 2 ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
}

// fragment of a KS x 16 block stored k-major: element(k, c) = p[k*ld + c]  (B operand)
template <typename T>
__device__ __forceinline__ typename MM<T>::frag frag_km(const Src<T>& s, int c0, int k0, int lane) {
  if constexpr (std::is_same<T, float>::value) {
    int k = k0 + (lane >> 4);
    if (k > s.rows - 1) k = s.rows - 1;
    return s.p[k * s.ld + c0 + (lane & 15)];
  } else {
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const bf16_t* a = s.p + (k0 + g * 8 + q) * s.ld + c0 + pp * 4;
    const bf16x4 lo = lds_read_tr16(a);
    const bf16x4 hi = lds_read_tr16(a + 4 * s.ld);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  }
}

// bf16 LDS image row stride in elements: 64 + 8 (144 B), or 16 unpadded (32 B: the row reads of a ds_read_b128 lane group
// fall on sixteen different 16-byte slots as they are — attention_v2.hip v2_ld; the k-major reads of frag_km, rows
// k0 .. k0 + 3 and k0 + 8 .. k0 + 11 per half wave, are 2-way there, on images of 1-3 KiB that these tiny rows hardly read)
// 96 / 128: 208- and 272-byte rows.  frag_km's rows k0 .. k0 + 3 and k0 + 8 .. k0 + 11 are 2-way at every stride that is a
// multiple of 16 bytes (8 rows apart is 0 or 128 bytes mod 256), so no padding makes these kernels conflict-free; + 8 is the
// one with which the 17-tile rung of 96-wide heads still fits LDS (attn_v1_fits, attention_common.hpp).
template <int HD> constexpr int IMG_LD = attn_v1_ld(HD);

// Stage a [S][HD] bf16 operand (rows = sequence positions) into an LDS image, zero padded
// to rows_pad rows.
template <int HD>
__device__ __forceinline__ void stage_image(bf16_t* img, const bf16_t* g, int64_t g_ld, int S, int rows_pad, int tid) {
  constexpr int CH = HD / 8;  // 16-B chunks per row
  for (int e = tid; e < rows_pad * CH; e += 256) {
    const int r = e / CH, c = e - r * CH;
    bf16x8 v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (r < S) v = *(const bf16x8*)(g + r * g_ld + c * 8);
    *(bf16x8*)(img + r * IMG_LD<HD> + c * 8) = v;
  }
}

template <typename T>
__device__ __forceinline__ int scratch_ld(int s_pad32) { return s_pad32 + (std::is_same<T, float>::value ? 1 : 8); }

// ---------------------------------------------------------------------------- forward
template <typename T, int HD, int NT, bool STRUCT, bool DROP>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnParams P) {
  constexpr bool BF = !std::is_same<T, float>::value;
  constexpr int KS = MM<T>::KS;
  constexpr int KW = (BF && HD < KS) ? HD : 32;          // bf16, 16-wide head: half a contraction step (frag_kc)
  constexpr int ND = HD / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const mdt_attn_fwd_args& a = P.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the item's setup, written out (attn_item, attention_common.hpp, says why)
  const int h = blockIdx.x, seq = blockIdx.y;
  const int SL = a.S, D = a.H * HD;                      // SL: lse / dropout-counter geometry
  const int S = a.seq_offsets ? a.seq_offsets[seq + 1] - a.seq_offsets[seq] : a.S;   // this sequence's length
  constexpr int s_pad32 = (NT * 16 + 31) & ~31;  // key range every tile loop covers
  const int64_t row0 = a.seq_offsets ? (int64_t)a.seq_offsets[seq] : (int64_t)seq * a.seq_stride;
  const T* qkv = (const T*)a.qkv + row0 * a.ld_qkv + h * HD;
  const int64_t tld = a.pos_stride * a.ld_qkv;  // row stride between consecutive positions

  Src<T> srcK, srcV;
  T* scratch;
  if constexpr (BF) {
    bf16_t* imgK = (bf16_t*)smem;
    bf16_t* imgV = imgK + s_pad32 * IMG_LD<HD>;
    stage_image<HD>(imgK, qkv + D, tld, S, s_pad32, tid);
    stage_image<HD>(imgV, qkv + 2 * D, tld, S, s_pad32, tid);
    srcK = Src<T>{imgK, IMG_LD<HD>, s_pad32};
    srcV = Src<T>{imgV, IMG_LD<HD>, s_pad32};
    scratch = (T*)(imgV + s_pad32 * IMG_LD<HD>) + wave * 16 * scratch_ld<T>(s_pad32);
    __syncthreads();
  } else {
    srcK = Src<T>{qkv + D, tld, S};
    srcV = Src<T>{qkv + 2 * D, tld, S};
    scratch = (T*)smem + wave * 16 * scratch_ld<T>(s_pad32);
  }
  const int sld = scratch_ld<T>(s_pad32);
  const Src<T> srcQ{qkv, tld, S};
  const Src<T> srcP{scratch, sld, 16};
  BiasCtx bc{seq, h, S, a.H, a.key_mask, a.key_pad, a.dense_bias, a.attn_bias, a.spatial_pos, a.sp_table, a.virt};   // written out: see bias_ctx

  float colb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) colb[t] = key_only_bias<T>(bc, t * 16 + (lane & 15));
  // zero the k-padding columns of the scratch rows once (columns >= NT*16 up to s_pad32)
  if constexpr (s_pad32 > NT * 16) {
    for (int e = lane; e < 16 * (s_pad32 - NT * 16); e += 64) {
      const int r = e / (s_pad32 - NT * 16), c = NT * 16 + e % (s_pad32 - NT * 16);
      scratch[r * sld + c] = from_f32<T>(0.f);
    }
  }

  const int n_qt = (S + 15) >> 4;
  for (int qt = wave; qt < n_qt; qt += 4) {
    const int q0 = qt * 16;
    f32x4 sc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k0 = 0; k0 < HD; k0 += KS) {
      const typename MM<T>::frag fa = frag_kc<T, false, KW>(srcQ, q0, k0, lane);
#pragma unroll
      for (int t = 0; t < NT; ++t) sc[t] = MM<T>::mma(fa, frag_kc<T, BF, KW>(srcK, t * 16, k0, lane), sc[t]);
    }
    // bias + softmax (rows = (lane>>4)*4 + r, cols = t*16 + (lane&15))
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int key = t * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sc[t][r] * a.scale + colb[t];
        if (a.dense_bias || STRUCT) {
          int q = q0 + (lane >> 4) * 4 + r;
          if (q > S - 1) q = S - 1;
          if (key < S) v += pair_bias<T, STRUCT>(bc, q, key);
        }
        sc[t][r] = v;
        mx[r] = fmaxf(mx[r], v);
      }
    }
    float sum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { mx[r] = row16_max(mx[r]); sum[r] = 0.f; }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = (sc[t][r] == -INFINITY) ? 0.f : __expf(sc[t][r] - mx[r]);
        sc[t][r] = e;
        sum[r] += e;
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sum[r] = row16_sum(sum[r]);
      const int q = q0 + (lane >> 4) * 4 + r;
      if ((lane & 15) == 0 && q < S && a.lse)
        a.lse[((int64_t)seq * a.H + h) * SL + q] = (sum[r] > 0.f) ? mx[r] + __logf(sum[r]) : -INFINITY;
      sum[r] = (sum[r] > 0.f) ? 1.0f / sum[r] : 0.f;
    }
    const int drop_bh = seq * a.H + h;   // counters: attention_common.hpp
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv = sc[t][r] * sum[r];
        if constexpr (DROP) {
          const int q = q0 + (lane >> 4) * 4 + r, key = t * 16 + (lane & 15);
          pv *= attn_drop_scale(P.drop, drop_bh, SL, q, key);
        }
        scratch[((lane >> 4) * 4 + r) * sld + t * 16 + (lane & 15)] = from_f32<T>(pv);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // O = P @ V
    f32x4 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kmax = BF ? s_pad32 : NT * 16;
    for (int k0 = 0; k0 < kmax; k0 += KS) {
      const typename MM<T>::frag fp = frag_kc<T, true>(srcP, 0, k0, lane);
#pragma unroll
      for (int d = 0; d < ND; ++d) o[d] = MM<T>::mma(fp, frag_km<T>(srcV, d * 16, k0, lane), o[d]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // scratch is rewritten by the next q tile
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = q0 + (lane >> 4) * 4 + r;
        if (q < S)
          ((T*)a.out)[(row0 + (int64_t)q * a.pos_stride) * a.ld_out + h * HD + d * 16 + (lane & 15)] = from_f32<T>(o[d][r]);
      }
  }
}

// ---------------------------------------------------------------------------- backward
// Pass A (per 16-query tile): S, P, dP = dO V^T, delta = rowsum(P*dP), dS = P*(dP-delta),
//                             dQ = scale * dS K, bias gradients.
// Pass B (per 16-key tile):   S^T, P^T, dP^T = V dO^T, dS^T, dV = P^T dO, dK = scale * dS^T Q.
template <typename T, int HD, int NT, bool STRUCT, bool DROP>
__global__ __launch_bounds__(256) void attn_bwd_kernel(AttnParams P) {
  constexpr bool BF = !std::is_same<T, float>::value;
  constexpr int KS = MM<T>::KS;
  constexpr int KW = (BF && HD < KS) ? HD : 32;          // bf16, 16-wide head: half a contraction step (frag_kc)
  constexpr int ND = HD / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const mdt_attn_fwd_args& a = P.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the item's setup, written out (attn_item, attention_common.hpp, says why)
  const int h = blockIdx.x, seq = blockIdx.y;
  const int SL = a.S, D = a.H * HD;                      // SL: lse / dropout-counter geometry
  const int S = a.seq_offsets ? a.seq_offsets[seq + 1] - a.seq_offsets[seq] : a.S;   // this sequence's length
  constexpr int s_pad32 = (NT * 16 + 31) & ~31;  // key range every tile loop covers
  const int64_t row0 = a.seq_offsets ? (int64_t)a.seq_offsets[seq] : (int64_t)seq * a.seq_stride;
  const T* qkv = (const T*)a.qkv + row0 * a.ld_qkv + h * HD;
  const T* dout = (const T*)P.dout + row0 * P.ld_dout + h * HD;
  T* dqkv = (T*)P.dqkv + row0 * P.ld_dqkv + h * HD;
  const int64_t tld = a.pos_stride * a.ld_qkv, dld = a.pos_stride * P.ld_dout, gld = a.pos_stride * P.ld_dqkv;
  const int sld = scratch_ld<T>(s_pad32);

  // LDS carve: [delta S_pad32 f32][lse S_pad32 f32][hist (num_spatial+1) f32]
  //            [image0][image1] (bf16 only) [scratch 4 waves]
  float* s_delta = (float*)smem;
  float* s_lse = s_delta + s_pad32;
  float* s_hist = s_lse + s_pad32;
  const int nhist = STRUCT ? attn_hist_size(a.num_spatial) : 0;
  char* after = (char*)(s_hist + nhist);
  bf16_t* img0 = (bf16_t*)after;
  bf16_t* img1 = img0 + (BF ? s_pad32 * IMG_LD<HD> : 0);
  T* scratch = (T*)(img1 + (BF ? s_pad32 * IMG_LD<HD> : 0)) + wave * 16 * sld;
  const Src<T> srcX{scratch, sld, 16};

  for (int i = tid; i < s_pad32; i += 256) {
    s_lse[i] = (i < S) ? a.lse[((int64_t)seq * a.H + h) * SL + i] : 0.f;
    s_delta[i] = 0.f;
  }
  for (int i = tid; i < nhist; i += 256) s_hist[i] = 0.f;

  Src<T> srcK, srcV;
  if constexpr (BF) {
    stage_image<HD>(img0, qkv + D, tld, S, s_pad32, tid);
    stage_image<HD>(img1, qkv + 2 * D, tld, S, s_pad32, tid);
    srcK = Src<T>{img0, IMG_LD<HD>, s_pad32};
    srcV = Src<T>{img1, IMG_LD<HD>, s_pad32};
  } else {
    srcK = Src<T>{qkv + D, tld, S};
    srcV = Src<T>{qkv + 2 * D, tld, S};
  }
  if constexpr (s_pad32 > NT * 16) {
    for (int e = lane; e < 16 * (s_pad32 - NT * 16); e += 64) {
      const int r = e / (s_pad32 - NT * 16), c = NT * 16 + e % (s_pad32 - NT * 16);
      scratch[r * sld + c] = from_f32<T>(0.f);
    }
  }
  __syncthreads();

  const BiasCtx bc = bias_ctx(a, seq, h, S);
  const int drop_bh = seq * a.H + h;   // counters: attention_common.hpp
  const Src<T> gQ{qkv, tld, S};
  const Src<T> gDO{dout, dld, S};
  const int n_t = (S + 15) >> 4;
  const int kmax = BF ? s_pad32 : NT * 16;

  // ------------------------------------------------------------------ pass A
  {
    float colb[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) colb[t] = key_only_bias<T>(bc, t * 16 + (lane & 15));
    for (int qt = wave; qt < n_t; qt += 4) {
      const int q0 = qt * 16;
      f32x4 sc[NT], dp[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) { sc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int k0 = 0; k0 < HD; k0 += KS) {
        const typename MM<T>::frag fq = frag_kc<T, false, KW>(gQ, q0, k0, lane);
        const typename MM<T>::frag fo = frag_kc<T, false, KW>(gDO, q0, k0, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          sc[t] = MM<T>::mma(fq, frag_kc<T, BF, KW>(srcK, t * 16, k0, lane), sc[t]);
          dp[t] = MM<T>::mma(fo, frag_kc<T, BF, KW>(srcV, t * 16, k0, lane), dp[t]);
          if (t & 1) __builtin_amdgcn_sched_barrier(0);   // bound operand prefetch depth (registers -> occupancy)
        }
      }
      float del[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int key = t * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int q = q0 + (lane >> 4) * 4 + r;
          const bool qok = q < S;
          if (q > S - 1) q = S - 1;
          float v = sc[t][r] * a.scale + colb[t];
          if ((a.dense_bias || STRUCT) && key < S) v += pair_bias<T, STRUCT>(bc, q, key);
          const float l = s_lse[q];
          const float p = (v == -INFINITY || l == -INFINITY || !qok) ? 0.f : __expf(v - l);
          sc[t][r] = p;
          if constexpr (DROP) dp[t][r] *= attn_drop_scale(P.drop, drop_bh, SL, q, key);   // dP = dD * M / (1-p)
          del[r] += p * dp[t][r];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        del[r] = row16_sum(del[r]);
        const int q = q0 + (lane >> 4) * 4 + r;
        if ((lane & 15) == 0 && q < S) s_delta[q] = del[r];
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int key = t * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ds = sc[t][r] * (dp[t][r] - del[r]);
          const int q = q0 + (lane >> 4) * 4 + r;
          scratch[((lane >> 4) * 4 + r) * sld + key] = from_f32<T>(ds);
          if (q < S && key < S) attn_bias_grad_add<STRUCT>(P, s_hist, seq, h, S, q, key, ds);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      f32x4 dq[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) dq[d] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < kmax; k0 += KS) {
        const typename MM<T>::frag fs = frag_kc<T, true>(srcX, 0, k0, lane);
#pragma unroll
        for (int d = 0; d < ND; ++d) dq[d] = MM<T>::mma(fs, frag_km<T>(srcK, d * 16, k0, lane), dq[d]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + (lane >> 4) * 4 + r;
          if (q < S) dqkv[(int64_t)q * gld + d * 16 + (lane & 15)] = from_f32<T>(dq[d][r] * a.scale);
        }
    }
  }
  __syncthreads();  // delta complete; K / V images no longer needed
  Src<T> srcQ, srcDO;
  if constexpr (BF) {
    stage_image<HD>(img0, qkv, tld, S, s_pad32, tid);
    stage_image<HD>(img1, dout, dld, S, s_pad32, tid);
    srcQ = Src<T>{img0, IMG_LD<HD>, s_pad32};
    srcDO = Src<T>{img1, IMG_LD<HD>, s_pad32};
    __syncthreads();
  } else {
    srcQ = gQ;
    srcDO = gDO;
  }
  if constexpr (STRUCT) attn_bias_grad_flush(P, s_hist, h, tid, 256);
  // ------------------------------------------------------------------ pass B
  {
    const Src<T> gK{qkv + D, tld, S};
    const Src<T> gV{qkv + 2 * D, tld, S};
    for (int kt = wave; kt < n_t; kt += 4) {
      const int key0 = kt * 16;
      f32x4 sc[NT], dp[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) { sc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
      for (int k0 = 0; k0 < HD; k0 += KS) {
        const typename MM<T>::frag fk = frag_kc<T, false, KW>(gK, key0, k0, lane);
        const typename MM<T>::frag fv = frag_kc<T, false, KW>(gV, key0, k0, lane);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          sc[t] = MM<T>::mma(fk, frag_kc<T, BF, KW>(srcQ, t * 16, k0, lane), sc[t]);
          dp[t] = MM<T>::mma(fv, frag_kc<T, BF, KW>(srcDO, t * 16, k0, lane), dp[t]);
          if (t & 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
      // rows = keys key0 + (lane>>4)*4 + r, cols = queries t*16 + (lane&15)
      float kb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) kb[r] = key_only_bias<T>(bc, key0 + (lane >> 4) * 4 + r);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int q = t * 16 + (lane & 15);
        const bool qok = q < S;
        const int qc = qok ? q : S - 1;
        const float l = s_lse[qc], de = s_delta[qc];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + (lane >> 4) * 4 + r;
          float v = sc[t][r] * a.scale + kb[r];
          if ((a.dense_bias || STRUCT) && key < S) v += pair_bias<T, STRUCT>(bc, qc, key);
          const float p = (v == -INFINITY || l == -INFINITY || !qok) ? 0.f : __expf(v - l);
          float ds = dp[t][r];
          float pd = p;
          if constexpr (DROP) {
            const float m = attn_drop_scale(P.drop, drop_bh, SL, qc, key);
            ds *= m;                          // dP^T = dD^T * M / (1-p)
            pd *= m;                          // D^T  = P^T * M / (1-p)
          }
          sc[t][r] = pd;                      // (dropped) P^T, the operand of dV
          dp[t][r] = p * (ds - de);           // dS^T
        }
      }
      // dV = P^T dO
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) scratch[((lane >> 4) * 4 + r) * sld + t * 16 + (lane & 15)] = from_f32<T>(sc[t][r]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      f32x4 acc[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < kmax; k0 += KS) {
        const typename MM<T>::frag fs = frag_kc<T, true>(srcX, 0, k0, lane);
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = MM<T>::mma(fs, frag_km<T>(srcDO, d * 16, k0, lane), acc[d]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + (lane >> 4) * 4 + r;
          if (key < S) dqkv[(int64_t)key * gld + 2 * D + d * 16 + (lane & 15)] = from_f32<T>(acc[d][r]);
        }
      // dK = scale * dS^T Q
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) scratch[((lane >> 4) * 4 + r) * sld + t * 16 + (lane & 15)] = from_f32<T>(dp[t][r]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int d = 0; d < ND; ++d) acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < kmax; k0 += KS) {
        const typename MM<T>::frag fs = frag_kc<T, true>(srcX, 0, k0, lane);
#pragma unroll
        for (int d = 0; d < ND; ++d) acc[d] = MM<T>::mma(fs, frag_km<T>(srcQ, d * 16, k0, lane), acc[d]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + (lane >> 4) * 4 + r;
          if (key < S) dqkv[(int64_t)key * gld + D + d * 16 + (lane & 15)] = from_f32<T>(acc[d][r] * a.scale);
        }
    }
  }
}

// materialised structural bias (API parity with GraphAttnBias.forward)
template <typename T>
__global__ void graph_attn_bias_kernel(int nseq, int S, int H, const float* attn_bias, const int32_t* sp, const T* table,
                                       const T* virt, float* out) {
  const int64_t n = (int64_t)nseq * H * S * S;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int key = (int)(i % S);
    const int q = (int)((i / S) % S);
    const int h = (int)((i / ((int64_t)S * S)) % H);
    const int seq = (int)(i / ((int64_t)S * S * H));
    BiasCtx bc{seq, h, S, H, nullptr, nullptr, nullptr, attn_bias, sp, table, virt};
    out[i] = pair_bias<T, true>(bc, q, key);
  }
}

// Head-averaged attention probabilities (modules/multihead_attention.py:205-214, need_weights=True): recomputed from the
// saved q, k and the forward's log-sum-exp — one thread per (sequence, query, key), looping over the heads.  Module-level
// API only (the encoder layers pass need_weights=False); fp32 output [nseq, S, S], masked keys give 0.
template <typename T>
__global__ __launch_bounds__(256) void attn_mean_probs_kernel(mdt_attn_fwd_args a, float* out) {
  const int S = a.S, H = a.H, hd = a.hd;
  const int64_t n = (int64_t)a.nseq * S * S;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int key = (int)(i % S), q = (int)((i / S) % S), seq = (int)(i / ((int64_t)S * S));
    const T* qrow = (const T*)a.qkv + ((int64_t)seq * a.seq_stride + (int64_t)q * a.pos_stride) * a.ld_qkv;
    const T* krow = (const T*)a.qkv + ((int64_t)seq * a.seq_stride + (int64_t)key * a.pos_stride) * a.ld_qkv + (int64_t)H * hd;
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
      const BiasCtx bc = bias_ctx(a, seq, h, S);
      float v = key_only_bias<T>(bc, key);
      if (v == 0.f) {
        float dot = 0.f;
        for (int d = 0; d < hd; ++d) dot += to_f32(qrow[h * hd + d]) * to_f32(krow[h * hd + d]);
        v = dot * a.scale + (a.attn_bias ? pair_bias<T, true>(bc, q, key) : pair_bias<T, false>(bc, q, key));
        const float l = a.lse[((int64_t)seq * H + h) * S + q];
        acc += (v == -INFINITY || l == -INFINITY) ? 0.f : __expf(v - l);
      }
    }
    out[i] = acc / (float)H;
  }
}

// ---------------------------------------------------------------------------- the plan of a launch
// The routing table of the attention family: which kernel a launch takes and at which geometry, as a pure host function of
// the argument block.  Everything else reads it: dispatch() below switches on the route, the three launchers turn the numbers
// into template arguments, mdt_attention_route reports it without launching (tests/test_attention_plan_cpu.py holds it
// against tests/attention_reference.py over the whole domain).  S <= 272 is what one workgroup holds of a (sequence, head).
//
// Refused before any route: seq_ids / s_cap (the length bins of a ragged set) on anything but a ragged bf16 launch with
// head_dim 64 and S <= 272; a head width other than 16, 64, 96 or 128.
// Forward and backward, in order:
//   S > 272                                              -> long (attention_long.hip: key-chunked, any length; takes neither
//                                                           ragged sequences nor q_limit and refuses them)
//   fp32                                                 -> v1 (attention.hip: the exact-fp32 parity path), but the backward
//                                                           of head_dim 96 | 128, S 209 .. 272 (the 17-tile rung) with structural
//                                                           bias AND dropout -> long: that v1 instantiation needs 512
//                                                           registers and 15-17 more in scratch memory and is not built
//                                                           (a structural bias is never ragged; q_limit is ignored there as v1 ignores it)
//   bf16, a dense bias without structural terms          -> v1 (the only bf16 kernels that take one); 128-wide heads of more
//                                                           than 208 tokens -> long (the v1 images do not fit LDS: attn_v1_fits)
// The bf16 forward otherwise                             -> v2 (attention_v2.hip: P stays in registers; length bins too), on
//                                                           the rung of the launch's longest sequence (cap: s_cap, else S)
// The bf16 backward otherwise (head_dim 16, 64, 96 or 128; S <= 272; length-binned launches, 64 only: s_cap <= 272), in order:
//   length-binned launches (seq_ids / s_cap)              -> the family below
//   S > 256 (ViT-L/14: 4 + 257 tokens)                   -> family
//   S <= 80, q_limit == 0, structural bias               -> v1 (LDS-scratch kernel: tiny graphs)
//   no dropout, q_limit == 0, S <= 112                   -> v2 (whole row in registers; with dropout it falls to 1 wave / SIMD)
//   otherwise                                            -> family
// The family, without a structural bias, where the one-pass dS image fits LDS (S <= 208): v5 (9-13 key tiles, persistent),
// v4x (<= 6 key tiles: delta = sum P o dP summed in the kernel, in fp32), v4 (7-8 key tiles); past that, and with a
// structural bias: the two-pass v3.  Measured at C2 shapes: profiles/round1_attention_v2.txt, tools/attn_onepass_ab.py.
// The one-pass kernels are written for 64-wide heads: with head_dim 16, 96 or 128 the family is always v3.
// MDT_ATTN_BWD=<kernel> takes that kernel for a bf16 backward wherever its preconditions (ok() below) hold.  v1 and v2 never
// see q_limit or length bins (they would read the out / lse rows the v2 forward skipped — unwritten memory; tests:
// ..._never_reads_what_forward_did_not_write), v2 takes S <= 112 only, the one-pass kernels take no structural bias.
// Runs on every attention launch: no allocation, no getenv, no HIP call but the cached device_cus().
static AttnPlan refuse(AttnPlan pl) { pl.status = MDT_ERR_UNSUPPORTED; return pl; }

static AttnPlan plan_long(AttnPlan pl, const mdt_attn_fwd_args& a) {
  // S <= 272 comes here for a plain dense bias on 128-wide heads and for the fp32 backward above: never ragged, and q_limit
  // is ignored as the kernels of this file ignore it — every row is computed
  if (a.seq_offsets || (a.q_limit > 0 && a.S > 272)) {
    set_error("attention: S=%d exceeds the 272-token limit of the single-pass kernels and the key-chunked path takes neither "
              "ragged sequences nor q_limit (text / image sequences are always shorter)", a.S);
    return refuse(pl);
  }
  if (!attn_head_dim_ok(a.hd)) { set_error("attention (long sequences): head_dim %d unsupported (16, 64, 96 or 128)", a.hd); return refuse(pl); }
  pl.route = AttnRoute::long_;
  return pl;
}

AttnPlan attn_plan(const AttnParams& p, bool bwd) {
  const mdt_attn_fwd_args& a = p.f;
  AttnPlan pl{};
  pl.bwd = bwd;
  pl.st_bias = a.attn_bias != nullptr;
  pl.drop = a.drop_p > 0.f;
  pl.binned = a.seq_ids != nullptr || a.s_cap > 0;
  pl.dense_only = (a.dense_bias != nullptr || p.d_dense_bias != nullptr) && !pl.st_bias;
  pl.cap = a.s_cap > 0 ? a.s_cap : a.S;
  pl.n_t = (pl.cap + 15) / 16;
  pl.nhist = (bwd && pl.st_bias) ? attn_hist_size(a.num_spatial) : 0;
  const bool bf = a.dtype == MDT_BF16;
  if (pl.binned) {
    if (a.S > 272 || !bf || a.hd != 64 || !a.seq_offsets) {
      set_error("attention: seq_ids / s_cap are for ragged bf16 launches with head_dim 64 and S <= 272");
      return refuse(pl);
    }
  } else if (a.S > 272) return plan_long(pl, a);      // discussion trees with more than 271 comments
  if (!attn_head_dim_ok(a.hd)) {
    set_error(bf ? "attention(bf16): head_dim %d unsupported (16, 64, 96 or 128)" : "attention: head_dim %d unsupported (16, 64, 96 or 128)", a.hd);
    return refuse(pl);
  }
  if (bf && pl.dense_only && !attn_v1_fits(a.hd, a.S)) return plan_long(pl, a);
  const bool one_pass = a.hd == 64 && !pl.st_bias && !pl.dense_only && attn_one_pass_lds_bytes(pl.n_t) <= ATTN_LDS_MAX && pl.n_t <= 16;
  pl.rows_img = attn_one_pass_rows(pl.n_t);
  pl.ldq = attn_one_pass_ldq(pl.n_t);
  auto ok = [&](AttnRoute r) {
    switch (r) {
      case AttnRoute::v1: return !pl.binned && a.q_limit == 0 && attn_v1_fits(a.hd, a.S);
      case AttnRoute::v2: return !pl.binned && !pl.dense_only && a.q_limit == 0 && a.S <= 112;
      case AttnRoute::v3: return !pl.dense_only;
      case AttnRoute::v4: return one_pass;
      case AttnRoute::v4x: return one_pass && pl.n_t <= 2 * V4_EXACT_PAIRS;
      case AttnRoute::v5: return one_pass && pl.n_t > 8 && pl.rows_img * 8 <= 4 * 512;     // long rows (one workgroup per CU by LDS)
      default: return false;
    }
  };
  if (!bf) pl.route = AttnRoute::v1;
  else if (!bwd) pl.route = pl.dense_only ? AttnRoute::v1 : AttnRoute::v2;
  else {
    const AttnRoute family = ok(AttnRoute::v5) ? AttnRoute::v5 : ok(AttnRoute::v4x) ? AttnRoute::v4x : one_pass ? AttnRoute::v4 : AttnRoute::v3;
    if (pl.binned) pl.route = family;
    else if (pl.dense_only) pl.route = AttnRoute::v1;
    else if (a.S > 256) pl.route = family;
    else if (a.S <= 80 && a.q_limit == 0 && pl.st_bias) pl.route = AttnRoute::v1;
    else if (!pl.drop && ok(AttnRoute::v2)) pl.route = AttnRoute::v2;
    else pl.route = family;
    const AttnRoute forced = switches().attn_bwd;
    if (forced != AttnRoute::none && ok(forced)) pl.route = forced;
  }
  switch (pl.route) {
    case AttnRoute::v1: {
      pl.rung = attn_rung<2, 5, 7, 9, 13, 17>((a.S + 15) / 16);      // 17 tiles: ViT-L/14, 4 + 257 tokens
      if (!pl.rung) { set_error("attention: S=%d exceeds the 272-token limit of the single-pass kernel", a.S); return refuse(pl); }
      const size_t lds = attn_v1_lds_bytes(bf, a.hd, pl.rung, bwd, pl.nhist);
      if (lds > ATTN_LDS_MAX) {
        set_error(bwd ? "attention_bwd (v1): S=%d with head_dim %d needs %zu bytes of LDS" : "attention (v1): S=%d with head_dim %d needs %zu bytes of LDS", a.S, a.hd, lds);
        return refuse(pl);
      }
      if (!bf && bwd && a.hd > 64 && pl.rung == 17 && pl.st_bias && pl.drop) return plan_long(pl, a);      // the fp32 line of the table
      break;
    }
    case AttnRoute::v2:
      pl.rung = attn_rung<2, 4, 5, 7, 9, 13, 17>(pl.n_t);
      if (!pl.rung) { set_error("attention_v2: S=%d exceeds 272", a.S); return refuse(pl); }
      // the whole-row backward runs out of registers past 112 keys; ok(v2) sends those to the v3 family
      if (bwd && pl.rung > 7) { set_error("attention_v2: backward supports S <= 112 (got %d)", a.S); return refuse(pl); }
      if (!bwd) pl.waves = attn_v2_fwd_waves(pl.rung, pl.st_bias);
      break;
    case AttnRoute::v3: {
      pl.tight = attn_v3_tight(a.hd, pl.cap);
      pl.s_pad = attn_v3_s_pad(pl.cap, pl.tight);
      const size_t lds = attn_v3_lds_bytes(a.hd, pl.s_pad, pl.tight, pl.nhist);
      if (lds > ATTN_LDS_MAX) { set_error("attention_bwd_v3: S=%d needs %zu bytes of LDS", pl.cap, lds); return refuse(pl); }
      // 64- and 16-wide heads without a structural bias, long sequences (ViT: 13 tiles): LDS allows two workgroups per CU; 8 waves
      // each in the 128-register build = 4 waves per SIMD instead of 2 (in-call A/B at the ViT shape: +0.7 % on the step)
      pl.threads = (a.hd <= 64 && !pl.st_bias && pl.s_pad > 128) ? 512 : 256;
      break;
    }
    case AttnRoute::v5:
      pl.items = (int)((int64_t)a.H * a.nseq);
      pl.wgs = pl.items < device_cus() ? pl.items : device_cus();      // persistent: at most one workgroup per CU
      break;
    case AttnRoute::v4:
    case AttnRoute::v4x:
      pl.waves = pl.n_t <= 4 ? 4 : pl.n_t <= 8 ? 8 : 16;          // two 16-byte chunks per thread and image, one key tile per wave
      break;
    default: break;
  }
  return pl;
}

// v1: the kernels of this file
int attention_v1_launch(hipStream_t st, const AttnParams& p, const AttnPlan& pl) {
  return with_dtype(p.f.dtype, [&](auto t) { return with_head_dim(p.f.hd, [&](auto hd) { return with_flags(pl, [&](auto s, auto d) {
    return with_rung<2, 5, 7, 9, 13, 17>(pl.rung, [&](auto nt) {
      using T = typename decltype(t)::type;
      constexpr int HD = decltype(hd)::value, NT = decltype(nt)::value;
      constexpr bool STRUCT = decltype(s)::value, DROP = decltype(d)::value, BF = !std::is_same<T, float>::value;
      const size_t lds = attn_v1_lds_bytes(BF, HD, NT, pl.bwd, pl.nhist);
      const dim3 grid(p.f.H, p.f.nseq);
      if (!pl.bwd) return launch_route<attn_fwd_kernel<T, HD, NT, STRUCT, DROP>>("v1", grid, 256, lds, st, p);
      // fp32, wide heads, 17 key tiles with structural bias and dropout: 512 registers and 15-17 more in scratch memory (as the
      // 16- and 64-wide instantiations have) — not instantiated; attn_plan sends them to the key-chunked path
      if constexpr (!BF && HD > 64 && NT == 17 && STRUCT && DROP) return attn_unplanned("the fp32 v1 backward of wide heads at 17 tiles with structural bias and dropout");
      else return launch_route<attn_bwd_kernel<T, HD, NT, STRUCT, DROP>>("v1", grid, 256, lds, st, p);
    });
  }); }); });
}

// The widest global access any kernel family makes to a row tensor decides what its base and row stride must be (the rule of
// include/mdt_hip.h).  bf16: 16-byte vectors — qkv and dout in the image loaders and fragment loads of v1 .. v5, out in the v2
// forward's row stores and the one-pass backwards' loads, dqkv in rows4_store (row_piece: 8 bytes) — so base and row pitch
// are multiples of 16 bytes.  fp32 (v1, the key-chunked path, head weights): one element at a time, any row stride; the base
// on an element boundary.  The head offset h * hd and the D | 2 D thirds keep either alignment (hd is a multiple of 16).
static bool attn_rows_aligned(int dtype, const void* base, int64_t ld) {
  return dtype == MDT_BF16 ? (ld % 8 == 0 && ((uintptr_t)base & 15) == 0) : ((uintptr_t)base & 3) == 0;
}

static int check_args(const mdt_attn_fwd_args& a) {
  MDT_CHECK_ARG(a.dtype == MDT_F32 || a.dtype == MDT_BF16, "attention: bad dtype %d", a.dtype);
  MDT_CHECK_ARG(a.nseq >= 0 && a.S > 0 && a.H > 0 && a.hd > 0, "attention: bad shape nseq=%d S=%d H=%d hd=%d", a.nseq,
                a.S, a.H, a.hd);
  MDT_CHECK_ARG(a.qkv && a.out && a.lse, "attention: null qkv / out / lse");
  MDT_CHECK_ARG(a.ld_qkv >= 3 * a.H * a.hd && a.ld_out >= a.H * a.hd, "attention: row strides too small");
  if (a.dtype == MDT_BF16) {
    MDT_CHECK_ARG(attn_rows_aligned(a.dtype, a.qkv, a.ld_qkv), "attention(bf16): qkv must be 16-byte aligned rows");
    MDT_CHECK_ARG(attn_rows_aligned(a.dtype, a.out, a.ld_out), "attention(bf16): out must be 16-byte aligned rows");
  } else {
    MDT_CHECK_ARG(attn_rows_aligned(a.dtype, a.qkv, a.ld_qkv), "attention(fp32): qkv must be 4-byte aligned");
    MDT_CHECK_ARG(attn_rows_aligned(a.dtype, a.out, a.ld_out), "attention(fp32): out must be 4-byte aligned");
  }
  if (a.attn_bias) MDT_CHECK_ARG(a.spatial_pos && a.sp_table && a.virt && a.num_spatial > 0, "attention: incomplete structural bias");
  MDT_CHECK_ARG(a.drop_p >= 0.f && a.drop_p < 1.f, "attention: dropout p=%f out of [0,1)", a.drop_p);
  if (a.seq_offsets)
    MDT_CHECK_ARG(a.pos_stride == 1 && !a.key_mask && !a.key_pad && !a.dense_bias && !a.attn_bias,
                  "attention: ragged sequences (seq_offsets) take no masks / biases and need pos_stride == 1");
  MDT_CHECK_ARG(a.s_cap >= 0 && a.s_cap <= a.S, "attention: s_cap=%d outside [0, S=%d]", a.s_cap, a.S);
  MDT_CHECK_ARG(!a.seq_ids || (a.seq_offsets && (a.nseq_total == 0 || a.nseq_total >= a.nseq)),
                "attention: seq_ids need seq_offsets (and nseq_total >= nseq)");
  MDT_CHECK_ARG(a.drop_p == 0.f || (uint64_t)(a.nseq_total > a.nseq ? a.nseq_total : a.nseq) * a.H * a.S * (a.S + 1) < (1ull << 32),
                "attention: dropout counters are 32-bit (nseq*H*S*(S+1) must stay below 2^32)");
  return MDT_OK;
}

// check_args and the backward block's own checks (b: null for a forward), then the kernels' argument block
static int checked_params(const mdt_attn_fwd_args& f, const mdt_attn_bwd_args* b, AttnParams& p) {
  if (int e = check_args(f)) return e;
  memset(&p, 0, sizeof(p));
  p.f = f;
  p.drop = make_drop(f.drop_p, f.drop_seed);
  if (!b) return MDT_OK;
  MDT_CHECK_ARG(b->dout && b->dqkv, "attention_bwd: null dout / dqkv");
  MDT_CHECK_ARG(b->ld_dqkv >= 3 * f.H * f.hd, "attention_bwd: ld_dqkv too small");
  MDT_CHECK_ARG(b->ld_dout >= f.H * f.hd, "attention_bwd: ld_dout too small");
  if (f.dtype == MDT_BF16) {
    MDT_CHECK_ARG(attn_rows_aligned(f.dtype, b->dout, b->ld_dout), "attention_bwd(bf16): dout must be 16-byte aligned rows");
    MDT_CHECK_ARG(attn_rows_aligned(f.dtype, b->dqkv, b->ld_dqkv), "attention_bwd(bf16): dqkv must be 16-byte aligned rows");
  } else {
    MDT_CHECK_ARG(attn_rows_aligned(f.dtype, b->dout, b->ld_dout), "attention_bwd(fp32): dout must be 4-byte aligned");
    MDT_CHECK_ARG(attn_rows_aligned(f.dtype, b->dqkv, b->ld_dqkv), "attention_bwd(fp32): dqkv must be 4-byte aligned");
  }
  p.dout = b->dout; p.ld_dout = b->ld_dout; p.dqkv = b->dqkv; p.ld_dqkv = b->ld_dqkv;
  p.d_dense_bias = b->d_dense_bias; p.d_sp_table = b->d_sp_table; p.d_virt = b->d_virt;
  return MDT_OK;
}

static int dispatch(hipStream_t st, const mdt_attn_fwd_args& f, const mdt_attn_bwd_args* b) {
  AttnParams p;
  if (int e = checked_params(f, b, p)) return e;
  if (p.d_sp_table || p.d_virt) note_float_atomic_launch();     // the structural-bias gradient (attn_bias_grad_add / _flush)
  const AttnPlan pl = attn_plan(p, b != nullptr);
  if (pl.status != MDT_OK) return pl.status;
  switch (pl.route) {
    case AttnRoute::v1: return attention_v1_launch(st, p, pl);
    case AttnRoute::long_: return attention_long_launch(st, p, pl);
    default: return attention_v2_launch(st, p, pl);      // v2 .. v5
  }
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_attention_fwd(void* stream, const mdt_attn_fwd_args* a) {
  MDT_CHECK_ARG(a, "attention_fwd: null args");
  if (a->nseq == 0) return MDT_OK;
  return dispatch((hipStream_t)stream, *a, nullptr);
}

extern "C" int mdt_attention_bwd(void* stream, const mdt_attn_bwd_args* a) {
  MDT_CHECK_ARG(a, "attention_bwd: null args");
  if (a->f.nseq == 0) return MDT_OK;
  return dispatch((hipStream_t)stream, a->f, a);
}

extern "C" int mdt_attention_route(const mdt_attn_bwd_args* a, int bwd, char* route, size_t route_bytes, int32_t geometry[2]) {
  MDT_CHECK_ARG(a && route && route_bytes > 0 && geometry, "attention_route: null args");
  route[0] = 0;
  geometry[0] = geometry[1] = 0;
  AttnParams p;
  if (int e = checked_params(a->f, bwd ? a : nullptr, p)) return e;
  const AttnPlan pl = attn_plan(p, bwd != 0);
  if (pl.status != MDT_OK) return pl.status;
  snprintf(route, route_bytes, "%s", route_name(pl.route));
  switch (pl.route) {
    case AttnRoute::v1:
    case AttnRoute::v2: geometry[0] = pl.rung; geometry[1] = pl.waves; break;      // waves: the v2 forward's
    case AttnRoute::v3: geometry[0] = pl.s_pad; geometry[1] = pl.threads; break;
    case AttnRoute::v4:
    case AttnRoute::v4x: geometry[0] = pl.waves; break;
    default: break;
  }
  return MDT_OK;
}

extern "C" int mdt_attention_mean_probs(void* stream, const mdt_attn_fwd_args* a, float* out) {
  MDT_CHECK_ARG(a && out, "attention_mean_probs: null args");
  if (a->nseq == 0) return MDT_OK;
  if (int e = check_args(*a)) return e;
  MDT_CHECK_ARG(!a->seq_offsets, "attention_mean_probs: ragged sequences are not supported (module-level API only)");
  const int64_t n = (int64_t)a->nseq * a->S * a->S;
  const int grid = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
  return with_dtype(a->dtype, [&](auto t) {
    return launch_plain<attn_mean_probs_kernel<typename decltype(t)::type>>("attention_mean_probs", grid, 256, (hipStream_t)stream, *a, out);
  });
}

// Per-head attention weights (modules/multihead_attention.py:91-102,186-214: ``need_head_weights`` — the softmax probabilities
// BEFORE dropout of every head — and ``before_softmax`` — the raw scores q k^T * scale + bias with masked keys at -inf),
// recomputed like the head average above: one thread per (sequence, head, query, key); fp32 output [nseq, H, S, S].
// Module-level API only (nothing in mDT asks for them).
template <typename T, bool RAW>
__global__ __launch_bounds__(256) void attn_head_weights_kernel(mdt_attn_fwd_args a, float* out) {
  const int S = a.S, H = a.H, hd = a.hd;
  const int64_t n = (int64_t)a.nseq * H * S * S;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int key = (int)(i % S), q = (int)((i / S) % S), h = (int)((i / ((int64_t)S * S)) % H), seq = (int)(i / ((int64_t)S * S * H));
    const T* qrow = (const T*)a.qkv + ((int64_t)seq * a.seq_stride + (int64_t)q * a.pos_stride) * a.ld_qkv + h * hd;
    const T* krow = (const T*)a.qkv + ((int64_t)seq * a.seq_stride + (int64_t)key * a.pos_stride) * a.ld_qkv + (int64_t)H * hd + h * hd;
    const BiasCtx bc = bias_ctx(a, seq, h, S);
    float v = key_only_bias<T>(bc, key);
    if (v == 0.f) {
      float dot = 0.f;
      for (int d = 0; d < hd; ++d) dot += to_f32(qrow[d]) * to_f32(krow[d]);
      v = dot * a.scale + (a.attn_bias ? pair_bias<T, true>(bc, q, key) : pair_bias<T, false>(bc, q, key));
    }
    if constexpr (RAW) {
      out[i] = v;
    } else {
      const float l = a.lse[((int64_t)seq * H + h) * S + q];
      out[i] = (v == -INFINITY || l == -INFINITY) ? 0.f : __expf(v - l);
    }
  }
}

extern "C" int mdt_attention_head_weights(void* stream, const mdt_attn_fwd_args* a, int raw_scores, float* out) {
  MDT_CHECK_ARG(a && out, "attention_head_weights: null args");
  if (a->nseq == 0) return MDT_OK;
  if (int e = check_args(*a)) return e;
  MDT_CHECK_ARG(!a->seq_offsets, "attention_head_weights: ragged sequences are not supported (module-level API only)");
  MDT_CHECK_ARG(raw_scores || a->lse, "attention_head_weights: probabilities need the forward's log-sum-exp");
  const int64_t n = (int64_t)a->nseq * a->H * a->S * a->S;
  const int grid = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(a->dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return raw_scores ? launch_plain<attn_head_weights_kernel<T, true>>("attention_head_weights", grid, 256, st, *a, out)
                      : launch_plain<attn_head_weights_kernel<T, false>>("attention_head_weights", grid, 256, st, *a, out);
  });
}

extern "C" int mdt_graph_attn_bias(void* stream, int dtype, int nseq, int S, int H, const float* attn_bias,
                                   const int32_t* spatial_pos, const void* sp_table, const void* virt, float* out) {
  MDT_CHECK_ARG(attn_bias && spatial_pos && sp_table && virt && out, "graph_attn_bias: null pointer");
  if (nseq == 0) return MDT_OK;
  const int64_t n = (int64_t)nseq * H * S * S;
  const int grid = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<graph_attn_bias_kernel<T>>("graph_attn_bias", grid, 256, st, nseq, S, H, attn_bias, spatial_pos, (const T*)sp_table, (const T*)virt, out);
  });
}
