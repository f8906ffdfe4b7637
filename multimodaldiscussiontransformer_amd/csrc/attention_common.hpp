// Shared pieces of the two attention kernel families (attention.hip, attention_v2.hip).
#pragma once
#include "common.hpp"

namespace mdt {

struct AttnParams {
  mdt_attn_fwd_args f;
  DropCfg drop;
  const void* dout; int64_t ld_dout;
  void* dqkv; int64_t ld_dqkv;
  float* d_dense_bias; float* d_sp_table; float* d_virt;
};

struct BiasCtx {
  int seq, h, S, H;
  const uint8_t* key_mask;
  const uint8_t* key_pad;
  const float* dense;
  const float* attn_bias;
  const int32_t* sp;
  const void* table;
  const void* virt;
};
// the bias context of sequence `seq` (length S), head h, of a launch.  The two forward kernels (attn_fwd_kernel, attn_fwd_v2_kernel)
// keep the initialiser written out: built through this function, seven instantiations of either are scheduled differently, and
// the plain v1 forward takes 2 - 9 more VGPRs and loses a wave per SIMD at five tile counts (attn_fwd_v2_kernel<128, 4>: 8 -> 7).
__device__ __forceinline__ BiasCtx bias_ctx(const mdt_attn_fwd_args& a, int seq, int h, int S) {
  return BiasCtx{seq, h, S, a.H, a.key_mask, a.key_pad, a.dense_bias, a.attn_bias, a.spatial_pos, a.sp_table, a.virt};
}

// One (sequence, head) work item of a launch: what a backward body derives from (AttnParams, head, sequence index) before it
// does anything else.  qkv / dout / out / dqkv point at the head's columns of the sequence's first row; tld / dld / old_ / gld
// are their strides between consecutive positions.
// Sites: attn_bwd_v3_body and attn_bwd_v4_body (attention_v2.hip).  The four whole-row kernels — attn_fwd_v2_kernel,
// attn_bwd_v2_kernel, attn_fwd_kernel, attn_bwd_kernel — keep the same lines written out: they are __global__ functions, and with
// their parameter block first read inside an inlined callee the compiler forms the preamble's branches differently and
// schedules the whole kernel after it — the plain v1 forward instantiations then take 3 - 9 more VGPRs and lose a wave per SIMD
// (7 -> 6 ... 4 -> 3), the v2 forward with a structural bias 1 - 5 more VGPRs.  v5's item_of reads its tables through the
// scalar cache and is no site either.
template <typename T>
struct AttnItem {
  int seq, S, SL, D;                    // S: this sequence's length; SL: lse / dropout-counter geometry
  int64_t row0;
  const T* qkv; const T* dout; const T* out; T* dqkv;
  int64_t tld, dld, old_, gld;
};
template <typename T, int HD>
__device__ __forceinline__ AttnItem<T> attn_item(const AttnParams& P, int h, unsigned si) {
  const mdt_attn_fwd_args& a = P.f;
  const int seq = a.seq_ids ? a.seq_ids[si] : (int)si;
  const int SL = a.S, D = a.H * HD;
  const int S = a.seq_offsets ? a.seq_offsets[seq + 1] - a.seq_offsets[seq] : a.S;
  const int64_t row0 = a.seq_offsets ? (int64_t)a.seq_offsets[seq] : (int64_t)seq * a.seq_stride;
  const T* qkv = (const T*)a.qkv + row0 * a.ld_qkv + h * HD;
  const T* dout = (const T*)P.dout + row0 * P.ld_dout + h * HD;
  const T* out = (const T*)a.out + row0 * a.ld_out + h * HD;
  T* dqkv = (T*)P.dqkv + row0 * P.ld_dqkv + h * HD;
  return AttnItem<T>{seq, S, SL, D, row0, qkv, dout, out, dqkv, a.pos_stride * a.ld_qkv, a.pos_stride * P.ld_dout, a.pos_stride * a.ld_out,
                     a.pos_stride * P.ld_dqkv};
}

template <typename T>
__device__ __forceinline__ float key_only_bias(const BiasCtx& b, int key) {
  if (key >= b.S) return -INFINITY;
  if (b.key_mask && !b.key_mask[(int64_t)b.seq * b.S + key]) return -INFINITY;
  if (b.key_pad && b.key_pad[(int64_t)b.seq * b.S + key]) return -INFINITY;
  return 0.f;
}

// additive bias of score (q, key), both < S
template <typename T, bool STRUCT>
__device__ __forceinline__ float pair_bias(const BiasCtx& b, int q, int key) {
  float v = 0.f;
  if (b.dense) v += b.dense[(((int64_t)b.seq * b.H + b.h) * b.S + q) * b.S + key];
  if constexpr (STRUCT) {
    v += 2.0f * b.attn_bias[((int64_t)b.seq * b.S + q) * b.S + key];  // graphormer_layers.py:93 and :108
    if (q >= 1 && key >= 1) {
      const int idx = b.sp[((int64_t)b.seq * (b.S - 1) + (q - 1)) * (b.S - 1) + (key - 1)];
      v += to_f32(((const T*)b.table)[(int64_t)idx * b.H + b.h]);
    } else {
      v += to_f32(((const T*)b.virt)[b.h]);  // row 0 (graph token as query) or column 0 (as key)
    }
  }
  return v;
}

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

// Attention-probability dropout counters: element (bh, q, key) -> (bh*S + q)*S2 + key with S2 = S rounded
// up to even, so keys 2i and 2i+1 of one query share a 32-bit word of the mixer (common.hpp "dropout RNG").
__device__ __forceinline__ uint32_t attn_row_pairs(int bh, int S, int q) {
  return (uint32_t)(bh * S + q) * (uint32_t)((S + 1) >> 1);
}
__device__ __forceinline__ uint32_t attn_drop_word(const DropCfg& d, uint32_t row_pairs, int key) {
  return drop_mix((row_pairs + (uint32_t)(key >> 1)) ^ d.key);
}
__device__ __forceinline__ bool drop_keep_lo(const DropCfg& d, uint32_t w) { return (w & 0xFFFFu) >= d.thresh; }
__device__ __forceinline__ bool drop_keep_hi(const DropCfg& d, uint32_t w) { return (w >> 16) >= d.thresh; }
// Queries on lanes: a lane holds four consecutive keys of one query = the two mixer words `pair` and `pair + 1`
// (pair = attn_row_pairs(bh, S, q) + key / 2 of the first key).
// Site: pass A of attn_bwd_v3_body.  attn_fwd_v2_kernel keeps the same five lines written out: with this call the compiler unrolls
// the tile loops of <16, 17, STRUCT, DROP> in full (7 022 -> 25 818 instructions) and <64, 7, STRUCT, DROP> drops from 7 to 5 waves.
__device__ __forceinline__ void attn_keep4_keys(const DropCfg& d, uint32_t pair, bool (&keep)[4]) {
  const uint32_t w0 = drop_mix(pair ^ d.key), w1 = drop_mix((pair + 1) ^ d.key);
  keep[0] = drop_keep_lo(d, w0); keep[1] = drop_keep_hi(d, w0);
  keep[2] = drop_keep_lo(d, w1); keep[3] = drop_keep_hi(d, w1);
}
// Keys on lanes: a lane holds four consecutive QUERIES (qb .. qb + 3) of one key, so its four dropout decisions sit in four
// different mixer words; the neighbouring lane (key ^ 1, `odd` = key & 1) needs the same four words (other half), so each
// lane of the pair computes two of them and they trade through one DPP quad swap each.  kh: pair index of the key in query
// row 0 (bh * S * s2h + key / 2), s2h: pairs per query row.  All lanes of a quad must be active.
__device__ __forceinline__ void attn_keep4_queries(const DropCfg& d, uint32_t kh, int qb, uint32_t s2h, int odd, bool (&keep)[4]) {
  const uint32_t ra = kh + (uint32_t)(qb + 2 * odd) * s2h;
  const uint32_t wa = drop_mix(ra ^ d.key), wb = drop_mix((ra + s2h) ^ d.key);
  const uint32_t pa = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)wa, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
  const uint32_t pb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)wb, 0xB1, 0xF, 0xF, false);
  const uint32_t w[4] = {odd ? pa : wa, odd ? pb : wb, odd ? wa : pa, odd ? wb : pb};
#pragma unroll
  for (int r = 0; r < 4; ++r) keep[r] = ((w[r] >> (16 * odd)) & 0xFFFFu) >= d.thresh;
}
// generic (one element): the same decision as the word helpers above
__device__ __forceinline__ float attn_drop_scale(const DropCfg& d, int bh, int S, int q, int key) {
  const uint32_t w = attn_drop_word(d, attn_row_pairs(bh, S, q), key);
  return ((key & 1) ? drop_keep_hi(d, w) : drop_keep_lo(d, w)) ? d.inv_keep : 0.f;
}

// Gradient of the biases from one dS element (q, key < S) of the whole-row kernels: the dense bias gradient is stored, the
// structural one is reduced in an LDS histogram of attn_hist_size(num_spatial) floats — bins 0 .. num_spatial - 1 for the
// spatial_pos table, bin num_spatial for the graph token (row 0 as query or column 0 as key) — and leaves with one atomic
// per bin (attn_bias_grad_flush).  attention_long.hip adds to global memory directly.
__host__ __device__ inline int attn_hist_size(int num_spatial) { return (num_spatial + 1 + 3) & ~3; }
template <bool STRUCT>
__device__ __forceinline__ void attn_bias_grad_add(const AttnParams& P, float* s_hist, int seq, int h, int S, int q, int key, float ds) {
  const mdt_attn_fwd_args& a = P.f;
  if (P.d_dense_bias) P.d_dense_bias[(((int64_t)seq * a.H + h) * S + q) * S + key] = ds;
  if constexpr (STRUCT) {
    if (P.d_sp_table && ds != 0.f) {
      if (q >= 1 && key >= 1) {
        const int idx = a.spatial_pos[((int64_t)seq * (S - 1) + (q - 1)) * (S - 1) + (key - 1)];
        if (idx != 0) atomicAdd(s_hist + idx, ds);  // nn.Embedding(padding_idx=0): row 0 gets no gradient
      } else {
        atomicAdd(s_hist + a.num_spatial, ds);
      }
    }
  }
}
__device__ __forceinline__ void attn_bias_grad_flush(const AttnParams& P, const float* s_hist, int h, int tid, int nthr) {
  const mdt_attn_fwd_args& a = P.f;
  if (P.d_sp_table) {
    for (int i = tid; i <= a.num_spatial; i += nthr) {
      const float v = s_hist[i];
      if (v != 0.f) {
        if (i < a.num_spatial) atomicAdd(P.d_sp_table + (int64_t)i * a.H + h, v);
        else if (P.d_virt) atomicAdd(P.d_virt + h, v);
      }
    }
  }
}

int attention_v2_dispatch(hipStream_t st, const AttnParams& p, bool bwd);
AttnRoute attn_bwd_route(const AttnParams& p);                                   // bf16, head_dim 16 | 64 | 96 | 128: attention_v2.hip
int attention_v3_bwd_dispatch(hipStream_t st, const AttnParams& p, AttnRoute r);   // r: v3 | v4 | v4x | v5
int attention_long_dispatch(hipStream_t st, const AttnParams& p, bool bwd);     // S > 272: attention_long.hip
// The bf16 kernels of attention.hip hold two [s_pad32][hd + 8] images and four score strips in LDS: with 128-wide heads the
// 17-tile rung (S 209 .. 272: 2 x 288 x 136 x 2 + 4 x 16 x 296 x 2 = 194560 bytes) is past the 160 KiB of a workgroup; every
// other (width, rung) fits.  A plain dense bias there takes the key-chunked long path in both directions.
inline bool attn_v1_fits(int hd, int S) { return hd < 128 || S <= 208; }

}  // namespace mdt
