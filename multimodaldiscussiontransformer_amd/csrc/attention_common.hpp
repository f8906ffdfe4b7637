// Shared pieces of the attention kernel families (attention.hip, attention_v2.hip, attention_long.hip): device helpers, the LDS
// sizes, the plan of a launch (AttnPlan) and the helpers that turn a plan into template arguments.
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

// ---------------------------------------------------------------------------------------------- host: plan and launchers
// LDS image row strides of the bf16 kernels, as functions of the head width (the kernels read them as IMG_LD<HD>,
// attention.hip, and v2_ld<HD, TIGHT>, attention_v2.hip, which say why these numbers).
constexpr int attn_v1_ld(int hd) { return hd >= 32 ? hd + 8 : hd; }
constexpr int attn_v2_ld(int hd, bool tight) { return hd < 32 ? hd : (hd <= 64 || tight) ? hd + 8 : hd + 16; }
template <int HD, bool TIGHT = false> constexpr int v2_ld = attn_v2_ld(HD, TIGHT);
template <int HD, int NT> constexpr int v2_ld_nt = v2_ld<HD, (HD == 128 && NT > 16)>;      // a whole-row kernel's stride
constexpr int V4_EXACT_PAIRS = 3;      // attn_bwd_v4x: key-tile pairs whose row sums it keeps (rows of up to 6 key tiles)
constexpr size_t ATTN_LDS_MAX = 160 * 1024;

// The bf16 kernels of attention.hip hold two [s_pad32][hd + 8] images and four score strips in LDS: with 128-wide heads the
// 17-tile rung (S 209 .. 272: 2 x 288 x 136 x 2 + 4 x 16 x 296 x 2 = 194560 bytes) is past the 160 KiB of a workgroup; every
// other (width, rung) fits.  A plain dense bias there takes the key-chunked long path in both directions.
constexpr bool attn_v1_fits(int hd, int S) { return hd < 128 || S <= 208; }

// Dynamic LDS of each family, written once: attn_plan sizes and refuses with these, the launchers pass what they return.
// nhist: attn_hist_size(num_spatial) where the launch reduces a structural-bias gradient (backward), else 0.
// v1 (attention.hip), rung nt: backward [delta][lse][hist], then (bf16) two images, then four waves' score strips
constexpr size_t attn_v1_lds_bytes(bool bf, int hd, int nt, bool bwd, int nhist) {
  const int s_pad32 = (nt * 16 + 31) & ~31, sld = s_pad32 + (bf ? 8 : 1);
  return (bwd ? (size_t)(2 * s_pad32 + nhist) * 4 : 0) + (size_t)4 * 16 * sld * (bf ? 2 : 4) + (bf ? (size_t)2 * s_pad32 * attn_v1_ld(hd) * 2 : 0);
}
// v2 whole-row kernels, rung nt: two images, one (forward) or three (backward) rows of floats, the histogram; forward: + the staging's spare chunk
constexpr size_t attn_v2_lds_bytes(int hd, int nt, bool bwd, int nhist) {
  const int s_pad = ((nt + 1) / 2) * 32;
  return (size_t)2 * s_pad * attn_v2_ld(hd, !bwd && hd == 128 && nt > 16) * 2 + (size_t)(bwd ? 3 : 1) * s_pad * 4 + (size_t)nhist * 4 + (bwd ? 0 : 16);
}
// v3: rows of up to cap keys are padded to s_pad (tight: 320 rows of 128-wide heads do not fit: 288 rows, 32-key chunks)
constexpr bool attn_v3_tight(int hd, int cap) { return hd == 128 && cap > 256; }
constexpr int attn_v3_s_pad(int cap, bool tight) { return tight ? (cap + 31) & ~31 : (cap + 63) & ~63; }
constexpr size_t attn_v3_lds_bytes(int hd, int s_pad, bool tight, int nhist) {
  return (size_t)2 * s_pad * attn_v2_ld(hd, tight) * 2 + (size_t)3 * s_pad * 4 + (size_t)nhist * 4;
}
// the one-pass kernels (v4, v4x, v5; 64-wide heads) for rows of n_t key tiles: two images of rows_img rows, three slabs of
// floats (attn_bwd_v4x: seven more, of per-key-tile row sums) and the dS^T image of row stride ldq
constexpr int attn_one_pass_rows(int n_t) { return ((n_t + 1) / 2) * 32; }
constexpr int attn_one_pass_ldq(int n_t) { return (n_t & 1) ? 16 * n_t : 16 * n_t + 16; }   // ldq / 2 = 8 (mod 16) banks: rows 0-7 of a transposed read fall on distinct 8-bank groups
constexpr size_t attn_one_pass_lds_bytes(int n_t) {
  const size_t rows = attn_one_pass_rows(n_t), slabs = n_t <= 2 * V4_EXACT_PAIRS ? 7 : 0;
  return 2 * rows * attn_v2_ld(64, false) * 2 + (3 + slabs) * rows * 4 + (size_t)16 * n_t * attn_one_pass_ldq(n_t) * 2;
}
// forward v2: 8 waves for the long (ViT) rows without a structural bias, 4 waves per SIMD
constexpr int attn_v2_fwd_waves(int nt, bool st_bias) { return (nt >= 13 && !st_bias) ? 8 : 4; }

// What one attention launch takes: the kernel family and every launch-geometry number that is no template body.  A pure
// host function of the argument block (attn_plan, attention.hip, holds the routing table and says what each route is for);
// mdt_attention_route reports it without launching.  status != MDT_OK: the launch is refused, the message is set.
struct AttnPlan {
  int status;
  AttnRoute route;
  bool bwd, st_bias, drop, binned, dense_only;
  int cap, n_t;                  // the longest sequence of this launch (s_cap, else S) and its 16-key tiles
  int nhist;                     // attn_hist_size(num_spatial) of a backward with a structural bias, else 0
  int rung;                      // v1, v2: the key-tile count the kernel is instantiated for
  int s_pad, threads; bool tight;   // v3
  int rows_img, ldq, waves;      // v4, v4x, v5 (waves also: the v2 forward's)
  int items, wgs;                // v5: (sequence, head) items and the persistent grid
};
AttnPlan attn_plan(const AttnParams& p, bool bwd);
// The three launchers: each turns the plan's numbers into template arguments and launches; none decides anything.
int attention_v1_launch(hipStream_t st, const AttnParams& p, const AttnPlan& pl);     // attention.hip
int attention_v2_launch(hipStream_t st, const AttnParams& p, const AttnPlan& pl);     // attention_v2.hip: v2 .. v5
int attention_long_launch(hipStream_t st, const AttnParams& p, const AttnPlan& pl);   // attention_long.hip
// a combination a launcher's `if constexpr` keeps uninstantiated: attn_plan refuses or reroutes it before any launcher runs
inline int attn_unplanned(const char* what) { set_error("attention: %s is not instantiated and attn_plan never plans it", what); return MDT_ERR_UNSUPPORTED; }

// Runtime values of a plan as template arguments (with_dtype, common.hpp, is the fourth): f is called with
// std::integral_constant / std::bool_constant tags.
constexpr bool attn_head_dim_ok(int hd) { return hd == 16 || hd == 64 || hd == 96 || hd == 128; }
template <typename F>
static int with_head_dim(int hd, F&& f) {
  switch (hd) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 64: return f(std::integral_constant<int, 64>{});
    case 96: return f(std::integral_constant<int, 96>{});
    case 128: return f(std::integral_constant<int, 128>{});
  }
  return attn_unplanned("this head width");
}
// (structural bias, dropout)
template <typename F>
static int with_flags(const AttnPlan& pl, F&& f) {
  using T = std::true_type;
  using N = std::false_type;
  if (pl.st_bias && pl.drop) return f(T{}, T{});
  if (pl.st_bias) return f(T{}, N{});
  if (pl.drop) return f(N{}, T{});
  return f(N{}, N{});
}
// A ladder of key-tile rungs: attn_rung is the first that holds nt tiles (0: none does), with_rung hands a rung over as a type.
template <int... RUNGS>
constexpr int attn_rung(int nt) {
  int r = 0;
  ((r = (r == 0 && nt <= RUNGS) ? RUNGS : r), ...);
  return r;
}
template <int... RUNGS, typename F>
static int with_rung(int rung, F&& f) {
  int e = MDT_ERR_UNSUPPORTED;
  const bool hit = ((rung == RUNGS ? (e = f(std::integral_constant<int, RUNGS>{}), true) : false) || ...);
  return hit ? e : attn_unplanned("this key-tile rung");
}

}  // namespace mdt
