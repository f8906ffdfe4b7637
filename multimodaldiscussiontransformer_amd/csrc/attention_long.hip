// Attention over sequences longer than one workgroup holds (S > 272): discussion trees with more than 271 comments.
// The reference runs any tree size as dense O(T^2) attention (--max-nodes 10000 is declared and never enforced,
// mDT/src/tasks/task.py:41-44; modules/multihead_attention.py:139-202); the single-pass MFMA kernels of attention*.hip
// keep a whole (sequence, head) on chip and stop at 272 tokens.  This file is the key-chunked path behind the same C ABI:
// flash-style online softmax in the forward, log-sum-exp based recomputation in the backward, the same masks /
// structural bias / dropout counters — so a long tree gives the same numbers the short kernels would.  Plain fp32 FMA
// (one query or key per lane, the other operand broadcast from LDS): such trees are rare in the pruned dataset
// (Pre-Processing/3-prune-trees.py), this path is about not refusing them, not about MFMA utilisation.
#include <type_traits>

#include "attention_common.hpp"

namespace mdt {

constexpr int LC = 64;      // chunk of keys (forward, dQ pass) or queries (dK / dV pass) staged in LDS
// Heads wider than 64 columns: NP = 2 lanes share a query (or key) and hold half of the head each, so the per-lane arrays
// stay at the 64 floats of a 64-wide head (four of them in the dK / dV pass: a whole 128-wide head per lane would be 512
// registers); the two halves of a dot product meet in one lane swap.  A workgroup then covers 32 queries and stages 32-row
// chunks (two [32][128] fp32 images: 32 KiB).
template <int HD> constexpr int long_parts = HD > 64 ? 2 : 1;
template <int NP> __device__ __forceinline__ float long_pair_sum(float v) {
  if constexpr (NP > 1) v += __shfl_xor(v, 1, 64);
  return v;
}

template <typename T, int HD, int ROWS = LC>
__device__ __forceinline__ void long_stage(float* dst, const T* src, int64_t ld, int row0, int rows, int lane) {
  // dst[ROWS][HD] fp32 <- rows row0 .. row0+ROWS of src (zero past `rows`)
  for (int e = lane; e < ROWS * HD; e += 64) {
    const int r = e / HD, c = e - r * HD;
    dst[e] = (row0 + r < rows) ? to_f32(src[(int64_t)(row0 + r) * ld + c]) : 0.f;
  }
}

template <typename T, int HD, bool STRUCT>
__global__ __launch_bounds__(64) void attn_long_fwd_kernel(AttnParams P) {
  constexpr int NP = long_parts<HD>, DL = HD / NP, LCK = LC / NP;
  __shared__ float sK[LCK * HD], sV[LCK * HD];
  const mdt_attn_fwd_args& a = P.f;
  const int lane = threadIdx.x, h = blockIdx.y, seq = blockIdx.z;
  const int S = a.S, D = a.H * HD;
  const int part = lane & (NP - 1), c0 = part * DL;      // this lane's columns c0 .. c0 + DL of the head
  const int q = blockIdx.x * (64 / NP) + lane / NP;
  const bool qok = q < S;
  const int qc = qok ? q : S - 1;
  const int64_t row0 = (int64_t)seq * a.seq_stride, tld = a.pos_stride * a.ld_qkv;
  const T* qkv = (const T*)a.qkv + row0 * a.ld_qkv + h * HD;
  const BiasCtx bc = bias_ctx(a, seq, h, S);
  float qv[DL], acc[DL];
#pragma unroll
  for (int d = 0; d < DL; ++d) { qv[d] = to_f32(qkv[(int64_t)qc * tld + c0 + d]) * a.scale; acc[d] = 0.f; }
  float m = -INFINITY, l = 0.f;
  const int bh = seq * a.H + h;
  const bool drop = a.drop_p > 0.f;
  for (int k0 = 0; k0 < S; k0 += LCK) {
    __syncthreads();
    long_stage<T, HD, LCK>(sK, qkv + D, tld, k0, S, lane);
    long_stage<T, HD, LCK>(sV, qkv + 2 * D, tld, k0, S, lane);
    __syncthreads();
    const int kn = S - k0 < LCK ? S - k0 : LCK;
    for (int j = 0; j < kn; ++j) {
      const int key = k0 + j;
      float s = key_only_bias<T>(bc, key);
      if (s == 0.f) {            // wave-uniform (one key): the lane swap below has every lane
#pragma unroll
        for (int d = 0; d < DL; ++d) s = __builtin_fmaf(qv[d], sK[j * HD + c0 + d], s);
        s = long_pair_sum<NP>(s);
        s += pair_bias<T, STRUCT>(bc, qc, key);
      }
      if (s == -INFINITY) continue;
      const float mn = fmaxf(m, s);
      const float corr = __expf(m - mn), p = __expf(s - mn);      // m = -inf on the first live key: corr = 0
      l = l * corr + p;
      const float pd = drop ? p * attn_drop_scale(P.drop, bh, S, qc, key) : p;
#pragma unroll
      for (int d = 0; d < DL; ++d) acc[d] = __builtin_fmaf(pd, sV[j * HD + c0 + d], acc[d] * corr);
      m = mn;
    }
  }
  if (qok) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    T* orow = (T*)a.out + (row0 + (int64_t)q * a.pos_stride) * a.ld_out + h * HD + c0;
#pragma unroll
    for (int d = 0; d < DL; ++d) orow[d] = from_f32<T>(acc[d] * inv);
    if (part == 0) a.lse[((int64_t)seq * a.H + h) * S + q] = l > 0.f ? m + __logf(l) : -INFINITY;
  }
}

// dQ (queries on lanes, keys streamed through LDS) + the bias gradients
template <typename T, int HD, bool STRUCT>
__global__ __launch_bounds__(64) void attn_long_dq_kernel(AttnParams P) {
  constexpr int NP = long_parts<HD>, DL = HD / NP, LCK = LC / NP;
  __shared__ float sK[LCK * HD], sV[LCK * HD];
  const mdt_attn_fwd_args& a = P.f;
  const int lane = threadIdx.x, h = blockIdx.y, seq = blockIdx.z;
  const int S = a.S, D = a.H * HD;
  const int part = lane & (NP - 1), c0 = part * DL;
  const int q = blockIdx.x * (64 / NP) + lane / NP;
  const bool qok = q < S;
  const int qc = qok ? q : S - 1;
  const int64_t row0 = (int64_t)seq * a.seq_stride, tld = a.pos_stride * a.ld_qkv;
  const T* qkv = (const T*)a.qkv + row0 * a.ld_qkv + h * HD;
  const T* dorow = (const T*)P.dout + (row0 + (int64_t)qc * a.pos_stride) * P.ld_dout + h * HD + c0;
  const T* orow = (const T*)a.out + (row0 + (int64_t)qc * a.pos_stride) * a.ld_out + h * HD + c0;
  const BiasCtx bc = bias_ctx(a, seq, h, S);
  float qv[DL], dov[DL], dq[DL];
  float delta = 0.f;
#pragma unroll
  for (int d = 0; d < DL; ++d) {
    qv[d] = to_f32(qkv[(int64_t)qc * tld + c0 + d]) * a.scale;
    dov[d] = to_f32(dorow[d]);
    delta = __builtin_fmaf(dov[d], to_f32(orow[d]), delta);
    dq[d] = 0.f;
  }
  delta = long_pair_sum<NP>(delta);
  const float lse = a.lse[((int64_t)seq * a.H + h) * S + qc];
  const int bh = seq * a.H + h;
  const bool drop = a.drop_p > 0.f;
  for (int k0 = 0; k0 < S; k0 += LCK) {
    __syncthreads();
    long_stage<T, HD, LCK>(sK, qkv + D, tld, k0, S, lane);
    long_stage<T, HD, LCK>(sV, qkv + 2 * D, tld, k0, S, lane);
    __syncthreads();
    const int kn = S - k0 < LCK ? S - k0 : LCK;
    for (int j = 0; j < kn; ++j) {
      const int key = k0 + j;
      float s = key_only_bias<T>(bc, key);
      if (s == 0.f) {
#pragma unroll
        for (int d = 0; d < DL; ++d) s = __builtin_fmaf(qv[d], sK[j * HD + c0 + d], s);
        s = long_pair_sum<NP>(s);
        s += pair_bias<T, STRUCT>(bc, qc, key);
      }
      if (s == -INFINITY || lse == -INFINITY || !qok) continue;      // the two lanes of a query leave together
      const float p = __expf(s - lse);
      float dp = 0.f;
#pragma unroll
      for (int d = 0; d < DL; ++d) dp = __builtin_fmaf(dov[d], sV[j * HD + c0 + d], dp);
      dp = long_pair_sum<NP>(dp);
      if (drop) dp *= attn_drop_scale(P.drop, bh, S, q, key);
      const float ds = p * (dp - delta);
#pragma unroll
      for (int d = 0; d < DL; ++d) dq[d] = __builtin_fmaf(ds, sK[j * HD + c0 + d], dq[d]);
      if (part != 0) continue;                                       // bias gradients: once per (query, key)
      if (P.d_dense_bias) P.d_dense_bias[(((int64_t)seq * a.H + h) * S + q) * S + key] = ds;
      if constexpr (STRUCT) {
        if (P.d_sp_table && ds != 0.f) {
          if (q >= 1 && key >= 1) {
            const int idx = a.spatial_pos[((int64_t)seq * (S - 1) + (q - 1)) * (S - 1) + (key - 1)];
            if (idx != 0) atomicAdd(P.d_sp_table + (int64_t)idx * a.H + h, ds);      // padding_idx row 0: no gradient
          } else if (P.d_virt) {
            atomicAdd(P.d_virt + h, ds);
          }
        }
      }
    }
  }
  if (qok) {
    T* drow = (T*)P.dqkv + (row0 + (int64_t)q * a.pos_stride) * P.ld_dqkv + h * HD + c0;
#pragma unroll
    for (int d = 0; d < DL; ++d) drow[d] = from_f32<T>(dq[d] * a.scale);
  }
}

// dK, dV (keys on lanes, queries streamed through LDS)
template <typename T, int HD, bool STRUCT>
__global__ __launch_bounds__(64) void attn_long_dkv_kernel(AttnParams P) {
  constexpr int NP = long_parts<HD>, DL = HD / NP, LCK = LC / NP;
  __shared__ float sQ[LCK * HD], sO[LCK * HD], sL[LCK], sD[LCK];
  const mdt_attn_fwd_args& a = P.f;
  const int lane = threadIdx.x, h = blockIdx.y, seq = blockIdx.z;
  const int S = a.S, D = a.H * HD;
  const int part = lane & (NP - 1), c0 = part * DL;
  const int key = blockIdx.x * (64 / NP) + lane / NP;
  const bool kok = key < S;
  const int kc = kok ? key : S - 1;
  const int64_t row0 = (int64_t)seq * a.seq_stride, tld = a.pos_stride * a.ld_qkv;
  const T* qkv = (const T*)a.qkv + row0 * a.ld_qkv + h * HD;
  const T* dout = (const T*)P.dout + row0 * P.ld_dout + h * HD;
  const T* outp = (const T*)a.out + row0 * a.ld_out + h * HD;
  const int64_t dld = a.pos_stride * P.ld_dout, old_ = a.pos_stride * a.ld_out;
  const BiasCtx bc = bias_ctx(a, seq, h, S);
  float kv[DL], vv[DL], dk[DL], dv[DL];
#pragma unroll
  for (int d = 0; d < DL; ++d) {
    kv[d] = to_f32(qkv[(int64_t)kc * tld + D + c0 + d]);
    vv[d] = to_f32(qkv[(int64_t)kc * tld + 2 * D + c0 + d]);
    dk[d] = dv[d] = 0.f;
  }
  const float kb = key_only_bias<T>(bc, kc);
  const int bh = seq * a.H + h;
  const bool drop = a.drop_p > 0.f;
  for (int q0 = 0; q0 < S; q0 += LCK) {
    __syncthreads();
    long_stage<T, HD, LCK>(sQ, qkv, tld, q0, S, lane);
    long_stage<T, HD, LCK>(sO, dout, dld, q0, S, lane);
    if (NP == 1 || lane < LCK) {
      const int qi = q0 + lane;
      float de = 0.f, l = -INFINITY;
      if (qi < S) {
        l = a.lse[((int64_t)seq * a.H + h) * S + qi];
        for (int d = 0; d < HD; ++d) de = __builtin_fmaf(to_f32(dout[(int64_t)qi * dld + d]), to_f32(outp[(int64_t)qi * old_ + d]), de);
      }
      sL[lane] = l;
      sD[lane] = de;
    }
    __syncthreads();
    const int qn = S - q0 < LCK ? S - q0 : LCK;
    if (!kok || kb == -INFINITY) continue;                         // the two lanes of a key leave together
    for (int j = 0; j < qn; ++j) {
      const int q = q0 + j;
      const float l = sL[j];
      if (l == -INFINITY) continue;
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < DL; ++d) {
        s = __builtin_fmaf(sQ[j * HD + c0 + d], kv[d], s);
        dp = __builtin_fmaf(sO[j * HD + c0 + d], vv[d], dp);
      }
      s = long_pair_sum<NP>(s);
      dp = long_pair_sum<NP>(dp);
      s = s * a.scale + pair_bias<T, STRUCT>(bc, q, key);
      if (s == -INFINITY) continue;
      const float p = __expf(s - l);
      const float mk = drop ? attn_drop_scale(P.drop, bh, S, q, key) : 1.0f;
      const float pd = p * mk;
      const float ds = p * (dp * mk - sD[j]);
#pragma unroll
      for (int d = 0; d < DL; ++d) {
        dv[d] = __builtin_fmaf(pd, sO[j * HD + c0 + d], dv[d]);
        dk[d] = __builtin_fmaf(ds, sQ[j * HD + c0 + d], dk[d]);
      }
    }
  }
  if (kok) {
    T* krow = (T*)P.dqkv + (row0 + (int64_t)key * a.pos_stride) * P.ld_dqkv + h * HD + D + c0;
    T* vrow = krow + D;
#pragma unroll
    for (int d = 0; d < DL; ++d) {
      krow[d] = from_f32<T>(dk[d] * a.scale);
      vrow[d] = from_f32<T>(dv[d]);
    }
  }
}

// The forward is one launch, the backward two (dQ with the bias gradients, then dK / dV).  attn_plan (attention.hip) has
// refused what this path does not take: ragged sequences, and q_limit past 272 tokens.
int attention_long_launch(hipStream_t st, const AttnParams& p, const AttnPlan& pl) {
  return with_dtype(p.f.dtype, [&](auto t) { return with_head_dim(p.f.hd, [&](auto hd) { return with_flags(pl, [&](auto s, auto) {
    using T = typename decltype(t)::type;
    constexpr int HD = decltype(hd)::value;
    constexpr bool STRUCT = decltype(s)::value;
    constexpr int per_wg = 64 / long_parts<HD>;      // queries (keys) of a workgroup
    const dim3 grid((unsigned)((p.f.S + per_wg - 1) / per_wg), (unsigned)p.f.H, (unsigned)p.f.nseq);
    if (!pl.bwd) return launch_route<attn_long_fwd_kernel<T, HD, STRUCT>>("long", grid, 64, 0, st, p);
    if (int e = launch_route<attn_long_dq_kernel<T, HD, STRUCT>>("long", grid, 64, 0, st, p)) return e;
    return launch_route<attn_long_dkv_kernel<T, HD, STRUCT>>("long", grid, 64, 0, st, p);
  }); }); });
}

}  // namespace mdt
