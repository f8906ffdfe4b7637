// HBM-bound glue kernels of the mDT hot path: the bottleneck-token exchange between the
// text / image / graph token spaces, embedding gathers and their scatter-add gradients,
// ViT patch gather, graph node features, the pooler tanh and the fp16 weighted
// cross-entropy with F1 counters.  All are row movers: one wavefront per row, 16-byte
// vector accesses, indices precomputed by the packer (no nonzero / host sync).
#include "common.hpp"

namespace mdt {

// The skeleton of every row mover: a 256-thread workgroup is four wavefronts, one row each.  Returns the wave's row, or -1
// when it lies past the last one, and the lane within the wave.
__device__ __forceinline__ int64_t wave_row(int64_t nrows, int& lane) {
  lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  return r < nrows ? r : -1;
}

__device__ __forceinline__ int64_t pick_row(const int32_t* idx, int64_t inner, int64_t stride, int64_t off, int64_t r) {
  if (idx) return (int64_t)idx[r];
  if (inner <= 1) return r * stride + off;
  const int64_t q = r / inner;
  return q * stride + (r - q * inner) + off;
}

// dst[dr] = alpha * a[ar] + beta * b[br] (+ dst[dr]): VN = Vec<T>::N with 16-byte accesses, VN = 1 for rows that are not
// vectorisable (e.g. the [M, 2] logits).  Both forms add the terms of an element in the same order.
template <typename T, int VN>
__global__ __launch_bounds__(256) void row_axpby_kernel(int64_t nrows, int D, T* dst, int64_t ldd, const int32_t* di,
                                                        int64_t d_inner, int64_t d_stride, int64_t d_off, const T* a, int64_t lda,
                                                        const int32_t* ai, int64_t a_inner, int64_t a_stride, int64_t a_off, float alpha,
                                                        const T* b, int64_t ldb, const int32_t* bi, int64_t b_inner, int64_t b_stride,
                                                        int64_t b_off, float beta, int accumulate) {
  int lane;
  const int64_t r = wave_row(nrows, lane);
  if (r < 0) return;
  const int64_t dr = pick_row(di, d_inner, d_stride, d_off, r);
  if (dr < 0) return;
  const int64_t ar = a ? pick_row(ai, a_inner, a_stride, a_off, r) : -1;
  const int64_t br = b ? pick_row(bi, b_inner, b_stride, b_off, r) : -1;
  for (int c = lane * VN; c < D; c += 64 * VN) {
    if constexpr (VN == 1) {
      float v = 0.f;
      if (ar >= 0) v += alpha * to_f32(a[ar * lda + c]);
      if (br >= 0) v += beta * to_f32(b[br * ldb + c]);
      if (accumulate) v += to_f32(dst[dr * ldd + c]);
      dst[dr * ldd + c] = from_f32<T>(v);
    } else {
      Vec<T> va, vb, vd, o;
      if (ar >= 0) va = *(const Vec<T>*)(a + ar * lda + c);
      if (br >= 0) vb = *(const Vec<T>*)(b + br * ldb + c);
      if (accumulate) vd = *(const Vec<T>*)(dst + dr * ldd + c);
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        float v = 0.f;
        if (ar >= 0) v += alpha * va.get(j);
        if (br >= 0) v += beta * vb.get(j);
        if (accumulate) v += vd.get(j);
        o.set(j, v);
      }
      *(Vec<T>*)(dst + dr * ldd + c) = o;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void row_scatter_add_kernel(int64_t nrows, int D, float* table, int64_t ldt,
                                                              const int32_t* idx, const T* src, int64_t lds_,
                                                              int64_t s_stride, int64_t s_off) {
  int lane;
  const int64_t r = wave_row(nrows, lane);
  if (r < 0) return;
  const int64_t t = idx[r];
  if (t < 0) return;
  const T* s = src + (r * s_stride + s_off) * lds_;
  for (int c = lane; c < D; c += 64) atomicAdd(table + t * ldt + c, to_f32(s[c]));
}

// BERT embeddings, one token per wave: out row = word[ids] + type[types] + pos[l] (bert_embed_vec).
//   RAGGED = false: token r = (m, l) of M padded sequences of L, out row m * out_seq_stride + out_off + l   (mdt_bert_embed_sum)
//   RAGGED = true:  one packed row per VALID token, l = pos_ids[r], out row r                                (mdt_bert_embed_rows)
template <typename T, bool RAGGED>
__global__ __launch_bounds__(256) void bert_embed_kernel(int64_t rows, int L, const int32_t* ids, const int32_t* types,
                                                         const int32_t* pos_ids, const T* word, const T* pos, const T* type, int D,
                                                         T* out, int64_t ldo, int64_t out_seq_stride, int64_t out_off) {
  typedef Vec<T> V;
  int lane;
  const int64_t r = wave_row(rows, lane);
  if (r < 0) return;
  int64_t l, orow;
  if constexpr (RAGGED) {
    l = pos_ids[r];
    orow = r;
  } else {
    const int64_t m = r / L;
    l = r - m * L;
    orow = m * out_seq_stride + out_off + l;
  }
  const int64_t w = ids[r], t = types[r];
  T* o = out + orow * ldo;
  for (int c = lane * V::N; c < D; c += 64 * V::N) {
    const V vw = *(const V*)(word + w * D + c);
    const V vp = *(const V*)(pos + l * D + c);
    const V vt = *(const V*)(type + t * D + c);
    *(V*)(o + c) = bert_embed_vec(vw, vt, vp);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vit_patchify_kernel(int I, int C, int HW, int p, const float* img, T* cols,
                                                           int64_t ldc) {
  // one workgroup per (image, patch row): reads p full image rows per channel (coalesced)
  const int gw = HW / p;
  const int i = blockIdx.y, py = blockIdx.x;
  const int K = C * p * p;
  for (int e = threadIdx.x; e < gw * K; e += 256) {
    // e enumerates (c, dy, x) with x = px*p + dx fastest so that global reads are contiguous
    const int x = e % HW;
    const int dy = (e / HW) % p;
    const int c = e / (HW * p);
    const int px = x / p, dx = x - px * p;
    const float v = img[(((int64_t)i * C + c) * HW + (py * p + dy)) * HW + x];
    cols[((int64_t)i * gw * gw + py * gw + px) * ldc + c * p * p + dy * p + dx] = from_f32<T>(v);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vit_assemble_kernel(int I, int np, int D, const T* patches, int64_t ldp,
                                                           const T* cls, const T* pos, T* tokens, int64_t ldt,
                                                           int64_t seq_stride, int64_t off) {
  int lane;
  const int64_t r = wave_row((int64_t)I * (np + 1), lane);
  if (r < 0) return;
  const int64_t i = r / (np + 1);
  const int j = (int)(r - i * (np + 1));
  T* o = tokens + (i * seq_stride + off + j) * ldt;
  const T* s = (j == 0) ? cls : patches + (i * np + (j - 1)) * ldp;
  for (int c = lane; c < D; c += 64) o[c] = from_f32<T>(to_f32(s[c]) + to_f32(pos[(int64_t)j * D + c]));
}

template <typename T>
__global__ __launch_bounds__(256) void graph_node_feature_kernel(int B, int Tn, int D, const T* src, int64_t lds_,
                                                                 const int32_t* node_row, const int32_t* in_degree,
                                                                 const int32_t* out_degree,
                                                                 const T* in_emb, const T* out_emb, const T* graph_token,
                                                                 T* x, int64_t ldx) {
  int lane;
  const int64_t r = wave_row((int64_t)B * Tn, lane);
  if (r < 0) return;
  const int64_t b = r / Tn;
  const int t = (int)(r - b * Tn);
  T* o = x + r * ldx;
  if (t == 0) {
    for (int c = lane; c < D; c += 64) o[c] = graph_token[c];
    return;
  }
  const int64_t n = b * (Tn - 1) + (t - 1);
  const int64_t sr = node_row[n];
  const int64_t dgi = in_degree[n], dgo = out_degree[n];
  for (int c = lane; c < D; c += 64) {
    float v = to_f32(in_emb[dgi * D + c]) + to_f32(out_emb[dgo * D + c]);
    if (sr >= 0) v += to_f32(src[sr * lds_ + c]);
    o[c] = from_f32<T>(v);
  }
}

template <typename T>
__global__ void tanh_fwd_kernel(int64_t n, const T* x, T* y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = from_f32<T>(tanhf(to_f32(x[i])));
}
template <typename T>
__global__ void tanh_bwd_kernel(int64_t n, const T* y, const T* dy, T* dx) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float t = to_f32(y[i]);
    dx[i] = from_f32<T>(to_f32(dy[i]) * (1.f - t * t));
  }
}

// fp16 round-trip (round to nearest even) — the reference casts logits with
// .type(torch.HalfTensor) (criterions/hatespeech_loss.py:95), so the loss and dL/dlogits
// see fp16-rounded logits.
__device__ __forceinline__ float round_f16(float v) { return (float)(_Float16)v; }

// Arithmetic of the reference's loss on its CPU path, step by step (PyTorch's Half kernels round where they store):
//   log_softmax (vec_log_softmax_lastdim, scalar_t = Half): the sum of exp(x - max) is stored as Half, so is its log,
//     then out = half((x - max) - logsum);
//   softmax for the predictions (vec_softmax_lastdim): exp and the sum stay in float, out = half(e * (1 / sum)) —
//     two close logits can tie after the rounding, and argmax then returns index 0;
//   nll_loss (nll_loss_out_frame, reduction "sum"): every term half(logp * w) is subtracted from Half partial sums
//     cascaded in blocks of 16 (level_power = max(4, ceil(log2 n) / 8)), the 8 levels are added up in Half;
//   backward: d logits = half(w * (exp(logp) - onehot)) (one rounding), cast back by the .type(HalfTensor) adjoint.
// Checked against torch 2.10 CPU on random logits: bit-equal but for 1-ulp differences between expf / logf here and
// sleef's there on knife-edge roundings (tests/test_kernels_gpu.py::test_node_ce_matches_torch_cpu_half).
template <typename T>
__global__ __launch_bounds__(256) void node_ce_kernel(int64_t M, int nlab, const T* logits, const int32_t* rows,
                                                      const int32_t* targets, float w_neg, float w_pos, int fp16_loss,
                                                      float grad_scale, float* out_loss, int32_t* counters, T* dlogits) {
  // single workgroup: nlab is the number of labelled comments in the batch (tens to a few thousand)
  __shared__ float s_loss[256];
  __shared__ int s_cnt[4][256];
  __shared__ float s_part[8];
  float loss = 0.f;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  int level_power = 4;
  if (fp16_loss) {
    int lg = 0;
    while ((1ll << lg) < (long long)nlab) ++lg;          // ceil(log2(nlab))
    if (lg / 8 > level_power) level_power = lg / 8;
    if (threadIdx.x < 8) s_part[threadIdx.x] = 0.f;
  }
  for (int base = 0; base < nlab; base += 256) {
    const int i = base + threadIdx.x;
    float term = 0.f;
    if (i < nlab) {
      const int64_t r = rows[i];
      const int y = targets[i];
      float l0 = to_f32(logits[r * 2]), l1 = to_f32(logits[r * 2 + 1]);
      float wn = w_neg, wp = w_pos;
      if (fp16_loss) { l0 = round_f16(l0); l1 = round_f16(l1); wn = round_f16(wn); wp = round_f16(wp); }
      const float m = fmaxf(l0, l1);
      const float e0 = expf(l0 - m), e1 = expf(l1 - m);
      float lp0, lp1;
      int pred;
      if (fp16_loss) {
        const float ls = round_f16(logf(round_f16(e0 + e1)));
        lp0 = round_f16((l0 - m) - ls);
        lp1 = round_f16((l1 - m) - ls);
        const float inv = 1.0f / (e0 + e1);
        pred = (round_f16(e1 * inv) > round_f16(e0 * inv)) ? 1 : 0;      // ties -> index 0 like torch.argmax
      } else {
        const float ls = logf(e0 + e1);
        lp0 = (l0 - m) - ls;
        lp1 = (l1 - m) - ls;
        pred = (l1 > l0) ? 1 : 0;
      }
      const float w = y ? wp : wn;
      term = w * (y ? lp1 : lp0);
      if (fp16_loss) term = round_f16(term);
      loss -= term;
      c0 += (pred == y);
      c1 += (pred == y && pred == 1);
      c2 += (y == 1);
      c3 += (pred == 1);
      if (dlogits) {
        // autograd differentiates through the (fp16-rounded) log-softmax output
        const float p0 = expf(lp0), p1 = expf(lp1);
        float g0 = w * (p0 - (y == 0 ? 1.f : 0.f)), g1 = w * (p1 - (y == 1 ? 1.f : 0.f));
        if (fp16_loss) { g0 = round_f16(g0); g1 = round_f16(g1); }
        dlogits[r * 2] = from_f32<T>(g0 * grad_scale);
        dlogits[r * 2 + 1] = from_f32<T>(g1 * grad_scale);
      }
    }
    if (fp16_loss) {
      // the Half cascade is order-dependent: one thread walks this chunk's terms in label order
      __syncthreads();
      s_loss[threadIdx.x] = term;
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = nlab - base < 256 ? nlab - base : 256;
        const int lmask = (1 << level_power) - 1;
        for (int k = 0; k < n; ++k) {
          const int idx = base + k;
          s_part[0] = round_f16(s_part[0] - s_loss[k]);
          for (int j = 0; j + 1 < 8; ++j) {
            if ((idx & (lmask << (j * level_power))) != 0) break;
            s_part[j + 1] = round_f16(s_part[j + 1] + s_part[j]);
            s_part[j] = 0.f;
          }
        }
      }
    }
  }
  __syncthreads();
  s_loss[threadIdx.x] = loss;
  s_cnt[0][threadIdx.x] = c0; s_cnt[1][threadIdx.x] = c1; s_cnt[2][threadIdx.x] = c2; s_cnt[3][threadIdx.x] = c3;
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f;
    int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int i = 0; i < 256; ++i) { L += s_loss[i]; a0 += s_cnt[0][i]; a1 += s_cnt[1][i]; a2 += s_cnt[2][i]; a3 += s_cnt[3][i]; }
    if (fp16_loss) {
      L = 0.f;
      for (int j = 0; j < 8; ++j) L = round_f16(L + s_part[j]);
    }
    out_loss[0] = L;
    counters[0] = a0; counters[1] = a1; counters[2] = a2; counters[3] = a3;
  }
}

}  // namespace mdt

using namespace mdt;

// the launch that goes with wave_row: four rows per 256-thread workgroup
template <auto Kern, typename... Args>
static int launch_rows(const char* name, hipStream_t st, int64_t nrows, Args... args) {
  return launch_plain<Kern>(name, (unsigned)((nrows + 3) / 4), 256, st, args...);
}

extern "C" int mdt_row_axpby(void* stream, int dtype, int64_t nrows, int D, void* dst, int64_t ldd, const int32_t* di,
                             int64_t d_inner, int64_t d_stride, int64_t d_off, const void* a, int64_t lda, const int32_t* ai,
                             int64_t a_inner, int64_t a_stride, int64_t a_off, float alpha, const void* b, int64_t ldb,
                             const int32_t* bi, int64_t b_inner, int64_t b_stride, int64_t b_off, float beta, int accumulate) {
  if (nrows == 0) return MDT_OK;
  MDT_CHECK_ARG(dst, "row_axpby: null dst");
  MDT_CHECK_ARG(dtype == MDT_F32 || dtype == MDT_BF16, "row_axpby: bad dtype %d", dtype);
  const bool vec = vec16_ok(dtype, D, {ldd, a ? lda : 0, b ? ldb : 0}, {dst, a, b});
  const int e = with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto launch = [&](auto vn) {
      return launch_rows<row_axpby_kernel<T, decltype(vn)::value>>("row_axpby", (hipStream_t)stream, nrows, nrows, D, (T*)dst, ldd, di, d_inner, d_stride,
                                                                   d_off, (const T*)a, lda, ai, a_inner, a_stride, a_off, alpha, (const T*)b, ldb, bi,
                                                                   b_inner, b_stride, b_off, beta, accumulate);
    };
    return vec ? launch(std::integral_constant<int, Vec<T>::N>{}) : launch(std::integral_constant<int, 1>{});
  });
  if (e == MDT_OK) set_last_route(vec ? "row_vec" : "row_scalar");
  return e;
}

extern "C" int mdt_row_scatter_add_f32(void* stream, int dtype, int64_t nrows, int D, float* table, int64_t ldt,
                                       const int32_t* idx, const void* src, int64_t lds_, int64_t s_stride, int64_t s_off) {
  if (nrows == 0) return MDT_OK;
  MDT_CHECK_ARG(table && idx && src, "row_scatter_add: null pointer");
  note_float_atomic_launch();
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_rows<row_scatter_add_kernel<T>>("row_scatter_add", (hipStream_t)stream, nrows, nrows, D, table, ldt, idx, (const T*)src, lds_, s_stride, s_off);
  });
}

// mdt_bert_embed_sum (padded: pos_ids null, rows = M * L) and mdt_bert_embed_rows (ragged: L, out_seq_stride, out_off unused)
template <bool RAGGED>
static int bert_embed(const char* name, void* stream, int dtype, int64_t rows, int L, const int32_t* ids, const int32_t* types,
                      const int32_t* pos_ids, const void* word, const void* pos, const void* type, int D, void* out, int64_t ldo,
                      int64_t out_seq_stride, int64_t out_off) {
  MDT_CHECK_ARG(ids && types && (pos_ids || !RAGGED) && word && pos && type && out, "%s: null pointer", name);
  MDT_CHECK_ARG(vec16_ok(dtype, D, {ldo}, {out}), "row op: D=%d / ld=%lld / pointer not 16-byte vectorisable", D, (long long)ldo);
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_rows<bert_embed_kernel<T, RAGGED>>(name, (hipStream_t)stream, rows, rows, L, ids, types, pos_ids, (const T*)word, (const T*)pos,
                                                     (const T*)type, D, (T*)out, ldo, out_seq_stride, out_off);
  });
}

extern "C" int mdt_bert_embed_sum(void* stream, int dtype, int64_t M, int L, const int32_t* ids, const int32_t* types,
                                  const void* word, const void* pos, const void* type, int D, void* out, int64_t ldo,
                                  int64_t out_seq_stride, int64_t out_off) {
  if (M == 0) return MDT_OK;
  return bert_embed<false>("bert_embed_sum", stream, dtype, M * L, L, ids, types, nullptr, word, pos, type, D, out, ldo, out_seq_stride, out_off);
}

extern "C" int mdt_bert_embed_rows(void* stream, int dtype, int64_t rows, const int32_t* ids, const int32_t* types,
                                   const int32_t* pos_ids, const void* word, const void* pos, const void* type, int D,
                                   void* out, int64_t ldo) {
  if (rows == 0) return MDT_OK;
  return bert_embed<true>("bert_embed_rows", stream, dtype, rows, 0, ids, types, pos_ids, word, pos, type, D, out, ldo, 0, 0);
}

extern "C" int mdt_vit_patchify(void* stream, int dtype, int I, int C, int HW, int p, const float* img, void* cols, int64_t ldc) {
  if (I == 0) return MDT_OK;
  MDT_CHECK_ARG(img && cols && p > 0 && HW % p == 0, "vit_patchify: bad arguments");
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<vit_patchify_kernel<T>>("vit_patchify", dim3(HW / p, I), 256, (hipStream_t)stream, I, C, HW, p, img, (T*)cols, ldc);
  });
}

extern "C" int mdt_vit_assemble(void* stream, int dtype, int I, int np, int D, const void* patches, int64_t ldp,
                                const void* cls, const void* pos, void* tokens, int64_t ldt, int64_t seq_stride, int64_t off) {
  if (I == 0) return MDT_OK;
  MDT_CHECK_ARG(patches && cls && pos && tokens, "vit_assemble: null pointer");
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_rows<vit_assemble_kernel<T>>("vit_assemble", (hipStream_t)stream, (int64_t)I * (np + 1), I, np, D, (const T*)patches, ldp, (const T*)cls,
                                               (const T*)pos, (T*)tokens, ldt, seq_stride, off);
  });
}

extern "C" int mdt_graph_node_feature(void* stream, int dtype, int B, int T, int D, const void* src, int64_t lds_,
                                      const int32_t* node_row, const int32_t* in_degree, const int32_t* out_degree,
                                      const void* in_emb, const void* out_emb, const void* graph_token, void* x,
                                      int64_t ldx) {
  if (B == 0) return MDT_OK;
  MDT_CHECK_ARG(node_row && in_degree && out_degree && in_emb && out_emb && graph_token && x, "graph_node_feature: null pointer");
  return with_dtype(dtype, [&](auto t) {
    using E = typename decltype(t)::type;
    return launch_rows<graph_node_feature_kernel<E>>("graph_node_feature", (hipStream_t)stream, (int64_t)B * T, B, T, D, (const E*)src, lds_, node_row,
                                                     in_degree, out_degree, (const E*)in_emb, (const E*)out_emb, (const E*)graph_token, (E*)x, ldx);
  });
}

// flat grid-stride launches of the pooler tanh: up to 2048 workgroups of 256
static unsigned tanh_grid(int64_t n) { return (unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256); }

extern "C" int mdt_tanh_fwd(void* stream, int dtype, int64_t n, const void* x, void* y) {
  if (n == 0) return MDT_OK;
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<tanh_fwd_kernel<T>>("tanh_fwd", tanh_grid(n), 256, (hipStream_t)stream, n, (const T*)x, (T*)y);
  });
}

extern "C" int mdt_tanh_bwd(void* stream, int dtype, int64_t n, const void* y, const void* dy, void* dx) {
  if (n == 0) return MDT_OK;
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<tanh_bwd_kernel<T>>("tanh_bwd", tanh_grid(n), 256, (hipStream_t)stream, n, (const T*)y, (const T*)dy, (T*)dx);
  });
}

extern "C" int mdt_node_ce(void* stream, int dtype, int64_t M, int nlab, const void* logits, const int32_t* rows,
                           const int32_t* targets, float w_neg, float w_pos, int fp16_loss, float grad_scale,
                           float* out_loss, int32_t* counters, void* dlogits) {
  MDT_CHECK_ARG(logits && out_loss && counters, "node_ce: null pointer");
  MDT_CHECK_ARG(nlab == 0 || (rows && targets), "node_ce: null rows / targets");
  hipStream_t st = (hipStream_t)stream;
  if (dlogits) {
    if (hipMemsetAsync(dlogits, 0, (size_t)M * 2 * dtype_size(dtype), st) != hipSuccess) {
      (void)hipGetLastError();
      set_error("node_ce: memset failed");
      return MDT_ERR_LAUNCH;
    }
  }
  return with_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch_plain<node_ce_kernel<T>>("node_ce", 1, 256, st, M, nlab, (const T*)logits, rows, targets, w_neg, w_pos, fp16_loss, grad_scale, out_loss,
                                           counters, (T*)dlogits);
  });
}
