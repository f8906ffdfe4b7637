/*
 * mdt_hip.h — C ABI of the MI355X-native (gfx950) mDT hot path.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes / a HIP stream
 * (as `void*` = hipStream_t) and NO torch types.  The caller owns every buffer,
 * workspace included; the library allocates nothing and never synchronises the host.
 * Its only state: a thread-local error string, the MDT_* environment switches read
 * once at the first launch (mdt_reload_env re-reads them) and the pointer to the
 * caller's tile-queue buffer (mdt_gemm_set_tile_queue, optional).  Entry points are
 * re-entrant, so forward and backward may run on different host threads and any call
 * sequence can be captured in a hipGraph.  (The profiling switch MDT_GEMM_STAMP=1 is
 * the one exception: it allocates, synchronises and prints — never set in production.)
 *
 * Return value: 0 on success, a negative mdt_status otherwise; the message is
 * available through mdt_last_error_string() on the calling thread.
 *
 * The reference has no native boundary for this path (it is eager PyTorch); each
 * function cites the reference operator sequence it replaces (paths relative to
 * /root/reference/mDT/src).  INTEGRATION.md shows the reference-side binding.
 */
#ifndef MDT_HIP_H
#define MDT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDT_ABI_VERSION 1

typedef enum { MDT_F32 = 0, MDT_BF16 = 1 } mdt_dtype;

typedef enum {
  MDT_OK = 0,
  MDT_ERR_ARG = -1,          /* shape / alignment / null-pointer contract violated */
  MDT_ERR_INVALID = MDT_ERR_ARG, /* the same status: what the ordered entry points return for a workspace that is too small */
  MDT_ERR_UNSUPPORTED = -2,  /* valid request this build has no kernel for */
  MDT_ERR_LAUNCH = -3        /* hipLaunch / hipMemsetAsync reported an error */
} mdt_status;

/* GEMM epilogue selector (bit flags) */
enum {
  MDT_EPI_BIAS = 1,      /* + bias[n] */
  MDT_EPI_GELU = 2,      /* erf-GELU; if aux != NULL the pre-activation is stored there */
  MDT_EPI_RESIDUAL = 4,  /* + residual[m, n] */
  MDT_EPI_DGELU = 8,     /* * gelu'(aux[m, n]) (backward of MDT_EPI_GELU) */
  MDT_EPI_ACCUM = 16,    /* C += result (plain read-modify-write, fp32 or T) */
  MDT_EPI_ATOMIC = 32,   /* C (fp32) += result with float atomics (split-K weight gradients) */
  MDT_EPI_COLSUM = 128,  /* colsum[n] += sum_m C[m, n] (fp32 atomics) — the bias gradient of the layer whose
                            output gradient this GEMM produces, fused instead of a separate pass.  Summed is the fp32
                            epilogue result r[m, n] of THIS call, before it is rounded to C's type: with MDT_EPI_ACCUM
                            (C = C_old + r) the old contents of C are not part of the sum — colsum[n] += sum_m r[m, n] */
  MDT_EPI_AUX_GRAD = 256, /* with MDT_EPI_GELU and aux != NULL: aux receives d out / d pre-activation
                            (GELU'(u), times the dropout scale of the element when MDT_EPI_DROPOUT is set)
                            instead of u — the backward pass is then a plain MDT_EPI_MULAUX */
  MDT_EPI_MULAUX = 512,  /* * aux[m, n] (backward of an epilogue that saved its derivative) */
  MDT_EPI_ASUM = 1024,   /* colsum[m] += sum_k op(A)[m, k] (fp32 atomics, NOT scaled by alpha): with trans_a = 1 the column sums of the STORED
                            A — the bias gradient db = colsum(dY) riding on the weight-gradient GEMM dW = dY^T X that
                            streams dY anyway (one extra MFMA against a vector of ones per A fragment, in the workgroups
                            of the first tile column only).  Needs trans_a = 1, MDT_EPI_ATOMIC and a colsum buffer of M
                            floats; excludes MDT_EPI_COLSUM (the two share the buffer argument) */
  MDT_EPI_DROPOUT = 64   /* inverted dropout on the value after bias / GELU and before the residual add
                            (with MDT_EPI_DGELU: on the incoming gradient, before the GELU' factor);
                            element (m, n) of site `drop_seed` uses counter m*N + n */
};

int mdt_abi_version(void);
const char* mdt_last_error_string(void);
/* The route of the calling thread's last successful GEMM, attention, LayerNorm or mdt_row_axpby launch ("" before the first): mdt_gemm "generic",
 * "tile128", "tile256x128", "pp256", "pp256p", "w4p", "w4s"; mdt_gemm_fp8 "f8_w4", "f8_pp256p"; attention "v1" ... "v5", "v4x",
 * "long" (forward and backward; mdt_attention_route names the route of an argument block without launching); mdt_layernorm_fwd "ln_fwd", mdt_layernorm_fwd_q8 with an fp8 copy "ln_fwd_q8", mdt_layernorm_bwd "ln_rows" (the
 * scalar-address kernel) or "ln_generic"; mdt_row_axpby "row_vec" (16-byte vectors) or "row_scalar" (D, a row stride or a base pointer
 * of dst / a / b not vectorisable); mdt_act_fwd "act_vec" or "act_scalar".  What MDT_GEMM_ROUTE / MDT_ATTN_BWD force is checked against it (a forced route whose preconditions fail runs the default). */
const char* mdt_last_route(void);
/* sha256 (hex) over csrc/ and this header at the time the library was linked (build.py source_hash()): the Python side
 * refuses a libmdt_hip.so that was not built from the sources next to it. */
const char* mdt_source_hash(void);

/* ------------------------------------------------------------------ GEMM
 * C[M,N] = epilogue( alpha * op(A)[M,K] @ op(B)[K,N] )
 *   trans_a = 0: A stored [M,K] (lda = row stride);  1: stored [K,M]
 *   trans_b = 0: B stored [N,K] (nn.Linear weight, y = x W^T);  1: stored [K,N]
 * Replaces nn.Linear forward and its autograd (modules/multihead_attention.py:134-137,203;
 * modules/graphormer_graph_encoder_layer.py:135-137; HF BertLayer/ViTLayer dense layers
 * called from modules/multi_graphormer_fusion_layer.py:94-96,138-146).
 * dtype: element type of A, B, bias, residual, aux.  out_dtype: element type of C.
 * split_k > 1 requires MDT_EPI_ATOMIC and a pre-zeroed (or accumulating) fp32 C.
 */
int mdt_gemm(void* stream, int dtype, int out_dtype, int trans_a, int trans_b,
             int64_t M, int64_t N, int64_t K,
             const void* A, int64_t lda, const void* B, int64_t ldb,
             void* C, int64_t ldc, int epilogue, float alpha,
             const void* bias, const void* residual, int64_t ldr,
             void* aux, int64_t ldaux, int split_k, float drop_p, uint64_t drop_seed, float* colsum);
/* Dynamic tile queue of the persistent GEMM (MDT_GEMM_DYNAMIC=1, for nodes where RCCL kernels hold compute units during
 * backward): the queue heads live in a CALLER-OWNED device buffer of mdt_gemm_tile_queue_bytes() bytes, zero-initialised
 * by the caller and registered once (NULL unregisters); the library allocates nothing.  Without it the static tile walk
 * is used. */
size_t mdt_gemm_tile_queue_bytes(void);
int mdt_gemm_set_tile_queue(void* zeroed_device_buffer, size_t bytes);
/* Re-read the MDT_* environment switches (tuning / diagnostics).  They are read once, at the first launch; a host that
 * changes them afterwards (tests, A/B tools) calls this. */
void mdt_reload_env(void);

/* Inverted dropout as a stand-alone op: y[m, n] = x[m, n] * keep(seed, m*D + n) / (1 - p).  The mask is
 * a pure function of (seed, counter), so calling it on the gradient with the same seed is the backward
 * (FairseqDropout / nn.Dropout in modules/graphormer_graph_encoder_layer.py:127,136,138,
 * modules/multigraphormer_graph_encoder.py:403 and inside HF BertLayer / ViTLayer). */
int mdt_dropout(void* stream, int dtype, int64_t rows, int D, const void* x, int64_t ldx, void* y, int64_t ldy,
                float p, uint64_t seed);
/* Test hook: mask[i] = 1 if counter i of site `seed` is kept. */
int mdt_dropout_mask(void* stream, int64_t n, float p, uint64_t seed, uint8_t* mask);

/* FFN activation as a launch of its own (fairseq utils.get_activation_fn as used by modules/graphormer_graph_encoder_layer.py:50,135;
 * the fused fc1 epilogue MDT_EPI_GELU | MDT_EPI_AUX_GRAD knows the erf GELU only): rows x N elements,
 *   h[r, c] = act(pre[r, c]) * s,  u[r, c] = act'(pre[r, c]) * s,  s = keep(drop_seed, r*N + c) / (1 - drop_p), 1 when drop_p == 0
 * (the counters of mdt_dropout, so mdt_dropout_mask regenerates the mask).  u is what the backward GEMM multiplies by
 * (MDT_EPI_MULAUX).  h may be pre; u may be NULL (forward without a tape).  fp32 arithmetic, one rounding per store.
 *   GELU           0.5 x (1 + erf(x / sqrt 2))   (the fp32 formula of the fused epilogue, for comparison with it)
 *   RELU           x > 0 ? x : 0, derivative x > 0; a NaN stays a NaN in h
 *   GELU_ACCURATE  0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))   (fairseq gelu_accurate, and its alias gelu_fast)
 *   TANH           derivative 1 - tanh^2
 *   LINEAR         h = x s, u = s
 * 16-byte loads and stores when N, the three row strides (multiples of 4 fp32 / 8 bf16 elements) and the pointers allow it,
 * else one element per lane; mdt_last_route() says which ran ("act_vec" / "act_scalar"). */
enum { MDT_ACT_GELU = 0, MDT_ACT_RELU = 1, MDT_ACT_GELU_ACCURATE = 2, MDT_ACT_TANH = 3, MDT_ACT_LINEAR = 4 };
int mdt_act_fwd(void* stream, int dtype, int kind, int64_t rows, int N, const void* pre, int64_t ld_pre, void* h, int64_t ld_h,
                void* u, int64_t ld_u, float drop_p, uint64_t drop_seed);

/* Column sums: out[n] (+)= sum_m w[m] * X[m,n]  (bias gradients; w = NULL means 1, otherwise an
 * int32 row weight — token-type embedding gradient).  out is fp32, accumulated with atomics —
 * zero it first unless accumulating. */
int mdt_colsum(void* stream, int dtype, int64_t M, int64_t N, const void* X, int64_t ldx, float* out,
               const int32_t* row_weight);

/* ------------------------------------------------------------------ LayerNorm
 * y = (x - mean) * rstd * gamma + beta, rows of width D (fairseq LayerNorm eps 1e-5,
 * HF LayerNorm eps 1e-12: modules/graphormer_graph_encoder_layer.py:127-130,138-141;
 * modules/multigraphormer_graph_encoder.py:400-403).  mean / rstd are fp32 [rows].
 */
int mdt_layernorm_fwd(void* stream, int dtype, int64_t rows, int D, const void* x, int64_t ldx,
                      const void* gamma, const void* beta, float eps,
                      void* y, int64_t ldy, float* mean, float* rstd);
/* mdt_layernorm_fwd (bf16 rows) whose output ALSO leaves as fp8 for the 8-bit GEMM that consumes it (fp8 operands, below):
 * q8_out u8[rows, D] (rows of ld_q8 bytes) = saturate(q8_format, y * *q8_scale), *q8_amax = max(*q8_amax, max |y|) — bit for bit
 * what mdt_fp8_quantize makes of y, without its pass over y.  q8_out NULL: plain mdt_layernorm_fwd. */
int mdt_layernorm_fwd_q8(void* stream, int dtype, int64_t rows, int D, const void* x, int64_t ldx, const void* gamma,
                         const void* beta, float eps, void* y, int64_t ldy, float* mean, float* rstd, void* q8_out,
                         int64_t ld_q8, int q8_format, const float* q8_scale, float* q8_amax);
/* dx = LN'(dy) (+ add[m,:] if add != NULL);  dgamma/dbeta fp32, atomically accumulated.
 * Optional fused tail for the layer that FEEDS this LayerNorm through a hidden dropout + residual:
 *   dxd (may be NULL) = dx * keep(drop_seed, m*D + n) / (1 - drop_p)   — gradient of the dense output,
 *   colsum (may be NULL, fp32[D]) += column sums of dxd (of dx when dxd is NULL) — that layer's bias gradient. */
int mdt_layernorm_bwd(void* stream, int dtype, int64_t rows, int D, const void* dy, int64_t lddy,
                      const void* x, int64_t ldx, const void* gamma, const float* mean, const float* rstd,
                      const void* add, int64_t ldadd, void* dx, int64_t lddx, float* dgamma, float* dbeta,
                      void* dxd, int64_t lddxd, float drop_p, uint64_t drop_seed, float* colsum);

/* ------------------------------------------------------------------ attention
 * Self-attention over `nseq` independent sequences of `S` tokens, `H` heads of `hd`,
 * q|k|v packed per token: qkv[row, 0:D | D:2D | 2D:3D], D = H*hd.  Row of token p of
 * sequence s = s*seq_stride + p*pos_stride (so batch-major and fairseq's time-major
 * [T,B,C] layouts need no copy).  scores = scale * q.k + bias, softmax in fp32,
 * out[row, h*hd:(h+1)*hd] = P @ v.  lse[s,h,p] (fp32) is saved for backward.
 * Head widths: hd = 16, 64, 96 or 128, in fp32 and in bf16 (any S; seq_ids / s_cap launches: bf16, hd = 64 only).
 *
 * Row tensors.  qkv / ld_qkv, out / ld_out, dout / ld_dout and dqkv / ld_dqkv are four independent (base, row stride in
 * elements) pairs; a stride is at least the row's width (3 D for qkv and dqkv, D for out and dout), and the columns past the
 * width are neither read nor written.  bf16: the kernels move all four in 16-byte vectors, so every base is 16-byte aligned and
 * every row stride a multiple of 8 elements.  fp32: every kernel family (v1, the key-chunked path, the weight outputs) moves
 * one element at a time — any row stride, the base on a 4-byte boundary.  Anything else is MDT_ERR_ARG with the
 * tensor's name in the message, from the launch and from mdt_attention_route alike.  Writes: rows of the launch's sequences
 * below their length, columns below the width; lse[s, h, 0 .. S) of those sequences; nothing else — not the rows between two
 * sequences (seq_stride > S), not a sequence that seq_ids does not name, not a byte outside d_dense_bias [nseq,H,S,S],
 * d_sp_table [num_spatial,H] or d_virt [H].
 *
 * Bias / mask sources, all optional (NULL):
 *   key_mask   u8[nseq,S]   1 = key may be attended (HF additive mask, quirk 9 of
 *                           −65504 / finfo.min ≡ excluded)
 *   dense_bias f32[nseq,H,S,S]   additive (modules/multihead_attention.py:173-174)
 *   structural (modules/graphormer_layers.py:86-110 fused, never materialised):
 *     attn_bias f32[nseq,S,S] (added TWICE, :93 and :108), spatial_pos i32[nseq,S-1,S-1],
 *     sp_table T[num_spatial,H], virt T[H] (graph-token virtual distance)
 *   key_pad    u8[nseq,S]   1 = padded key → −inf (multihead_attention.py:180-187)
 */
typedef struct {
  int dtype;
  int nseq, S, H, hd;
  int64_t seq_stride, pos_stride; /* in rows */
  float scale;
  const void* qkv; int64_t ld_qkv;
  void* out; int64_t ld_out;
  float* lse;
  const uint8_t* key_mask;
  const float* dense_bias;
  const float* attn_bias;
  const int32_t* spatial_pos;
  const void* sp_table;
  const void* virt;
  const uint8_t* key_pad;
  int num_spatial;
  float drop_p;              /* attention-probability dropout (0 = off); counter ((s*H + h)*S + q)*S2 + key, S2 = S rounded up to even */
  uint64_t drop_seed;
  const int32_t* seq_offsets; /* NULL, or i32[nseq + 1]: RAGGED sequences — sequence s is the S_s = off[s+1] - off[s] <= S
                                 consecutive rows starting at row off[s] (seq_stride unused, pos_stride must be 1, no masks /
                                 biases: every packed token is valid).  S stays the bound that sizes lse [nseq,H,S] and the
                                 dropout counters.  This is how padded token positions of a comment batch are never computed. */
  int q_limit;                /* 0 = every query row.  n > 0: only the first n rows of each sequence are needed as QUERIES
                                 (keys / values are always the whole sequence): forward leaves `out` / `lse` of the other rows
                                 unwritten (backward never reads them), backward assumes their `dout` is zero and does not
                                 write their dQ — the caller zeroes the dQ third of dqkv beforehand; dK / dV are written for
                                 every row.  Kernels may round n up (they work in 16-row tiles) or ignore it. */
  const int32_t* seq_ids;     /* NULL, or i32[nseq] (ragged bf16 launches only): this launch covers the sequences
                                 seq_ids[0 .. nseq) of a ragged set of `nseq_total` sequences — seq_offsets has nseq_total + 1
                                 entries, lse is [nseq_total, H, S] and the dropout counters use the sequence's own index, so a
                                 set may be processed as several launches (length bins) with bit-identical results. */
  int s_cap;                  /* 0, or: no sequence of THIS launch is longer than s_cap (<= S) rows.  Kernels size their LDS
                                 images and unrolled key loops by it instead of by S (a bin of short comments then runs the
                                 small kernels); S keeps defining the lse / dropout-counter geometry.  A longer sequence is
                                 skipped, not computed wrongly — the caller's host-side lengths are the contract. */
  int nseq_total;             /* with seq_ids: size of the whole ragged set (0 = nseq) */
} mdt_attn_fwd_args;
int mdt_attention_fwd(void* stream, const mdt_attn_fwd_args* a);

typedef struct {
  mdt_attn_fwd_args f;        /* same tensors as forward (out = forward output, lse filled) */
  const void* dout; int64_t ld_dout;
  void* dqkv; int64_t ld_dqkv;
  float* d_dense_bias;        /* f32[nseq,H,S,S] or NULL */
  float* d_sp_table;          /* f32[num_spatial,H], atomically accumulated, or NULL */
  float* d_virt;              /* f32[H], atomically accumulated, or NULL */
} mdt_attn_bwd_args;
int mdt_attention_bwd(void* stream, const mdt_attn_bwd_args* a);
/* What mdt_attention_fwd (bwd = 0: only a->f is read) or mdt_attention_bwd (bwd = 1) would do with this argument block, without
 * launching anything: the same argument checks and the same plan (attn_plan, csrc/attention.hip — the routing table is
 * documented there).  route receives the name mdt_last_route() would report after the launch ("v1" ... "v5", "v4x", "long");
 * geometry what tells two launches of one route apart: {key-tile rung, 0} for "v1" and the "v2" backward, {rung, waves} for
 * the "v2" forward, {padded length, threads} for "v3", {waves, 0} for "v4" / "v4x", {0, 0} for "v5" / "long".  Returns what
 * the launch would return: for a refused block the error code, with the message in mdt_last_error_string(), route "" and
 * geometry {0, 0}.  MDT_ATTN_BWD is honoured as a launch honours it.  Pointers in the block are looked at for null-ness and
 * alignment only and never dereferenced, so any non-null, 16-byte aligned values will do; no device is needed. */
int mdt_attention_route(const mdt_attn_bwd_args* a, int bwd, char* route, size_t route_bytes, int32_t geometry[2]);
/* Head-averaged attention probabilities, fp32 [nseq, S, S] (modules/multihead_attention.py:205-214, need_weights=True):
 * recomputed from the qkv buffer and the log-sum-exp mdt_attention_fwd wrote (same args struct; out / dropout fields are
 * not read).  Masked keys give 0. */
int mdt_attention_mean_probs(void* stream, const mdt_attn_fwd_args* a, float* out);
/* Per-head weights of the same attention (need_head_weights / before_softmax of modules/multihead_attention.py:91-102,186-214):
 * out fp32 [nseq, H, S, S] = softmax probabilities before dropout (raw_scores = 0; needs a->lse) or the scores
 * q k^T * scale + bias with masked keys at -inf (raw_scores = 1).  Dense sequences only. */
int mdt_attention_head_weights(void* stream, const mdt_attn_fwd_args* a, int raw_scores, float* out);

/* Materialise the [nseq,H,S,S] structural bias (API parity with GraphAttnBias.forward,
 * modules/graphormer_layers.py:86-110); the fused encoder path never calls this. */
int mdt_graph_attn_bias(void* stream, int dtype, int nseq, int S, int H, const float* attn_bias,
                        const int32_t* spatial_pos, const void* sp_table, const void* virt,
                        float* out);

/* ------------------------------------------------------------------ row movers
 * dst[di(r), :] = alpha * a[ai(r), :] + beta * b[bi(r), :] (+ dst if accumulate)
 * for r in [0, nrows); an index array may be NULL and then a two-level affine map is
 * applied: row = (r / inner) * stride + r % inner + offset (inner = 1: r*stride + offset).
 * A negative index skips the row (dst) or contributes zero (a, b).  Rows of 16-byte vectors (D and every row stride a multiple of
 * 4 fp32 / 8 bf16 elements, dst / a / b on a 16-byte boundary) take the vector kernel, everything else the scalar one, with the
 * same arithmetic; mdt_last_route() says which ran ("row_vec" / "row_scalar").  This one kernel is the bottleneck-token
 * exchange between the text, image and graph token spaces
 * (modules/multigraphormer_graph_encoder.py:339,363-371,425,435;
 *  modules/multi_graphormer_fusion_layer.py:37-66) on precomputed CSR indices — the
 * reference's boolean-mask indexing (implicit nonzero + host sync) is gone.
 */
int mdt_row_axpby(void* stream, int dtype, int64_t nrows, int D,
                  void* dst, int64_t ldd, const int32_t* di, int64_t d_inner, int64_t d_stride, int64_t d_off,
                  const void* a, int64_t lda, const int32_t* ai, int64_t a_inner, int64_t a_stride, int64_t a_off, float alpha,
                  const void* b, int64_t ldb, const int32_t* bi, int64_t b_inner, int64_t b_stride, int64_t b_off, float beta,
                  int accumulate);
/* fp32 table[idx[r], :] += src[r, :]  (embedding backward; atomics).  idx < 0 skipped. */
int mdt_row_scatter_add_f32(void* stream, int dtype, int64_t nrows, int D, float* table, int64_t ldt,
                            const int32_t* idx, const void* src, int64_t lds, int64_t s_stride, int64_t s_off);

/* BERT embeddings: out[r,:] = word[ids[r]] + pos[r % L] + type[types[r]]  (pre-LayerNorm sum;
 * HF BertEmbeddings, call site modules/multigraphormer_graph_encoder.py:325-329).
 * Row r of the [M, L] id matrix goes to out row (r / L) * out_seq_stride + out_off + r % L. */
int mdt_bert_embed_sum(void* stream, int dtype, int64_t M, int L, const int32_t* ids, const int32_t* types,
                       const void* word, const void* pos, const void* type, int D,
                       void* out, int64_t ldo, int64_t out_seq_stride, int64_t out_off);

/* Ragged form of the same sum: one output row per VALID token (padded positions are never materialised);
 * out[r,:] = word[ids[r]] + pos[pos_ids[r]] + type[types[r]]. */
int mdt_bert_embed_rows(void* stream, int dtype, int64_t rows, const int32_t* ids, const int32_t* types,
                        const int32_t* pos_ids, const void* word, const void* pos, const void* type, int D,
                        void* out, int64_t ldo);
/* The same sum followed by its LayerNorm in ONE pass (HF BertEmbeddings incl. its LayerNorm, as run by the truncated
 * BertModel at modules/multigraphormer_graph_encoder.py:325-329): xs[r,:] = T(word + type + pos) exactly as mdt_bert_embed_rows
 * leaves it (xs may be NULL: nobody will read the sum), y[r,:] = LayerNorm(xs[r,:]) * gamma + beta, mean / rstd fp32[rows] (may be
 * NULL) — bit-identical to mdt_bert_embed_rows + mdt_layernorm_fwd. */
int mdt_bert_embed_ln_rows(void* stream, int dtype, int64_t rows, const int32_t* ids, const int32_t* types,
                           const int32_t* pos_ids, const void* word, const void* pos, const void* type, int D,
                           const void* gamma, const void* beta, float eps, void* xs, int64_t ldxs, void* y, int64_t ldy,
                           float* mean, float* rstd);

/* ViT patch gather (Conv2d k=s=p is a pure re-index, modules/multigraphormer_graph_encoder.py:333):
 * cols[(i*np + py*gw + px), c*p*p + dy*p + dx] = img[i, c, py*p+dy, px*p+dx]  (img fp32 → T). */
int mdt_vit_patchify(void* stream, int dtype, int I, int C, int HW, int p, const float* img, void* cols, int64_t ldc);
/* tokens[i, off + 0] = cls + pos[0]; tokens[i, off + 1 + j] = patches[i*np + j] + pos[1 + j]. */
int mdt_vit_assemble(void* stream, int dtype, int I, int np, int D, const void* patches, int64_t ldp,
                     const void* cls, const void* pos, void* tokens, int64_t ldt, int64_t seq_stride, int64_t off);
/* The three steps above as ONE launch for bf16 weights and 16 x 16 patches (a GEMM whose A loader gathers from
 * pixel_values; replaces HF ViTEmbeddings as invoked at modules/multigraphormer_graph_encoder.py:332-335):
 * tokens[i, off + 0] = cls + pos[0]; tokens[i, off + 1 + j] = Conv2d(img[i])[:, py, px] + bias + pos[1 + j], j = py*gw + px,
 * w bf16 [D, C*p*p] with row stride ldw (the Conv2d weight viewed flat), one rounding to bf16 at the end.
 * MDT_ERR_UNSUPPORTED for other patch sizes or D not a multiple of 128: the caller takes the three-launch route. */
int mdt_vit_patch_embed(void* stream, int I, int C, int HW, int p, const float* img, const void* w, int64_t ldw,
                        const void* bias, const void* cls, const void* pos, int D, void* tokens, int64_t ldt,
                        int64_t seq_stride, int64_t off);

/* Graph node features (modules/graphormer_layers.py:39-50) on the padded [B, T] grid:
 * x[b,0] = graph_token; x[b,1+n] = (node_row[b,n] >= 0 ? src[node_row[b,n]] : 0)
 *                                  + in_emb[in_degree[b,n]] + out_emb[out_degree[b,n]]. */
int mdt_graph_node_feature(void* stream, int dtype, int B, int T, int D, const void* src, int64_t lds,
                           const int32_t* node_row, const int32_t* in_degree, const int32_t* out_degree,
                           const void* in_emb, const void* out_emb, const void* graph_token, void* x, int64_t ldx);

/* Head tail (models/multi_modal_discussion_transformer.py:265-274): logits[m, c] =
 * 0.5 * (cls(pooled_text[m]) + cls(pooled_bn[m])), pooled = tanh(pre-activation) given. */
int mdt_tanh_fwd(void* stream, int dtype, int64_t n, const void* x, void* y);
int mdt_tanh_bwd(void* stream, int dtype, int64_t n, const void* y, const void* dy, void* dx);

/* Weighted 2-class cross entropy in fp16 arithmetic + counters
 * (criterions/hatespeech_loss.py:95-118, quirk 14): logits T[M,2] gathered by rows[r];
 * out_loss f32[1] (sum), counters i32[4] = ncorrect, num_positive_correct, total_positive,
 * num_pred_positive; dlogits T[M,2] (zero for unlabelled rows) scaled by grad_scale. */
int mdt_node_ce(void* stream, int dtype, int64_t M, int nlab, const void* logits, const int32_t* rows,
                const int32_t* targets, float w_neg, float w_pos, int fp16_loss, float grad_scale,
                float* out_loss, int32_t* counters, void* dlogits);

/* Label-smoothed / focal objective of the same classifier (--label-smoothing, --focal-gamma), csrc/node_objective.hip.
 * Operands as mdt_node_ce; label_smoothing eps in [0, 1), focal_gamma >= 0, both finite.  Per labelled row, y the
 * target and o = 1 - y: nll = -w_y lp_y, f = expf(gamma lp_o) = (1 - p_y)^gamma,
 *   loss = (1 - eps) f nll + (eps / 2) sum_c (-w_c lp_c)
 * (gamma = 0: F.cross_entropy(weight, label_smoothing = eps, reduction "sum"); eps = 0: the focal loss with alpha_t = w_y;
 * the focal factor modulates the hard-target term only and is differentiated).  out f32[2] = sum loss, sum nll;
 * counters as mdt_node_ce (equal integers on the same logits); dlogits T[M,2] = grad_scale * dL/d logits, zero for
 * unlabelled rows (NULL: forward only).  fp16_loss: the logits and the class weights are rounded to fp16 first and the
 * predictions use the half-rounded softmax, as in mdt_node_ce; everything else is fp32.  The sums run in a fixed order: two
 * calls on the same operands give the same bits.  A refused call (MDT_ERR_ARG / MDT_ERR_UNSUPPORTED) writes nothing. */
int mdt_node_objective(void* stream, int dtype, int64_t M, int nlab, const void* logits, const int32_t* rows,
                       const int32_t* targets, float w_neg, float w_pos, int fp16_loss, float label_smoothing,
                       float focal_gamma, float grad_scale, float* out, int32_t* counters, void* dlogits);

/* ------------------------------------------------------------------ fp8 operands (BASELINE.json configs[4])
 * Per-tensor-scaled OCP fp8 for the big k-contiguous GEMMs of the encoder blocks (every nn.Linear forward and, against a
 * transposed weight copy, every input gradient): C[M,N] (bf16) = epilogue((1/scale_a)(1/scale_b) * A[M,K] B[N,K]^T), A in
 * e4m3 (a_format 0: activations) or e5m2 (1: gradients), B in e4m3, fp32 accumulation on v_mfma_f32_16x16x128_f8f6f4 (4-wave
 * kernel, K % 128 == 0, K >= 640) or v_mfma_f32_16x16x32_{fp8,bf8}_fp8 (8-wave kernel, the rest),
 * same epilogues as mdt_gemm (bf16 store forms).  inv_scale_a / inv_scale_b are DEVICE floats (delayed scaling keeps
 * every scale on the device).  Returns MDT_ERR_UNSUPPORTED for shapes the 8-bit kernel is not built for (N % 256, K % 64,
 * K < 256, unaligned rows): the caller then stays in bf16. */
int mdt_gemm_fp8(void* stream, int a_format, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                 int64_t ldb, void* C, int64_t ldc, int epilogue, const float* inv_scale_a, const float* inv_scale_b,
                 const void* bias, const void* residual, int64_t ldr, void* aux, int64_t ldaux, float drop_p,
                 uint64_t drop_seed, float* colsum);
/* mdt_gemm_fp8 whose output ALSO leaves as fp8, for the next 8-bit GEMM to consume without a quantisation pass of its own
 * ("quantise inside the producer": the GELU forward hands fc2 its operand, fc2's input gradient hands fc1's): q8_out u8[M, N]
 * (rows of ld_q8 bytes) = saturate(q8_format, bf16(C) * *q8_scale), *q8_amax = max(*q8_amax, max |bf16(C)|) — bit for bit what
 * mdt_fp8_quantize makes of C.  q8_out NULL: plain mdt_gemm_fp8.  MDT_ERR_UNSUPPORTED when no kernel writes the copy for this
 * epilogue / shape (only the block-MFMA kernel does, for bias + GELU + saved derivative → e4m3 and saved-derivative multiply +
 * column sums → e5m2): the caller then quantises C itself. */
int mdt_gemm_fp8_q8(void* stream, int a_format, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                    int64_t ldb, void* C, int64_t ldc, int epilogue, const float* inv_scale_a, const float* inv_scale_b,
                    const void* bias, const void* residual, int64_t ldr, void* aux, int64_t ldaux, float drop_p,
                    uint64_t drop_seed, float* colsum, void* q8_out, int64_t ld_q8, int q8_format, const float* q8_scale,
                    float* q8_amax);
/* dst u8[rows, cols] = saturate_fp8(src * *scale_dev) (fmt 0: e4m3, |x| <= 448; 1: e5m2, |x| <= 57344; scale_dev NULL: 1);
 * *amax_dev = max(*amax_dev, max |src|) (NULL: not tracked) — the input of the next step's scale. */
int mdt_fp8_quantize(void* stream, int src_dtype, int fmt, int64_t rows, int64_t cols, const void* src, int64_t ld_src,
                     void* dst, int64_t ld_dst, const float* scale_dev, float* amax_dev);
/* Delayed scaling, all sites at once: scale[i] = fmt_max[i] / (amax[i] * margin), inv_scale[i] = 1 / scale[i] for every
 * site whose amax is positive and finite (others keep their scale); amax[i] = 0. */
int mdt_fp8_scale_update(void* stream, int n, float* amax, float* scale, float* inv_scale, const float* fmt_max, float margin);

/* Community-contrastive loss on the global discussion embeddings (criterions/contrastive_loss.py:76-180):
 * emb T[B, D] (row stride ld), y / hard_y f32[B] (community label of every tree and of its polar-opposite community);
 * sim = scale * normalize(emb) normalize(emb)^T, weighted BCE against [y_i == y_j] with the reference's soft-negative
 * weights (adaptive != 0: 2 * #hard / #soft per row, applied along the LAST axis as the reference's broadcast does;
 * otherwise soft_negative_weight), diagonal excluded.  out_loss f32[1] (sum over the B x B pairs), counters i32[4] =
 * ncorrect, positive_correct, total_positive, pred_positive as the reference defines them (:153-161);
 * d_emb T[B, D] = grad_scale * dL/d emb (NULL: forward only).  workspace: mdt_contrastive_loss_workspace_bytes(B, D)
 * bytes owned by the caller. */
size_t mdt_contrastive_loss_workspace_bytes(int B, int D);
int mdt_contrastive_loss(void* stream, int dtype, int B, int D, const void* emb, int64_t ld, const float* y,
                         const float* hard_y, float scale, float soft_negative_weight, int adaptive, void* workspace,
                         float grad_scale, float* out_loss, int32_t* counters, void* d_emb, int64_t ldd);

/* Elementwise cast / transpose helpers for the bf16 weight shadow copies. */
int mdt_cast(void* stream, int src_dtype, int dst_dtype, int64_t n, const void* src, void* dst);
int mdt_transpose2d(void* stream, int src_dtype, int dst_dtype, int64_t rows, int64_t cols,
                    const void* src, int64_t lds, void* dst, int64_t ldd);

/* ------------------------------------------------------------------ optimiser (the step after the path)
 * Fused Adam with FairSeq semantics over one tensor: g = grad * (*grad_scale if given);
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= wd*lr*p; p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v)+eps).
 * `master` (fp32, optional) is the high-precision copy of a bf16 `param`.  grad_scale is a DEVICE scalar
 * (e.g. 1 / global sample size) so no host synchronisation is needed. */
int mdt_adam_step(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                  float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  const float* grad_scale);

/* Multi-tensor form: ONE launch over a device-resident table of same-dtype parameter tensors.  chunk_first[t] = first
 * 4096-element chunk of tensor t, chunk_first[n_tensors] = total_chunks (int64, device). */
typedef struct {
  void* param;          /* T[numel] */
  float* master;        /* fp32 copy or NULL */
  const float* grad;    /* fp32 */
  float* m;
  float* v;
  int64_t numel;
} mdt_adam_tensor;
int mdt_adam_step_multi(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                        const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int step, const float* grad_scale);

/* Global gradient norm, clipping and the non-finite guard (FairSeq --clip-norm, the gnorm meter, its skipped / refused
 * non-finite update), without a host synchronisation.  Three steps on one stream:
 *   1. sum of squares: every 4096-element chunk of every gradient tensor writes ONE fp32 partial, partials[chunk], to a
 *      caller-owned buffer (multi: total_chunks of them, walking the table of the Adam step; single tensor:
 *      (n + 4095) / 4096).  No atomics and a fixed order inside a chunk: the same bits on every call, for any grid.
 *      Views need only 4-byte alignment; 16-byte aligned ones are read 16 bytes at a time.
 *   2. finalize: one block adds the n_partials partials in index order in fp64 and writes the guard state:
 *        gnorm = s_in * sqrt(sum g^2)          s_in = *grad_scale, or 1 when grad_scale is NULL
 *        scale = s_in * min(1, max_norm / (gnorm + 1e-6))      max_norm <= 0: scale = s_in, bit for bit
 *        skip  = gnorm is not finite (Inf / NaN in a gradient, or a sum beyond fp32): this update is skipped
 *      and the running counters: skipped, clipped (gnorm > max_norm > 0, update not skipped), applied = step - skipped.
 *      `step` is the host's count of attempted updates (>= 1), as handed to the Adam step.  Once skipped > 0 step_size
 *      holds (float)(lr * sqrt(1 - beta2^applied) / (1 - beta1^applied)): Adam's bias correction follows the updates
 *      applied.  reset != 0: the counters start from zero at this call — nothing of *guard is read.
 *   3. the guarded Adam steps: as mdt_adam_step / mdt_adam_step_multi with `scale` of the guard state in place of
 *      *grad_scale; a skipped update stores nothing (param, master, m, v keep their bits); the host's step size is used
 *      verbatim while skipped == 0, the guard state's afterwards. */
typedef struct {
  float scale;          /* effective gradient scale of this update */
  float gnorm;          /* norm of the scaled gradient of this update */
  float step_size;      /* bias-corrected step size for `applied` updates; meaningful once skipped > 0 */
  int32_t skip;         /* 1: this update is skipped */
  int32_t applied;      /* running: updates applied */
  int32_t clipped;      /* running: updates clipped */
  int32_t skipped;      /* running: updates skipped */
  int32_t reserved;
} mdt_adam_guard;
int mdt_grad_sumsq_multi(void* stream, int n_tensors, const mdt_adam_tensor* table_dev, const int64_t* chunk_first_dev,
                         int64_t total_chunks, float* partials);
int mdt_grad_sumsq(void* stream, int64_t n, const float* grad, float* partials);
int mdt_grad_norm_finalize(void* stream, const float* partials, int64_t n_partials, float max_norm,
                           const float* grad_scale, float lr, float beta1, float beta2, int step, int reset,
                           mdt_adam_guard* guard);
int mdt_adam_step_guarded(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                          float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                          const mdt_adam_guard* guard);
int mdt_adam_step_multi_guarded(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                                float eps, float weight_decay, int step, const mdt_adam_guard* guard);

/* The weight average (FairSeq --store-ema) riding on the Adam step: the four entry points above with an fp32 average per tensor.
 * After the element's new value p is final — the value stored to `master`, or to `param` where master is NULL — the kernel does
 *        e = ema[i];  e = d * e + (1.0f - d) * p;  ema[i] = e;          d = ema_decay, `1.0f - d` ONE fp32 subtraction in the kernel
 * two fp32 products and one fp32 sum (the build does not contract them; a bound should allow either FMA as well).  ema_decay
 * must lie in [0, 1].  ema_decay == 0 stores p itself: ema == p bit for bit, for every p (FairSeq's "copy until
 * --ema-start-update").  param, master, m and v come out with exactly the bits of the entry point without `_ema` on the same
 * inputs.  A skipped update (guard->skip) stores nothing: the average keeps its bits too.  The averages need 4-byte alignment only.
 * Single tensor: `ema` is float[n], not NULL.  Table form: `ema_dev` is a DEVICE array of n_tensors pointers parallel to the
 * table (mdt_adam_tensor keeps its layout); a NULL entry: that tensor has no average and gets the plain arithmetic. */
int mdt_adam_step_ema(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                      float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                      const float* grad_scale, float* ema, float ema_decay);
int mdt_adam_step_multi_ema(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                            const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                            float eps, float weight_decay, int step, const float* grad_scale, float* const* ema_dev,
                            float ema_decay);
int mdt_adam_step_ema_guarded(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m,
                              float* v, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                              const mdt_adam_guard* guard, float* ema, float ema_decay);
int mdt_adam_step_multi_ema_guarded(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                                    const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int step, const mdt_adam_guard* guard, float* const* ema_dev,
                                    float ema_decay);
/* Evaluate with the averaged weights: ONE launch over the same table and the same ema_dev swaps the average into the working
 * parameters (restore = 0) and the raw weights back (restore = 1).
 *   tensor with a master:   restore = 0: param = T(ema)         restore = 1: param = T(master) — the bits it had, as the Adam
 *                           step keeps param == T(master)
 *   fp32 tensor without:    param[i] and ema[i] trade contents; restore = 1 trades them back (the exchange is its own inverse)
 * master, grad, m and v are never touched (grad, m, v of the table are not even read); a NULL entry of ema_dev leaves the tensor
 * alone, and so does a bf16 tensor without a master (there is nowhere to keep its raw bits).  4-byte alignment suffices;
 * 16-byte aligned tensors move 16 bytes at a time.  No atomics. */
int mdt_ema_swap_multi(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev, float* const* ema_dev,
                       const int64_t* chunk_first_dev, int64_t total_chunks, int restore);

/* Parameter groups: a learning-rate scale and a weight decay PER TENSOR on the same one launch (lower rates for pretrained
 * blocks, layer-wise rate decay, no decay on biases and LayerNorm weights).  One record per table entry, in a DEVICE array
 * parallel to the table and indexed by tensor, as ema_dev is (mdt_adam_tensor keeps its layout).  For the tensor's record g the
 * kernel computes, once per tensor (per 4096-element chunk in the table form), after the guard state has been read:
 *        lr_t        = lr * g.lr_scale                  ONE fp32 product
 *        step_size_t = step_size * g.lr_scale           ONE fp32 product; step_size is the host's
 *                                                       (float)(lr * sqrt(1 - beta2^step) / (1 - beta1^step)), or the guard state's
 *                                                       once an update has been skipped: that one is scaled too
 *        wd_t        = g.weight_decay
 * and every element then takes the update of mdt_adam_step with (lr_t, wd_t, step_size_t) in place of (lr, weight_decay,
 * step_size): p -= (wd_t * lr_t) * p;  p -= step_size_t * m' / (sqrtf(v') + eps).  Consequences:
 *   - lr_scale == 1.0f and weight_decay equal to a global value: the bits of the entry point without groups called with that
 *     weight_decay (x * 1.0f == x), in every output;
 *   - lr_scale == 0: m and v advance, param and master keep their bits for finite values (torch's lr = 0 group): both
 *     subtrahends are +-0;
 *   - the gradient norm, the guard and the average do not know about groups: one norm over all gradients, a skipped update
 *     stores nothing, e = d e + (1 - d) p follows the p this tensor's group produced.
 * The optional parts are nullable: at most one of grad_scale / guard (both: MDT_ERR_ARG), ema_dev / ema NULL: no average
 * (ema_decay is then ignored).  groups_dev NULL is MDT_ERR_ARG: the entry points above are the forms without groups.  The single
 * form takes the record by value, does the same two products in the kernel and so equals the table form bit for bit; it refuses
 * a non-finite or negative lr_scale or weight_decay (the table's records live on the device and are the caller's to validate).
 * Nothing but the tensors' own param, master, m, v and ema is written; no atomics. */
typedef struct {
  float lr_scale;
  float weight_decay;
} mdt_adam_group;
int mdt_adam_step_multi_groups(void* stream, int dtype, int n_tensors, const mdt_adam_tensor* table_dev,
                               const int64_t* chunk_first_dev, int64_t total_chunks, float lr, float beta1, float beta2,
                               float eps, int step, const mdt_adam_group* groups_dev, const float* grad_scale,
                               const mdt_adam_guard* guard, float* const* ema_dev, float ema_decay);
int mdt_adam_step_group(void* stream, int dtype, int64_t n, void* param, float* master, const float* grad, float* m, float* v,
                        float lr, float beta1, float beta2, float eps, int step, float lr_scale, float weight_decay,
                        const float* grad_scale, const mdt_adam_guard* guard, float* ema, float ema_decay);

/* ------------------------------------------------------------------ ordered (bit-reproducible) gradient reductions
 * The backward pass accumulates gradients with fp32 atomics (MDT_EPI_ATOMIC / _ASUM / _COLSUM, mdt_colsum, mdt_layernorm_bwd,
 * mdt_row_scatter_add_f32, the structural-bias gradient of mdt_attention_bwd): two runs of one step agree to ~1e-7, not bit for
 * bit.  The entry points below compute the same gradients with plain stores of per-workgroup partials into a CALLER-OWNED
 * workspace and one fixed-order reducer, so their results are functions of the operands alone (and of the library build) — not
 * of timing, of which workgroup ran first, or of other work on the device.  They are NOT bit-equal to the atomic forms (another
 * summation order).  Each ..._workspace_bytes() is what the call with the same arguments needs; a smaller (or NULL) workspace is
 * MDT_ERR_INVALID before anything is launched.  Workspaces must be 16-byte aligned and need no initialisation.
 *
 * mdt_sum_slices_f32 — THE reducer: out[r][c] = (accumulate ? out[r][c] : 0) + (((ws[0][r][c] + ws[1][r][c]) + ws[2][r][c]) + ...)
 *   with ws[z][r][c] = ws[z * slice_stride + r * ld_ws + c]: the slices are added left to right in fp32, one rounding per add (there
 *   is no multiply, hence no FMA), the old value of out joins last.  Any row strides >= cols. */
int mdt_sum_slices_f32(void* stream, int64_t rows, int64_t cols, int slices, const float* ws, int64_t ld_ws, int64_t slice_stride,
                       float* out, int64_t ldo, int accumulate);
/* The weight-gradient GEMM: C[M,N] (fp32, row stride ldc) += alpha * op(A) @ op(B), operands as mdt_gemm.  One launch computes
 * the K slabs (grid z = slab); slab z stores alpha * its fp32 partial tile to slice z of the workspace ([slabs][M][N]) and
 * mdt_sum_slices_f32 adds the slices into C in ascending z.  The 4-wave weight-gradient kernel ("w4s") runs under the preconditions
 * it has in mdt_gemm, the 128 x 128 tile kernel ("tile128") takes the other tile-aligned bf16 launches and the any-shape kernel
 * ("generic") the rest, fp32 operands included (mdt_last_route()).  The slab count the planner chooses (<= split_k) stays inside;
 * the result depends on it, so it is reproducible for one (shape, strides, alignment, split_k).  No bias sum rides here. */
size_t mdt_gemm_splitk_ordered_workspace_bytes(int64_t M, int64_t N, int split_k);
int mdt_gemm_splitk_ordered(void* stream, int dtype, int trans_a, int trans_b, int64_t M, int64_t N, int64_t K,
                            const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, float alpha,
                            int split_k, void* workspace, size_t workspace_bytes);
/* mdt_colsum in a fixed order: out[n] += sum_m w[m] * X[m, n].  Rows are cut into blocks of 256; inside a block, row lane j of 4
 * adds the terms of rows j, j + 4, ... in ascending order (each product w * x rounded first) and the block's partial is
 * ((lane 0 + lane 1) + lane 2) + lane 3; mdt_sum_slices_f32 then adds the blocks in ascending order, the old out last. */
size_t mdt_colsum_ordered_workspace_bytes(int64_t M, int64_t N);
int mdt_colsum_ordered(void* stream, int dtype, int64_t M, int64_t N, const void* X, int64_t ldx, float* out,
                       const int32_t* row_weight, void* workspace, size_t workspace_bytes);
/* mdt_layernorm_bwd with the per-workgroup partials of dgamma, dbeta and the column sums stored to the workspace and added by
 * mdt_sum_slices_f32 in ascending workgroup order (the old dgamma / dbeta / colsum joins last).  dx and dxd are bit-identical to
 * mdt_layernorm_bwd's; the number of workgroups is a function of `rows` alone (MDT_LN_BWD_WGS is not read).  Runs the generic
 * kernel ("ln_generic") for every D. */
size_t mdt_layernorm_bwd_ordered_workspace_bytes(int64_t rows, int D);
int mdt_layernorm_bwd_ordered(void* stream, int dtype, int64_t rows, int D, const void* dy, int64_t lddy,
                              const void* x, int64_t ldx, const void* gamma, const float* mean, const float* rstd,
                              const void* add, int64_t ldadd, void* dx, int64_t lddx, float* dgamma, float* dbeta,
                              void* dxd, int64_t lddxd, float drop_p, uint64_t drop_seed, float* colsum,
                              void* workspace, size_t workspace_bytes);
/* The scatter-add of mdt_row_scatter_add_f32 in a fixed order, from segments in CSR form: segment s adds the source rows
 * order[seg_off[s]] .. order[seg_off[s + 1] - 1] (source row r is src row r * s_stride + s_off, T = bf16 or fp32, converted to fp32)
 * to table row seg_row[s] (seg_row < 0: skipped; every other seg_row at most once).  TWO-LEVEL ORDER: the segment's sources are
 * taken in chunks of 64 in the order listed; a chunk is summed left to right, the chunk sums are added left to right, and the
 * table's old value joins last:  table[seg_row[s]] = table[seg_row[s]] + ((chunk 0 + chunk 1) + chunk 2 ...).  An empty segment
 * leaves its row untouched.  The CSR is the caller's (a stable sort of the index vector): the result is the same for any
 * construction that lists a segment's sources in ascending source-row order.  No workspace: one thread owns one table element. */
int mdt_row_segment_sum_f32(void* stream, int dtype, int nseg, int D, float* table, int64_t ldt, const int32_t* seg_row,
                            const int32_t* seg_off, const int32_t* order, const void* src, int64_t lds, int64_t s_stride,
                            int64_t s_off);
/* Structural-bias gradient from a dense dS f32[nseq,H,S,S] (what mdt_attention_bwd stores through d_dense_bias, launched with
 * d_sp_table = d_virt = NULL): d_sp_table[i][h] += sum of dS[s,h,q,key] over q >= 1, key >= 1 with spatial_pos[s,q-1,key-1] == i
 * (row 0, the padding index, receives nothing); d_virt[h] += sum over q == 0 or key == 0.  One workgroup of T threads per
 * (sequence, head): thread t adds elements t, t + T, ... of the row-major S x S matrix in that order into a private histogram;
 * the T histograms are folded by halving (t += t + T / 2, then + T / 4, ... + 1); mdt_sum_slices_f32 then adds the sequences in
 * ascending order, the old value last.  T is a function of num_spatial alone — 256 up to 95 table rows, 128 up to 191, 64 up to
 * 383, 32 up to 767 — so that the (num_spatial + 1) x T floats of histogram stay within 96 KiB of the 160 KiB of LDS a workgroup
 * has; MDT_ERR_UNSUPPORTED for more rows.  Either output may be NULL. */
size_t mdt_attn_bias_grad_ordered_workspace_bytes(int nseq, int H, int num_spatial);
int mdt_attn_bias_grad_ordered(void* stream, int nseq, int S, int H, int num_spatial, const float* dS,
                               const int32_t* spatial_pos, float* d_sp_table, float* d_virt, void* workspace,
                               size_t workspace_bytes);
/* Host-side count of the launches that accumulate with float atomics into caller memory (every site named above adds one per
 * call); reset != 0 also puts it back to zero.  Nothing inside a kernel is inspected: a step that ran in ordered mode leaves it
 * unchanged. */
int64_t mdt_float_atomic_launches(int reset);

/* ------------------------------------------------------------------ low-rank adapters (LoRA) on the fused QKV projection
 * The three skinny products of an adapter pair A_j [r, D], B_j^T [r, D] beside a frozen weight: one dimension n (the rank, or
 * |targets| * rank) of 8 ... 192 against ~10^5 token rows.  They replace the PEFT-style eager sequence around an adapted nn.Linear,
 *     t = x @ A.T;  y = base(x) + scale * (t @ B.T);   autograd: dB = t.T @ dy, dt = dy @ B, dA = dt.T @ x, dx += dt @ A
 * (the reference fine-tunes every weight and has no counterpart).  Both parameters are stored [n, D], so W below is always a
 * row-major [n, wide] matrix.  All three are memory-bound: the [R, wide] operand is read once (up_add: read and written once),
 * the small operand stays in registers / LDS / L2, nothing is staged through global memory or transposed in it.
 *   dtype MDT_BF16 (v_mfma_f32_16x16x32_bf16, fp32 accumulators) or MDT_F32 (plain fp32 loops: the parity path);
 *   n a multiple of 8 with 8 <= n <= 192; K / N a positive multiple of 16; bf16 bases and rows on 16-byte boundaries (row strides
 *   multiples of 8 elements), fp32 ones on 4-byte boundaries; a row stride may exceed the width (column slices of the [R, 3D]
 *   qkv / dqkv buffers: ld = 3D) and only columns below the width are read or written; R = 0 is a no-op.  Anything else is
 *   MDT_ERR_ARG with the numbers in the message, before any launch.  One rounding to the stored type per element;
 *   mdt_last_route(): "lora_down", "lora_up", "lora_wgrad" (bf16), "lora_down_f32", "lora_up_f32", "lora_wgrad_f32".
 *
 * mdt_lora_down    T[R, n] = alpha * X[R, K] W[n, K]^T        (t = src A^T;  dt_j = s dqkv[:, c_j : c_j + D] Bt_j^T)
 * mdt_lora_up_add  Y[R, N] += alpha * T[R, n] W[n, N]         (qkv[:, c_j : c_j + D] += s t_j Bt_j;  dx += dt A): Y is read in its type,
 *                  the fp32 product joins by one FMA, the sum is rounded once
 * mdt_lora_wgrad   dW[n, N] (fp32) += alpha * T[R, n]^T X[R, N]   (dBt_j, dA) in a FIXED order and without float atomics: token rows
 *                  are cut into slabs of mdt_lora_wgrad_slab_rows() rows; the workgroup of (slab, column tile) stores alpha * its fp32
 *                  partial [n, tile] to slice `slab` of the workspace ([slabs][n][N]) and mdt_sum_slices_f32 adds the slices in
 *                  ascending order, the old dW last.  Inside a slab the rows are accumulated in ascending 32-row MFMA steps
 *                  (fp32: one row at a time).  The result is a function of the operands and R alone — the same call in the
 *                  default and in the deterministic mode.  Workspace: caller-owned, 16-byte aligned, uninitialised;
 *                  a smaller one is MDT_ERR_INVALID before anything is launched. */
int mdt_lora_down(void* stream, int dtype, int64_t R, int n, int K, const void* X, int64_t ldx,
                  const void* W, int64_t ldw, void* T, int64_t ldt, float alpha);
int mdt_lora_up_add(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt,
                    const void* W, int64_t ldw, void* Y, int64_t ldy, float alpha);
/* Epilogue forms of mdt_lora_up_add, for the adapters of the dense layers whose GEMM has a fused epilogue (the attention output
 * projection, fc1, fc2): the same kernel, the same contract (lora_check), p = (T W)[r, c] in its fp32 accumulator, a lane owning
 * 16 consecutive columns of one token; fp32 arithmetic, ONE rounding per stored element.
 *   mdt_last_route(): "lora_up_drop", "lora_up_mul", "lora_up_act" (bf16), the same with "_f32" (fp32).
 * mdt_lora_up_add_drop  Y[r, c] = Y[r, c] + (alpha s(r, c)) p,  s = keep(drop_seed, r N + c) / (1 - drop_p): the counters of
 *                  MDT_EPI_DROPOUT and mdt_dropout, so the adapter sum enters res + dropout(x W^T + b) UNDER that GEMM's mask.
 *                  An element whose counter is dropped keeps its bits; drop_p = 0 is mdt_lora_up_add bit for bit.
 *                  0 <= drop_p < 1 and R N < 2^33, else MDT_ERR_ARG.
 * mdt_lora_up_add_mul   Y[r, c] = Y[r, c] + (alpha p) aux[r, c], aux [R, N] of Y's type: the adapter's share of the FFN's du behind
 *                  MDT_EPI_MULAUX (aux = u, the saved activation derivative).
 * mdt_lora_up_act       v = pre[r, c] + alpha p (fp32, not rounded);  h = act(v) s,  u = act'(v) s: kinds, formulas and dropout
 *                  counters of mdt_act_fwd (one device function serves both), so with T = 0 the two agree bit for bit.
 *                  h may be pre; u may be NULL (a forward without a tape). */
int mdt_lora_up_add_drop(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt,
                         const void* W, int64_t ldw, void* Y, int64_t ldy, float alpha, float drop_p, uint64_t drop_seed);
int mdt_lora_up_add_mul(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt,
                        const void* W, int64_t ldw, void* Y, int64_t ldy, const void* aux, int64_t ld_aux, float alpha);
int mdt_lora_up_act(void* stream, int dtype, int kind, int64_t R, int n, int N, const void* T, int64_t ldt,
                    const void* W, int64_t ldw, const void* pre, int64_t ld_pre, void* h, int64_t ld_h,
                    void* u, int64_t ld_u, float alpha, float drop_p, uint64_t drop_seed);
int mdt_lora_wgrad_slab_rows(void);
size_t mdt_lora_wgrad_workspace_bytes(int64_t R, int n, int N);
int mdt_lora_wgrad(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt,
                   const void* X, int64_t ldx, float* dW, int64_t lddw, float alpha,
                   void* workspace, size_t workspace_bytes);
/* Adapter-input dropout (PEFT's lora_dropout: y = base(x) + s B A dropout(x)): the forms of the entry points above whose [R, wide]
 * operand X is dropped on its way into the product.  The keep decision of X[r, c] is that of counter r W + c of site drop_seed
 * (mdt_dropout / mdt_dropout_mask over R W elements), r the row of X AS PASSED (of a view: the row of the view) and W its logical
 * width K or N, never its row stride.  A dropped element is replaced by +0 by a select before it enters the MFMA fragment (down)
 * or the LDS image (wgrad): kept elements stay exact, nothing is rounded to x / (1 - p), a non-finite value at a dropped position
 * does not reach the result, and no dropped copy of X is written anywhere.  1 / (1 - drop_p) (fp32, make_drop's) joins alpha as
 * ONE fp32 factor fl(alpha / (1 - p)), applied where alpha is applied.  Contract of the plain forms plus 0 <= drop_p < 1 and
 * R W < 2^33 (MDT_ERR_ARG); drop_p = 0 is the plain entry point bit for bit.
 *   mdt_last_route(): "lora_down_drop", "lora_wgrad_drop", "lora_up_mul_drop" (bf16), the same with "_f32" (fp32).
 * mdt_lora_down_drop        T[R, n] = fl(alpha / (1 - p)) * (m o X)[R, K] W[n, K]^T, counters r K + k
 * mdt_lora_wgrad_drop       dW[n, N] += fl(alpha / (1 - p)) * T[R, n]^T (m o X)[R, N], counters r N + c: slabs, order, workspace and
 *                           the absence of float atomics as in mdt_lora_wgrad
 * mdt_lora_up_add_mul_drop  Y[r, c] = Y[r, c] + (alpha s(r, c) p) aux[r, c], s as in mdt_lora_up_add_drop: the share of fc2's du of
 *                           an adapter whose input h was dropped.  An element whose counter is dropped keeps its bits.
 * The adapter's share of every other input gradient, dx += s o (dt A), is mdt_lora_up_add_drop with N = K and the site's seed. */
int mdt_lora_down_drop(void* stream, int dtype, int64_t R, int n, int K, const void* X, int64_t ldx,
                       const void* W, int64_t ldw, void* T, int64_t ldt, float alpha, float drop_p, uint64_t drop_seed);
int mdt_lora_wgrad_drop(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt,
                        const void* X, int64_t ldx, float* dW, int64_t lddw, float alpha, float drop_p, uint64_t drop_seed,
                        void* workspace, size_t workspace_bytes);
int mdt_lora_up_add_mul_drop(void* stream, int dtype, int64_t R, int n, int N, const void* T, int64_t ldt,
                             const void* W, int64_t ldw, void* Y, int64_t ldy, const void* aux, int64_t ld_aux,
                             float alpha, float drop_p, uint64_t drop_seed);

/* ------------------------------------------------------------------ packer (host, C++)
 * Native replacement of preprocess_item + collator (data/pyg_datasets/pre_processing.py:18-69,
 * data/collator.py:69-179): integer tensors are bit-exact with the reference.
 * All outputs are caller-allocated (pinned) host buffers sized for B x nmax.
 */
int mdt_pack_structure(int B, const int64_t* n_nodes, const int64_t* const* parents, int nmax,
                       int spatial_pos_max, float* attn_bias /*[B,nmax+1,nmax+1]*/,
                       int32_t* spatial_pos /*[B,nmax,nmax]*/, int64_t* in_degree /*[B,nmax]*/);
/* Same, with the (hops up, hops down) pairs of a tree given explicitly: updown[b] = i64[n_b, n_b, 2] or NULL (derive
 * them from parents[b]).  The reference stores this matrix per graph (``distance_matrix``,
 * experiments/hateful_discussions/datasets/hateful_discussions.py:148-165) and feeds it to preprocess_item; for a
 * well-formed tree it is a function of the parent array, for discussions with repeated comment ids it is not. */
int mdt_pack_structure_ud(int B, const int64_t* n_nodes, const int64_t* const* parents, const int64_t* const* updown,
                          int nmax, int spatial_pos_max, float* attn_bias, int32_t* spatial_pos, int64_t* in_degree);

/* ------------------------------------------------------------------ image front end
 * Replaces the ViTImageProcessor call of the reference's dataset builder
 * (mDT/experiments/hateful_discussions/datasets/hateful_discussions.py:47-49,168-184): PIL bilinear (antialiased) resize to
 * out_size x out_size, x * rescale (double, rounded once to float), (x - mean) / std (float) — for a batch of decoded RGB images
 * of different sizes, on the device, byte-exact against PIL's resampler.
 *   mdt_resize_plan_ksize / mdt_resize_plan (HOST): the taps of one axis — bounds[2 * out_size] = (first source sample,
 *     tap count) per output sample, coeffs[out_size * ksize] 22-bit fixed-point weights (Pillow Resample.c precompute_coeffs +
 *     normalize_coeffs_8bpc restated).
 *   mdt_image_norm_lut (HOST): lut[3 * 256] = ((float)(u * rescale) - mean[c]) / std[c].
 *   mdt_image_preprocess (DEVICE pointers): pixels = the images' HWC uint8 bytes back to back; desc[n][8] (int64) =
 *     {pixel byte offset, tmp byte offset, H, W, horizontal plan offset, horizontal ksize, vertical plan offset, vertical ksize};
 *     plan (int32) = at each plan offset the bounds followed by the coeffs of that axis; tmp = scratch of sum_i H_i * out_size * 3
 *     bytes; out = [n, 3, out_size, out_size] in out_dtype (may be NULL), out_u8 = [n, out_size, out_size, 3] resized bytes (may
 *     be NULL); max_h = the largest H. */
int mdt_resize_plan_ksize(int in_size, int out_size);
int mdt_resize_plan(int in_size, int out_size, int32_t* bounds, int32_t* coeffs, int ksize);
int mdt_image_norm_lut(double rescale, const float* mean3, const float* std3, float* lut);
int mdt_image_preprocess(void* stream, int n_images, int max_h, const uint8_t* pixels, const int64_t* desc, const int32_t* plan,
                         uint8_t* tmp, const float* lut, int out_dtype, void* out, uint8_t* out_u8, int out_size);

#ifdef __cplusplus
}
#endif
#endif /* MDT_HIP_H */
