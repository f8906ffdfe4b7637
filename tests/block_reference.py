"""fp64 restatement of engine.transformer_block and engine.attention_layer, pure torch autograd: no device, no native library.

The block is oracle.mdt_ref_cpu.bert_layer / graph_layer (post-LN) and vit_layer / graph_layer(pre_ln=True) (pre-LN) written
once over ROWS — the [rows, D] storage the engine works on, whatever the launch geometry (batch-major, time-major, ragged) —
with what the oracle leaves out because its parity runs switch it off:

  * the four dropout sites.  Masks are regenerated on the CPU from the site seeds by the ports of the counter hash:
    attention probabilities with attention_reference.drop_scale (counter ((s H + h) S + q) S2 + key), the two dense outputs
    and the activation with gemm_reference.drop_scale (counter row N + col of the GEMM that applies it: with ``keep_rows`` the
    row is the index INTO keep_rows);
  * ``keep_rows`` as indexing: the output projection, both LayerNorms and the FFN see x[keep_rows] / ctx[keep_rows] only;
  * every mask or bias source of AttnSpec: key_mask (0 = dead key), key_pad (1 = dead key), a dense bias, the structural bias
    2 attn_bias + table[spatial_pos] / virt (attention_reference.struct_bias: Graphormer adds attn_bias twice), ragged lengths;
  * the activation kinds of activation_reference.

Everything is computed from the STORED operands (bf16 or fp32 values, widened exactly), so the only difference to the device
result is the device's arithmetic.  ``reference()`` returns y, dx, the twelve parameter gradients and the bias-source
gradients, plus for the key bias the norm of what is summed (its gradient cancels to zero: see ``summed``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import tests.activation_reference as ACT
import tests.attention_reference as AR
import tests.gemm_reference as GR

PARAMS = ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_w", "ln1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ln2_w", "ln2_b")
NEG = float("-inf")


# ------------------------------------------------------------------------------------------------ launch geometry
def row_map(nseq, S, seq_stride=None, pos_stride=1, seq_offsets=None):
    """(m i64[nseq, S], lens): the storage row of token ``pos`` of sequence ``s`` (-1: a ragged sequence has no such token) and
    the lengths of a ragged launch (None otherwise).  seq_stride None: S rows per sequence."""
    ar = torch.arange(S)
    if seq_offsets is not None:
        off = seq_offsets.long()
        lens = off[1:] - off[:-1]
        assert int(lens.max()) <= S and int(lens.min()) >= 1
        m = off[:-1, None] + ar[None]
        return torch.where(ar[None] < lens[:, None], m, torch.full_like(m, -1)), lens
    ss = S if seq_stride is None else int(seq_stride)
    return torch.arange(nseq)[:, None] * ss + ar[None] * int(pos_stride), None


def to_logical(t, m):
    """rows [R, W] -> [nseq, S, W] (zeros where the token does not exist)"""
    return t[m.clamp(min=0)] * (m >= 0)[..., None].to(t.dtype)


def from_logical(L, m, rows):
    """[nseq, S, W] -> rows [R, W] (rows no token maps to stay zero)"""
    have = m >= 0
    return torch.zeros(rows, L.shape[-1], dtype=L.dtype).index_put((m[have],), L[have])


def spec_geometry(spec):
    return row_map(spec["nseq"], spec["S"], spec.get("seq_stride"), spec.get("pos_stride", 1), spec.get("seq_offsets"))


# ------------------------------------------------------------------------------------------------ attention
def attention64(qkv, spec, W, p_attn, seed):
    """ctx rows [R, D] of fp64 qkv rows [R, 3 D].  ``spec``: host values of AttnSpec's fields; ``W``: fp64 leaves, of which
    sp_table / virt / dense_bias are read when the spec names that source."""
    nseq, S, H = spec["nseq"], spec["S"], spec["H"]
    m, lens = spec_geometry(spec)
    D = qkv.shape[1] // 3
    hd = D // H
    q, k, v = (to_logical(qkv[:, i * D:(i + 1) * D], m).view(nseq, S, H, hd).transpose(1, 2) for i in range(3))
    scale = spec.get("scale") or hd ** -0.5
    s = scale * (q @ k.transpose(-1, -2))
    dead = torch.zeros(nseq, 1, 1, S, dtype=torch.bool)
    if lens is not None:
        dead = dead | (torch.arange(S)[None] >= lens[:, None])[:, None, None, :]
    if spec.get("key_mask") is not None:
        dead = dead | (spec["key_mask"] == 0)[:, None, None, :]
    if spec.get("key_pad") is not None:
        dead = dead | (spec["key_pad"] != 0)[:, None, None, :]
    bias = torch.zeros(nseq, H, S, S, dtype=torch.float64)
    if spec.get("dense_bias") is not None:
        bias = bias + W["dense_bias"]
    if spec.get("attn_bias") is not None:
        bias = bias + AR.struct_bias(spec["attn_bias"], spec["spatial_pos"], W["sp_table"], W["virt"].view(-1))[0]
    dead = dead | (bias.detach() == NEG)
    s = torch.where(dead, torch.full_like(s, NEG), s + torch.where(dead, torch.zeros_like(bias), bias))
    assert bool(torch.isfinite(s.detach().max(-1).values).all()), "block reference: a query row without a live key"
    P = torch.softmax(s, -1)
    ctx = (P * AR.drop_scale(nseq, H, S, p_attn, seed)) @ v
    return from_logical(ctx.transpose(1, 2).reshape(nseq, S, D), m, qkv.shape[0])


def hidden_drop(v, p, seed):
    return v if not p else v * GR.drop_scale(v.shape[0], v.shape[1], p, seed)


# ------------------------------------------------------------------------------------------------ the block
def block64(x, W, cfg, seeds, kept=None):
    """The block's output rows in fp64.  ``cfg``: pre_ln, eps, p_hidden, p_attn, p_act, act, keep_rows (i64 or None), spec.
    ``seeds``: (s_attn, s_o, s_act, s_f2).  ``kept``: a dict that receives the qkv tensor (its gradient is read afterwards)."""
    s_attn, s_o, s_act, s_f2 = seeds
    D = x.shape[1]
    pre_ln, keep = cfg["pre_ln"], cfg.get("keep_rows")

    def ln(t, n):
        return F.layer_norm(t, (D,), W[n + "_w"], W[n + "_b"], cfg["eps"])

    a_in = ln(x, "ln1") if pre_ln else x
    qkv = F.linear(a_in, W["qkv_w"], W["qkv_b"])
    if kept is not None:
        qkv.retain_grad()
        kept["qkv"] = qkv
    ctx = attention64(qkv, cfg["spec"], W, cfg["p_attn"], s_attn)
    ctx_k, x_k = (ctx, x) if keep is None else (ctx[keep.long()], x[keep.long()])
    t = x_k + hidden_drop(F.linear(ctx_k, W["o_w"], W["o_b"]), cfg["p_hidden"], s_o)
    f_in = ln(t, "ln2" if pre_ln else "ln1")
    pre = F.linear(f_in, W["fc1_w"], W["fc1_b"])
    h = ACT.act(cfg["act"], pre) * ACT.drop_scale(pre.shape[0], pre.shape[1], cfg["p_act"], s_act)
    y = (t if pre_ln else f_in) + hidden_drop(F.linear(h, W["fc2_w"], W["fc2_b"]), cfg["p_hidden"], s_f2)
    return y if pre_ln else ln(y, "ln2")


def _leaves(tensors):
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in tensors.items() if v is not None}


def _finish(out, cot, x, W, kept, D):
    (out * cot.double()).sum().backward()
    grads = {k: (torch.zeros_like(w) if w.grad is None else w.grad) for k, w in W.items()}
    if "sp_table" in grads:
        grads["sp_table"] = grads["sp_table"].clone()
        grads["sp_table"][0] = 0.0                      # nn.Embedding(padding_idx=0): row 0 is read, never trained
    dk = kept["qkv"].grad[:, D:2 * D]
    return dict(y=out.detach(), dx=x.grad, grads=grads, summed={"qkv_b.k": float(dk.abs().sum(0).norm())})


def reference(x, params, cot, cfg, seeds):
    """→ dict(y, dx, grads {name: fp64}, summed).  ``params``: the twelve stored parameters by name plus, where the spec has
    them, sp_table / virt / dense_bias.  ``summed["qkv_b.k"]``: ‖Σ_rows |dK|‖ — the key bias gradient is the column sum of dK,
    which cancels to zero (a key bias shifts every score of a row alike), so its error is measured against what is summed."""
    W = _leaves(params)
    xr = x.detach().double().clone().requires_grad_(True)
    kept = {}
    return _finish(block64(xr, W, cfg, seeds, kept), cot, xr, W, kept, x.shape[1])


def attention_layer_reference(x, params, cot, spec, p_attn, seed):
    """engine.attention_layer: the attention half without residual, LayerNorm or hidden dropout; qkv_b / o_b may be absent."""
    W = _leaves(params)
    xr = x.detach().double().clone().requires_grad_(True)
    qkv = F.linear(xr, W["qkv_w"], W.get("qkv_b"))
    qkv.retain_grad()
    out = F.linear(attention64(qkv, spec, W, p_attn, seed), W["o_w"], W.get("o_b"))
    return _finish(out, cot, xr, W, {"qkv": qkv}, x.shape[1])


def rel_l2(got, ref, floor=0.0):
    """‖got - ref‖ / max(‖ref‖, floor)"""
    return float((got.double() - ref).norm()) / max(float(ref.norm()), floor, 1e-300)
