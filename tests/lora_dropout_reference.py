"""fp64 references and per-element error bounds for adapter-input dropout (include/mdt_hip.h "Adapter-input dropout":
mdt_lora_down_drop, mdt_lora_wgrad_drop, mdt_lora_up_add_mul_drop) and the fp64 autograd restatement of a block whose six
adapter sites read dropout(x).  Pure torch: no device, no native library.  Builds on tests/lora_reference.py and
tests/lora_dense_reference.py (every function returns (value, δ)) and on tests/block_reference.py.

The mask is gemm_reference.drop_scale's: counter r W + c of the operand as passed, W its logical width.  A dropped element of X
is replaced by +0 by a select (a non-finite value there does not reach the result) and 1 / (1 - p) joins alpha as ONE fp32 factor
fl32(alpha) * fl32(inv_keep), rounded to fp32 — so the masked down / wgrad are lora_reference.down / wgrad on (m ∘ X) with that
factor, and their error model carries over unchanged: the kept operands are exact bf16 / fp32 values.  With integer operands,
p = 0.5 (inv_keep 2) and a power-of-two alpha the factor is a power of two and δ = 0.

up_add_mul_drop   Y + fl(fl(alpha s) p̂) aux: the products alpha s and (alpha s) p̂ are rounded (2 u |alpha s p aux|), then the FMA
                  with Y rounds once.  A dropped element (s = 0) is not written: exact, the old bits.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import tests.activation_reference as ACT
import tests.block_reference as BR
import tests.gemm_reference as GR
import tests.lora_reference as LR
from tests.lora_reference import F24, U32, _gamma, _integral, _pow2

SITES = ("qkv", "out", "fc1", "fc2")


def factor(alpha: float, p: float) -> float:
    """fl32(alpha) * fl32(1 / (1 - p)) rounded to fp32: the one factor the masked kernels apply where alpha is applied."""
    return float(np.float32(alpha) * np.float32(GR.drop_params(p)[1]))


def masked(x: torch.Tensor, p: float, seed: int, counter_ld=None, apply_mask=True) -> torch.Tensor:
    """fp64 m ∘ X: +0 where counter r W + c of site ``seed`` is dropped (a select: NaN / Inf there do not survive).
    ``counter_ld`` replaces W and ``apply_mask=False`` keeps everything: the two mutants of the kernel tests."""
    X = x.double()
    if not apply_mask:
        return X
    keep = GR.drop_scale(X.shape[0], X.shape[1], p, seed, counter_ld=counter_ld) != 0
    return torch.where(keep, X, torch.zeros_like(X))


def down_drop(x, w, alpha, p, seed, counter_ld=None, apply_mask=True):
    """mdt_lora_down_drop: T[R, n] = fl32(alpha inv_keep) (m ∘ X) W^T."""
    return LR.down(masked(x, p, seed, counter_ld, apply_mask), w, factor(alpha, p))


def wgrad_drop(t, x, dw_old, alpha, p, seed, slab=1024, counter_ld=None, apply_mask=True):
    """mdt_lora_wgrad_drop: dW[n, N] = dW_old + fl32(alpha inv_keep) T^T (m ∘ X), the slabs of lora_reference.wgrad."""
    return LR.wgrad(t, masked(x, p, seed, counter_ld, apply_mask), dw_old, factor(alpha, p), slab)


def up_add_mul_drop(t, w, y_old, aux, alpha, scale):
    """mdt_lora_up_add_mul_drop: Y = Y_old + (alpha s (T W)) aux where s != 0, Y_old (its bits) where s = 0.  ``scale``: fp64
    [R, N] (lora_dense_reference.scale_of)."""
    T, W = t.double(), w.double()
    acc, S, n = T @ W, T.abs() @ W.abs(), T.shape[1]
    Y, A = y_old.double(), aux.double()
    al = float(np.float32(alpha))
    keep = scale != 0
    v = torch.where(keep, Y + al * scale * acc * A, Y)
    smax = float(scale.max()) if scale.numel() else 1.0
    exact = (_integral(T) and _integral(W) and _integral(Y) and _integral(A) and _pow2(al) and _pow2(smax if smax else 1.0)
             and float((abs(al) * scale * S * A.abs() + Y.abs()).max()) / min(abs(al), 1.0) < F24)
    if exact:
        return v, torch.zeros_like(v)
    d = _gamma(n) * abs(al) * scale * S * A.abs() + 2.0 * U32 * (al * scale * acc * A).abs()
    d = d + U32 * (v.abs() + d)
    return v, torch.where(keep, d, torch.zeros_like(d))


# ------------------------------------------------------------------------------------------------ the block
def site_names(lora: dict):
    """The adapter sites present, in the order their seeds are drawn: qkv (ONE site for the fused q / k / v adapters), out, fc1, fc2."""
    return [s for s in SITES if s + "_A" in lora]


def block64_lora(x, W, cfg, seeds, kept=None):
    """block_reference.block64 restated with the adapter sites and their input dropout.  ``W`` additionally holds the adapter leaves
    present: qkv_A / qkv_Bt [|J| r, D] (target-major), out_A / out_Bt [r, D], fc1_A [r, D] / fc1_Bt [r, F], fc2_A [r, F] /
    fc2_Bt [r, D].  ``cfg`` additionally: lora_scale, lora_cols (thirds of qkv the fused adapters add to), p_lora.
    ``seeds``: the block's four, then one per site present (site_names order) when p_lora > 0."""
    s_attn, s_o, s_act, s_f2 = seeds[:4]
    D = x.shape[1]
    pre_ln, keep = cfg["pre_ln"], cfg.get("keep_rows")
    p, sc = cfg.get("p_lora", 0.0), cfg.get("lora_scale", 1.0)
    present = [s for s in SITES if s + "_A" in W]
    ls = dict(zip(present, seeds[4:])) if p > 0 else {}

    def ln(t, n):
        return F.layer_norm(t, (D,), W[n + "_w"], W[n + "_b"], cfg["eps"])

    def adapter(site, src):
        """scale (dropout_p(src) A^T) Bt of a dense site, or 0"""
        if site not in present:
            return 0.0
        xd = src * GR.drop_scale(src.shape[0], src.shape[1], p, ls[site]) if p > 0 else src
        return sc * ((xd @ W[site + "_A"].t()) @ W[site + "_Bt"])

    a_in = ln(x, "ln1") if pre_ln else x
    qkv = F.linear(a_in, W["qkv_w"], W["qkv_b"])
    if "qkv" in present:
        cols = cfg["lora_cols"]
        r = W["qkv_A"].shape[0] // len(cols)
        xd = a_in * GR.drop_scale(a_in.shape[0], D, p, ls["qkv"]) if p > 0 else a_in        # one dropped source for q, k and v
        t = xd @ W["qkv_A"].t()
        parts = []
        for c in range(3):
            if c in cols:
                j = cols.index(c)
                parts.append(sc * (t[:, j * r:(j + 1) * r] @ W["qkv_Bt"][j * r:(j + 1) * r]))
            else:
                parts.append(torch.zeros_like(qkv[:, :D]))
        qkv = qkv + torch.cat(parts, 1)
    if kept is not None:
        qkv.retain_grad()
        kept["qkv"] = qkv
    ctx = BR.attention64(qkv, cfg["spec"], W, cfg["p_attn"], s_attn)
    ctx_k, x_k = (ctx, x) if keep is None else (ctx[keep.long()], x[keep.long()])
    t = x_k + BR.hidden_drop(F.linear(ctx_k, W["o_w"], W["o_b"]) + adapter("out", ctx_k), cfg["p_hidden"], s_o)
    f_in = ln(t, "ln2" if pre_ln else "ln1")
    pre = F.linear(f_in, W["fc1_w"], W["fc1_b"]) + adapter("fc1", f_in)
    h = ACT.act(cfg["act"], pre) * ACT.drop_scale(pre.shape[0], pre.shape[1], cfg["p_act"], s_act)
    y = (t if pre_ln else f_in) + BR.hidden_drop(F.linear(h, W["fc2_w"], W["fc2_b"]) + adapter("fc2", h), cfg["p_hidden"], s_f2)
    return y if pre_ln else ln(y, "ln2")


def reference(x, params, cot, cfg, seeds):
    """block_reference.reference over block64_lora: ``params`` holds the twelve stored parameters and the adapter leaves."""
    W = BR._leaves(params)
    xr = x.detach().double().clone().requires_grad_(True)
    kept = {}
    return BR._finish(block64_lora(xr, W, cfg, seeds, kept), cot, xr, W, kept, x.shape[1])
