"""fp64 reference and per-element error bounds for the attention family (mdt_attention_fwd, mdt_attention_bwd,
mdt_attention_head_weights, mdt_attention_mean_probs, mdt_graph_attn_bias; include/mdt_hip.h), pure torch: no device, no
native library.

reference() computes the documented result of a launch from the exact stored operands (qkv, dout, the masks and biases) and,
next to every value, a bound δ on the arithmetic error a kernel may make.  tests/gemm_reference.py turns (value, δ) into a
tolerance (bound(): half an ulp of the storage type plus δ) and checks it (assert_within()); check() below adds the caps
that refuse a vacuous bound and keeps the worst err / bound per output.  Nothing a kernel stored is an operand here: the
backward is the gradient of the exact forward, so a forward that saved a wrong lse shows in the gradients too.

Layout.  Operands are logical tensors — qkv [nseq, S, 3 D], dout [nseq, S, D] — whatever seq_stride / pos_stride the launch
uses; a ragged launch (seq_offsets) is the same thing with a length per sequence: keys at or past the length are excluded,
query rows there do not exist.  Dropout counters follow the header, ((s H + h) S + q) S2 + key with S2 = S rounded up to
even and S the bound that sizes lse; keep-bits come from the hash port of gemm_reference.py.

The error model, u = 2^-24, γ_n = n u / (1 - n u), B = 2^-8 in a bf16 launch (the unit roundoff of bf16: half an ulp is 2^-9 of a value
only at the top of its binade, 2^-8 at the bottom — an emulated kernel exceeds a 2^-9 model) and 0 in fp32.
Sums of n terms in any order err by γ_n Σ|terms| (+ Σ of the terms' own errors); every further fp32 operation adds u times
the magnitude it rounds; δ = 0 where the arithmetic is provably exact.

Scores     s = scale (q . k) + bias, accumulated in fp32.  δdot = γ_hd Σ|q||k|, and 0 where k holds integers and q multiples
           of one power of two g with Σ|q||k| / g < 2^24 (every partial sum is an fp32 number: the "pointer" operands).  The bf16 kernels work in the exp2
           domain — fp32(scale log2 e), fused multiply-adds of the bias with fp32(log2 e), lse multiplied back by fp32(ln 2) —
           and a structural bias is summed from up to three terms: C_S = 8 roundings of u (|scale q . k| + |dense| + 2 |attn_bias|
           + |table or virt|), 2 attn_bias being exact.  An excluded key (key_mask 0, key_pad 1, a -inf bias entry, a key past
           a ragged length) has s = -inf exactly.
exp        __expf (fp32 kernels, the v1 bf16 kernels, the key-chunked path, head weights) and __builtin_amdgcn_exp2f (v2 forward,
           v2 - v5 backward): neither the HIP headers nor the kernel guides state an accuracy, so it was measured —
           tools/probes/exp_probe.hip sweeps every fp32 mantissa of the arguments (-64, 1) against fp64.  __expf is exp2 of the
           rounded product x log2 e, so its error grows with |x|: worst 1.30e-7 = 2.18 u per max(1, |x|) (__expf), 8.5e-8 = 1.42 u
           (exp2) on an MI355X (EXP_MEASURED, docs/experiment_log.md); the model allows twice the larger one, ε(x) =
           EXP_REL max(1, |x|) + u |x| (the subtraction that forms x).  Likewise __logf / log2 on the row sums [1, 512): worst
           absolute error 9.5e-7 (LOG_MEASURED), and the reciprocal 9.1e-8 relative (RCP_MEASURED); twice each is allowed.
Softmax    Δ = max δs over a row's live keys.  The kernel's P_j = e^(s~_j)(1 + ε_j) / Σ_k e^(s~_k)(1 + ε_k): against the exact P_j
           it is off by its own factor, r_own_j = expm1(δs_j) + ε(x_j), x = s - max, and by the row's normaliser, ONE number per
           row, r_row = expm1(Δ) + Σ_k P_k ε(x_k) + γ_S + RCP_REL + 3 u.  What is common to a row multiplies the row's sum
           (|out|, |delta|) and not the sum of magnitudes.
           lse = max + log Σ: δlse = Δ + Σ_k P_k ε(x_k) + γ_S + LOG_ABS + u (|max| + |log Σ|) + 3 u |lse|.
           The key-chunked path rescales its running sum and accumulators by e^(old max - new max) at every key: a
           multiplication by e^0 = 1 (exact: the probe checks that the device exp of 0 is 1) unless the key is a new running
           maximum.  Each real rescale costs lse another ε(jump); the reference counts the records R of the exact row and
           allows R' = 2 R + 2 of them (near ties may add records).  In out the rescale factors cancel (numerator and
           denominator carry the same ones) up to their roundings: γ_(S + R') in the forward sums of that path.
Forward    D = P keep / (1 - p) (fp32(1 / (1 - p)) as make_drop computes it).  The bf16 MFMA kernels round P (or the
           unnormalised e^x) to bf16 for P V: r_j = ((1 + r_own_j)(1 + B) - 1)(1 + r_row).  out = Σ_j D_j v_j: δout = Σ_j |D_j v_j| r_j +
           r_row |out| + (γ_S + 4 u) Σ_j |D_j v_j|.  The key-chunked path keeps P in fp32 (B = 0 there, also in a bf16 launch).
Backward   The kernels recompute P from the STORED lse: ρb_j = expm1(δs_j + tol(lse)) + ε(s_j - lse), tol(lse) = bound of the
           stored lse + 2 u |lse|.   dP = dO V^T: δdP = γ_hd Σ|dO||v|, dropout multiplies by keep / (1 - p) (one u).
           delta is documented as rowsum(dO . O_stored); the one-pass kernel for short rows (v4x) forms Σ_j P_j dP_j in fp32
           instead.  The reference's delta is Σ_j D_j dP_j in fp64 from the exact P and its δ is the larger of the two forms'
           errors: rowsum(dO . O~) = Σ_j D~_j dP_j up to the roundings of O~, so Σ_j |D_j| r_j |dP_j| + r_row |delta| + Σ_d |dO_d| (half an
           ulp of out_d in the storage type + (γ_S + 4 u) Σ_j |D_j v_jd|) + (γ_hd + u) Σ_d |dO_d out_d|,
           and Σ_j |P_j| (ρb_j |dPd_j| + δdPd_j) + γ_S Σ_j |P_j dPd_j|; + 2 u |delta| (kernels that fold 1 / (1 - p) out of it).
           dS = P (dPd - delta): with t = dPd - delta, δt = δdPd + δdelta + u |t|, δdS = P ρb (|t| + δt) + P δt + 3 u |dS|.
           That fp32 dS is what the dense dbias stores and what d_sp_table / d_virt sum (float atomics: the sum rule over
           the number of terms of each bin; nn.Embedding's padding row 0 of the table receives nothing, δ = 0).
           The bf16 MFMA kernels round dS to bf16 for the dQ and dK products: δdS_op = δdS + B (|dS| + δdS).
           dQ = scale dS K, dK = scale dS^T Q: δ = |scale| (δdS_op |K| summed + (γ_S + 3 u) Σ|dS||k|) — in dQ the part of δdS that is
           P_j δdelta is taken out of the sum and enters as δdelta |Σ_j P_j k_j| (+ ρb): one row's delta is one number; dV = D_b^T dO with
           D_b the recomputed, dropped and (bf16) rounded P: relative error (1 + ρb)(1 + B) - 1 + 2 u per term, + γ_S + 2 u.
Rows       A fully masked row has out = 0, lse = -inf and contributes nothing to any gradient: compared, δ = 0.  With q_limit
           the rows of out / lse at or past it are unspecified — the only elements left out ("valid") — and their dQ is
           compared: dout is zero there, every δ above is proportional to |dout|, so the reference demands exactly 0.
Others     head weights: P with ρb (it is recomputed from the stored lse), or with raw_scores s and δs; mean_probs: their mean
           over the heads (γ_H + u); graph_attn_bias: 2 attn_bias + table / virt, one rounding where the sum is no fp32 number.

Vacuous bounds are refused (AssertionError), as layernorm_reference.py does for δw > w / 2: a case whose median bound /
|value| exceeds CAPS — out 5 % (bf16) / 1e-4 (fp32), dqkv 10 % / 1e-3 — does not test its kernel, and its inputs are changed.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

import tests.gemm_reference as R
from tests.gemm_reference import assert_within, bound, drop_params, gen, keep_bits, ulp  # noqa: F401  (one import site for the tests)

U32 = R.U32
BF = torch.bfloat16
F32 = torch.float32
B16 = 2.0 ** -8
EXP_MEASURED = 1.30e-7            # __expf, per max(1, |x|); exp2: 8.5e-8
EXP_REL = 2.0 * EXP_MEASURED
LOG_MEASURED = 9.54e-7            # absolute, arguments in [1, 512)
LOG_ABS = 2.0 * LOG_MEASURED
RCP_MEASURED = 9.15e-8
RCP_REL = 2.0 * RCP_MEASURED
C_S = 8
CAPS = {("out", BF): 0.05, ("out", F32): 1e-4, ("dqkv", BF): 0.10, ("dqkv", F32): 1e-3}

_gamma, F24 = R._gamma, R.F24
NEG = -math.inf


def _eps(x):
    """ε(x): relative error of the device exp of x = a - b, the subtraction included (module docstring)."""
    ax = x.abs()
    return EXP_REL * ax.clamp(min=1.0) + U32 * ax


def drop_scale(nseq, H, S, p, seed, device="cpu", s2=None):
    """fp64 [nseq, H, S, S]: 0 or fp32(1 / (1 - p)), counter ((s H + h) S + q) S2 + key (``s2`` replaces S2: mutant tests)."""
    if not p:
        return torch.ones(nseq, H, S, S, dtype=torch.float64, device=device)
    S2 = (S + 1) & ~1 if s2 is None else s2
    bh = torch.arange(nseq * H, device=device, dtype=torch.int64).view(nseq, H, 1, 1)
    q = torch.arange(S, device=device, dtype=torch.int64).view(1, 1, S, 1)
    k = torch.arange(S, device=device, dtype=torch.int64).view(1, 1, 1, S)
    return keep_bits((bh * S + q) * S2 + k, p, seed).double() * drop_params(p)[1]


def struct_bias(attn_bias, spatial_pos, sp_table, virt):
    """The finite-or--inf structural bias [nseq, H, S, S] in fp64 and the magnitude its fp32 sum rounds: 2 attn_bias (graphormer
    adds it twice) + table[spatial_pos] on (q >= 1, key >= 1), virt[h] on row 0 and column 0."""
    nseq, S, _ = attn_bias.shape
    H = sp_table.shape[1]
    ab = attn_bias.double()
    b = (2.0 * ab)[:, None].expand(nseq, H, S, S).clone()
    t = torch.zeros(nseq, H, S, S, dtype=torch.float64)
    t[:, :, 0, :] = virt.double().view(1, H, 1)
    t[:, :, :, 0] = virt.double().view(1, H, 1)
    if S > 1:
        t[:, :, 1:, 1:] = sp_table.double()[spatial_pos.long()].permute(0, 3, 1, 2)
    return b + t, b.abs() + t.abs()


def _heads(x, H):
    n, S, D = x.shape
    return x.double().view(n, S, H, D // H).transpose(1, 2)          # [n, H, S, hd]


def _unheads(x):
    n, H, S, hd = x.shape
    return x.transpose(1, 2).reshape(n, S, H * hd)


def _integral(x):
    return bool((x == torch.round(x)).all())


def reference(qkv, dout, H, scale, dtype, *, key_mask=None, key_pad=None, dense_bias=None, attn_bias=None, spatial_pos=None,
              sp_table=None, virt=None, drop_p=0.0, drop_seed=0, lens=None, q_limit=0, long=False, want_bwd=True, drop_s2=None):
    """{name: (fp64 value, δ)} for out [nseq, S, D], lse [nseq, H, S], probs / scores [nseq, H, S, S] (head weights),
    mean_probs [nseq, S, S] and, with ``want_bwd``, dqkv [nseq, S, 3 D], dbias [nseq, H, S, S] and (structural bias) d_sp_table
    [num_spatial, H], d_virt [H]; "valid" [nseq, S]: the query rows whose out / lse are specified.  ``lens``: the lengths of a
    ragged launch.  ``long``: the key-chunked path runs (S > 272, or a dense bias on 128-wide heads past 208 tokens)."""
    u = U32
    nseq, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    sc = float(np.float32(scale))
    Q, K, V = (_heads(qkv[..., i * D:(i + 1) * D], H) for i in range(3))
    Bp = B16 if (dtype == BF and not long) else 0.0
    g_s, g_hd = _gamma(S), _gamma(hd)
    # ------------------------------------------------------------------ scores
    dot = Q @ K.transpose(-1, -2)
    A = Q.abs() @ K.abs().transpose(-1, -2)
    exact = any(_integral(Q * 2.0 ** g) and _integral(K) and float(A.max()) * 2.0 ** g < F24 for g in range(0, 6))   # q on a 2^-g grid
    d_dot = torch.zeros_like(A) if exact else g_hd * A
    dead = torch.zeros(nseq, 1, 1, S, dtype=torch.bool)
    klen = torch.full((nseq,), S, dtype=torch.int64) if lens is None else torch.as_tensor(lens, dtype=torch.int64)
    ar = torch.arange(S)
    dead = dead | (ar[None, :] >= klen[:, None])[:, None, None, :]
    if key_mask is not None:
        dead = dead | (key_mask == 0)[:, None, None, :]
    if key_pad is not None:
        dead = dead | (key_pad != 0)[:, None, None, :]
    bias = torch.zeros(nseq, H, S, S, dtype=torch.float64)
    bmag = torch.zeros(nseq, H, S, S, dtype=torch.float64)
    if dense_bias is not None:
        bias = bias + dense_bias.double()
        bmag = bmag + dense_bias.double().abs()
    if attn_bias is not None:
        sb, sm = struct_bias(attn_bias, spatial_pos, sp_table, virt)
        bias, bmag = bias + sb, bmag + sm
    dead = dead | (bias == NEG)
    bias = torch.where(dead, torch.zeros_like(bias), bias)
    bmag = torch.where(dead, torch.zeros_like(bmag), bmag)
    s_fin = sc * dot + bias
    d_s = abs(sc) * d_dot + C_S * u * (abs(sc) * (dot.abs() + d_dot) + bmag)
    d_s = torch.where(dead, torch.zeros_like(d_s), d_s)
    s = torch.where(dead, torch.full_like(s_fin, NEG), s_fin)
    qrow = (ar[None, :] < klen[:, None])                                     # [nseq, S]: the query rows that exist
    # ------------------------------------------------------------------ softmax
    m = s.max(-1).values
    live = torch.isfinite(m) & qrow[:, None, :]
    m0 = torch.where(live, m, torch.zeros_like(m))
    x = s - m0[..., None]
    e = torch.exp(x)
    Z = e.sum(-1)
    Zs = torch.where(live, Z, torch.ones_like(Z))
    P = torch.where(live[..., None], e / Zs[..., None], torch.zeros_like(e))
    logZ = torch.log(Zs)
    lse = torch.where(live, m0 + logZ, torch.full_like(m0, NEG))
    Dl = d_s.max(-1).values
    g_f, lse_long = g_s, 0.0
    if long:      # records of the running maximum: the rescales that are no multiplication by e^0 = 1
        sx = torch.where(dead, torch.full_like(s, -1e300), s)
        run = torch.cummax(sx, -1).values
        prev = torch.cat([torch.full_like(run[..., :1], -1e300), run[..., :-1]], -1)
        rec = (sx > prev) & ~dead
        nres = 2 * rec.sum(-1).double() + 2
        first = torch.where(rec, sx, torch.full_like(sx, 1e300)).min(-1).values
        rise = torch.where(live, m0 - first, torch.zeros_like(m0)).clamp(min=0.0)
        g_f = _gamma(S + nres)[..., None]
        lse_long = nres * (EXP_REL + 2 * u) + (EXP_REL + u) * 2 * rise
    ex = torch.where(dead | ~live[..., None], torch.zeros_like(x), _eps(torch.where(dead, torch.zeros_like(x), x)))
    avg = (P * ex).sum(-1)
    r_own = torch.expm1(d_s) + ex                                          # this key's score and exp
    g_r = g_f[..., 0] if long else g_f
    r_row = torch.expm1(Dl) + avg + g_r + RCP_REL + 3 * u                  # the row's normaliser: one number per row
    d_lse = Dl + avg + g_r + LOG_ABS + u * (m0.abs() + logZ.abs()) + 3 * u * (m0 + logZ).abs() + lse_long
    d_lse = torch.where(live, d_lse, torch.zeros_like(d_lse))
    ks = drop_scale(nseq, H, S, drop_p, drop_seed, s2=drop_s2)
    Dm = P * ks
    out_h = Dm @ V
    r = ((1 + r_own) * (1 + Bp) - 1) * (1 + r_row)[..., None]
    d_out_h = (Dm * r) @ V.abs() + r_row[..., None] * out_h.abs() + (g_f + 4 * u) * (Dm @ V.abs())
    ql = torch.full((nseq,), S, dtype=torch.int64) if not q_limit else torch.full((nseq,), int(q_limit), dtype=torch.int64)
    valid = qrow & (ar[None, :] < ql[:, None])
    res = {"out": (_unheads(out_h), _unheads(d_out_h)), "lse": (lse, d_lse), "valid": valid, "rows": qrow,
           "scores": (s, d_s)}
    # ------------------------------------------------------------------ recomputed P (backward, head weights)
    t_lse = bound(lse, d_lse, F32) + 2 * u * lse.abs()
    t_lse = torch.where(live, t_lse, torch.zeros_like(t_lse))
    xb = torch.where(dead | ~live[..., None], torch.zeros_like(s), s - torch.where(live, lse, torch.zeros_like(lse))[..., None])
    rho_b = torch.expm1(d_s + t_lse[..., None]) + _eps(xb)
    rho_b = torch.where(P > 0, rho_b, torch.zeros_like(rho_b))
    res["probs"] = (P, P * rho_b)
    res["mean_probs"] = (P.mean(1), (P * rho_b).mean(1) + (_gamma(H) + u) * P.mean(1))
    if not want_bwd:
        return res
    # ------------------------------------------------------------------ backward
    dO = _heads(dout, H)
    dP = dO @ V.transpose(-1, -2)
    d_dP = g_hd * (dO.abs() @ V.abs().transpose(-1, -2))
    dPd = dP * ks
    d_dPd = d_dP * ks + (u * dPd.abs() if drop_p else 0.0)
    delta = (P * dPd).sum(-1)
    half = 0.5 * ulp(out_h.abs() + d_out_h, dtype)
    d_del_a = (Dm * r * dP.abs()).sum(-1) + r_row * delta.abs() + (dO.abs() * (half + (g_f + 4 * u) * (Dm @ V.abs()))).sum(-1) + \
        (g_hd + u) * (dO * out_h).abs().sum(-1)
    d_del_b = (P * (rho_b * dPd.abs() + d_dPd)).sum(-1) + g_s * (P * dPd).abs().sum(-1)
    d_delta = torch.maximum(d_del_a, d_del_b) + 2 * u * delta.abs()
    t = dPd - delta[..., None]
    d_t = d_dPd + d_delta[..., None] + u * t.abs()
    dS = P * t
    d_dS = P * rho_b * (t.abs() + d_t) + P * d_t + 3 * u * dS.abs()
    d_op = d_dS + Bp * (dS.abs() + d_dS)
    asc = abs(sc)
    dQ = sc * (dS @ K)
    # dQ: a row's delta is ONE number, so its error reaches dQ through |Σ_j P_j k_j|, not Σ_j P_j |k_j|
    d_dS_q = P * rho_b * (t.abs() + d_t) + P * (d_t - d_delta[..., None]) + 3 * u * dS.abs()
    d_op_q = d_dS_q + Bp * (dS.abs() + d_dS)
    d_dQ = asc * (d_op_q @ K.abs() + d_delta[..., None] * ((P @ K).abs() + (P * rho_b) @ K.abs()) + (g_s + 3 * u) * (dS.abs() @ K.abs()))
    dK = sc * (dS.transpose(-1, -2) @ Q)
    d_dK = asc * (d_op.transpose(-1, -2) @ Q.abs() + (g_s + 3 * u) * (dS.abs().transpose(-1, -2) @ Q.abs()))
    rb = (1 + rho_b) * (1 + Bp) - 1 + 2 * u
    DbT = Dm.transpose(-1, -2)
    dV = DbT @ dO
    d_dV = (Dm * rb).transpose(-1, -2) @ dO.abs() + (g_s + 2 * u) * (DbT @ dO.abs())
    res["dqkv"] = (torch.cat([_unheads(dQ), _unheads(dK), _unheads(dV)], -1),
                   torch.cat([_unheads(d_dQ), _unheads(d_dK), _unheads(d_dV)], -1))
    res["dbias"] = (dS, d_dS)
    if attn_bias is not None:
        ns = sp_table.shape[0]
        tab = torch.zeros(ns, H, dtype=torch.float64)
        d_tab = torch.zeros(ns, H, dtype=torch.float64)
        mag = torch.zeros(ns, H, dtype=torch.float64)
        cnt = torch.zeros(ns, dtype=torch.float64)
        if S > 1:
            idx = spatial_pos.long().reshape(-1)                                           # [nseq (S-1) (S-1)]
            pick = lambda z: z[:, :, 1:, 1:].permute(0, 2, 3, 1).reshape(-1, H)
            tab.index_add_(0, idx, pick(dS))
            d_tab.index_add_(0, idx, pick(d_dS))
            mag.index_add_(0, idx, pick(dS.abs() + d_dS))
            cnt.index_add_(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
        d_tab = d_tab + _gamma(cnt)[:, None] * mag
        tab[0], d_tab[0] = 0.0, 0.0
        res["d_sp_table"] = (tab, d_tab)
        edge = lambda z: z[:, :, 0, :].sum((0, 2)) + z[:, :, 1:, 0].sum((0, 2))
        n_e = nseq * (2 * S - 1)
        res["d_virt"] = (edge(dS), edge(d_dS) + _gamma(n_e) * edge(dS.abs() + d_dS))
    return res


def reference_graph_bias(attn_bias, spatial_pos, sp_table, virt):
    """mdt_graph_attn_bias: (value, δ) of the fp32 [nseq, H, S, S] structural bias; -inf entries stay -inf."""
    v, mag = struct_bias(attn_bias, spatial_pos, sp_table, virt)
    fin = torch.isfinite(v)
    d = torch.where(fin & ~R._rep32(torch.where(fin, v, torch.zeros_like(v))), U32 * mag, torch.zeros_like(mag))
    return v, torch.where(fin, d, torch.zeros_like(d))


WORST = {}        # (output name, dtype) -> worst err / bound seen by check() (the GPU matrix reports it)


def check(got: dict, ref: dict, dtype, what: str = ""):
    """assert_within for every entry of ``got`` ({name: logical tensor}) against ``ref``; out / lse only on ref["valid"] rows;
    an output with a cap (CAPS) must have a bound that is not vacuous.  Returns {name: worst err / bound} and keeps it in WORST."""
    worst = {}
    for name, t in got.items():
        v, d = ref[name]
        dt = dtype if name in ("out", "dqkv") else F32
        t = t.double()
        if name == "out":
            t = torch.where(ref["valid"][:, :, None], t, v)
        elif name == "lse":
            t = torch.where(ref["valid"][:, None, :], t, v)
        elif name == "dqkv":
            t = torch.where(ref["rows"][:, :, None], t, v)
        bnd = bound(torch.where(torch.isfinite(v), v, torch.zeros_like(v)), d, dt)
        fin = torch.isfinite(v)
        ratio = torch.where(fin, (t - v).abs() / bnd.clamp(min=1e-300), torch.zeros_like(v))
        rmax = float(ratio.max()) if ratio.numel() else 0.0
        worst[name] = rmax if rmax == rmax else float("inf")
        WORST[(name, dtype)] = max(WORST.get((name, dtype), 0.0), worst[name])
        assert bool(((t == v) | fin).all()), f"{what} {name}: a -inf element of the reference is not -inf"
        # dtype fp32: the rounding-bias statistic of assert_within is for outputs whose only error is their final rounding
        assert_within(t, v, bnd, what=f"{what} {name}", dtype=F32, median_limit=CAPS.get((name, dt), 1e30))
    return worst


# ------------------------------------------------------------------------------------------------ routing, mirrored
V4_EXACT_PAIRS = 3


def v1_fits(hd, S):
    return hd < 128 or S <= 208


def v1_rung(S):
    nt = (S + 15) // 16
    return next(r for r in (2, 5, 7, 9, 13, 17) if nt <= r)


def v2_rung(S):
    nt = (S + 15) // 16
    return next(r for r in (2, 4, 5, 7, 9, 13, 17) if nt <= r)


def _one_pass_fits(cap):
    n_t = (cap + 15) // 16
    rows_img = ((n_t + 1) // 2) * 32
    ldq = 16 * n_t if n_t & 1 else 16 * n_t + 16
    slabs = 7 if n_t <= 2 * V4_EXACT_PAIRS else 0
    b = 2 * rows_img * 72 * 2 + (3 + slabs) * rows_img * 4 + 16 * n_t * ldq * 2
    return b <= 160 * 1024 and n_t <= 16, rows_img


def bwd_ok(route, hd, S, mode, qlim=0, cap=0):
    """ok() of attn_plan (csrc/attention.hip) for a bf16 launch of S <= 272: may MDT_ATTN_BWD=route be honoured."""
    binned = cap > 0
    c = cap or S
    n_t = (c + 15) // 16
    fits, rows_img = _one_pass_fits(c)
    one_pass = hd == 64 and mode not in ("struct", "dense") and fits
    return {"v1": not binned and not qlim and v1_fits(hd, S),
            "v2": not binned and mode != "dense" and not qlim and S <= 112,
            "v3": mode != "dense",
            "v4": one_pass,
            "v4x": one_pass and n_t <= 2 * V4_EXACT_PAIRS,
            "v5": one_pass and n_t > 8 and rows_img * 8 <= 4 * 512}[route]


def bwd_route(dtype, hd, S, mode, p=0.0, qlim=0, cap=0, forced=None):
    """The backward route of a launch (attn_plan of csrc/attention.hip, restated independently: this module never asks the
    library for a route; tests/test_attention_plan_cpu.py holds the two against each other over the whole domain)."""
    if S > 272:
        return "long"
    if dtype != BF:
        return "long" if fp32_bwd_long(hd, S, mode, p) else "v1"
    if mode == "dense" and not v1_fits(hd, S):
        return "long"
    if forced and bwd_ok(forced, hd, S, mode, qlim, cap):
        return forced
    family = next((r for r in ("v5", "v4x", "v4") if bwd_ok(r, hd, S, mode, qlim, cap)), "v3")
    if cap:
        return family
    if mode == "dense":
        return "v1"
    if S > 256:
        return family
    if S <= 80 and not qlim and mode == "struct":
        return "v1"
    if not p and bwd_ok("v2", hd, S, mode, qlim, cap):
        return "v2"
    return family


def fp32_bwd_long(hd, S, mode, p):
    """The fp32 v1 backward that is not built — wide heads, the 17-tile rung (14 .. 17 key tiles: S 209 .. 272), structural bias
    and dropout (512 registers and scratch memory) — runs on the key-chunked path."""
    return hd > 64 and v1_rung(S) == 17 and mode == "struct" and p > 0


def fwd_route(dtype, hd, S, mode):
    if S > 272:
        return "long"
    if dtype != BF:
        return "v1"
    if mode == "dense":
        return "v1" if v1_fits(hd, S) else "long"
    return "v2"


WIDTHS = (16, 64, 96, 128)


def refusal(dtype, hd, S, qlim=0, ragged=False, cap=0):
    """None, or why a launch that passed the argument checks is refused before any route (in the order the library decides):
    "bins": seq_ids / s_cap on anything but a ragged bf16 launch of 64-wide heads with S <= 272; "long": the key-chunked path
    (S > 272) takes neither ragged sequences nor q_limit; "head_dim": a width outside WIDTHS.  (A v3 launch whose structural-bias
    histogram does not fit LDS beside its images is refused too: that depends on num_spatial, which no case here varies.)"""
    if cap:
        if S > 272 or dtype != BF or hd != 64 or not ragged:
            return "bins"
    elif S > 272 and (ragged or qlim):
        return "long"
    return None if hd in WIDTHS else "head_dim"


def fwd_rung(route, S, mode, cap=0):
    """The forward's counterpart of bwd_rung: the rung of v1, (rung, waves) of v2 — 8 waves for the long rows (13 key tiles
    and more) without a structural bias — and nothing for long."""
    if route == "v1":
        return v1_rung(S)
    if route == "v2":
        r = v2_rung(cap or S)
        return (r, 8 if r >= 13 and mode != "struct" else 4)
    return 0


def bwd_rung(route, hd, S, cap=0, mode="none"):
    """What distinguishes two launches of one route: the tile-count rung (v1, v2), the padded length and thread count (v3),
    the wave count (v4, v4x), nothing (v5, long)."""
    c = cap or S
    n_t = (c + 15) // 16
    if route == "v1":
        return v1_rung(S)
    if route == "v2":
        return v2_rung(c)
    if route == "v3":
        tight = hd == 128 and c > 256
        s_pad = (c + 31) & ~31 if tight else (c + 63) & ~63
        return (s_pad, 512 if (hd <= 64 and s_pad > 128 and mode != "struct") else 256)   # 512 threads: the plain (no structural bias) build
    if route in ("v4", "v4x"):
        return 4 if n_t <= 4 else 8 if n_t <= 8 else 16
    return 0


# ------------------------------------------------------------------------------------------------ the matrix
NSEQ, HEADS = 2, 3
SIZES = (1, 8, 32, 33, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 144, 145, 192, 193, 208, 209, 256, 257, 272)
MODES = (("none", False), ("mask", False), ("dense", False), ("dense", True), ("struct", False), ("struct", True))   # (mode, time-major)
ROUTES = ("v1", "v2", "v3", "v4", "v4x", "v5")
P_DROP = 0.25
POINTER_C, SOFT_GAIN = 2.0, 0.5
Case = namedtuple("Case", "dtype hd S mode family p qlim lens")


def operands(c: Case, seed=0):
    """The logical operands of a case: qkv, dout (bf16-exact values, so fp32 and bf16 launches see the same numbers) and the
    mask / bias tensors of its mode as keyword arguments of reference() / the ops.  Families (module docstring of
    tests/test_attention_reference_cpu.py): "uniform"; "pointer": k rows of +-1, q_i = c k_pi(i) with c = 2 — every key is one
    query's dominant key; "soft": the same with c chosen so that P_i,pi(i) ~ 0.5."""
    nseq, H, S, hd = NSEQ, HEADS, c.S, c.hd
    D = H * hd
    seed = seed + 1000 * S + hd
    qkv = gen((nseq, S, 3 * D), seed + 1, 1.0, BF).float()
    # v around 1 and q around 1/2: out and dK, means over S keys / queries that each matter 1 / S, then do not cancel to 1 / sqrt(S) of the
    # bound's sum of magnitudes (a worst-case bound of a sum that cancels is vacuous: CAPS); the scores stay soft, std 0.6
    qkv[..., 2 * D:] = 1.0 + 0.5 * qkv[..., 2 * D:]
    if c.family == "uniform":
        qkv[..., :D] = 0.5 + 0.5 * qkv[..., :D]
    if c.family != "uniform":
        g = torch.Generator().manual_seed(seed + 2)
        k = (torch.randint(0, 2, (nseq, S, H, hd), generator=g) * 2 - 1).float()
        perm = torch.stack([torch.stack([torch.randperm(S, generator=g) for _ in range(H)]) for _ in range(nseq)])   # [nseq, H, S]
        kp = torch.gather(k.permute(0, 2, 1, 3), 2, perm[..., None].expand(nseq, H, S, hd)).permute(0, 2, 1, 3)
        if c.family == "pointer":
            cq = POINTER_C
        else:      # softmax weight of the pointed key 1 / (1 + (S - 1) e^(σ²/2 - c hd scale)) ~ 0.5, other scores ~ N(0, c² hd scale²)
            want = math.log(max(S - 1, 1)) + SOFT_GAIN
            cq = max(round(want / math.sqrt(hd) * 16) / 16, 1.0 / 16)                                # on a 1/16 grid: bf16-exact products
        qkv[..., :D] = (cq * kp).reshape(nseq, S, D)
        qkv[..., D:2 * D] = k.reshape(nseq, S, D)
    qkv = qkv.to(BF).float()
    # dout: one column of every head carries +-1 (+1 in the uniform family: dK is a sum over queries), the others 2^-8 gen(): delta's error is a worst-case sum over the head's columns
    # of |dout| x the rounding of O, so a dense dout of one size makes the bound of dQ / dK sqrt(hd) times what kernels do
    dout = gen((nseq, S, D), seed + 3, 1.0, BF).float()
    strong = (torch.arange(D) % hd == 5)
    dout = torch.where(strong, torch.ones_like(dout) if c.family == "uniform" else torch.sign(dout) + (dout == 0).float(),
                       (dout.abs() if c.family == "uniform" else dout) * 2.0 ** -8)
    if c.qlim:
        dout[:, c.qlim:] = 0
    kw = {}
    if c.mode == "mask":
        km = torch.ones(nseq, S, dtype=torch.uint8)
        km[1, max(1, S - 3):] = 0                                       # sequence 1: the last three keys (all but key 0 when S < 4)
        kw["key_mask"] = km
    elif c.mode == "dense":
        b = gen((nseq, H, S, S), seed + 4, 1.0, BF).float()
        if S > 2:
            b[:, :, :, S - 2] = NEG
        b[0, 1, S // 2, :] = NEG                                        # one fully masked row
        kw["dense_bias"] = b
    elif c.mode == "struct":
        g = torch.Generator().manual_seed(seed + 5)
        ns = 24
        kw["attn_bias"] = gen((nseq, S, S), seed + 6, 0.5, BF).float()
        if S > 4:
            far = torch.rand(nseq, S, S, generator=g) < 0.1
            far[:, 0, :] = False
            far[:, :, 0] = False
            far[:, ar_(S), ar_(S)] = False
            kw["attn_bias"][far] = NEG
        kw["spatial_pos"] = torch.randint(0, ns, (nseq, max(S - 1, 0), max(S - 1, 0)), generator=g, dtype=torch.int32)
        kw["sp_table"] = gen((ns, H), seed + 7, 1.0, c.dtype)
        kw["sp_table"][0] = 0                                           # nn.Embedding(padding_idx=0)
        kw["virt"] = gen((H,), seed + 8, 1.0, c.dtype)
        kp_ = torch.zeros(nseq, S, dtype=torch.uint8)
        if S > 2:
            kp_[1, S - 1] = 1                                           # a padded sequence: its last key is padding
        kw["key_pad"] = kp_
    if c.p:
        kw.update(drop_p=c.p, drop_seed=4242 + S)
    if c.lens:
        kw["lens"] = c.lens
    if c.qlim:
        kw["q_limit"] = c.qlim
    return qkv, dout, kw


def ar_(S):
    return torch.arange(S)


def is_long(c: Case):
    """The key-chunked path runs: past 272 tokens, a dense bias on bf16 heads the v1 images do not fit, and — the backward
    only, whose forward ran v1 in fp32 and is held to the looser of the two models' bounds — the fp32 launch of fp32_bwd_long."""
    return c.S > 272 or (c.dtype == BF and c.mode == "dense" and not v1_fits(c.hd, c.S)) or \
        (c.dtype == F32 and fp32_bwd_long(c.hd, c.S, c.mode, c.p))


_REF = {}


def case_reference(c: Case, want_bwd=True):
    """operands(c) and reference() of them, computed once per case and shared (the tests leave both unchanged)."""
    key = (c, want_bwd)
    if key not in _REF:
        qkv, dout, kw = operands(c)
        if len(_REF) > 8:
            _REF.clear()
        _REF[key] = (qkv, dout, kw, reference(qkv, dout, HEADS, c.hd ** -0.5, c.dtype, long=is_long(c), want_bwd=want_bwd, **kw))
    return _REF[key]


def main_cases():
    """The head-width-64 matrix: per (dtype, mode, S) the "pointer" forward, the "soft" forward + backward without dropout and
    the "uniform" forward + backward with dropout."""
    out = []
    for dtype in (F32, BF):
        for mode, tm in MODES:
            for S in SIZES:
                out.append((dtype, mode, tm, S))
    return out


def families(dtype, hd, S, mode):
    return (Case(dtype, hd, S, mode, "pointer", 0.0, 0, None), Case(dtype, hd, S, mode, "soft", 0.0, 0, None),
            Case(dtype, hd, S, mode, "uniform", P_DROP, 0, None))


QLIM = 9
QLIM_SIZES = (33, 97, 129, 209, 257)
RAGGED = ((33, (33, 16)), (97, (97, 81)), (129, (129, 112)), (209, (209, 193)), (257, (257, 240)))      # (S, lengths): one past, one on a tile edge
BINS = ((129, (129, 47), 48), (209, (209, 97), 112))                                                   # (S, lengths, cap of the short bin)
LONG = tuple((dtype, 64, S, mode) for dtype in (F32, BF) for S in (273, 320) for mode in ("none", "mask", "dense", "struct")) + \
    ((F32, 128, 209, "dense"), (BF, 128, 209, "dense"))
WIDE = (  # (hd, S, mode): one case per reachable forward / backward route of the other widths
    (16, 33, "dense"), (16, 65, "struct"), (16, 97, "none"), (16, 129, "struct"), (16, 257, "mask"),
    (96, 33, "dense"), (96, 65, "struct"), (96, 97, "none"), (96, 129, "struct"), (96, 257, "mask"),
    (96, 257, "struct"),          # fp32 with dropout: the backward v1 does not build (fp32_bwd_long) -> long; bf16: the v3 family
    (128, 33, "dense"), (128, 65, "struct"), (128, 97, "none"), (128, 129, "struct"), (128, 256, "none"), (128, 257, "none"),
)
