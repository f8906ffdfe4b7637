"""The bounds of tests/attention_reference.py, proven on the CPU for every case of tests/test_attention_routes_gpu.py: a torch
emulation of a correct fp32 kernel and one of a correct bf16 kernel (exp2 domain, P rounded to bf16 for P V, dS rounded to bf16
for the dQ / dK products, delta from the stored bf16 O, P recomputed from the stored lse) stay inside the bound on every
output, and each subtly wrong kernel — the same emulation with one mutation, applied to forward and backward alike — is
rejected on the output named, in both types and at every length of the matrix where the mutation changes anything.

Operand families (attention_reference.operands), all bf16-exact so that fp32 and bf16 launches see the same numbers:
    uniform   k = gen(scale 1), q = 1/2 + gen / 2, v = 1 + gen / 2: the soft case, every key matters a little (1 / S); it carries
              the dropout cases.  q and v are not centred on 0 because out and dK are then means over S terms of both signs,
              1 / sqrt(S) of the sum of magnitudes a worst-case bound is made of: such a bound is vacuous and is refused
    pointer   k rows of +-1, q_i = 2 k_pi(i) for a random permutation pi: P_i,pi(i) ~ 1, every key is one query's dominant key
              — a skipped, shifted or wrongly masked key or tile breaks a whole output row by O(1); scores are exact integers / 4
    soft      the same with q_i = c k_pi(i), c = (ln(S - 1) + 1/2) / sqrt(hd) on a 1/16 grid: P_i,pi(i) ~ 0.5, so that dS does
              not vanish (with a one-hot P it does, and dQ / dK say nothing); this family carries the backward mutants
dout is +-1 in one column of every head (+1 in the uniform family) and 2^-8 gen() in the others: delta's error is a worst-case sum
over a head's columns of |dout| times the rounding of O, and with a dout of one size everywhere that sum, not the kernel,
decides the bound of dQ / dK (60 % of their values; with this dout 2 - 9 %).
"""
import math

import pytest
import torch

import tests.attention_reference as A
from tests.attention_reference import BF, F32, Case

LOG2E, LN2 = float(torch.tensor(1.4426950408889634, dtype=F32)), float(torch.tensor(0.6931471805599453, dtype=F32))


def rb(x):
    return x.to(BF).float()


def emulate(qkv, dout, H, scale, dtype, kw, mutant=None, long=False, want_bwd=True):
    """A correct kernel in fp32 torch arithmetic (``dtype`` bf16: rounding at the documented points), or with ``mutant`` a
    subtly wrong one.  Logical layouts in and out, as attention_reference.reference()."""
    bf = dtype == BF
    nseq, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    p_drop, seed, qlim = kw.get("drop_p", 0.0), kw.get("drop_seed", 0), kw.get("q_limit", 0)
    lens = kw.get("lens") or (S,) * nseq
    hv = lambda t: t.float().view(nseq, S, H, -1).transpose(1, 2)
    unh = lambda t: t.transpose(1, 2).reshape(nseq, S, -1)
    Q, K, V, dO = hv(qkv[..., :D]), hv(qkv[..., D:2 * D]), hv(qkv[..., 2 * D:]), hv(dout)
    sc = torch.tensor(scale, dtype=F32)
    if mutant == "scale_ulp":
        sc = sc * (1 + 2.0 ** -8)
    ar = torch.arange(S)
    klen = torch.tensor(lens)
    dead = (ar[None, :] >= klen[:, None])[:, None, None, :].expand(nseq, H, S, S).clone()
    if "key_mask" in kw:
        dead |= (kw["key_mask"] == 0)[:, None, None, :]
    if "key_pad" in kw:
        kp = kw["key_pad"].clone()
        if mutant == "pad_attended":
            kp[:, S - 1] = 0
        dead |= (kp != 0)[:, None, None, :]
    bias = torch.zeros(nseq, H, S, S)
    if "dense_bias" in kw:
        b = kw["dense_bias"]
        if mutant == "neighbour_bias":      # query row 5 reads row 6's bias
            b = b.clone()
            b[:, :, 5] = kw["dense_bias"][:, :, 6]
        bias = bias + b
    if "attn_bias" in kw:
        tab, virt = kw["sp_table"].float(), kw["virt"].float()
        if mutant == "next_head_table":
            tab, virt = tab.roll(-1, 1), virt.roll(-1, 0)
        ab = kw["attn_bias"]
        if mutant == "neighbour_bias":
            ab = ab.clone()
            ab[:, 5] = kw["attn_bias"][:, 6]
        sb = ((1.0 if mutant == "bias_once" else 2.0) * ab)[:, None].expand(nseq, H, S, S).clone()
        t = torch.zeros(nseq, H, S, S)
        t[:, :, 0, :] = virt.view(1, H, 1)
        t[:, :, :, 0] = virt.view(1, H, 1)
        if S > 1:
            t[:, :, 1:, 1:] = tab[kw["spatial_pos"].long()].permute(0, 3, 1, 2)
        bias = bias + (sb + t)
    dead |= bias == -math.inf
    if mutant in ("drop_last_key", "drop_last_tile"):
        for n in range(nseq):
            last = int(lens[n]) - 1
            lo = last if mutant == "drop_last_key" else (last // 16) * 16
            dead[n, :, :, lo:last + 1] = True
    bias = torch.where(dead, torch.zeros_like(bias), bias)
    dot = Q @ K.transpose(-1, -2)
    if bf:      # exp2 domain
        s = dot * (sc * LOG2E) + bias * LOG2E
    else:
        s = dot * sc + bias
    s = torch.where(dead, torch.full_like(s, -math.inf), s)
    rows = (ar[None, :] < klen[:, None])[:, None, :].expand(nseq, H, S)
    m = s.max(-1).values
    live = torch.isfinite(m) & rows
    m0 = torch.where(live, m, torch.zeros_like(m))
    e = torch.exp2(s - m0[..., None]) if bf else torch.exp(s - m0[..., None])
    e = torch.where(live[..., None], e, torch.zeros_like(e))
    Z = e.sum(-1)
    Zs = torch.where(live, Z, torch.ones_like(Z))
    lse = (m0 + torch.log2(Zs)) * LN2 if bf else m0 + torch.log(Zs)
    lse = torch.where(live, lse, torch.full_like(lse, -math.inf))
    if mutant == "lse_off":
        lse = lse + 1e-3
    s2 = S if mutant == "drop_s" else None
    ks = A.drop_scale(nseq, H, S, p_drop, seed, s2=s2).float()
    keep = (ks != 0).float()
    ik = float(ks.max()) if p_drop else 1.0
    if bf and not long:
        o = (rb(e * keep) @ V) * ((1.0 / Zs) * ik)[..., None]
    else:
        o = ((e * (1.0 / Zs)[..., None]) * ks) @ V
    out = unh(o).to(dtype)
    res = {"out": out, "lse": lse}
    lse0 = torch.where(live, lse, torch.zeros_like(lse))
    if bf and not long:
        P = torch.exp2(s - (lse0 * LOG2E)[..., None])
    elif bf:
        P = torch.exp(s * LN2 - lse0[..., None])
    else:
        P = torch.exp(s - lse0[..., None])
    P = torch.where(live[..., None] & ~dead, P, torch.zeros_like(P))
    res["probs"] = P
    res["mean_probs"] = P.sum(1) / H
    res["scores"] = s * LN2 if bf else s
    if not want_bwd:
        return res
    dPd = (dO @ V.transpose(-1, -2)) * ks
    delta = (dO * hv(out)).sum(-1)
    if mutant == "delta_no_keep":
        delta = delta * (1.0 - p_drop)
    dS = P * (dPd - delta[..., None])
    dS_op = rb(dS) if (bf and not long) else dS
    Db = P * ks
    Db_op = rb(Db) if (bf and not long) else Db
    dQ = (dS_op @ K) * sc
    dS_k = dS_op
    if mutant == "dk_prev_tile":            # the last 16-row query tile never reaches dK
        dS_k = dS_op.clone()
        dS_k[:, :, max(S - 16, 0):, :] = 0
    dK = (dS_k.transpose(-1, -2) @ Q) * sc
    dV = Db_op.transpose(-1, -2) @ dO
    if mutant == "qlim_dq":
        dQ = dQ.clone()
        dQ[:, :, qlim:, :] = 2.0 ** -12
    res["dqkv"] = torch.cat([unh(dQ), unh(dK), unh(dV)], -1).to(dtype)
    res["dbias"] = dS
    if "attn_bias" in kw:
        ns = kw["sp_table"].shape[0]
        tabg = torch.zeros(ns, H)
        if S > 1:
            tabg.index_add_(0, kw["spatial_pos"].long().reshape(-1), dS[:, :, 1:, 1:].permute(0, 2, 3, 1).reshape(-1, H))
        if mutant != "table_row0":
            tabg[0] = 0
        res["d_sp_table"] = tabg
        res["d_virt"] = dS[:, :, 0, :].sum((0, 2)) + (0 if mutant == "virt_no_col" else dS[:, :, 1:, 0].sum((0, 2)))
    return res


def run(c: Case, mutant=None, want_bwd=True):
    qkv, dout, kw, ref = A.case_reference(c, want_bwd)
    got = emulate(qkv, dout, A.HEADS, c.hd ** -0.5, c.dtype, kw, mutant, long=A.is_long(c), want_bwd=want_bwd)
    return got, ref


def outputs(c: Case, got):
    names = ["out", "lse"] + (["dqkv"] if "dqkv" in got else [])
    if "dqkv" in got and c.mode == "dense":
        names.append("dbias")
    if "d_sp_table" in got:
        names += ["d_sp_table", "d_virt"]
    return {n: got[n] for n in names}


def every_case():
    """The operand cases of the GPU matrix (layouts and forced routes share theirs)."""
    cs = []
    for dtype in (F32, BF):
        for mode in ("none", "mask", "dense", "struct"):
            for S in A.SIZES:
                cs += A.families(dtype, 64, S, mode)
        for S in A.QLIM_SIZES:
            cs += [Case(BF, 64, S, m, "soft", A.P_DROP, q, None) for m in ("none", "struct") for q in (A.QLIM, 0)] if dtype == BF else []
        for S, lens in A.RAGGED + tuple((s, l) for s, l, _ in A.BINS):
            cs.append(Case(dtype, 64, S, "none", "soft", A.P_DROP, 0, lens))
    for dtype, hd, S, mode in A.LONG:
        cs += [Case(dtype, hd, S, mode, "soft", 0.0, 0, None), Case(dtype, hd, S, mode, "uniform", A.P_DROP, 0, None)]
    for hd, S, mode in A.WIDE:
        for dtype in (F32, BF):
            cs += [Case(dtype, hd, S, mode, "soft", 0.0, 0, None), Case(dtype, hd, S, mode, "uniform", A.P_DROP, 0, None)]
    return cs


def cid(c):
    if not isinstance(c, Case):
        return None
    return f"{'bf16' if c.dtype == BF else 'fp32'}-hd{c.hd}-S{c.S}-{c.mode}-{c.family}" + (f"-p{c.p}" if c.p else "") + \
        (f"-q{c.qlim}" if c.qlim else "") + (f"-len{'_'.join(map(str, c.lens))}" if c.lens else "")


@pytest.mark.parametrize("c", every_case(), ids=cid)
def test_faithful_emulation_is_within_the_bound(c):
    """The emulation of a correct kernel of the case's type passes on every output, and no output's bound is vacuous (CAPS)."""
    want_bwd = c.family != "pointer"
    got, ref = run(c, want_bwd=want_bwd)
    worst = A.check(outputs(c, got), ref, c.dtype, what=cid(c))
    print(cid(c), " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("S", (33, 129))
@pytest.mark.parametrize("mode", ("struct", "mask"))
@pytest.mark.parametrize("dtype", (F32, BF), ids=("fp32", "bf16"))
def test_non_training_outputs_within_the_bound(dtype, mode, S):
    c = Case(dtype, 64, S, mode, "soft", 0.0, 0, None)
    got, ref = run(c, want_bwd=False)
    print(cid(c), A.check({n: got[n] for n in ("probs", "scores", "mean_probs")}, ref, dtype, what=cid(c)))
    if mode == "struct":
        _, _, kw, _ = A.case_reference(c, False)
        v, d = A.reference_graph_bias(kw["attn_bias"], kw["spatial_pos"], kw["sp_table"], kw["virt"])
        t = (2.0 * kw["attn_bias"])[:, None] + torch.zeros(1, A.HEADS, 1, 1)
        A.assert_within(v.float(), v, A.bound(torch.nan_to_num(v, neginf=0.0), d, F32), what="graph_attn_bias", dtype=F32)
        with pytest.raises(AssertionError):      # attn_bias added once
            A.assert_within((v - t.double().nan_to_num(neginf=0.0)).float(), v, A.bound(torch.nan_to_num(v, neginf=0.0), d, F32), dtype=F32)


# mutant -> (mode, family, dropout, the outputs that must fail (any of a tuple inside), smallest S it changes anything at)
MUTANTS = {
    "drop_last_key": ("none", "soft", 0.0, ["out", "lse"], 1),
    "drop_last_tile": ("none", "soft", 0.0, ["out", "lse"], 17),
    "neighbour_bias": ("dense", "soft", 0.0, ["out"], 8),
    "next_head_table": ("struct", "soft", 0.0, ["out"], 8),
    "bias_once": ("struct", "soft", 0.0, ["out"], 8),
    "pad_attended": ("struct", "soft", 0.0, ["out"], 8),
    "scale_ulp": ("none", "soft", 0.0, [("out", "dqkv")], 8),
    "lse_off": ("none", "soft", 0.0, ["lse", "dqkv"], 8),         # bf16: lse only, see test_mutant_is_rejected
    "delta_no_keep": ("none", "uniform", A.P_DROP, ["dqkv"], 8),
    "drop_s": ("none", "uniform", A.P_DROP, ["out"], 33),          # S2 = S at every even S
    "dk_prev_tile": ("none", "soft", 0.0, ["dqkv"], 8),
    "table_row0": ("struct", "soft", 0.0, ["d_sp_table"], 8),
    "virt_no_col": ("struct", "uniform", A.P_DROP, ["d_virt"], 8),
}


def fails(name, got, ref, dtype):
    try:
        A.check({name: got[name]}, ref, dtype)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("S", A.SIZES + (273, 320))
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
@pytest.mark.parametrize("dtype", (F32, BF), ids=("fp32", "bf16"))
def test_mutant_is_rejected(dtype, mutant, S):
    """Each mutant fails on the outputs named, in both types, at every length where it changes anything.  One exception, by
    arithmetic: lse off by 1e-3 scales every recomputed P by 0.999, and a bf16 kernel that is right may itself be off by 2^-8
    = 3.9e-3 of every P it rounds for the dV product (and of every dS for dQ / dK), so no bound that admits correct bf16
    kernels can see 1e-3 in the bf16 dqkv (measured: the mutant's dqkv sits at 0.8 - 0.9 of its bound there).  A bf16 launch
    shows this mutant in lse, which is fp32 in both types; its dqkv is asked to fail in fp32 only."""
    mode, family, p, must, s_min = MUTANTS[mutant]
    if mutant == "lse_off" and dtype == BF:
        must = ["lse"]
    if S < s_min or (mutant == "drop_s" and S % 2 == 0):
        return                          # the mutation changes nothing here
    c = Case(dtype, 64, S, mode, family, p, 0, None)
    got, ref = run(c, mutant)
    for name in must:
        names = name if isinstance(name, tuple) else (name,)
        assert any(fails(n, got, ref, dtype) for n in names), f"{mutant} at S={S} passes on {names}"


@pytest.mark.parametrize("S", A.QLIM_SIZES)
def test_query_limit_mutant_is_rejected(S):
    c = Case(BF, 64, S, "none", "soft", A.P_DROP, A.QLIM, None)
    got, ref = run(c, "qlim_dq")
    assert fails("dqkv", got, ref, BF)
    assert not fails("out", got, ref, BF)


def test_vacuous_bound_is_refused():
    """Operands whose bound says nothing are refused: uniform q, k of scale 16 make bf16 scores err by more than the outputs."""
    c = Case(F32, 64, 65, "none", "uniform", 0.0, 0, None)
    qkv, dout, kw = A.operands(c)
    qkv = qkv * 64.0
    ref = A.reference(qkv, dout, A.HEADS, 0.125, F32)
    got = emulate(qkv, dout, A.HEADS, 0.125, F32, kw)
    with pytest.raises(AssertionError, match="vacuous"):
        A.check({"out": got["out"]}, ref, F32)


def test_matrix_reaches_every_route_and_rung():
    """attn_plan (csrc/attention.hip), mirrored in attention_reference, over the launches of the GPU matrix: every
    (route, rung) pair a head-width-64 launch can take is reached, by default or forced."""
    fwd, bwd = set(), set()
    for dtype, mode, tm, S in A.main_cases():
        r = A.fwd_route(dtype, 64, S, mode)
        fwd.add((dtype, r, A.v2_rung(S) if r == "v2" else A.v1_rung(S)))
        for p in (0.0, A.P_DROP):
            for forced in (None,) + (A.ROUTES if dtype == BF else ()):
                r = A.bwd_route(dtype, 64, S, mode, p, forced=forced)
                bwd.add((dtype, r, A.bwd_rung(r, 64, S)))
    for S in A.QLIM_SIZES:
        for mode in ("none", "struct"):
            r = A.bwd_route(BF, 64, S, mode, A.P_DROP, A.QLIM)
            assert r == ("v3" if mode == "struct" or S > 208 else {33: "v4x", 97: "v4", 129: "v5", 209: "v3"}.get(S, "v5")), (S, mode, r)
    assert {(BF, "v2", n) for n in (2, 4, 5, 7, 9, 13, 17)} <= fwd
    assert {(d, "v1", n) for n in (2, 5, 7, 9, 13, 17) for d in (F32, BF)} <= fwd
    assert {(d, "v1", n) for n in (2, 5, 7, 9, 13, 17) for d in (F32, BF)} <= bwd
    assert {(BF, "v2", n) for n in (2, 4, 5, 7)} <= bwd
    assert {(BF, "v4x", 4), (BF, "v4x", 8), (BF, "v4", 4), (BF, "v4", 8), (BF, "v4", 16), (BF, "v5", 0)} <= bwd
    assert {(BF, "v3", (sp, 256 if sp <= 128 else 512)) for sp in (64, 128, 192, 256, 320)} <= bwd, sorted(x for x in bwd if x[1] == "v3")
    # the default rule over the whole domain returns nothing the matrix does not reach
    every = {(r, A.bwd_rung(r, 64, S)) for S in range(1, 273) for mode in ("none", "mask", "dense", "struct") for p in (0.0, 0.1)
             for q in (0, 9) for r in [A.bwd_route(BF, 64, S, mode, p, q)]}
    reached = {(r, g) for d, r, g in bwd if d == BF} | {(A.bwd_route(BF, 64, S, m, A.P_DROP, A.QLIM), A.bwd_rung(A.bwd_route(BF, 64, S, m, A.P_DROP, A.QLIM), 64, S))
                                                      for S in A.QLIM_SIZES for m in ("none", "struct")}
    assert every <= reached, sorted(every - reached, key=str)
    # boundaries: both sides of every rung
    for lo in (32, 64, 80, 96, 112, 128, 144, 192, 208, 256):
        assert lo in A.SIZES and lo + 1 in A.SIZES
    # other widths: every route the rule returns for them, and the long path
    for hd in (16, 96, 128):
        got = {A.bwd_route(BF, h, S, m, p) for h, S, m in A.WIDE if h == hd for p in (0.0, A.P_DROP)}
        assert got == {"v1", "v2", "v3"}, (hd, got)
    assert A.bwd_route(BF, 128, 209, "dense") == "long" and A.fwd_route(BF, 128, 209, "dense") == "long"
    assert A.bwd_rung("v3", 128, 256) != A.bwd_rung("v3", 128, 257)
