"""tests/loss_optim_reference.py proves itself without a GPU: at every case of the GPU matrix (tests/test_loss_optim_gpu.py) a
CPU emulation of each kernel's arithmetic — fp32 tensors, the kernel's order of operations, round-to-nearest to half / bf16 where
it rounds — is accepted by the reference, and each named mutant of that arithmetic is rejected at the cases where it can differ
at all (a mutant of the weight decay needs a weight decay, one of the guard needs a guard; the cases that apply are counted and
must exist).  Where a mutant slipped through the inputs were made harder, never the bound wider.

One mutant of the issue's list cannot be rejected by any input: contrastive counters compared with y_i instead of y_j.  The
prediction matrix is symmetric (x_ij and x_ji are the same sum of the same products), so #{pred_ij == y_j} = #{pred_ij == y_i}
identically, and likewise for the positive-correct count; the test runs it and asserts that the counters are the same, and the
oracle comparison pins the counters instead.  The projection applied on a clamped row is told apart by the row of norm 1e-13 (n_i
of norm 0.1, not zero); on the exactly zero row both forms give acc * 1e12.  The finaliser's "scale recomputed" mutant is
FairSeq's clamp(max_norm / (gnorm + 1e-6), max=1) applied always: it differs from the bit copy where
gnorm <= max_norm < gnorm + 1e-6, which the gnorm == max_norm case reaches."""
import numpy as np
import pytest
import torch

import tests.loss_optim_reference as R
from tests.loss_optim_reference import bf16, f32


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_constants_relations():
    for name in ("EXPF", "LOGF", "LOG1PF", "SQRTF", "DIV"):
        measured, rel = getattr(R, name + "_MEASURED"), getattr(R, name + "_REL")
        assert measured > 0, f"{name}_MEASURED: tools/probes/libm_probe.hip has not been run"
        assert rel == max(2.0 * measured, R.U32)
        assert rel < 8 * R.U32, f"{name}: {rel / R.U32:.2f} u is not the accuracy of a precise libm function"
    assert R.U32 == 2.0 ** -24 and R.CHUNK == 4096 and R.SUMSQ_DEPTH == 16 + 6 + 2
    assert R.ADAM_BIG > 8192 * 256 and max(R.chunk_first(R.table_layouts()["many_ones"])) > 65536


# ------------------------------------------------------------------------------------------------ Adam
def emulate_adam(p0, grad, m0, v0, hyp, step, gs=None, guard=None, dtype=f32, mutant=None):
    """adam_kernel in fp32 tensors → (m, v, p (master / fp32 parameter), bf16 parameter or None)."""
    lr, b1, b2, eps, wd = (np.float32(hyp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    t = step - 1 if mutant == "bias_tm1" else step
    ss = R.adam_step_size(hyp["lr"], hyp["beta1"], hyp["beta2"], t)
    if guard is not None:
        if guard["skip"]:
            return m0.clone(), v0.clone(), p0.clone(), (p0.to(bf16) if dtype == bf16 else None)
        gs = guard["scale"]
        if guard["skipped"] and mutant != "ignore_guard_step":
            ss = guard["step_size"]
    gsf = 1.0 if gs is None else R.f32v(gs)
    g_raw = grad.clone()
    if mutant == "sweep_im1":
        first = 8192 * 256
        g_raw[first:] = grad[first - 1:-1]
    g = g_raw * gsf
    if mutant == "wd_in_grad":
        g = g + float(wd) * p0
    omb1, omb2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
    mi = (float(b2) if mutant == "beta2_for_m" else float(b1)) * m0 + omb1 * g
    vi = float(b2) * v0 + ((omb2 * (gsf * g_raw) * g_raw) if mutant == "g2_once" else (omb2 * g * g))
    p = p0.clone()
    if mutant not in ("wd_skipped", "wd_in_grad"):
        p = p - float(wd * lr) * p
    if mutant == "eps_in_sqrt":
        den = torch.sqrt(vi + float(eps))
    elif mutant == "eps_dropped":
        den = torch.sqrt(vi)
    else:
        den = torch.sqrt(vi) + float(eps)
    p = p - (ss * mi) / den
    pb = None
    if dtype == bf16:
        pb = p.to(bf16)
        if mutant == "bf16_pre":
            pb = p0.to(bf16)
        if mutant == "bf16_trunc":
            pb = (p.view(torch.int32) & -65536).view(f32).to(bf16)
    return mi, vi, p, pb


def check_adam(out, ref, what, dtype=f32):
    m, v, p, pb = out
    R.check("adam m", m, ref["m"], what)
    R.check("adam v", v, ref["v"], what)
    R.check("adam p", p, ref["p"], what)
    if dtype == bf16:
        assert torch.equal(pb, p.to(bf16)), f"{what}: the bf16 parameter is not master.to(bfloat16)"


ADAM_MUTANTS = {"eps_in_sqrt": lambda c: True, "eps_dropped": lambda c: True, "g2_once": lambda c: c["gs"] not in (None, 1.0),
                "bias_tm1": lambda c: 2 <= c["step"] <= 3246 and not (c["guard"] and c["guard"]["skipped"]), "wd_in_grad": lambda c: c["hyp"]["wd"] != 0,
                "wd_skipped": lambda c: c["hyp"]["wd"] != 0, "beta2_for_m": lambda c: True,
                "bf16_pre": lambda c: c["dtype"] == bf16, "bf16_trunc": lambda c: c["dtype"] == bf16,
                "ignore_guard_step": lambda c: bool(c["guard"] and c["guard"]["skipped"] and not c["guard"]["skip"]
                                                    and c["guard"]["applied"] != c["step"] and c["step"] <= 3246)}


def _adam_matrix():
    for name, n, hyp, step, gs in R.adam_cases():
        for dtype in (f32, bf16):
            yield dict(name=f"{name}_{dtype}", n=n, hyp=hyp, step=step, gs=gs, guard=None, dtype=dtype)
            for gname, g in R.ADAM_GUARDS:
                yield dict(name=f"{name}_{dtype}_{gname}", n=n, hyp=hyp, step=step, gs=None, guard=R.adam_guard(g, hyp, step), dtype=dtype)


def test_adam_emulation_accepted_and_mutants_rejected():
    hits = {k: 0 for k in ADAM_MUTANTS}
    for c in _adam_matrix():
        p0, grad, m0, v0 = R.adam_inputs(c["n"], R.SEED + c["n"])
        h = c["hyp"]
        ref = R.reference_adam(p0, grad, m0, v0, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], c["step"], c["gs"], c["guard"])
        check_adam(emulate_adam(p0, grad, m0, v0, h, c["step"], c["gs"], c["guard"], c["dtype"]), ref, c["name"], c["dtype"])
        if c["guard"] is not None and c["guard"]["skip"]:
            continue                                            # a skipped update computes nothing: no arithmetic to mutate
        for mut, applies in ADAM_MUTANTS.items():
            if not applies(c) or (c["n"] < 8 and mut not in ("beta2_for_m", "wd_skipped")):
                continue
            hits[mut] += 1
            out = emulate_adam(p0, grad, m0, v0, h, c["step"], c["gs"], c["guard"], c["dtype"], mutant=mut)
            assert rejected(lambda: check_adam(out, ref, c["name"], c["dtype"])), f"{c['name']}: mutant {mut} accepted"
    assert all(v > 0 for v in hits.values()), hits


def test_adam_second_sweep_and_bit_determined_cases():
    n = R.ADAM_BIG                      # adam_kernel's second sweep starts at element 8192 * 256 (optim.hip: the grid-stride loop)
    p0, grad, m0, v0 = R.adam_inputs(n, R.SEED + 1)
    h = R.RECIPE
    ref = R.reference_adam(p0, grad, m0, v0, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], 2, 0.37)
    check_adam(emulate_adam(p0, grad, m0, v0, h, 2, 0.37), ref, "big")
    assert rejected(lambda: check_adam(emulate_adam(p0, grad, m0, v0, h, 2, 0.37, mutant="sweep_im1"), ref, "big"))
    # lr = 0, wd = 0: the parameter keeps its bits (δ = 0), m and v still move; bf16 = RNE of the master at the tie patterns
    p0 = R.tie_masters()
    _, grad, m0, v0 = R.adam_inputs(p0.numel(), R.SEED + 2)
    h0 = dict(R.RECIPE, lr=0.0, wd=0.0)
    ref = R.reference_adam(p0, grad, m0, v0, 0.0, h0["beta1"], h0["beta2"], h0["eps"], 0.0, 3)
    assert bool((ref["p"][1] == 0).all()) and bool((ref["p"][0] == p0.double()).all()) and bool((ref["m"][0] != m0.double()).any())
    out = emulate_adam(p0, grad, m0, v0, h0, 3, dtype=bf16)
    check_adam(out, ref, "lr0", bf16)
    assert torch.equal(out[2], p0)
    for mut in ("bf16_trunc",):
        assert rejected(lambda: check_adam(emulate_adam(p0, grad, m0, v0, h0, 3, dtype=bf16, mutant=mut), ref, "lr0", bf16))
    # grad = 0 with m = v = 0 and wd = 0: every bit determined
    z = torch.zeros(9)
    pz = R.adam_inputs(9, R.SEED + 3)[0]
    hz = dict(R.RECIPE, wd=0.0)
    ref = R.reference_adam(pz, z, z, z, hz["lr"], hz["beta1"], hz["beta2"], hz["eps"], 0.0, 1, 0.37)
    assert all(bool((ref[k][1] == 0).all()) for k in "mvp") and bool((ref["p"][0] == pz.double()).all())
    check_adam(emulate_adam(pz, z, z, z, hz, 1, 0.37), ref, "zero")
    # a skipped update
    g = R.adam_guard(dict(R.ADAM_GUARDS)["skip"], R.RECIPE, 4)
    p0, grad, m0, v0 = R.adam_inputs(300, R.SEED + 4)
    ref = R.reference_adam(p0, grad, m0, v0, *(R.RECIPE[k] for k in ("lr", "beta1", "beta2", "eps", "wd")), 4, None, g)
    assert all(bool((ref[k][1] == 0).all()) for k in "mvp")
    g_live = dict(g, skip=0)
    assert rejected(lambda: check_adam(emulate_adam(p0, grad, m0, v0, R.RECIPE, 4, None, g_live), ref, "skip"))


# ------------------------------------------------------------------------------------------------ sum of squares
def emulate_chunks(x):
    """chunk_sumsq over the fp32 vector x (zero-padded to whole chunks): thread t owns the groups (k 256 + t) 4 .. + 3, adds its
    16 squares in index order, a 6-level tree folds the wave, (w0 + w1) + (w2 + w3)."""
    n = x.numel()
    nc = (n + 4095) // 4096
    buf = torch.zeros(nc * 4096)
    buf[:n] = x
    q = buf.view(nc, 4, 256, 4)                    # [chunk, k, thread, j]
    acc = torch.zeros(nc, 256)
    for k in range(4):
        for j in range(4):
            acc = acc + q[:, k, :, j] * q[:, k, :, j]
    w = acc.view(nc, 4, 64)
    o = 32
    while o:
        w = w[:, :, :o] + w[:, :, o:2 * o]
        o //= 2
    w = w[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def emulate_sumsq(arena, off, n, mutant=None):
    if mutant == "drop_last":
        x = arena[off:off + n].clone()
        x[-1] = 0.0
    elif mutant == "count_after":               # n % 4096 != 0: in a full chunk no thread owns the element after the end
        x = arena[off:off + n + 1]
    elif mutant == "aligned_down":
        x = arena[off & ~3:(off & ~3) + n]
    else:
        x = arena[off:off + n]
    return emulate_chunks(x)


def emulate_sumsq_multi(views, mutant=None):
    """grad_sumsq_multi_kernel over [(arena, off, n)]: partials in chunk order.  ``neighbour``: a tensor's first chunk is
    attributed to the tensor before it (tensor_of_chunk comparing with < instead of <=)."""
    first = R.chunk_first([n for _, _, n in views])
    out = torch.zeros(first[-1])
    for t, (arena, off, n) in enumerate(views):
        if n == 1:
            out[first[t]] = arena[off] * arena[off]            # adding exact zeros does not round
        elif n:
            out[first[t]:first[t + 1]] = emulate_chunks(arena[off:off + n])
    if mutant == "neighbour":
        for t in range(1, min(len(views), 50)):
            if first[t + 1] > first[t]:
                arena, off, n = views[t - 1]
                base = (first[t] - first[t - 1]) * 4096
                out[first[t]] = emulate_chunks(arena[off + base:off + n])[0] if n > base else 0.0
    return out


def check_sumsq(part, ref, what):
    R.check("sumsq partial", part, ref, what)


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
def test_sumsq_emulation_accepted_and_mutants_rejected(integer):
    for n in R.SUMSQ_SIZES:
        for off in R.SUMSQ_OFFSETS:
            a = R.sumsq_arena(n, off, R.SEED + n + off, integer)
            ref = R.reference_sumsq(a[off:off + n])
            if integer:
                assert bool((ref[1] == 0).all())
            check_sumsq(emulate_sumsq(a, off, n), ref, f"n{n} off{off}")
            # one element among random ones can be below the bound, and two small integers can have equal squares: a lost or
            # doubled element is judged on the integer cases (a difference of at least 1 against δ = 0), the start address on both
            muts = (("drop_last", "count_after") if integer else ()) + (("aligned_down",) if off else ())
            for mut in muts:
                if mut == "count_after" and n % 4096 == 0:
                    continue
                assert rejected(lambda: check_sumsq(emulate_sumsq(a, off, n, mut), ref, "")), f"n{n} off{off}: mutant {mut} accepted"


def test_sumsq_multi_tables():
    for name, numels in R.table_layouts().items():
        arena = R.sumsq_inputs(sum(numels) + 8, R.SEED + len(numels), integer=True)
        arena[arena == 0] = 2.0
        views, o = [], 0
        for n in numels:
            views.append((arena, o, n))
            o += n
        ref = R.reference_sumsq_multi([arena[o:o + n] for _, o, n in views])
        check_sumsq(emulate_sumsq_multi(views), ref, name)
        assert rejected(lambda: check_sumsq(emulate_sumsq_multi(views, "neighbour"), ref, name)), f"{name}: neighbour accepted"


# ------------------------------------------------------------------------------------------------ finaliser
def emulate_finalize(partials, s_in, max_norm, lr, b1, b2, step, reset, prev, mutant=None):
    p = partials.double()
    n = p.numel()
    red = [0.0] * 256
    for t in range(256):
        acc = 0.0
        for i in range(t, n, 256):
            acc += float(p[i])
            if mutant == "first_256":
                break
        red[t] = acc
    o = 128
    while o:
        for t in range(o):
            red[t] += red[t + o]
        o //= 2
    s = np.float32(1.0 if s_in is None else s_in)
    with np.errstate(all="ignore"):
        total = np.float64(red[0])
        gnorm = np.float32(np.float64(s) * np.sqrt(total))
        mx = np.float32(max_norm)
        finite = bool(np.isfinite(gnorm))
        clip = finite and mx > 0 and (gnorm >= mx if mutant == "ge" else gnorm > mx)
        clipped = 0 if (reset and mutant != "no_reset") else prev["clipped"]
        skipped = 0 if (reset and mutant != "no_reset") else prev["skipped"]
        scale = s
        if mutant == "recomputed" and finite and mx > 0:        # clamp(max_norm / (gnorm + 1e-6), max = 1) times s_in, always
            scale = np.float32(np.float64(s) * min(1.0, np.float64(mx) / (np.float64(gnorm) + 1e-6)))
        if clip:
            scale = np.float32(np.float64(s) * (np.float64(mx) / (np.float64(gnorm) + (0.0 if mutant == "no_1e-6" else 1e-6))))
    skipped += 0 if finite else 1
    clipped += 1 if clip else 0
    applied = step - (0 if mutant == "applied_attempts" else skipped)
    ss = 0.0
    if skipped > 0 and applied > 0:
        ss = R.adam_step_size(lr, b1, b2, applied)
    f = [float(scale), float(gnorm), ss]
    i = [0, 0, 0, 0 if finite else 1, applied, clipped, skipped, 0]
    return f + [0.0] * 5, i


FIN_MUTANTS = {"first_256": lambda c: c[1].numel() > 256, "ge": lambda c: c[0] == "edge_equal",
               "no_1e-6": lambda c: c[0] in ("edge_below", "edge_equal_scaled"),
               "recomputed": lambda c: c[0] == "edge_equal", "no_reset": lambda c: c[5] == 1 and c[6] is None,
               "applied_attempts": lambda c: c[0] in ("nan", "inf", "keep_counters", "one_skip", "first_update_skipped")}


def test_finalize_emulation_accepted_and_mutants_rejected():
    hits = {k: 0 for k in FIN_MUTANTS}
    h = R.RECIPE
    garbage = dict(clipped=-7, skipped=1 << 20, applied=12345)              # what reset = 1 must not read
    for c in R.finalize_cases():
        name, p, s_in, mx, step, reset, prev = c
        ref = R.reference_finalize(p, s_in, mx, h["lr"], h["beta1"], h["beta2"], step, reset, prev)
        live = prev if prev is not None else garbage
        f, i = emulate_finalize(p, s_in, mx, h["lr"], h["beta1"], h["beta2"], step, reset, live)
        R.check_guard(f, i, ref, name)
        for mut, applies in FIN_MUTANTS.items():
            if applies(c):
                hits[mut] += 1
                f, i = emulate_finalize(p, s_in, mx, h["lr"], h["beta1"], h["beta2"], step, reset, live, mutant=mut)
                assert rejected(lambda: R.check_guard(f, i, ref, name)), f"{name}: mutant {mut} accepted"
    assert all(v > 0 for v in hits.values()), hits
    ref = R.reference_finalize(torch.tensor([9.0, 16.0]), 1.0, 5.0, h["lr"], h["beta1"], h["beta2"], 3, 1)
    assert ref["gnorm"] == (5.0, 0.0) and ref["scale"] == (1.0, 0.0) and ref["clipped"][0] == 0


# ------------------------------------------------------------------------------------------------ node_ce
def _h(x):
    return x.half().float()


def emulate_node_ce(logits, rows, y, w_neg, w_pos, fp16_loss, grad_scale, dl0=None, mutant=None):
    """node_ce_kernel → (loss fp32, counters, dlogits [M, 2] of the logits' type or None).  ``dl0``: the output buffer's start
    content (the entry point zero-fills it before the launch)."""
    T = logits.dtype
    r, yy = rows.long(), y.long()
    n = yy.numel()
    l = logits.float()[r]
    wn, wp = torch.tensor(w_neg, dtype=f32), torch.tensor(w_pos, dtype=f32)
    if fp16_loss or mutant == "logits_half":
        l = _h(l)
    if fp16_loss and mutant != "weight_not_half":
        wn, wp = _h(wn), _h(wp)
    m = l.max(1, keepdim=True).values
    a = l - m
    e = torch.exp(a)
    S = e[:, :1] + e[:, 1:]
    inv = 1.0 / S
    hp = _h(e * inv)
    if fp16_loss:
        ls = _h(torch.log(_h(S)))
        lp = _h(a - ls)
        pred = (hp[:, 1] >= hp[:, 0]) if mutant == "tie_to_1" else (hp[:, 1] > hp[:, 0])
    else:
        lp = a - torch.log(S)
        pred = (hp[:, 1] > hp[:, 0]) if mutant == "pred_half" else (l[:, 1] > l[:, 0])
    pred = pred.long()
    w = torch.where(yy == 1, wp, wn)
    term = w * lp.gather(1, yy[:, None])[:, 0] if n else torch.zeros(0)
    if fp16_loss:
        term = _h(term)
        part = np.zeros(8, dtype=np.float16)
        lg = 0
        while (1 << lg) < n:
            lg += 1
        level_power = max(4, lg // 8)
        lmask = (1 << level_power) - 1
        tv = term.numpy().astype(np.float16)
        for idx in range(n):
            part[0] = np.float16(part[0] - tv[idx])
            for j in range(7):
                if idx & (lmask << (j * level_power)):
                    break
                if mutant == "no_level3" and j + 1 == 3:
                    part[j] = 0
                    continue
                part[j + 1] = np.float16(part[j + 1] + part[j])
                part[j] = 0
        L = np.float16(0)
        for j in range(8):
            L = np.float16(L + part[j])
        loss = float(L)
    else:
        loss = 0.0
        parts = []
        for t in range(256):
            acc = torch.zeros((), dtype=f32)
            for v in term[t::256]:
                acc = acc - v
            parts.append(acc)
        tot = torch.zeros((), dtype=f32)
        for v in parts:
            tot = tot + v
        loss = float(tot)
    counters = [int((pred == yy).sum()), int(((pred == yy) & (pred == 1)).sum()), int((yy == 1).sum()), int((pred == 1).sum())]
    dl = None
    if dl0 is not None:
        dl = dl0.clone() if mutant == "unlabelled_unwritten" else torch.zeros_like(dl0)
        if n:
            onehot = torch.nn.functional.one_hot(yy, 2).float()
            g = w[:, None] * (torch.exp(lp) - onehot)
            if fp16_loss:
                g = _h(g)
            dl[r] = (g * R.f32v(grad_scale)).to(T)
    return loss, counters, dl


def check_node_f32(out, ref, what):
    loss, counters, dl = out
    R.check("node_ce f32 loss", torch.tensor([loss], dtype=f32), ref["loss"], what)
    assert counters == ref["counters"], f"{what}: counters {counters} against {ref['counters']}"
    R.check("node_ce f32 dlogits", dl, ref["dlogits"], what)


def test_node_ce_emulations_accepted_and_mutants_rejected():
    hits = {}
    for nlab, near, dtype, (wn, wp), gs in R.node_matrix():
        l, rows, y = R.node_case_inputs(nlab, near, dtype, R.SEED + nlab)
        what = f"nlab{nlab} {dtype} near{near}"
        nan0 = torch.full(l.shape, float("nan"), dtype=dtype)
        # fp32 path
        ref = R.reference_node_ce_f32(l, rows, y, wn, wp, gs)
        assert ref["margin"] > 0
        check_node_f32(emulate_node_ce(l, rows, y, wn, wp, 0, gs, nan0), ref, what)
        for mut in ("logits_half", "pred_half"):         # a bf16 logit is a half value already: logits_half is the identity there
            if nlab < 255 or (mut == "pred_half" and not near) or (mut == "logits_half" and dtype == bf16):
                continue
            hits[mut] = hits.get(mut, 0) + 1
            out = emulate_node_ce(l, rows, y, wn, wp, 0, gs, nan0, mutant=mut)
            assert rejected(lambda: check_node_f32(out, ref, what)), f"{what}: mutant {mut} accepted"
        # fp16 path
        loss, c, dl = emulate_node_ce(l, rows, y, wn, wp, 1, gs, nan0)
        R.check_node_ce_f16(loss, c, dl, l, rows, y, wn, wp, gs, near, what)
        assert bool((dl.float()[_unlabelled(l, rows)] == 0).all())
        for mut, applies in (("weight_not_half", nlab >= 255), ("no_level3", nlab > 4096), ("tie_to_1", near),
                             ("unlabelled_unwritten", True)):
            if not applies:
                continue
            hits[mut] = hits.get(mut, 0) + 1
            out = emulate_node_ce(l, rows, y, wn, wp, 1, gs, nan0, mutant=mut)
            assert rejected(lambda: (R.check_node_ce_f16(*out, l, rows, y, wn, wp, gs, near, what),
                                     _assert_unlabelled_zero(out[2], l, rows))), f"{what}: mutant {mut} accepted"
    assert set(hits) == {"logits_half", "pred_half", "weight_not_half", "no_level3", "tie_to_1", "unlabelled_unwritten"}, hits


def _unlabelled(l, rows):
    mask = torch.ones(l.shape[0], dtype=torch.bool)
    mask[rows.long()] = False
    return mask


def _assert_unlabelled_zero(dl, l, rows):
    assert bool((dl.float()[_unlabelled(l, rows)] == 0).all()), "d logits of an unlabelled row is not 0"


# ------------------------------------------------------------------------------------------------ contrastive
def emulate_contrastive(emb, ld_view, y, hard, scale, soft_w, adaptive, grad_scale, mutant=None):
    """The four kernels of mdt_contrastive_loss in fp32 tensors → dict(n, inv, extra, G, d_emb, loss, counters).  ``ld_view``:
    the padded buffer [B, ld] the rows live in (``ld_ignored`` reads it at stride D)."""
    T = emb.dtype
    B, D = emb.shape
    E = emb.float()
    if mutant == "ld_ignored":
        E = ld_view.float().reshape(-1)[:B * D].view(B, D)
    sc = R.f32v(scale)
    ss = (E * E).sum(1)
    nrm = torch.sqrt(ss)
    r = 1.0 / torch.clamp(nrm, min=R.f32v(1e-12))
    n = E * r[:, None]
    inv = torch.where(nrm > R.f32v(1e-12), r, torch.full_like(r, -R.f32v(1e12)))
    t = y[:, None] == y[None, :]
    h = hard[:, None] == y[None, :]
    soft = ~t & ~h
    if adaptive:
        extra = ((t | h).sum(1).float() / soft.sum(1).float()) * 2.0
    else:
        extra = torch.full((B,), R.f32v(soft_w))
    w = torch.where(soft, (extra[:, None] if mutant == "extra_i" else extra[None, :]).expand(B, B), torch.ones(B, B))
    eye = torch.eye(B, dtype=torch.bool)
    if mutant != "diag_in_loss":
        w = torch.where(eye, torch.zeros_like(w), w)
    x = (n @ n.t()) * sc
    x = torch.triu(x) + torch.triu(x, 1).t()        # x_ij and x_ji are the same sum in the kernel
    tf = t.float()
    ls = torch.minimum(x, torch.zeros_like(x)) - torch.log1p(torch.exp(-x.abs()))
    e = _h((1.0 - tf) * x)
    e = _h(e - ls)
    e = _h(e * w)
    loss = float(_h(torch.where(w != 0, e, torch.zeros_like(e)).sum()))
    sg = 1.0 / (1.0 + torch.exp(-x))
    wg = torch.where(eye, torch.zeros_like(w), w)
    G = torch.where(wg != 0, (_h(wg) if mutant == "weight_half_bwd" else wg) * (sg - tf), torch.zeros_like(sg))
    pred = torch.round(sg)
    ok = pred == (y[:, None] if mutant == "counters_y_i" else y[None, :])
    counters = [int(ok.sum()), int((ok & (pred == 1)).sum()), int((y == 1).sum()), int((pred == 1).sum())]
    H = G if mutant == "g_ij_only" else G + G.t()
    acc = (H @ n) * sc
    dot = (acc * n).sum(1)
    proj = (acc - n * dot[:, None]) * r[:, None]
    clamped = acc * R.f32v(1e12)
    if mutant == "no_projection":
        proj = acc * r[:, None]
    g = torch.where((inv > 0)[:, None], proj, proj if mutant == "project_clamped" else clamped)
    gsf = 1.0 if mutant == "grad_scale_dropped" else R.f32v(grad_scale)
    return dict(n=n, inv=inv, extra=extra, G=G, d_emb=(g * gsf).to(T), loss=loss, counters=counters)


def check_contrastive(out, ref, what, T):
    for k in ("n", "inv", "extra", "G"):
        R.check("contrastive " + k, out[k], ref[k], what, dtype=f32)
    R.check("contrastive d_emb", out["d_emb"], ref["d_emb"], what, dtype=T, cancels=out["n"].shape[1] == 1)
    assert out["counters"] == ref["counters"], f"{what}: counters {out['counters']} against {ref['counters']}"
    R.check_loss_interval(out["loss"], ref["loss"], what)


def _live(c):
    """The case has a gradient at all: in strict mode (soft weight 0) the one off-diagonal pair of B = 2 is a soft negative."""
    return c["B"] >= 2 and not (c["mode"] == "strict" and c["B"] == 2)


CL_MUTANTS = {"project_clamped": lambda c: c["B"] >= 7 and c["D"] > 1,      # the row of norm 1e-13: n_i is not zero
              "extra_i": lambda c: c["mode"] == "adaptive" and c["B"] >= 7, "g_ij_only": lambda c: _live(c) and c["D"] > 1,          # D = 1: the projection leaves no gradient at all
              "no_projection": _live, "diag_in_loss": lambda c: c["mode"] == "strict" or c["B"] == 7,   # scale 20: a diagonal term is softplus(-20) = 0 in half, and
              # the zero row's ln 2 is below half an ulp of the larger batches' loss
              "weight_half_bwd": lambda c: c["mode"] == "adaptive" and c["B"] >= 7, "ld_ignored": lambda c: c["pad"] > 0 and c["B"] >= 2,
              "grad_scale_dropped": lambda c: c["gs"] != 1.0 and _live(c) and c["D"] > 1}


def padded(emb, pad, fill=0.75):
    B, D = emb.shape
    buf = torch.full((B, D + pad), fill, dtype=emb.dtype)
    buf[:, :D] = emb
    return buf


def test_contrastive_emulation_accepted_oracle_agrees_and_mutants_rejected():
    from oracle import mdt_ref_cpu as O
    hits = {k: 0 for k in CL_MUTANTS}
    for name, B, D, mode, kw, dtype, pad, gs in R.contrastive_cases():
        emb, y, hard = R.contrastive_case_inputs(name, B, D, dtype)
        args = (y, hard, kw["scale"], kw["soft_negative_weight"], kw["adaptive"], gs)
        ref = R.reference_contrastive(emb, *args, knife_limit=R.knife_limit(name))      # refuses a vacuous case itself
        assert ref["knife"] <= R.knife_limit(name)
        if B >= 7:                                                  # the zero row and the tiny one are both decidably clamped
            assert float(ref["inv"][0][B // 2]) < 0 and float(ref["inv"][0][B // 2 - 1]) < 0
            assert bool((ref["n"][0][B // 2] == 0).all()) and 0.09 < float(ref["n"][0][B // 2 - 1].norm()) < 0.11
        # the oracle is the judge of the semantics: its loss lies in the interval, its counters are the reference's
        er = emb.float().clone().requires_grad_(True)
        lo, c = O.contrastive_loss(er, y, hard, kw["scale"], kw["soft_negative_weight"], kw["adaptive"])
        R.check_loss_interval(float(lo), ref["loss"], name + " oracle")
        assert [c[k] for k in ("ncorrect", "positive_correct", "total_positive", "pred_positive")] == ref["counters"], name
        if B > 1:
            lo.backward()
            zero_rows = ref["inv"][0] < 0                          # clamped rows: F.normalize's adjoint is its own matter
            v, d = ref["d_emb"]
            want = (er.grad.double() * R.f32v(gs))[~zero_rows]
            tol = 1e-4 * want.abs().max(1, keepdim=True).values.clamp(min=1e-30) + 4 * d[~zero_rows]
            assert bool(((want - v[~zero_rows]).abs() <= tol).all()), f"{name}: reference gradient against the oracle's autograd"
        buf = padded(emb, pad)
        out = emulate_contrastive(emb, buf, *args)
        check_contrastive(out, ref, name, dtype)
        same = emulate_contrastive(emb, buf, *args, mutant="counters_y_i")            # equivalent by symmetry: demonstrated
        assert same["counters"] == out["counters"], f"{name}: counters against y_i differ from counters against y_j"
        case = dict(mode=mode, B=B, D=D, pad=pad, gs=gs)
        for mut, applies in CL_MUTANTS.items():
            if not applies(case):
                continue
            hits[mut] += 1
            bad = emulate_contrastive(emb, buf, *args, mutant=mut)
            assert rejected(lambda: check_contrastive(bad, ref, name, dtype)), f"{name}: mutant {mut} accepted"
    assert all(v > 0 for v in hits.values()), hits


def test_contrastive_single_row_is_what_the_oracle_gives():
    """B = 1: loss 0, counters 1, 1, [y == 1], 1, zero gradient in every mode."""
    for mode, kw in R.CL_MODES:
        for yv in (0.0, 1.0):
            emb = torch.tensor([[0.3, -1.2, 2.0]])
            y, hard = torch.tensor([yv]), torch.tensor([5.0])
            ref = R.reference_contrastive(emb, y, hard, kw["scale"], kw["soft_negative_weight"], kw["adaptive"])
            assert ref["loss"] == (0.0, 0.0) and ref["counters"] == [int(yv == 1), int(yv == 1), int(yv == 1), 1]
            assert float(ref["d_emb"][0].abs().max()) == 0.0 and float(ref["d_emb"][1].max()) == 0.0


def test_round_half_is_one_rounding():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, 2.0 ** -25, 3 * 2.0 ** -25, -0.1, 0.0,
                      1.0 + 2.0 ** -11 + 2.0 ** -40], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -9, 65504.0, float("inf"), 0.0, 2.0 ** -23, float(torch.tensor(-0.1).half()), 0.0,
                         1.0 + 2.0 ** -10], dtype=torch.float64)
    assert torch.equal(R.round_half(x), want)
