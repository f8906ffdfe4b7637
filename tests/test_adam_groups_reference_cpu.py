"""tests/adam_groups_reference.py proves itself without a GPU: at every case tests/test_adam_groups_gpu.py runs, a CPU emulation of
the group form of adam_multi_kernel — fp32 tensors, the kernel's order of operations, the record looked up per 4096-element chunk
by TENSOR, the two fp32 products the header pins — is accepted by the reference, and each named mutant of that lookup and of that
arithmetic is rejected.  The per-element Adam arithmetic is tests/test_loss_optim_reference_cpu.py's emulate_adam(), as it stands.

Where a mutant can differ at all:
    chunk_index, neighbour       every case that stores something (records differ from tensor to tensor)
    step_only, decay_only,
    decay_twice, wd_global       every case that stores something: the table holds records with lr_scale not in {0, 1} and a decay
                                 that is neither 0 nor the global one
    guard_step_unscaled          the case whose guard has counted skipped updates (after_skips): elsewhere the guard's step size
                                 is not read, and the mutant IS the kernel
    zero_freezes_mv              every case that stores something (the tensor with lr_scale == 0)
A skipped update computes nothing: no mutant applies there.  No mutant had to be left unseparated at a case where it applies; the
first half of every larger tensor carries parameters of 1e1 .. 1e2 beside a small Adam term so that a wrong decay moves them by many
bounds (tests/adam_groups_reference.py: table_inputs)."""
import numpy as np
import pytest
import torch

import tests.adam_groups_reference as A
import tests.loss_optim_reference as R
import tests.test_loss_optim_reference_cpu as C
from tests.loss_optim_reference import bf16, f32

MUTANTS = ("chunk_index", "neighbour", "step_only", "decay_only", "decay_twice", "wd_global", "guard_step_unscaled", "zero_freezes_mv")


def emulate_table(inputs, numels, records, hyp, step, gs=None, guard=None, dtype=f32, mutant=None):
    """The group form of adam_multi_kernel over a table → (m, v, p, bf16 parameter or None), flat."""
    p0, grad, m0, v0 = inputs
    m, v, p = m0.clone(), v0.clone(), p0.clone()
    if guard is not None and guard["skip"]:
        return m, v, p, (p.to(bf16) if dtype == bf16 else None)
    seg = A.segments(numels)
    first = R.chunk_first(list(numels))
    lr = np.float32(hyp["lr"])
    base = np.float32(R.adam_step_size(hyp["lr"], hyp["beta1"], hyp["beta2"], step))
    gbase = np.float32(guard["step_size"]) if guard is not None and guard["skipped"] else base
    for t, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        for chunk in range(first[t], first[t + 1]):
            lo = int(a) + (chunk - first[t]) * A.CHUNK
            hi = min(lo + A.CHUNK, int(b))
            r = {"chunk_index": chunk % len(records), "neighbour": (t + 1) % len(records)}.get(mutant, t)
            scale, wd = (np.float32(x) for x in records[r])
            lr_t, ss_t = lr * scale, gbase * scale                       # the two fp32 products
            if mutant == "step_only":
                lr_t = lr
            elif mutant == "decay_only":
                ss_t = gbase
            elif mutant == "decay_twice":
                lr_t = lr * scale * scale
            elif mutant == "wd_global":
                wd = np.float32(A.GLOBAL_WD)
            elif mutant == "guard_step_unscaled" and guard is not None and guard["skipped"]:
                ss_t = gbase                                             # scaled BEFORE the guard's step size replaced it
            eff = dict(scale=1.0 if gs is None else gs, skip=0, skipped=1, step_size=float(ss_t))
            if guard is not None:
                eff["scale"] = guard["scale"]
            h = dict(hyp, lr=float(lr_t), wd=float(wd))
            mi, vi, pi, _ = C.emulate_adam(p0[lo:hi], grad[lo:hi], m0[lo:hi], v0[lo:hi], h, step, None, eff)
            if mutant == "zero_freezes_mv" and scale == 0:
                mi, vi = m0[lo:hi], v0[lo:hi]
            m[lo:hi], v[lo:hi], p[lo:hi] = mi, vi, pi
    return m, v, p, (p.to(bf16) if dtype == bf16 else None)


def _cases():
    for gname in A.GUARDS:
        for dtype in (f32, bf16):
            yield gname, dtype


def test_emulation_accepted_and_mutants_rejected():
    inputs = A.table_inputs()
    hits = {k: 0 for k in MUTANTS}
    for gname, dtype in _cases():
        guard = A.guard_words(gname)
        gs = A.GS if guard is None else None
        ref = A.reference_table(inputs, A.NUMELS, A.RECORDS, A.HYP, A.STEP, gs, guard)
        what = f"{gname} {dtype}"
        C.check_adam(emulate_table(inputs, A.NUMELS, A.RECORDS, A.HYP, A.STEP, gs, guard, dtype), ref, what, dtype)
        if guard is not None and guard["skip"]:
            assert all(bool((ref[k][1] == 0).all()) for k in "mvp"), "a skipped update keeps every bit"
            continue
        for mut in MUTANTS:
            if mut == "guard_step_unscaled" and not (guard is not None and guard["skipped"]):
                continue
            hits[mut] += 1
            out = emulate_table(inputs, A.NUMELS, A.RECORDS, A.HYP, A.STEP, gs, guard, dtype, mutant=mut)
            assert C.rejected(lambda: C.check_adam(out, ref, what, dtype)), f"{what}: mutant {mut} accepted"
    assert all(n > 0 for n in hits.values()), hits


def test_trivial_records_are_the_plain_reference():
    """lr_scale == 1 and the global decay: lr_t, step_size_t and wd_t are the plain call's numbers, so the reference is
    reference_adam's of the plain entry point — value and δ."""
    inputs = A.table_inputs()
    for gname in A.GUARDS:
        guard = A.guard_words(gname)
        gs = A.GS if guard is None else None
        got = A.reference_table(inputs, A.NUMELS, ((1.0, A.GLOBAL_WD),) * len(A.NUMELS), A.HYP, A.STEP, gs, guard)
        want = R.reference_adam(*inputs, *(A.HYP[k] for k in ("lr", "beta1", "beta2", "eps", "wd")), A.STEP, gs, guard)
        for k in "mvp":
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]), f"{gname} {k}"


def test_zero_scale_keeps_the_parameter_and_moves_the_moments():
    inputs = A.table_inputs()
    seg = A.segments(A.NUMELS)
    a, b = int(seg[A.ZERO_TENSOR]), int(seg[A.ZERO_TENSOR + 1])
    assert A.RECORDS[A.ZERO_TENSOR] == (0.0, 0.0)
    ref = A.reference_table(inputs, A.NUMELS, A.RECORDS, A.HYP, A.STEP, A.GS, None)
    assert bool((ref["p"][1][a:b] == 0).all()) and bool((ref["p"][0][a:b] == inputs[0][a:b].double()).all())
    assert bool((ref["m"][0][a:b] != inputs[2][a:b].double()).any()) and bool((ref["v"][0][a:b] != inputs[3][a:b].double()).any())
    out = emulate_table(inputs, A.NUMELS, A.RECORDS, A.HYP, A.STEP, A.GS, None)
    assert torch.equal(out[2][a:b].view(torch.int32), inputs[0][a:b].view(torch.int32))


def test_matrix_relations():
    assert len(A.RECORDS) == len(A.NUMELS) == len(set(A.RECORDS)) and A.RECORDS[0] == (1.0, A.GLOBAL_WD) and (0.5, 0.0) in A.RECORDS
    first = R.chunk_first(list(A.NUMELS))
    assert first[-1] > len(A.NUMELS), "no tensor owns a second chunk: a chunk-indexed record could not go wrong"
    assert A.BIG_TENSORS > 65536
    lr_t, ss_t = A.group_hyper(A.HYP, A.STEP, 0.37)
    assert lr_t == float(np.float32(A.HYP["lr"]) * np.float32(0.37))
    assert ss_t == float(np.float32(R.adam_step_size(A.HYP["lr"], A.HYP["beta1"], A.HYP["beta2"], A.STEP)) * np.float32(0.37))
    g = A.guard_words("after_skips")
    assert A.group_hyper(A.HYP, A.STEP, 0.37, g)[1] == float(np.float32(g["step_size"]) * np.float32(0.37)) != ss_t
