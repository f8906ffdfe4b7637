"""tests/ema_reference.py proves itself without a GPU: at every tensor size and decay of the GPU matrix (tests/test_ema_gpu.py)
faithful fp32 emulations of the `_ema` Adam step — two products and a sum, and both FMA contractions — are accepted by the
reference, and each named mutant is rejected.  The Adam arithmetic is emulate_adam() of tests/test_loss_optim_reference_cpu.py."""
import numpy as np
import pytest
import torch

import tests.ema_reference as E
import tests.loss_optim_reference as R
from tests.loss_optim_reference import bf16, f32
from tests.test_loss_optim_reference_cpu import emulate_adam, rejected

HYP = R.RECIPE
STEP, GS = 3, 0.37
SKIP = R.adam_guard(dict(R.ADAM_GUARDS)["skip"], HYP, STEP)
CLIPPED = R.adam_guard(dict(R.ADAM_GUARDS)["clipped"], HYP, STEP)


def _f32(x):
    return x.to(torch.float64).to(f32)          # one rounding, to nearest even


def emulate_ema(e, p, d, form="plain", mutant=None):
    """The kernel's ``e = d * e + (1.0f - d) * p`` on fp32 tensors.  form: "plain" rounds both products and the sum (three fp32
    operations), "fma_e" is fma(d, e, rn(omd p)), "fma_p" is fma(omd, p, rn(d e)): the fused product is exact in fp64 (24 + 24 bits)."""
    d32 = R.f32v(d)
    omd = E.one_minus(d)
    if mutant == "omd_double":
        omd = float(np.float32(1.0 - float(d)))             # 1 - d formed from the host's double, then rounded
    if mutant == "swapped":
        d32, omd = omd, d32
    if d32 == 0.0 and mutant is None:
        return p.clone()
    if form == "plain":
        return (d32 * e) + (omd * p)                        # torch CPU: separate mul, mul, add kernels — one rounding each
    if form == "fma_e":
        return _f32(d32 * e.double() + (omd * p).double())
    return _f32(omd * p.double() + (d32 * e).double())


def emulate_step(inputs, d, guard=None, gs=GS, dtype=bf16, form="plain", mutant=None):
    """One `_ema` Adam step of one tensor → (m, v, p, bf16 parameter, ema)."""
    p0, grad, m0, v0, e0 = inputs
    m, v, p, pb = emulate_adam(p0, grad, m0, v0, HYP, STEP, None if guard else gs, guard, dtype)
    if guard is not None and guard["skip"] and mutant != "on_skip":
        return m, v, p, pb, e0.clone()
    src = p
    if mutant == "pre_update":
        src = p0
    if mutant == "from_bf16":
        src = p.to(bf16).float()
    e_in = e0
    if mutant == "neighbour":
        e_in = torch.roll(e0, 1)                            # the slot of the table's neighbour: an off-by-one in the pointer array
    return m, v, p, pb, emulate_ema(e_in, src, d, form, mutant if mutant in ("swapped", "omd_double") else None)


def _ref(inputs, d, guard=None, gs=GS):
    p0, grad, m0, v0, e0 = inputs
    return E.reference_adam_ema(p0, grad, m0, v0, e0, HYP, STEP, d, None if guard else gs, guard)


def _cases():
    for n in E.EMA_NUMELS:
        for d in E.EMA_DECAYS:
            yield n, d


def test_emulations_accepted_at_every_case():
    """Both references: chained behind reference_adam (p carries Adam's δ) and from the stored p (the form the GPU test uses)."""
    for n, d in _cases():
        inputs = E.ema_inputs(n, E.SEED + n)
        for guard in (None, CLIPPED, SKIP):
            ref = _ref(inputs, d, guard)
            for form in ("plain", "fma_e", "fma_p"):
                m, v, p, pb, ema = emulate_step(inputs, d, guard, form=form)
                what = f"n{n} d{d} {form} guard {None if guard is None else guard['skip']}"
                E.check(ema, ref["ema"], what)
                stored = E.reference_ema(inputs[4], p, d, skip=bool(guard and guard["skip"]))
                E.check(ema, stored, what + " (stored p)")
                if not (guard and guard["skip"]) and d != 0.0:
                    E.check_not_vacuous(inputs[4], p, stored, what)


def test_exact_cases():
    inputs = E.ema_inputs(4097, E.SEED + 1)
    # d = 0: the copy, bit for bit, -0 included
    m, v, p, pb, ema = emulate_step(inputs, 0.0)
    p[5] = -0.0
    val, dl = E.reference_ema(inputs[4], p, 0.0)
    assert bool((dl == 0).all()) and torch.equal(val.float().view(torch.int32), p.view(torch.int32))
    E.check(emulate_ema(inputs[4], p, 0.0), (val, dl), "d0")
    # a skipped update: the bits of e
    val, dl = E.reference_ema(inputs[4], p, 0.9, skip=True)
    assert bool((dl == 0).all()) and torch.equal(val.float().view(torch.int32), inputs[4].view(torch.int32))
    # p == e: e is met within the bound of ONE update at every decay, and exactly where omd is exact and d e, omd e are too
    for d in E.EMA_DECAYS:
        for form in ("plain", "fma_e", "fma_p"):
            out = emulate_ema(p, p, d, form)
            ref = E.reference_ema(p, p, d)
            E.check(out, ref, f"p == e d{d}")
            err = (out.double() - p.double()).abs()
            assert bool((err <= E.bound(ref[0], ref[1], f32) + (ref[0] - p.double()).abs()).all())
    ones = torch.tensor([1.0, 2.0, -4.0, 0.0])
    assert torch.equal(emulate_ema(ones, ones, 0.5), ones) and bool((E.reference_ema(ones, ones, 0.5)[1] == 0).all())


MUTANTS = ("swapped", "pre_update", "from_bf16", "on_skip", "neighbour", "omd_double")


def test_mutants_rejected():
    assert np.float32(1.0 - 0.9999) != np.float32(1.0) - np.float32(0.9999), "d = 0.9999: the two forms of 1 - d are one number"
    hits = {k: 0 for k in MUTANTS}
    for n, d in _cases():
        if n < 8:
            continue                                      # one element: too few for a neighbour or for the inputs' special slots
        inputs = E.ema_inputs(n, E.SEED + n)
        for mut in MUTANTS:
            guard = SKIP if mut == "on_skip" else None
            if mut == "omd_double" and np.float32(1.0 - d) == np.float32(1.0) - np.float32(d):
                continue                                  # this decay rounds to the same float either way: nothing to tell apart
            if d == 0.0 and mut == "neighbour":
                continue                                  # d = 0 reads no e at all (swapped at d = 0 keeps e instead of copying p)
            hits[mut] += 1
            ref = _ref(inputs, d, guard)
            out = emulate_step(inputs, d, guard, mutant=mut)
            p = out[2]
            stored = E.reference_ema(inputs[4], p, d, skip=guard is not None)
            assert rejected(lambda: E.check(out[4], stored, mut)), f"n{n} d{d}: mutant {mut} accepted by the stored-p reference"
            if mut not in ("pre_update",) or d <= 0.9:    # behind Adam's own δ a 1e-4 share of one small update can hide
                assert rejected(lambda: E.check(out[4], ref["ema"], mut)), f"n{n} d{d}: mutant {mut} accepted by the chained reference"
    assert all(v > 0 for v in hits.values()), hits


def test_vacuous_check_fires():
    """e one fp32 step away from p: the bound (about an ulp) is no narrower than their distance, and the check says so."""
    p = R.adam_inputs(300, E.SEED)[0]
    e = torch.nextafter(p, torch.full_like(p, float("inf")))
    ref = E.reference_ema(e, p, 0.9)
    with pytest.raises(AssertionError, match="vacuous"):
        E.check_not_vacuous(e, p, ref, "neighbours")


def test_recurrence_follows_single_updates():
    """reference_recurrence over a schedule with copies, plain steps and updates accepts the emulation run step by step."""
    gen = torch.Generator().manual_seed(E.SEED)
    e0 = torch.randn(500, generator=gen)
    snaps = [e0 + 0.01 * (k + 1) * torch.randn(500, generator=gen) for k in range(6)]
    decays = [0.0, None, 0.9, None, 0.9, 0.9]
    for form in ("plain", "fma_e", "fma_p"):
        e = e0.clone()
        for p, d in zip(snaps, decays):
            if d is not None:
                e = emulate_ema(e, p, d, form)
        E.check(e, E.reference_recurrence(e0, snaps, decays), f"recurrence {form}")
    wrong = e0.clone()
    for p, d in zip(snaps, decays):
        wrong = emulate_ema(wrong, p, 0.9 if d is None else d)          # updated on the plain steps too
    assert rejected(lambda: E.check(wrong, E.reference_recurrence(e0, snaps, decays), "recurrence"))
