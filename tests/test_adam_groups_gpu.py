"""The parameter-group forms of the Adam step on the GPU, through the C ABI, against tests/adam_groups_reference.py
(mdt_adam_step_multi_groups, mdt_adam_step_group; include/mdt_hip.h: mdt_adam_group).

Hand-built tables as in tests/test_loss_optim_gpu.py and tests/test_ema_gpu.py (their Carve / AdamRun / EmaRun helpers are used as
they are): every buffer a kernel writes, and the record array it reads, lies between sentinels.  One table holds tensors of 1, 255,
256, 4095, 4096, 4097 and 2 * 4096 + 3 elements, each with its own (lr_scale, weight_decay); a second one has more chunks than the
launch's grid.  The operands are those tests/test_adam_groups_reference_cpu.py proves the bound (and rejects the mutants) at."""
import numpy as np
import pytest
import torch

import tests.adam_groups_reference as A
import tests.ema_reference as E
import tests.loss_optim_reference as R
import tests.test_ema_gpu as T
import tests.test_loss_optim_gpu as G
from multimodaldiscussiontransformer_amd import _lib as L
from tests.loss_optim_reference import bf16, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
HYP, STEP, GS = A.HYP, A.STEP, A.GS
DECAY = 0.9
bits = T.bits


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    before = L.lib.mdt_float_atomic_launches(0)
    yield
    assert L.lib.mdt_float_atomic_launches(0) == before, "a group launch was counted as a float-atomic launch"


def table_inputs_ema(numels=A.NUMELS, seed=A.SEED):
    """table_inputs plus an average per element that is never the parameter (tests/ema_reference.py ema_inputs' recipe)."""
    p0, grad, m0, v0 = A.table_inputs(numels, seed)
    gen = torch.Generator().manual_seed(seed + 77)
    n = p0.numel()
    e0 = p0 * (1.0 + (torch.rand(n, generator=gen) * 0.4 + 0.05) * R._signs(n, gen))
    return p0, grad, m0, v0, e0


class Records:
    """The mdt_adam_group array of a table between sentinels."""

    def __init__(self, records):
        self.host = torch.from_numpy(A.records_array(records).reshape(-1).copy())
        self.c = G.Carve([self.host.numel()], f32)
        self.c.view(0).copy_(self.host)

    def ptr(self):
        return int(self.c.ptrs()[0])

    def intact(self):
        return self.c.untouched() and torch.equal(bits(self.c.view(0).cpu()), bits(self.host))


def hyper_head():
    return [float(HYP[k]) for k in ("lr", "beta1", "beta2", "eps")]


def run_groups(run, recs, gs, guard, ema, step=STEP):
    """mdt_adam_step_multi_groups over ``run``'s table; ``ema``: the decay (run is an EmaRun) or None.  The guard words and the
    records must survive."""
    gc = gbuf = None
    if guard is not None:
        gc, gbuf = G.guard_buffer(guard)
        before = gbuf.clone()
    sc = G.scalar(gs) if guard is None else None
    rec, first, nt, total = run.table()
    rc = L.lib.mdt_adam_step_multi_groups(L.stream(), 0 if run.dtype == f32 else 1, nt, L.ptr(rec), L.ptr(first), total, *hyper_head(), step,
                                          recs.ptr(), L.ptr(sc), L.ptr(gbuf), None if ema is None else L.ptr(run.eptr),
                                          0.0 if ema is None else float(ema))
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)
    assert recs.intact(), "the Adam step wrote the records or a sentinel around them"
    if gc:
        assert torch.equal(gbuf.view(torch.int32), before.view(torch.int32)) and gc.untouched(), "the Adam step wrote the guard"


def run_group_one(run, k, record, gs, guard, ema, step=STEP):
    """mdt_adam_step_group on tensor k of ``run``."""
    gc = gbuf = None
    if guard is not None:
        gc, gbuf = G.guard_buffer(guard)
    sc = G.scalar(gs) if guard is None else None
    rc = L.lib.mdt_adam_step_group(L.stream(), 0 if run.dtype == f32 else 1, *run.one(k), *hyper_head(), step, float(record[0]), float(record[1]),
                                   L.ptr(sc), L.ptr(gbuf), None if ema is None else int(run.e.ptrs()[k]), 0.0 if ema is None else float(ema))
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)


def make_run(numels, inputs, dtype, ema, gap=8):
    return T.EmaRun(numels, inputs, dtype, gap=gap) if ema is not None else G.AdamRun(numels, *inputs[:4], dtype, gap=gap)


def state(run):
    cs = [run.g, run.m, run.v, run.pm, run.pb] + ([run.e] if hasattr(run, "e") else [])
    return [bits(c.flat()) for c in cs if c is not None]


def sentinels_intact(run):
    cs = [run.g, run.m, run.v, run.pm, run.pb] + ([run.e] if hasattr(run, "e") else [])
    return all(c.untouched() for c in cs if c is not None)


@pytest.mark.parametrize("ema", [None, DECAY], ids=["noema", "ema"])
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("gname", list(A.GUARDS))
def test_groups_table_against_reference(gname, dtype, ema):
    """{grad_scale, guard (clipped, after skipped updates, skip)} x {no average, average}, bf16 with masters and fp32 without: every
    tensor under its own record meets reference_adam's bound for (lr_t, step_size_t, wd_t); lr_scale == 0 keeps the parameter's
    bits while m and v move; the single-tensor form gives the table form's bits, tensor by tensor."""
    numels = list(A.NUMELS)
    inputs = table_inputs_ema()
    guard = A.guard_words(gname)
    gs = GS if guard is None else None
    skip = bool(guard and guard["skip"])
    ref = A.reference_table(inputs[:4], numels, A.RECORDS, HYP, STEP, gs, guard)
    recs = Records(A.RECORDS)
    run = make_run(numels, inputs, dtype, ema)
    if skip and run.pb:
        for k in range(len(numels)):
            run.pb.view(k).fill_(7.0)                   # a skipped update does not even refresh the bf16 parameter
    before = state(run)
    run_groups(run, recs, gs, guard, ema)
    what = f"groups {gname} ema {ema}"
    if skip:
        assert all(torch.equal(x, y) for x, y in zip(before, state(run))), f"{what}: a skipped update stored something"
        assert sentinels_intact(run)
        return
    run.check(ref, what)                                # bounds, sentinels, the gradient, bf16 == T(master)
    if ema is not None:
        T.check_ema(run, inputs[4], ema, False, what)
    seg = A.segments(numels)
    a, b = int(seg[A.ZERO_TENSOR]), int(seg[A.ZERO_TENSOR + 1])
    assert torch.equal(bits(run.pm.flat()[a:b]), bits(inputs[0][a:b])), f"{what}: lr_scale == 0 moved the parameter"
    assert not torch.equal(run.m.flat()[a:b], inputs[2][a:b]) and not torch.equal(run.v.flat()[a:b], inputs[3][a:b]), \
        f"{what}: lr_scale == 0 froze the moments"
    # the single-tensor form, tensor by tensor, on a fresh copy: the table form's bits in every output, the neighbours untouched
    one = make_run(numels, inputs, dtype, ema)
    for k in range(len(numels)):
        run_group_one(one, k, A.RECORDS[k], gs, guard, ema)
    assert sentinels_intact(one), f"{what}: the single form overwrote a sentinel"
    assert all(torch.equal(x, y) for x, y in zip(state(one), state(run))), f"{what}: the single form differs from the table form"


PLAIN = {(False, False): "mdt_adam_step_multi", (True, False): "mdt_adam_step_multi_guarded", (False, True): "mdt_adam_step_multi_ema",
         (True, True): "mdt_adam_step_multi_ema_guarded"}


@pytest.mark.parametrize("ema", [None, DECAY], ids=["noema", "ema"])
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("gname", ["unguarded", "clipped", "after_skips"])
def test_trivial_records_equal_the_plain_entry_points(gname, dtype, ema):
    """Every record (1, global weight decay): the bits of the four existing multi-tensor entry points, in every output."""
    numels = list(A.NUMELS)
    inputs = table_inputs_ema()
    guard = A.guard_words(gname)
    gs = GS if guard is None else None
    run = make_run(numels, inputs, dtype, ema)
    run_groups(run, Records(((1.0, A.GLOBAL_WD),) * len(numels)), gs, guard, ema)
    plain = make_run(numels, inputs, dtype, ema)
    gbuf = G.guard_buffer(guard)[1] if guard is not None else None
    rec, first, nt, total = plain.table()
    tail = () if ema is None else (L.ptr(plain.eptr), float(ema))
    fn = getattr(L.lib, PLAIN[(guard is not None, ema is not None)])
    rc = fn(L.stream(), 0 if dtype == f32 else 1, nt, L.ptr(rec), L.ptr(first), total, *hyper_head(), float(A.GLOBAL_WD), STEP,
            L.ptr(gbuf) if guard is not None else L.ptr(G.scalar(gs)), *tail)
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)
    assert all(torch.equal(x, y) for x, y in zip(state(run), state(plain))), f"{gname}: trivial records differ from the plain entry point"


def test_scaled_guard_step_size_is_used():
    """Guard words written by the test: two updates skipped before, step_size that of ONE applied update.  The scaled guard step
    size is what the kernel uses (the reference is built from it), and it is told apart from the scaled host step size: the two
    differ by more than the bound on most elements."""
    numels = list(A.NUMELS)
    inputs = A.table_inputs()
    guard = A.guard_words("after_skips")
    assert guard["skipped"] == 2 and guard["step_size"] != R.adam_step_size(HYP["lr"], HYP["beta1"], HYP["beta2"], STEP)
    run = G.AdamRun(numels, *inputs, f32)
    run_groups(run, Records(A.RECORDS), None, guard, None)
    run.check(A.reference_table(inputs, numels, A.RECORDS, HYP, STEP, None, guard), "after_skips")
    host = A.reference_table(inputs, numels, A.RECORDS, HYP, STEP, None, dict(guard, skipped=0))
    with pytest.raises(AssertionError):
        R.check("adam p (host step size)", run.pm.flat(), host["p"], "after_skips against the host's step size")
    R.WORST.pop("adam p (host step size)", None)


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
def test_more_chunks_than_the_grid(dtype):
    """65 540 one-element tensors with alternating records: total_chunks > 65 536, so blocks 0 .. 3 take a second chunk in the
    grid-stride loop and must look up that chunk's TENSOR record (the chunk-loop case of tests/test_loss_optim_gpu.py, rebuilt
    with records)."""
    numels = [1] * A.BIG_TENSORS
    records = [A.BIG_RECORDS[k % 2] for k in range(A.BIG_TENSORS)]
    records[-1] = records[-2] = (0.043, 0.3)            # the chunks past the grid (65 536 ..) carry records of their own
    records[-3] = records[-4] = (0.81, 0.02)
    inputs = table_inputs_ema(numels, A.SEED + 3)
    inputs[0][-8:] = torch.tensor([50.0, -60.0, 70.0, -80.0, 90.0, -15.0, 25.0, -35.0])     # a decay that shows in the tail
    run = T.EmaRun(numels, inputs, dtype, gap=0)
    run_groups(run, Records(records), GS, None, DECAY)
    what = "many_ones"
    run.check(A.reference_table(inputs[:4], numels, records, HYP, STEP, GS, None), what)
    assert run.e.untouched()
    T.check_ema(run, inputs[4], DECAY, False, what)


def test_refusals_write_nothing():
    """Both grad_scale and guard, a NULL record array, a non-finite or negative lr_scale / weight_decay handed to the single form,
    an unknown dtype: an error code, a message, and no store."""
    n = 300
    inputs = E.ema_inputs(n, E.SEED + 7)
    run = T.EmaRun([n], inputs, f32)
    before = run.state()
    rec, first, nt, total = run.table()
    recs = Records(((0.5, 0.0),))
    h = hyper_head()
    sc = G.scalar(0.37)
    _, gbuf = G.guard_buffer(A.guard_words("clipped"))
    e = int(run.e.ptrs()[0])
    multi = lambda *tail: L.lib.mdt_adam_step_multi_groups(L.stream(), 0, nt, L.ptr(rec), L.ptr(first), total, *h, STEP, *tail)  # noqa: E731
    one = lambda *tail: L.lib.mdt_adam_step_group(L.stream(), 0, *run.one(), *h, STEP, *tail)                                       # noqa: E731
    calls = [("both", lambda: multi(recs.ptr(), L.ptr(sc), L.ptr(gbuf), None, 0.0)),
             ("groups_dev NULL", lambda: multi(None, L.ptr(sc), None, None, 0.0)),
             ("ema decay", lambda: multi(recs.ptr(), None, None, L.ptr(run.eptr), 1.5)),
             ("one both", lambda: one(0.5, 0.0, L.ptr(sc), L.ptr(gbuf), None, 0.0)),
             ("one scale < 0", lambda: one(-0.5, 0.0, None, None, None, 0.0)),
             ("one scale nan", lambda: one(float("nan"), 0.0, None, None, None, 0.0)),
             ("one scale inf", lambda: one(float("inf"), 0.0, None, None, None, 0.0)),
             ("one wd < 0", lambda: one(0.5, -0.01, None, None, None, 0.0)),
             ("one wd nan", lambda: one(0.5, float("nan"), None, None, None, 0.0)),
             ("one ema decay", lambda: one(0.5, 0.0, None, None, e, -0.1)),
             ("dtype", lambda: L.lib.mdt_adam_step_multi_groups(L.stream(), 2, nt, L.ptr(rec), L.ptr(first), total, *h, STEP, recs.ptr(),
                                                                None, None, None, 0.0))]
    for name, call in calls:
        rc = call()
        msg = L.lib.mdt_last_error_string().decode()
        assert rc in (-1, -2) and msg, f"{name}: status {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, run.state()))
    for c in run.carves():
        assert c.untouched()
    assert L.lib.mdt_abi_version() == 1
