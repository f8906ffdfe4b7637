"""The `_ema` forms of the Adam step and mdt_ema_swap_multi on the GPU, through the C ABI, against tests/ema_reference.py.

Hand-built tables as in tests/test_loss_optim_gpu.py (its Carve / AdamRun helpers are used as they are): every buffer a kernel
writes lies between sentinels, the averages in an arena of their own.  One table holds tensors of 1, 4095, 4096, 4097 and
3 * 4096 + 5 elements (five levels of the binary search, full chunks and chunk tails); one EMA view starts 4 bytes past a 16-byte
boundary (the element-by-element form of the swap), one EMA entry in the middle of the table is NULL.  A second table has more
chunks than the launch's grid.  The operands are those tests/test_ema_reference_cpu.py proves the bound at."""
import numpy as np
import pytest
import torch

import tests.ema_reference as E
import tests.loss_optim_reference as R
import tests.test_loss_optim_gpu as G
from multimodaldiscussiontransformer_amd import _lib as L
from tests.loss_optim_reference import bf16, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
HYP = R.RECIPE
STEP, GS = 3, 0.37
GUARDS = {"unguarded": None, "clipped": dict(R.ADAM_GUARDS)["clipped"], "after_skips": dict(R.ADAM_GUARDS)["after_skips"],
          "skip": dict(R.ADAM_GUARDS)["skip"]}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"
    before = L.lib.mdt_float_atomic_launches(0)
    yield
    assert L.lib.mdt_float_atomic_launches(0) == before, "an EMA launch was counted as a float-atomic launch"


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


class EmaRun(G.AdamRun):
    """AdamRun plus the averages: tensor k's average between sentinels, the views of the tensors in ``offset`` moved one element
    (4 bytes) off their 16-byte boundaries, ``null``'s entry of the pointer array NULL (its slot exists and must keep its bits)."""

    def __init__(self, numels, inputs, dtype, null=None, offset=(), gap=8):
        p0, grad, m0, v0, e0 = inputs
        super().__init__(numels, p0, grad, m0, v0, dtype, gap=gap)
        self.e = G.Carve(numels, f32, gap, None if gap else 1)
        for k in offset:
            self.e.start[k] += 1                           # into its own trailing gap: 7 sentinels are left behind it
        self.e.fill_flat(e0)
        self.null = null
        ptrs = np.asarray(self.e.ptrs(), dtype=np.int64).copy()
        assert all(ptrs[k] % 16 == (4 if k in offset else 0) for k in range(len(numels))) or gap == 0
        if null is not None:
            ptrs[null] = 0
        self.eptr = torch.from_numpy(ptrs).to(DEV)
        seg = np.concatenate([[0], np.cumsum(numels)])
        self.live = torch.ones(int(seg[-1]), dtype=torch.bool)
        if null is not None:
            self.live[int(seg[null]):int(seg[null + 1])] = False

    def carves(self):
        return [c for c in (self.g, self.m, self.v, self.pm, self.pb, self.e) if c is not None]

    def state(self):
        return [bits(c.flat()) for c in self.carves()]


def run_ema(entry, run, d, gs, guard, k=0):
    """entry "multi" / "one" (tensor k) / with "_guarded"; the guard words must survive."""
    h = [float(HYP[x]) for x in G.HYP]
    dt = 0 if run.dtype == f32 else 1
    gc = None
    if entry.endswith("guarded"):
        gc, gbuf = G.guard_buffer(guard)
        before = gbuf.clone()
        last = L.ptr(gbuf)
    else:
        sc = G.scalar(gs)
        last = L.ptr(sc)
    if entry.startswith("multi"):
        rec, first, nt, total = run.table()
        fn = L.lib.mdt_adam_step_multi_ema_guarded if gc else L.lib.mdt_adam_step_multi_ema
        rc = fn(L.stream(), dt, nt, L.ptr(rec), L.ptr(first), total, *h, STEP, last, L.ptr(run.eptr), float(d))
    else:
        fn = L.lib.mdt_adam_step_ema_guarded if gc else L.lib.mdt_adam_step_ema
        rc = fn(L.stream(), dt, *run.one(k), *h, STEP, last, int(run.e.ptrs()[k]), float(d))
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)
    if gc:
        assert torch.equal(gbuf.view(torch.int32), before.view(torch.int32)) and gc.untouched(), "the Adam step wrote the guard"


def check_ema(run, e0, d, skip, what):
    """The averages against the reference fed with the STORED fp32 weights; a NULL entry's slot and a skipped update keep e0's bits."""
    assert run.e.untouched(), f"{what}: a sentinel around an average was overwritten"
    got = run.e.flat()
    p = run.pm.flat()
    val, dl = E.reference_ema(e0, p, d, skip=skip)
    val = torch.where(run.live, val, e0.double())
    dl = torch.where(run.live, dl, torch.zeros_like(dl))
    E.check(got, (val, dl), what)
    if skip or d == 0.0:
        want = e0 if skip else torch.where(run.live, p, e0)
        assert torch.equal(bits(got), bits(want)), f"{what}: the average is not bit-exact"
    elif int(run.live.sum()) > 8:
        assert not torch.equal(got[run.live], e0[run.live]), f"{what}: the average did not move"


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("gname", list(GUARDS))
def test_adam_ema_table(gname, dtype):
    """The five-tensor table through the multi-tensor form at every decay: Adam's outputs carry the bits of the plain entry point,
    the averages meet the reference (exactly at d = 0 and on a skipped update, where NOTHING of the table is stored)."""
    numels = list(E.EMA_NUMELS)
    inputs = E.ema_inputs(sum(numels), E.SEED)
    guard = None if GUARDS[gname] is None else R.adam_guard(GUARDS[gname], HYP, STEP)
    entry = "multi" if guard is None else "multi_guarded"
    gs = GS if guard is None else None
    plain = G.AdamRun(numels, *inputs[:4], dtype)
    G.run_adam(entry, plain, HYP, STEP, gs, guard)
    ref = R.reference_adam(*inputs[:4], *(HYP[k] for k in G.HYP), STEP, gs, guard)
    skip = bool(guard and guard["skip"])
    for d in E.EMA_DECAYS:
        run = EmaRun(numels, inputs, dtype, null=E.EMA_NULL, offset=(E.EMA_OFFSET,))
        before = run.state()
        run_ema(entry, run, d, gs, guard)
        what = f"{gname} d{d}"
        run.check(ref, what)                                                  # bounds, sentinels, the gradient, bf16 == T(master)
        for a, b in ((run.pm, plain.pm), (run.m, plain.m), (run.v, plain.v), (run.pb, plain.pb)):
            assert a is None or torch.equal(bits(a.flat()), bits(b.flat())), f"{what}: not the bits of the plain entry point"
        check_ema(run, inputs[4], d, skip, what)
        if skip:
            assert all(torch.equal(x, y) for x, y in zip(before, run.state())), f"{what}: a skipped update stored something"


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("entry", ["one", "one_guarded"])
def test_adam_ema_single_tensor(entry, dtype):
    """The single-tensor form on the 4097-element tensor (a second block, a tail) with the average at a 4-byte offset."""
    n = 4097
    inputs = E.ema_inputs(n, E.SEED + n)
    for gname in (("unguarded",) if entry == "one" else ("clipped", "skip")):
        guard = None if GUARDS[gname] is None else R.adam_guard(GUARDS[gname], HYP, STEP)
        gs = GS if guard is None else None
        plain = G.AdamRun([n], *inputs[:4], dtype)
        G.run_adam(entry, plain, HYP, STEP, gs, guard)
        ref = R.reference_adam(*inputs[:4], *(HYP[k] for k in G.HYP), STEP, gs, guard)
        for d in (0.9, 0.0):
            run = EmaRun([n, 8], tuple(torch.cat([x, x[:8]]) for x in inputs), dtype, offset=(0,))
            before = run.state()
            run_ema(entry, run, d, gs, guard, k=0)
            what = f"{entry} {gname} d{d}"
            sl = slice(0, n)
            for a, b in ((run.pm, plain.pm), (run.m, plain.m), (run.v, plain.v), (run.pb, plain.pb)):
                assert a is None or torch.equal(bits(a.flat()[sl]), bits(b.flat())), f"{what}: not the bits of the plain entry point"
            R.check("adam p", run.pm.flat()[sl], ref["p"], what)
            run.live[n:] = False                                              # tensor 1 was not part of the call
            check_ema(run, torch.cat([inputs[4], inputs[4][:8]]), d, bool(guard and guard["skip"]), what)
            for c in run.carves():
                assert c.untouched(), f"{what}: a sentinel was overwritten"
            after = run.state()
            assert all(torch.equal(x[n:], y[n:]) for x, y in zip(before, after)), f"{what}: the neighbouring tensor was written"
            if guard and guard["skip"]:
                assert all(torch.equal(x, y) for x, y in zip(before, after))


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
def test_adam_ema_more_chunks_than_the_grid(dtype):
    """65 540 one-element tensors in one arena: total_chunks > 65 536, blocks 0 .. 3 take a second chunk and its EMA pointer."""
    numels = [1] * E.EMA_BIG_TENSORS
    inputs = E.ema_inputs(len(numels), E.SEED + 3)
    plain = G.AdamRun(numels, *inputs[:4], dtype, gap=0)
    G.run_adam("multi", plain, HYP, STEP, GS, None)
    run = EmaRun(numels, inputs, dtype, null=len(numels) - 2, gap=0)
    run_ema("multi", run, 0.9, GS, None)
    for a, b in ((run.pm, plain.pm), (run.m, plain.m), (run.v, plain.v), (run.pb, plain.pb)):
        assert a is None or torch.equal(bits(a.flat()), bits(b.flat()))
    for c in run.carves():
        assert c.untouched()
    check_ema(run, inputs[4], 0.9, False, "many_ones")


def swap(run, restore):
    rec, first, nt, total = run.table()
    rc = L.lib.mdt_ema_swap_multi(L.stream(), 0 if run.dtype == f32 else 1, nt, L.ptr(rec), L.ptr(run.eptr), L.ptr(first), total, restore)
    torch.cuda.synchronize()
    assert rc == 0, G.status(rc)


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", ["five", "many_ones"])
def test_swap(layout, dtype):
    """restore = 0 puts T(ema) into the parameter (bf16, with a master) or trades parameter and average (fp32, without);
    restore = 1 gives every bit back.  master, m, v, the gradient, the NULL entry's tensor and every sentinel stay."""
    many = layout == "many_ones"
    numels = [1] * E.EMA_BIG_TENSORS if many else list(E.EMA_NUMELS)
    inputs = E.ema_inputs(len(numels) if many else sum(numels), E.SEED + 5)
    run = EmaRun(numels, inputs, dtype, null=len(numels) - 2 if many else E.EMA_NULL, offset=() if many else (E.EMA_OFFSET,),
                 gap=0 if many else 8)
    if dtype == bf16:
        run.pb.fill_flat(inputs[0])                     # the invariant the Adam step keeps: param == T(master)
    e0, live = inputs[4], run.live
    start = run.state()
    prm = run.pb if run.pb else run.pm
    p_start = prm.flat()
    swap(run, 0)
    for c in run.carves():
        assert c.untouched(), "restore = 0: a sentinel was overwritten"
    keep = [run.g, run.m, run.v] + ([run.pm, run.e] if run.pb else [])
    mid = {id(c): bits(c.flat()) for c in keep}
    for c, s in zip(run.carves(), start):
        if any(c is k for k in keep):
            assert torch.equal(mid[id(c)], s), "restore = 0 wrote a tensor it must not touch"
    want = torch.where(live, e0.to(dtype), p_start)
    assert torch.equal(bits(prm.flat()), bits(want)), "restore = 0: the parameter is not T(ema)"
    if not run.pb:
        assert torch.equal(bits(run.e.flat()), bits(torch.where(live, p_start, e0))), "restore = 0: the average does not hold the raw weights"
    swap(run, 1)
    for c in run.carves():
        assert c.untouched(), "restore = 1: a sentinel was overwritten"
    assert all(torch.equal(x, y) for x, y in zip(start, run.state())), "restore = 1 did not give every bit back"


def test_refusals_write_nothing():
    """A decay outside [0, 1], a NULL average (single form) or pointer array (table forms), restore = 2: an error code and no store."""
    n = 300
    inputs = E.ema_inputs(n, E.SEED + 7)
    h = [float(HYP[x]) for x in G.HYP]
    run = EmaRun([n], inputs, f32)
    before = run.state()
    rec, first, nt, total = run.table()
    e = int(run.e.ptrs()[0])
    rcs = [L.lib.mdt_adam_step_ema(L.stream(), 0, *run.one(), *h, STEP, None, e, 1.5),
           L.lib.mdt_adam_step_ema(L.stream(), 0, *run.one(), *h, STEP, None, e, -0.1),
           L.lib.mdt_adam_step_ema(L.stream(), 0, *run.one(), *h, STEP, None, e, float("nan")),
           L.lib.mdt_adam_step_ema(L.stream(), 0, *run.one(), *h, STEP, None, None, 0.9),
           L.lib.mdt_adam_step_ema_guarded(L.stream(), 0, *run.one(), *h, STEP, None, e, 0.9),
           L.lib.mdt_adam_step_multi_ema(L.stream(), 0, nt, L.ptr(rec), L.ptr(first), total, *h, STEP, None, None, 0.9),
           L.lib.mdt_adam_step_multi_ema(L.stream(), 0, nt, L.ptr(rec), L.ptr(first), total, *h, STEP, None, L.ptr(run.eptr), 2.0),
           L.lib.mdt_adam_step_multi_ema_guarded(L.stream(), 0, nt, L.ptr(rec), L.ptr(first), total, *h, STEP, None, L.ptr(run.eptr), 0.9),
           L.lib.mdt_ema_swap_multi(L.stream(), 0, nt, L.ptr(rec), L.ptr(run.eptr), L.ptr(first), total, 2),
           L.lib.mdt_ema_swap_multi(L.stream(), 0, nt, L.ptr(rec), None, L.ptr(first), total, 0),
           L.lib.mdt_ema_swap_multi(L.stream(), 2, nt, L.ptr(rec), L.ptr(run.eptr), L.ptr(first), total, 0)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    assert all(torch.equal(x, y) for x, y in zip(before, run.state()))
    for c in run.carves():
        assert c.untouched()
