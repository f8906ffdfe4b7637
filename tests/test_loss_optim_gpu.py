"""The tail of the training step on the GPU against tests/loss_optim_reference.py: the four Adam entry points, the two sum-of-squares
kernels and the norm finaliser (csrc/optim.hip), mdt_node_ce (csrc/rowops.hip) and mdt_contrastive_loss (csrc/contrastive.hip).

The C ABI is called directly so that nothing is hidden: hand-built tensor tables, guard words written by the test, NULL outputs,
row strides, pre-filled outputs.  Every buffer a kernel writes is carved out of a sentinel-filled allocation with gaps around
every tensor, and every sentinel must survive.  The operands are those tests/test_loss_optim_reference_cpu.py proves the bounds
(and rejects the mutants) at; every case is small.

Not reached: the grid cap of the single-tensor sum of squares (grad_sumsq_kernel loops only beyond 65 536 chunks = 268 M
elements, 1 GiB of gradient), out of reach of a small test; the same loop in the table form is run by the 65 540-tensor table."""
import numpy as np
import pytest
import torch

import tests.loss_optim_reference as R
from multimodaldiscussiontransformer_amd import _lib as L
from tests.loss_optim_reference import bf16, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
_BITS = {f32: (torch.int32, 0x7FA5A5A5), bf16: (torch.int16, 0x7FA5), torch.int32: (torch.int32, 0x5A5A5A5A)}
HYP = ("lr", "beta1", "beta2", "eps", "wd")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a device"


class Carve:
    """Tensors of one type carved out of ONE sentinel-filled device buffer: tensor k starts ``gap`` elements after the end of
    tensor k - 1, rounded up to ``align`` elements (16 bytes), and ``gap`` sentinel elements close the buffer."""

    def __init__(self, numels, dtype, gap=8, align=None):
        self.itype, self.bits = _BITS[dtype]
        align = align or 16 // torch.empty(0, dtype=dtype).element_size()
        n = np.asarray(numels, dtype=np.int64)
        start = np.zeros(len(n), dtype=np.int64)
        pos = gap
        if gap == 0 and align == 1:
            start = np.concatenate([[0], np.cumsum(n)[:-1]]) if len(n) else start
            pos = int(n.sum())
        else:
            for k in range(len(n)):
                pos = (pos + align - 1) // align * align
                start[k] = pos
                pos += int(n[k]) + gap
        self.start, self.numels, self.esize = start, n, torch.empty(0, dtype=dtype).element_size()
        self.buf = torch.empty(pos + 8, dtype=dtype, device=DEV)
        self.buf.view(self.itype).fill_(self.bits)

    def view(self, k):
        return self.buf[int(self.start[k]):int(self.start[k] + self.numels[k])]

    def fill(self, tensors):
        for k, t in enumerate(tensors):
            if t.numel():
                self.view(k).copy_(t.view(-1))
        return self

    def fill_flat(self, flat):
        """Tensor k = the next numels[k] elements of ``flat`` (host)."""
        idx = np.concatenate([np.arange(s, s + n) for s, n in zip(self.start, self.numels)]) if len(self.numels) < 1000 else \
            (np.repeat(self.start - np.concatenate([[0], np.cumsum(self.numels)[:-1]]), self.numels) + np.arange(int(self.numels.sum())))
        self.idx = torch.from_numpy(idx).to(DEV)
        self.buf[self.idx] = flat.to(DEV).to(self.buf.dtype)
        return self

    def flat(self):
        return self.buf[self.idx].cpu()

    def ptrs(self):
        return self.buf.data_ptr() + self.start * self.esize

    def untouched(self):
        own = torch.zeros(self.buf.numel(), dtype=torch.bool)
        if hasattr(self, "idx"):
            own[self.idx.cpu()] = True
        else:
            for s, n in zip(self.start, self.numels):
                own[int(s):int(s + n)] = True
        return bool((self.buf.view(self.itype).cpu()[~own] == self.bits).all())


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=f32, device=DEV)


def guard_buffer(words=None):
    """An mdt_adam_guard (8 words) inside a sentinel-filled buffer: (carve, fp32 view).  ``words``: dict to start from, None: NaN."""
    c = Carve([8], f32)
    g = c.view(0)
    if words is None:
        g.fill_(float("nan"))
    else:
        g[:3] = torch.tensor([words.get("scale", 0.0), words.get("gnorm", 0.0), words.get("step_size", 0.0)], dtype=f32)
        g.view(torch.int32)[3:] = torch.tensor([words.get("skip", 0), words.get("applied", 0), words.get("clipped", 0),
                                                words.get("skipped", 0), 0], dtype=torch.int32)
    return c, g


def status(rc):
    return rc, L.lib.mdt_last_error_string().decode()


# ------------------------------------------------------------------------------------------------ Adam
class AdamRun:
    """One set of tensors (a table of ``numels``) on the device for one Adam call, every tensor between sentinels."""

    def __init__(self, numels, p0, grad, m0, v0, dtype, gap=8):
        align = None if gap else 1
        self.dtype, self.numels = dtype, numels
        self.g = Carve(numels, f32, gap, align).fill_flat(grad)
        self.m = Carve(numels, f32, gap, align).fill_flat(m0)
        self.v = Carve(numels, f32, gap, align).fill_flat(v0)
        self.pm = Carve(numels, f32, gap, align).fill_flat(p0)            # the fp32 parameter, or the master
        self.pb = Carve(numels, bf16, gap, align).fill_flat(p0) if dtype == bf16 else None
        self.grad0 = self.g.flat()

    def table(self):
        nt = len(self.numels)
        rec = np.zeros((nt, 6), dtype=np.int64)
        rec[:, 0] = (self.pb if self.pb else self.pm).ptrs()
        rec[:, 1] = self.pm.ptrs() if self.pb else 0
        rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5] = self.g.ptrs(), self.m.ptrs(), self.v.ptrs(), self.numels
        first = np.asarray(R.chunk_first(list(self.numels)), dtype=np.int64)
        return torch.from_numpy(rec).to(DEV), torch.from_numpy(first).to(DEV), nt, int(first[-1])

    def one(self, k=0):
        """(n, param, master, grad, m, v) pointers of tensor k for the per-tensor entry points."""
        prm = (self.pb if self.pb else self.pm)
        return (int(self.numels[k]), int(prm.ptrs()[k]), int(self.pm.ptrs()[k]) if self.pb else None, int(self.g.ptrs()[k]),
                int(self.m.ptrs()[k]), int(self.v.ptrs()[k]))

    def check(self, ref, what):
        R.check("adam m", self.m.flat(), ref["m"], what)
        R.check("adam v", self.v.flat(), ref["v"], what)
        R.check("adam p", self.pm.flat(), ref["p"], what)
        assert torch.equal(self.g.flat(), self.grad0), f"{what}: the gradient was written"
        for c in (self.g, self.m, self.v, self.pm, self.pb):
            assert c is None or c.untouched(), f"{what}: a sentinel around a tensor was overwritten"
        if self.pb:
            assert torch.equal(self.pb.flat(), self.pm.flat().to(bf16)), f"{what}: the bf16 parameter is not master.to(bfloat16)"


def run_adam(entry, run, hyp, step, gs, guard):
    h = [float(hyp[k]) for k in HYP]
    dt = 0 if run.dtype == f32 else 1
    gc = None
    if entry.endswith("guarded"):
        gc, gbuf = guard_buffer(guard)
        before = gbuf.clone()
        last = L.ptr(gbuf)
    else:
        sc = scalar(gs)
        last = L.ptr(sc)
    if entry.startswith("multi"):
        rec, first, nt, total = run.table()
        fn = L.lib.mdt_adam_step_multi_guarded if gc else L.lib.mdt_adam_step_multi
        rc = fn(L.stream(), dt, nt, L.ptr(rec), L.ptr(first), total, *h, step, last)
    else:
        fn = L.lib.mdt_adam_step_guarded if gc else L.lib.mdt_adam_step
        rc = fn(L.stream(), dt, *run.one(), *h, step, last)
    torch.cuda.synchronize()
    assert rc == 0, status(rc)
    if gc:
        assert torch.equal(gbuf.view(torch.int32), before.view(torch.int32)) and gc.untouched(), "the Adam step wrote the guard"


ENTRIES = ("one", "multi", "one_guarded", "multi_guarded")


def _adam_reference(inputs, hyp, step, gs, guard):
    return R.reference_adam(*inputs, *(hyp[k] for k in HYP), step, gs, guard)


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", R.adam_cases(), ids=lambda c: c[0])
def test_adam_entry_points(case, dtype):
    name, n, hyp, step, gs = case
    inputs = R.adam_inputs(n, R.SEED + n)
    refs = {None: _adam_reference(inputs, hyp, step, gs, None)}
    for entry in ENTRIES:
        guards = [None] if not entry.endswith("guarded") else [R.adam_guard(g, hyp, step) for _, g in R.ADAM_GUARDS]
        for k, guard in enumerate(guards):
            ref = refs[None] if guard is None else _adam_reference(inputs, hyp, step, None, guard)
            run = AdamRun([n], *inputs, dtype)
            run_adam(entry, run, hyp, step, gs, guard)
            run.check(ref, f"{name} {entry} guard {k}")


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("entry", ["one", "one_guarded"])
def test_adam_second_sweep(entry, dtype):
    """8192 * 256 + 4097 elements: adam_kernel's grid is capped at 8192 blocks (adam_step_one), so the elements from 2 097 152 on
    are updated in the SECOND sweep of the grid-stride loop `i += gridDim.x * 256` (adam_kernel)."""
    inputs = R.adam_inputs(R.ADAM_BIG, R.SEED + 1)
    guard = R.adam_guard(dict(R.ADAM_GUARDS)["clipped"], R.RECIPE, 2) if entry == "one_guarded" else None
    ref = _adam_reference(inputs, R.RECIPE, 2, 0.37, guard)
    run = AdamRun([R.ADAM_BIG], *inputs, dtype)
    run_adam(entry, run, R.RECIPE, 2, 0.37, guard)
    run.check(ref, f"second sweep {entry}")


@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("entry", ["multi", "multi_guarded"])
@pytest.mark.parametrize("layout", list(R.table_layouts()))
def test_adam_tables(layout, entry, dtype):
    """Hand-built tables (FusedAdam._tables' records): empty tensors in the middle and at the end, a 1-element tensor between
    multi-chunk ones, and 65 540 one-element tensors in one arena — total_chunks > 65 536, so blocks 0 .. 3 take a second chunk
    in adam_multi_kernel's loop `chunk += gridDim.x` and tensor_of_chunk searches 17 levels."""
    numels = R.table_layouts()[layout]
    inputs = R.adam_inputs(sum(numels), R.SEED + len(numels))
    guard = R.adam_guard(dict(R.ADAM_GUARDS)["after_skips"], R.RECIPE, 3246) if entry == "multi_guarded" else None
    ref = _adam_reference(inputs, R.RECIPE, 3246, 0.37, guard)
    run = AdamRun(numels, *inputs, dtype, gap=0 if layout == "many_ones" else 8)
    run_adam(entry, run, R.RECIPE, 3246, 0.37, guard)
    run.check(ref, f"{layout} {entry}")


@pytest.mark.parametrize("entry", ENTRIES)
def test_adam_bit_determined_cases(entry):
    """lr = 0, wd = 0 on masters whose low 16 bits are 0x7FFF, 0x8000 (even and odd upper half), 0x8001: the master keeps its bits,
    m and v move, the bf16 parameter is the round-to-nearest-even of the master.  grad = m = v = 0 with wd = 0: every bit stays.
    A skipped update stores nothing."""
    guarded = entry.endswith("guarded")
    p0 = R.tie_masters()
    _, grad, m0, v0 = R.adam_inputs(p0.numel(), R.SEED + 2)
    h0 = dict(R.RECIPE, lr=0.0, wd=0.0)
    guard = R.adam_guard(dict(R.ADAM_GUARDS)["clipped"], h0, 3) if guarded else None
    ref = _adam_reference((p0, grad, m0, v0), h0, 3, None, guard)
    assert bool((ref["p"][1] == 0).all())
    run = AdamRun([p0.numel()], p0, grad, m0, v0, bf16)
    run.pb.view(0).fill_(7.0)                               # the parameter is rewritten from the master, whatever it held
    run_adam(entry, run, h0, 3, None, guard)
    run.check(ref, f"lr0 {entry}")
    assert torch.equal(run.pm.flat().view(torch.int32), p0.view(torch.int32))
    assert not torch.equal(run.m.flat(), m0)
    z = torch.zeros(9)
    pz = R.adam_inputs(9, R.SEED + 3)[0]
    hz = dict(R.RECIPE, wd=0.0)
    for dtype in (f32, bf16):
        ref = _adam_reference((pz, z, z, z), hz, 1, 0.37, R.adam_guard(dict(R.ADAM_GUARDS)["clipped"], hz, 1) if guarded else None)
        run = AdamRun([9], pz, z, z, z, dtype)
        run_adam(entry, run, hz, 1, 0.37, R.adam_guard(dict(R.ADAM_GUARDS)["clipped"], hz, 1) if guarded else None)
        run.check(ref, f"zero {entry}")
        assert torch.equal(run.pm.flat().view(torch.int32), pz.view(torch.int32))
    if guarded:
        g = R.adam_guard(dict(R.ADAM_GUARDS)["skip"], R.RECIPE, 4)
        inputs = R.adam_inputs(300, R.SEED + 4)
        run = AdamRun([300], *inputs, bf16)
        run.pb.view(0).fill_(7.0)                           # a skipped update does not even refresh the bf16 parameter
        run_adam(entry, run, R.RECIPE, 4, None, g)
        for c, want in ((run.g, inputs[1]), (run.m, inputs[2]), (run.v, inputs[3]), (run.pm, inputs[0])):
            assert torch.equal(c.flat().view(torch.int32), want.view(torch.int32)) and c.untouched()
        assert bool((run.pb.flat() == 7.0).all()) and run.pb.untouched()


# ------------------------------------------------------------------------------------------------ sum of squares
def _sumsq_single(arena_host, off, n):
    arena = arena_host.to(DEV)
    assert arena.data_ptr() % 16 == 0
    nc = (n + 4095) // 4096
    out = Carve([nc], f32)
    rc = L.lib.mdt_grad_sumsq(L.stream(), n, arena.data_ptr() + 4 * off, L.ptr(out.view(0)))
    torch.cuda.synchronize()
    assert rc == 0, status(rc)
    assert out.untouched()
    return out.view(0).cpu()


def _sumsq_multi(arena_host, offs, numels):
    arena = arena_host.to(DEV)
    nt = len(numels)
    rec = np.zeros((nt, 6), dtype=np.int64)
    rec[:, 2] = arena.data_ptr() + 4 * np.asarray(offs, dtype=np.int64)
    rec[:, 5] = numels
    first = np.asarray(R.chunk_first(list(numels)), dtype=np.int64)
    out = Carve([int(first[-1])], f32)
    rec_d, first_d = torch.from_numpy(rec).to(DEV), torch.from_numpy(first).to(DEV)      # both alive until the kernel has run
    rc = L.lib.mdt_grad_sumsq_multi(L.stream(), nt, L.ptr(rec_d), L.ptr(first_d), int(first[-1]), L.ptr(out.view(0)))
    torch.cuda.synchronize()
    assert rc == 0, status(rc)
    assert out.untouched()
    return out.view(0).cpu()


@pytest.mark.parametrize("integer", [False, True], ids=["random", "integer"])
@pytest.mark.parametrize("off", R.SUMSQ_OFFSETS)
def test_sumsq_single_and_multi(off, integer):
    """Views at element offsets 0 .. 3 of a 16-byte aligned arena (the float4 path and the element path of chunk_sumsq); on
    integer gradients |g| <= 3 every partial is demanded exactly: one lost or doubled element is a difference of at least 1."""
    for n in R.SUMSQ_SIZES:
        a = R.sumsq_arena(n, off, R.SEED + n + off, integer)
        ref = R.reference_sumsq(a[off:off + n])
        if integer:
            assert bool((ref[1] == 0).all())
        one = _sumsq_single(a, off, n)
        R.check("sumsq partial", one, ref, f"single n{n} off{off}")
        multi = _sumsq_multi(a, [off], [n])
        R.check("sumsq partial", multi, ref, f"multi n{n} off{off}")
        assert torch.equal(one.view(torch.int32), multi.view(torch.int32)), "the two forms give different bits"


@pytest.mark.parametrize("layout", list(R.table_layouts()))
def test_sumsq_tables(layout):
    """The hand-built tables through grad_sumsq_multi_kernel; many_ones: total_chunks = 65 540 > 65 536, the loop
    `chunk += gridDim.x` of grad_sumsq_multi_kernel runs a second time for blocks 0 .. 3."""
    numels = R.table_layouts()[layout]
    arena = R.sumsq_inputs(sum(numels) + 8, R.SEED + len(numels), integer=True)
    arena[arena == 0] = 2.0
    offs = np.concatenate([[0], np.cumsum(numels)[:-1]])
    ref = R.reference_sumsq_multi([arena[o:o + n] for o, n in zip(offs, numels)])
    assert bool((ref[1] == 0).all())
    R.check("sumsq partial", _sumsq_multi(arena, offs, numels), ref, layout)


# ------------------------------------------------------------------------------------------------ finaliser
def _finalize(p, s_in, mx, step, reset, prev):
    gc, g = guard_buffer(prev)
    part = p.to(DEV) if p.numel() else None
    sc = scalar(s_in)
    h = R.RECIPE
    rc = L.lib.mdt_grad_norm_finalize(L.stream(), L.ptr(part), p.numel(), float(mx), L.ptr(sc), h["lr"], h["beta1"], h["beta2"], step,
                                      reset, L.ptr(g))
    torch.cuda.synchronize()
    assert rc == 0, status(rc)
    assert gc.untouched()
    return g.cpu(), g.view(torch.int32).cpu()


@pytest.mark.parametrize("case", R.finalize_cases(), ids=lambda c: c[0])
def test_finalize(case):
    """Hand-written partials.  n257 / n1000: the loop `i += 256` of grad_norm_finalize_kernel runs more than once per thread.
    reset = 1 runs over a NaN-filled guard, reset = 0 over live counters."""
    name, p, s_in, mx, step, reset, prev = case
    h = R.RECIPE
    ref = R.reference_finalize(p, s_in, mx, h["lr"], h["beta1"], h["beta2"], step, reset, prev)
    f, i = _finalize(p, s_in, mx, step, reset, prev)
    R.check_guard(f, i, ref, name)
    if name == "edge_equal":
        assert int(i[5]) == 0 and float(f[0]) == 1.0 and float(f[1]) == 5.0
    if name == "edge_below":
        assert int(i[5]) == 1 and float(f[0]) < 1.0


# ------------------------------------------------------------------------------------------------ node_ce
def _node_ce(l, rows, y, wn, wp, fp16_loss, gs, with_grad=True):
    M, nlab = l.shape[0], int(y.numel())
    ld = l.to(DEV)
    rd = rows.to(DEV) if nlab else None
    yd = y.to(DEV) if nlab else None
    out = Carve([1], f32)
    cnt = Carve([4], torch.int32)
    dl = Carve([M * 2], l.dtype)
    dl.view(0).fill_(float("nan"))
    rc = L.lib.mdt_node_ce(L.stream(), 0 if l.dtype == f32 else 1, M, nlab, L.ptr(ld), L.ptr(rd), L.ptr(yd), wn, wp, fp16_loss, gs,
                           L.ptr(out.view(0)), L.ptr(cnt.view(0)), L.ptr(dl.view(0)) if with_grad else None)
    torch.cuda.synchronize()
    assert rc == 0, status(rc)
    assert out.untouched() and cnt.untouched() and dl.untouched()
    if not with_grad:
        assert bool(torch.isnan(dl.view(0).float()).all())
    return out.view(0).cpu(), cnt.view(0).cpu().tolist(), dl.view(0).cpu().view(M, 2) if with_grad else None


@pytest.mark.parametrize("case", list(R.node_matrix()), ids=lambda c: f"nlab{c[0]}_{'bf16' if c[2] == bf16 else 'f32'}")
def test_node_ce(case):
    """nlab 4097 / 4113: label 4096 is the first to fold cascade level 2 into level 3 (node_ce_kernel: `s_part[j + 1]` with j = 2).
    fp16_loss = 0 runs the else-branch of node_ce_kernel (`lp0 = (l0 - m) - ls`, pred from l1 > l0).  dlogits = NULL: the
    `if (dlogits)` block is skipped and the loss and the counters keep their bits."""
    nlab, near, dtype, (wn, wp), gs = case
    l, rows, y = R.node_case_inputs(nlab, near, dtype, R.SEED + nlab)
    what = f"nlab{nlab} {dtype}"
    mask = torch.ones(l.shape[0], dtype=torch.bool)
    mask[rows.long()] = False
    for fp16_loss in (1, 0):
        loss, c, dl = _node_ce(l, rows, y, wn, wp, fp16_loss, gs)
        if fp16_loss:
            R.check_node_ce_f16(float(loss), c, dl, l, rows, y, wn, wp, gs, near, what)
        else:
            ref = R.reference_node_ce_f32(l, rows, y, wn, wp, gs)
            assert ref["margin"] > 0                             # the counters are exact
            R.check("node_ce f32 loss", loss, ref["loss"], what)
            assert c == ref["counters"], f"{what}: counters {c} against {ref['counters']}"
            R.check("node_ce f32 dlogits", dl, ref["dlogits"], what)
        assert bool((dl.float()[mask] == 0).all()), f"{what}: d logits of an unlabelled row is not 0"
        loss2, c2, _ = _node_ce(l, rows, y, wn, wp, fp16_loss, gs, with_grad=False)
        assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and c == c2, f"{what}: dlogits = NULL changes the result"


# ------------------------------------------------------------------------------------------------ contrastive
def _contrastive(emb, pad, y, hard, kw, gs, with_grad=True):
    B, D = emb.shape
    T = emb.dtype
    ld = D + pad                                                   # ld > D: rows of the input are read at their stride
    src = torch.full((B, ld), 0.75, dtype=T)
    src[:, :D] = emb
    src = src.to(DEV)
    nws = L.lib.mdt_contrastive_loss_workspace_bytes(B, D) // 4
    assert nws == B * D + B * B + 2 * B
    ws = Carve([nws], f32)
    ws.view(0).fill_(float("nan"))
    out = Carve([1], f32)
    cnt = Carve([4], torch.int32)
    g = R.Guarded(B, D, T, DEV, ld=D + 5)                           # ldd = D + 5: sentinel columns beside every gradient row
    yd, hd = y.to(DEV), hard.to(DEV)
    rc = L.lib.mdt_contrastive_loss(L.stream(), 0 if T == f32 else 1, B, D, L.ptr(src), ld, L.ptr(yd), L.ptr(hd), kw["scale"],
                                    kw["soft_negative_weight"], int(kw["adaptive"]), L.ptr(ws.view(0)), gs, L.ptr(out.view(0)),
                                    L.ptr(cnt.view(0)), g.view.data_ptr() if with_grad else None, D + 5)
    torch.cuda.synchronize()
    assert rc == 0, status(rc)
    assert ws.untouched() and out.untouched() and cnt.untouched() and g.untouched()
    w = ws.view(0).cpu()
    res = dict(n=w[:B * D].view(B, D), G=w[B * D:B * D + B * B].view(B, B), inv=w[B * D + B * B:B * D + B * B + B],
               extra=w[B * D + B * B + B:], loss=out.view(0).cpu(), counters=cnt.view(0).cpu().tolist())
    if with_grad:
        res["d_emb"] = g.view.cpu()
    else:
        assert bool((g.view.contiguous().view(g.itype) == g.bits).all()), "d_emb = NULL and the buffer was written"
    return res


@pytest.mark.parametrize("case", R.contrastive_cases(), ids=lambda c: c[0])
def test_contrastive(case):
    """Rows of norm 1e-3 .. 1e3 and, from B = 7 on, an exactly zero row and one of norm 1e-13: cl_normalize_kernel stores
    inv = -1e12 for both and cl_grad_kernel takes `s_acc[c] * 1e12f` (the clamped-norm branch; the tiny row's n_i is not zero, so
    a projection there would show).  The dense cases run the dot products and the gradient sums over all D products.  Odd cases read the input at ld = D + 3; every case
    writes the gradient at ldd = D + 5.  B = 45: 2025 pairs, a second sweep of cl_pair_kernel's 1024 threads.  d_emb = NULL skips
    cl_grad_kernel: same loss bits, same counters."""
    name, B, D, mode, kw, dtype, pad, gs = case
    emb, y, hard = R.contrastive_case_inputs(name, B, D, dtype)
    ref = R.reference_contrastive(emb, y, hard, kw["scale"], kw["soft_negative_weight"], kw["adaptive"], gs, knife_limit=R.knife_limit(name))
    out = _contrastive(emb, pad, y, hard, kw, gs)
    for k in ("n", "inv", "extra", "G"):
        R.check("contrastive " + k, out[k], ref[k], name, dtype=f32)
    R.check("contrastive d_emb", out["d_emb"], ref["d_emb"], name, dtype=dtype, cancels=D == 1)
    assert out["counters"] == ref["counters"], f"{name}: counters {out['counters']} against {ref['counters']}"
    R.check_loss_interval(float(out["loss"]), ref["loss"], name)
    if B >= 7:
        assert float(out["inv"][B // 2]) == -R.f32v(1e12) and bool((out["n"][B // 2] == 0).all())
        assert float(out["inv"][B // 2 - 1]) == -R.f32v(1e12) and 0.09 < float(out["n"][B // 2 - 1].norm()) < 0.11
    nograd = _contrastive(emb, pad, y, hard, kw, gs, with_grad=False)
    assert torch.equal(nograd["loss"].view(torch.int32), out["loss"].view(torch.int32)) and nograd["counters"] == out["counters"]


@pytest.mark.parametrize("yv", [0.0, 1.0], ids=["y0", "y1"])
@pytest.mark.parametrize("mode,kw", R.CL_MODES)
def test_contrastive_single_row(mode, kw, yv):
    """B = 1: loss 0, counters [y == 1], [y == 1], [y == 1], 1 (the one prediction is 1), zero gradient in every mode."""
    emb = torch.tensor([[0.3, -1.2, 2.0]])
    y, hard = torch.tensor([yv]), torch.tensor([5.0])
    out = _contrastive(emb, 0, y, hard, kw, 1.0)
    k = int(yv == 1)
    assert float(out["loss"]) == 0.0 and out["counters"] == [k, k, k, 1]
    ref = R.reference_contrastive(emb, y, hard, kw["scale"], kw["soft_negative_weight"], kw["adaptive"])
    assert out["counters"] == ref["counters"]
    R.check("contrastive d_emb", out["d_emb"], ref["d_emb"], "B1")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing():
    """Host-side argument checks: an error code, and no output is touched (nothing is launched)."""
    h = [float(R.RECIPE[k]) for k in HYP]
    inputs = R.adam_inputs(300, R.SEED + 9)
    for what in ("step0", "null_guard", "dtype2"):
        run = AdamRun([300], *inputs, f32)
        rec, first, nt, total = run.table()
        if what == "step0":
            rcs = [L.lib.mdt_adam_step(L.stream(), 0, *run.one(), *h, 0, None),
                   L.lib.mdt_adam_step_multi(L.stream(), 0, nt, L.ptr(rec), L.ptr(first), total, *h, 0, None)]
        elif what == "null_guard":
            rcs = [L.lib.mdt_adam_step_guarded(L.stream(), 0, *run.one(), *h, 1, None),
                   L.lib.mdt_adam_step_multi_guarded(L.stream(), 0, nt, L.ptr(rec), L.ptr(first), total, *h, 1, None)]
        else:
            rcs = [L.lib.mdt_adam_step(L.stream(), 2, *run.one(), *h, 1, None),
                   L.lib.mdt_adam_step_multi(L.stream(), 2, nt, L.ptr(rec), L.ptr(first), total, *h, 1, None)]
        torch.cuda.synchronize()
        assert all(rc != 0 for rc in rcs), (what, rcs)
        for c, want in ((run.g, inputs[1]), (run.m, inputs[2]), (run.v, inputs[3]), (run.pm, inputs[0])):
            assert torch.equal(c.flat().view(torch.int32), want.view(torch.int32)) and c.untouched(), what
    kw = dict(R.CL_MODES)
    for what, B, D, ld, ldd, mode_kw in (("ld<D", 2, 8, 7, 13, kw["fixed"]), ("ldd<D", 2, 8, 8, 7, kw["fixed"]),
                                         ("adaptive+soft", 2, 8, 8, 13, dict(scale=20.0, soft_negative_weight=0.25, adaptive=True)),
                                         ("D=40705", 1, 40705, 40705, 40705, kw["fixed"]), ("B=0", 0, 8, 8, 13, kw["fixed"])):
        rows = max(B, 1)
        src = torch.ones(rows, max(ld, D), device=DEV)
        ws = Carve([rows * D + rows * rows + 2 * rows], f32)
        out, cnt, g = Carve([1], f32), Carve([4], torch.int32), Carve([rows * max(ldd, D)], f32)
        yd = torch.zeros(rows, device=DEV)
        rc = L.lib.mdt_contrastive_loss(L.stream(), 0, B, D, L.ptr(src), ld, L.ptr(yd), L.ptr(yd), mode_kw["scale"],
                                        mode_kw["soft_negative_weight"], int(mode_kw["adaptive"]), L.ptr(ws.view(0)), 1.0,
                                        L.ptr(out.view(0)), L.ptr(cnt.view(0)), L.ptr(g.view(0)), ldd)
        torch.cuda.synchronize()
        assert rc != 0, what
        for c in (ws, out, cnt, g):
            assert bool((c.buf.view(c.itype) == c.bits).all()), f"{what}: an output was written"
    l = torch.zeros(4, 2, device=DEV)
    out, cnt, dl = Carve([1], f32), Carve([4], torch.int32), Carve([8], f32)
    yd = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = L.lib.mdt_node_ce(L.stream(), 0, 4, 2, L.ptr(l), None, L.ptr(yd), 1.0, 1.0, 1, 1.0, L.ptr(out.view(0)), L.ptr(cnt.view(0)),
                           L.ptr(dl.view(0)))
    torch.cuda.synchronize()
    assert rc != 0
    for c in (out, cnt, dl):
        assert bool((c.buf.view(c.itype) == c.bits).all()), "node_ce: an output was written by a refused call"


def test_report_worst_error_over_bound():
    """Not a check of its own: prints the worst err / bound each output reached in this run (pytest -s, or the log)."""
    print("\nloss / optimiser worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(R.WORST.items())))
    assert all(v <= 1.0 or "interval" in k for k, v in R.WORST.items())
