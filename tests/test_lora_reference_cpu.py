"""tests/lora_reference.py can be trusted and its bounds can fail: the reference pipeline (forward and the four backward
products) agrees with torch autograd on an fp64 x (W + s Bt^T A)^T linear, a CPU emulation of the kernels' arithmetic (fp32
accumulation, the documented roundings, slabs in ascending order) stays inside the bounds, and the mutants a kernel or its
caller could realistically be — a dropped scale, a dropped last slab, a slice at the wrong column offset, Bt used untransposed
— are caught by them."""
import pytest
import torch

import tests.lora_reference as LR

SLAB = 64          # a small slab for the emulation: the bounds take it as a parameter


def _emul_down(x, w, alpha, dtype):
    return (alpha * (x.float() @ w.float().t())).to(dtype)


def _emul_up_add(t, w, y, alpha, dtype):
    prod = t.float() @ w.float()
    return (y.double() + alpha * prod.double()).float().to(dtype)        # the FMA: alpha * prod is exact in fp64


def _emul_wgrad(t, x, dw, alpha, slab=SLAB, drop_last=False):
    R = t.shape[0]
    parts = [alpha * (t[a:a + slab].float().t() @ x[a:a + slab].float()) for a in range(0, R, slab)]
    if drop_last:
        parts = parts[:-1]
    total = parts[0].clone()
    for p in parts[1:]:
        total = total + p
    return dw + total


def _check(out, ref, dtype, what):
    v, d = ref
    LR.assert_within(out, v, LR.bound(v, d, dtype), what=what, dtype=dtype)


def test_pipeline_agrees_with_autograd_fp64():
    torch.manual_seed(0)
    R, D, r, s = 37, 32, 8, 0.75
    for targets in (("q", "v"), ("k",), ("q", "k", "v")):
        nj = len(targets)
        x = torch.randn(R, D, dtype=torch.float64, requires_grad=True)
        W = torch.randn(3 * D, D, dtype=torch.float64)
        A = torch.randn(nj * r, D, dtype=torch.float64, requires_grad=True)
        Bt = torch.randn(nj * r, D, dtype=torch.float64, requires_grad=True)
        rows = []
        for name in ("q", "k", "v"):
            Wj = W[LR.TARGET_INDEX[name] * D:(LR.TARGET_INDEX[name] + 1) * D]
            if name in targets:
                j = targets.index(name)
                Wj = Wj + s * Bt[j * r:(j + 1) * r].t() @ A[j * r:(j + 1) * r]
            rows.append(Wj)
        qkv = x @ torch.cat(rows).t()
        dqkv = torch.randn(R, 3 * D, dtype=torch.float64)
        qkv.backward(dqkv)
        base = (x @ W.t()).detach()
        dx_base = dqkv @ W                                   # the frozen projection's own input gradient
        p = LR.pipeline(x.detach(), A.detach(), Bt.detach(), s, targets, base, dqkv, dx_base, dtype=torch.float64, slab=16)
        for got, want in ((p["qkv"], qkv.detach()), (p["dx"], x.grad), (p["dA"], A.grad), (p["dBt"], Bt.grad)):
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_emulation_is_within_the_bounds(dtype):
    R, D, n = 3 * SLAB + 5, 48, 24
    x = LR.gen((R, D), 1, 1.0, dtype)
    w = LR.gen((n, D), 2, 0.25, dtype)
    _check(_emul_down(x, w, 0.5, dtype), LR.down(x, w, 0.5), dtype, "down")
    t = LR.gen((R, n), 3, 1.0, dtype)
    y = LR.gen((R, D), 4, 2.0, dtype)
    _check(_emul_up_add(t, w, y, 1.5, dtype), LR.up_add(t, w, y, 1.5), dtype, "up_add")
    dw = LR.gen((n, D), 5, 3.0, torch.float32)
    _check(_emul_wgrad(t, x, dw, 1.5), LR.wgrad(t, x, dw, 1.5, SLAB), torch.float32, "wgrad")
    ti, xi = LR.int_operands(R, n, D, dtype=dtype)
    dwi = LR.gen_int((n, D), 6, 50, torch.float32)
    v, d = LR.wgrad(ti, xi, dwi, 2.0, SLAB)
    assert float(d.max()) == 0.0                              # exact operands: nothing to hide in
    assert torch.equal(_emul_wgrad(ti, xi, dwi, 2.0).double(), v)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mutants_are_caught(dtype):
    R, D, r, s = 3 * SLAB + 5, 32, 16, 0.5
    src = LR.gen((R, D), 11, 1.0, dtype)
    A = LR.gen((2 * r, D), 12, 0.25, dtype)
    Bt = LR.gen((2 * r, D), 13, 0.25, dtype)
    qkv = LR.gen((R, 3 * D), 14, 1.0, dtype)
    t = _emul_down(src, A, 1.0, dtype)
    # dropped s in the forward sum
    ref = LR.up_add(t[:, :r], Bt[:r], qkv[:, :D], s)
    _check(_emul_up_add(t[:, :r], Bt[:r], qkv[:, :D], s, dtype), ref, dtype, "up_add")
    with pytest.raises(AssertionError):
        _check(_emul_up_add(t[:, :r], Bt[:r], qkv[:, :D], 1.0, dtype), ref, dtype, "up_add without s")
    # the v adapter added at the k slice (c_j = D) instead of c_j = 2 D
    full = LR.pipeline(src, A, Bt, s, ("q", "v"), qkv, qkv, src, dtype=dtype, slab=SLAB)
    wrong = qkv.clone()
    wrong[:, :D] = _emul_up_add(t[:, :r], Bt[:r], qkv[:, :D], s, dtype)
    wrong[:, D:2 * D] = _emul_up_add(t[:, r:], Bt[r:], qkv[:, D:2 * D], s, dtype)
    zero = torch.zeros_like(full["qkv"])
    with pytest.raises(AssertionError):
        LR.assert_within(wrong, full["qkv"], LR.bound(full["qkv"], zero, dtype), what="v at the k slice", dtype=dtype)
    # dropped last slab of the weight gradient (integer operands: exact)
    ti, xi = LR.int_operands(R, r, D, dtype=dtype)
    dwi = torch.zeros(r, D)
    refw = LR.wgrad(ti, xi, dwi, 1.0, SLAB)
    _check(_emul_wgrad(ti, xi, dwi, 1.0), refw, torch.float32, "wgrad")
    with pytest.raises(AssertionError):
        _check(_emul_wgrad(ti, xi, dwi, 1.0, drop_last=True), refw, torch.float32, "wgrad without its last slab")
    # Bt used untransposed in dt = s dqkv Bt^T (square Bt_j: D = r = 16)
    dq = LR.gen((R, 16), 15, 1.0, dtype)
    Bs = LR.gen((16, 16), 16, 0.5, dtype)
    refd = LR.down(dq, Bs, s)
    _check(_emul_down(dq, Bs, s, dtype), refd, dtype, "dt")
    with pytest.raises(AssertionError):
        _check(_emul_down(dq, Bs.t().contiguous(), s, dtype), refd, dtype, "dt with Bt untransposed")
