"""tests/lora_dense_reference.py against torch autograd in fp64: the adapted dense layer with dropout and residual,
y = res + m (x W^T + b + s (x A^T) B), and the adapted FFN with each activation.  No device, no native library."""
import pytest
import torch

import tests.activation_reference as AR
import tests.lora_dense_reference as DR

F64 = torch.float64


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=F64) * 2 - 1) * scale


def _close(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-11 * max(1.0, float(b.abs().max())), f"{what}: {err:.3e}"


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_dense_site_is_the_autograd_of_the_adapted_layer(p):
    R, K, N, r, s = 37, 48, 32, 8, 1.75
    x, W, b = _rand((R, K), 1), _rand((N, K), 2, 0.3), _rand((N,), 3)
    A, Bt, res, g = _rand((r, K), 4, 0.3), _rand((r, N), 5, 0.3), _rand((R, N), 6), _rand((R, N), 7)
    m = DR.cpu_scale(R, N, p, 99)
    assert p == 0.0 or 0 < int((m == 0).sum()) < R * N
    got = DR.dense_site(x, W, b, A, Bt, s, res, m, g)
    leaves = [t.clone().requires_grad_() for t in (x, W, b, A, Bt)]
    xx, WW, bb, AA, BB = leaves
    y = res + m * (xx @ WW.t() + bb + s * (xx @ AA.t()) @ BB)
    y.backward(g)
    _close(got["y"], y.detach(), "y")
    for name, leaf in zip(("dx", "dW", "db", "dA", "dBt"), leaves):
        _close(got[name], leaf.grad, name)


@pytest.mark.parametrize("kind", DR.KINDS)
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_pipeline_is_the_autograd_of_the_adapted_ffn(kind, p):
    R, D, F, r, s = 29, 32, 64, 8, 0.5
    x, g = _rand((R, D), 1, 2.0), _rand((R, D), 2)
    P = dict(W1=_rand((F, D), 3, 0.4), b1=_rand((F,), 4), A1=_rand((r, D), 5, 0.4), Bt1=_rand((r, F), 6, 0.4),
             W2=_rand((D, F), 7, 0.3), b2=_rand((D,), 8), A2=_rand((r, F), 9, 0.3), Bt2=_rand((r, D), 10, 0.3))
    m_act, m_hid = DR.cpu_scale(R, F, p, 5), DR.cpu_scale(R, D, p, 6)
    got = DR.pipeline(kind, x, P, s, m_act, m_hid, g)
    L = {k: v.clone().requires_grad_() for k, v in P.items()}
    xx = x.clone().requires_grad_()
    v = xx @ L["W1"].t() + L["b1"] + s * (xx @ L["A1"].t()) @ L["Bt1"]
    if kind == "relu":
        h = torch.relu(v) * m_act
    else:
        h = AR.act(kind, v) * m_act
    y = xx + m_hid * (h @ L["W2"].t() + L["b2"] + s * (h @ L["A2"].t()) @ L["Bt2"])
    y.backward(g)
    _close(got["y"], y.detach(), "y")
    _close(got["dx"], xx.grad, "dx")
    _close(got["fc1"]["h"], h.detach(), "h")
    _close(got["fc1"]["u"], AR.act_grad(kind, v.detach()) * m_act, "u")
    for site, names in (("fc1", dict(dW="W1", db="b1", dA="A1", dBt="Bt1")), ("fc2", dict(dW="W2", db="b2", dA="A2", dBt="Bt2"))):
        for k, leaf in names.items():
            _close(got[site][k], L[leaf].grad, f"{site} {k}")


def test_drop_keeps_dropped_elements_and_p0_is_up_add():
    R, N, n = 9, 32, 8
    t, w, y = _rand((R, n), 1), _rand((n, N), 2), _rand((R, N), 3)
    m = DR.cpu_scale(R, N, 0.5, 3)
    v, d = DR.up_add_drop(t, w, y, 0.75, m)
    assert torch.equal(v[m == 0], y[m == 0]) and float(d[m == 0].abs().max()) == 0.0
    _close(v, y + 0.75 * m * (t @ w), "drop")
    v0, _ = DR.up_add_drop(t, w, y, 0.75, torch.ones(R, N, dtype=F64))
    assert torch.equal(v0, DR.up_add(t, w, y, 0.75)[0])
    _close(DR.up_add_mul(t, w, y, m, 0.5)[0], y + 0.5 * (t @ w) * m, "mul")


def test_integer_operands_have_no_error_term():
    t = torch.randint(-1, 2, (40, 64), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    w = torch.randint(-1, 2, (64, 32), generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    y = torch.randint(-4, 5, (40, 32), generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    m = DR.cpu_scale(40, 32, 0.5, 7)
    assert float(DR.up_add_drop(t, w, y, 1.0, m)[1].max()) == 0.0
    assert float(DR.up_add_mul(t, w, y, y, 2.0)[1].max()) == 0.0
    assert float(DR.up_add_drop(t, w, y, 1.5, m)[1].max()) > 0.0


def test_lipschitz_constants():
    assert 1.12 < DR.LIPSCHITZ["gelu"][0] < 1.15 and 0.79 < DR.LIPSCHITZ["gelu"][1] < 0.82
    assert 1.0 <= DR.LIPSCHITZ["tanh"][0] < 1.02 and 0.76 < DR.LIPSCHITZ["tanh"][1] < 0.79
    assert 1.0 <= DR.LIPSCHITZ["relu"][0] < 1.02 and DR.LIPSCHITZ["linear"] == (1.01, 0.0)
