"""tests/lora_dropout_reference.py against the references it extends (CPU): at p = 0 the masked forms are the plain ones, integer
operands with p = 0.5 and a power-of-two alpha have δ = 0, the two mutants the kernel tests rely on (no mask; counters strided by
the row stride) leave their bounds, the masked reference's bound is not vacuous on its own, and block64_lora without adapters is
block_reference.block64."""
import pytest
import torch

import tests.block_reference as BR
import tests.gemm_reference as GR
import tests.lora_dense_reference as LD
import tests.lora_dropout_reference as LDR
import tests.lora_reference as LR
from tests.test_engine_block_gpu import make_case, tape_seeds

bf16, f32 = torch.bfloat16, torch.float32


def test_p0_is_the_plain_reference():
    x, w = LR.gen((33, 80), 1, 1.0, bf16), LR.gen((16, 80), 2, 0.25, bf16)
    for got, ref in ((LDR.down_drop(x, w, 0.75, 0.0, 7), LR.down(x, w, 0.75)),
                     (LDR.wgrad_drop(LR.gen((33, 16), 3, 1.0, bf16), x, torch.ones(16, 80), 0.75, 0.0, 7),
                      LR.wgrad(LR.gen((33, 16), 3, 1.0, bf16), x, torch.ones(16, 80), 0.75))):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    t, y, aux = LR.gen((33, 16), 4, 1.0, bf16), LR.gen((33, 80), 5, 1.0, bf16), LR.gen((33, 80), 6, 1.0, bf16)
    v, d = LDR.up_add_mul_drop(t, w, y, aux, 1.5, LD.scale_of(None, 0.0, 33, 80))
    v0, d0 = LD.up_add_mul(t, w, y, aux, 1.5)
    assert torch.equal(v, v0) and bool((d >= d0).all()) and bool((d <= 2.0 * d0 + 1e-300).all())


def test_factor_is_one_fp32_number():
    import numpy as np
    assert LDR.factor(0.75, 0.0) == 0.75 and LDR.factor(2.0, 0.5) == 4.0
    assert LDR.factor(0.75, 0.1) == float(np.float32(0.75) * (np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))))


@pytest.mark.parametrize("dtype", [bf16, f32])
def test_integer_operands_are_exact(dtype):
    R, n, N = 300, 24, 80
    x, w = LR.gen_int((R, N), 1, 4, dtype), LR.gen_int((n, N), 2, 2, dtype)
    v, d = LDR.down_drop(x, w, 2.0, 0.5, 11)
    assert float(d.max()) == 0.0 and float(v.abs().max()) > 0
    t = LR.gen_int((R, n), 3, 2, dtype)
    v, d = LDR.wgrad_drop(t, x, LR.gen_int((n, N), 4, 50, f32), 2.0, 0.5, 11)
    assert float(d.max()) == 0.0
    y, aux = LR.gen_int((R, N), 5, 8, dtype), LR.gen_int((R, N), 6, 2, dtype)
    v, d = LDR.up_add_mul_drop(t, w, y, aux, 2.0, GR.drop_scale(R, N, 0.5, 11))
    assert float(d.max()) == 0.0


def test_dropped_non_finite_values_do_not_reach_the_result():
    R, K = 20, 80
    x = LR.gen((R, K), 1, 1.0, bf16)
    keep = GR.drop_scale(R, K, 0.5, 3) != 0
    r, c = [int(i) for i in torch.nonzero(~keep)[0]]
    x[r, c] = float("nan")
    assert bool(torch.isfinite(LDR.down_drop(x, LR.gen((8, K), 2, 0.25, bf16), 1.0, 0.5, 3)[0]).all())


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("R,D,n", [(15, 128, 16), (255, 80, 192), (1025, 1024, 24)])
def test_mutants_leave_the_bound_and_the_bound_is_not_vacuous(R, D, n, p):
    x, w = LR.gen((R, D), 1, 1.0, bf16), LR.gen((n, D), 2, 0.25, bf16)
    v, d = LDR.down_drop(x, w, 0.75, p, 99)
    bnd = LR.bound(v, d, bf16)
    nz = v != 0
    assert float((bnd / v.abs())[nz].median()) <= 2.0 ** -7
    no_mask = LDR.down_drop(x, w, 0.75, p, 99, apply_mask=False)[0]
    assert float(((no_mask - v).abs() > bnd).double().mean()) >= 0.5
    strided = LDR.down_drop(x, w, 0.75, p, 99, counter_ld=3 * D)[0]
    assert float(((strided - v).abs() > bnd).double().mean()) >= 0.5


@pytest.mark.parametrize("pre_ln", [False, True])
def test_block64_lora_without_adapters_is_block64(pre_ln):
    cfg = make_case("Sr", f32, pre_ln)
    seeds = tape_seeds(1234, 4)
    ref = BR.reference(cfg["x"], cfg["params"], cfg["cot"], cfg, seeds)
    got = LDR.reference(cfg["x"], cfg["params"], cfg["cot"], dict(cfg, p_lora=0.25), seeds)
    assert torch.equal(got["y"], ref["y"]) and torch.equal(got["dx"], ref["dx"])
    for k in BR.PARAMS:
        assert torch.equal(got["grads"][k], ref["grads"][k]), k


def test_block64_lora_sites_take_their_seeds_in_order():
    """Each site's mask matters and is its own: swapping two site seeds changes y; p_lora = 0 ignores them."""
    cfg = make_case("S", f32, False)
    D, Fd, r = cfg["D"], cfg["F"], 8
    ad = dict(qkv_A=LR.gen((3 * r, D), 1, 0.3, f32), qkv_Bt=LR.gen((3 * r, D), 2, 0.3, f32), out_A=LR.gen((r, D), 3, 0.3, f32),
              out_Bt=LR.gen((r, D), 4, 0.3, f32), fc1_A=LR.gen((r, D), 5, 0.3, f32), fc1_Bt=LR.gen((r, Fd), 6, 0.3, f32),
              fc2_A=LR.gen((r, Fd), 7, 0.3, f32), fc2_Bt=LR.gen((r, D), 8, 0.3, f32))
    params = dict(cfg["params"], **ad)
    assert LDR.site_names(ad) == ["qkv", "out", "fc1", "fc2"]
    c = dict(cfg, lora_scale=2.0, lora_cols=(0, 1, 2), p_lora=0.25)
    seeds = tape_seeds(77, 8)
    y = LDR.reference(cfg["x"], params, cfg["cot"], c, seeds)["y"]
    swapped = seeds[:4] + [seeds[5], seeds[4]] + seeds[6:]
    assert not torch.equal(LDR.reference(cfg["x"], params, cfg["cot"], c, swapped)["y"], y)
    c0 = dict(c, p_lora=0.0)
    assert torch.equal(LDR.reference(cfg["x"], params, cfg["cot"], c0, seeds)["y"], LDR.reference(cfg["x"], params, cfg["cot"], c0, seeds[:4])["y"])
