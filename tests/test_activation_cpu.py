"""The FFN activation kinds without a device: the fp64 restatement of tests/activation_reference.py against torch autograd,
the module surface (every fairseq name constructs, the layer's own default is relu, an unknown name raises in fairseq's
words, the parser takes the flag) and the restated Graphormer layer against the oracle's."""
import argparse

import pytest
import torch
import torch.nn.functional as F

import tests.activation_reference as AR
from oracle import mdt_ref_cpu as R

NAMES = ["relu", "gelu", "gelu_fast", "gelu_accurate", "tanh", "linear"]
TORCH_FN = {"relu": F.relu, "tanh": torch.tanh, "gelu": F.gelu, "gelu_accurate": lambda x: F.gelu(x, approximate="tanh"),
            "linear": lambda x: x * 1.0}


def grid():
    pts = [0.0, 1e-300, -1e-300, 2.0 ** -100, -2.0 ** -100, 20.0, -20.0]
    return torch.cat([torch.tensor(pts, dtype=torch.float64), torch.linspace(-8.0, 8.0, 1601, dtype=torch.float64)])


@pytest.mark.parametrize("kind", sorted(TORCH_FN))
def test_reference_value_and_derivative_equal_torch_autograd_fp64(kind):
    x = grid().requires_grad_(True)
    y = TORCH_FN[kind](x)
    y.sum().backward()
    xv = x.detach()
    val, der = AR.act(kind, xv), AR.act_grad(kind, xv)
    # the same closed forms evaluated in fp64 by two routes: a few ulp of the largest term
    assert float((val - y.detach()).abs().max()) <= 1e-14 * 20.0, kind
    assert float((der - x.grad).abs().max()) <= 1e-13, (kind, float((der - x.grad).abs().max()))
    if kind == "relu":
        assert float(val[0]) == 0.0 and float(der[0]) == 0.0            # 0 at 0, as torch
        assert torch.equal(val, y.detach()) and torch.equal(der, x.grad)


def test_reference_propagates_nan_and_inf_as_torch_does():
    x = torch.tensor([float("inf"), -float("inf"), float("nan"), 65504.0, -65504.0, 0.0, -0.0], dtype=torch.float64)
    for kind, fn in TORCH_FN.items():
        ours, theirs = AR.act(kind, x), fn(x)
        assert torch.equal(torch.isnan(ours), torch.isnan(theirs)), kind
        ok = ~torch.isnan(ours)
        assert torch.equal(ours[ok], theirs[ok]), (kind, ours, theirs)


def test_reference_dropout_scale_is_the_generator_of_the_gemm_reference():
    import tests.gemm_reference as GR
    assert torch.equal(AR.drop_scale(5, 12, 0.3, 99), GR.drop_scale(5, 12, 0.3, 99))
    assert torch.equal(AR.drop_scale(3, 4, 0.0, 7), torch.ones(3, 4, dtype=torch.float64))
    s = AR.drop_scale(64, 64, 0.5, 11)
    assert set(s.unique().tolist()) == {0.0, 2.0} and 0.4 < float((s == 0).double().mean()) < 0.6


def test_relu_and_linear_references_are_exact_and_the_others_bounded():
    x = torch.tensor([[0.5, -0.25, 0.0, -0.0, 3.0, -3.0, float("nan"), float("inf")]])
    for kind in ("relu", "linear"):
        ref = AR.reference(kind, x, 0.5, 3)
        assert bool(ref["h"][2].all()) and bool(ref["u"][2].all()) and float(ref["h"][1].max()) == 0.0
    for kind in ("gelu", "gelu_accurate", "tanh"):
        ref = AR.reference(kind, x[:, :6])
        assert not bool(ref["h"][2].any())
        assert bool((ref["h"][1] >= 0).all()) and bool((ref["u"][1] > 0).all())
        # not vacuous: a few dozen fp32 roundings at the most, at arguments where nothing cancels
        assert float((ref["h"][1] / AR.U32).max()) < 64 and float((ref["u"][1] / AR.U32).max()) < 64, kind


@pytest.mark.parametrize("name", NAMES)
def test_layer_and_stack_construct_with_every_name(name):
    from multimodaldiscussiontransformer_amd.modules.graphormer_graph_encoder_layer import GraphEncoderStack, GraphormerGraphEncoderLayer
    layer = GraphormerGraphEncoderLayer(64, 96, 4, activation_fn=name)
    assert layer.activation_fn == name
    stack = GraphEncoderStack(2, 64, 96, 4, activation_fn=name)
    assert stack.activation_fn == name and all(m.activation_fn == name for m in stack.layers)


def test_layer_default_arguments_mean_relu():
    from multimodaldiscussiontransformer_amd.modules.graphormer_graph_encoder_layer import GraphormerGraphEncoderLayer
    layer = GraphormerGraphEncoderLayer()
    assert layer.activation_fn == "relu" and layer.fc1.weight.shape == (3072, 768)


def test_unknown_name_raises_in_fairseq_words():
    from multimodaldiscussiontransformer_amd.modules.graphormer_graph_encoder_layer import GraphormerGraphEncoderLayer
    with pytest.raises(RuntimeError, match="--activation-fn swish not supported"):
        GraphormerGraphEncoderLayer(64, 96, 4, activation_fn="swish")


def test_kind_table_matches_the_header_and_the_reference():
    from multimodaldiscussiontransformer_amd import ops
    assert ops.ACT_KINDS == dict(AR.KINDS, gelu_fast=AR.KINDS["gelu_accurate"])
    assert (ops.ACT_GELU, ops.ACT_RELU, ops.ACT_GELU_ACCURATE, ops.ACT_TANH, ops.ACT_LINEAR) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("name", NAMES)
def test_parser_accepts_the_flag(name):
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    parser = argparse.ArgumentParser()
    GraphormerModel.add_args(parser)
    args, _ = parser.parse_known_args(["--activation-fn", name])
    assert args.activation_fn == name
    with pytest.raises(SystemExit):
        parser.parse_known_args(["--activation-fn", "swish"])


def layer_operands(D=64, Fg=96, H=4, T=9, B=3, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    p = "layers.0.layers.0"
    shapes = {f"{p}.self_attn.{n}_proj.weight": (D, D) for n in "qkv"}
    shapes.update({f"{p}.self_attn.{n}_proj.bias": (D,) for n in "qkv"})
    shapes.update({f"{p}.self_attn.out_proj.weight": (D, D), f"{p}.self_attn.out_proj.bias": (D,),
                   f"{p}.fc1.weight": (Fg, D), f"{p}.fc1.bias": (Fg,), f"{p}.fc2.weight": (D, Fg), f"{p}.fc2.bias": (D,)})
    for n in ("self_attn_layer_norm", "final_layer_norm"):
        shapes.update({f"{p}.{n}.weight": (D,), f"{p}.{n}.bias": (D,)})
    W = {n: ((torch.rand(*s, generator=g) * 2 - 1) * 0.2 + (1.0 if n.endswith("norm.weight") else 0.0)).to(dtype) for n, s in shapes.items()}
    x = ((torch.rand(T, B, D, generator=g) * 2 - 1)).to(dtype)
    bias = ((torch.rand(B, H, T, T, generator=g) * 2 - 1)).to(dtype)
    kpm = torch.zeros(B, T, dtype=torch.bool)
    kpm[1, T - 2:] = True
    return p, W, x, bias, kpm


@pytest.mark.parametrize("pre_ln", [False, True])
def test_restated_layer_with_gelu_is_the_oracle_layer_bit_for_bit(pre_ln):
    p, W, x, bias, kpm = layer_operands()
    a = R.graph_layer(x, W, p, 4, bias, kpm, pre_ln)
    b = AR.graph_layer(x, W, p, 4, bias, kpm, pre_ln, activation="gelu")
    assert a.dtype == torch.float32 and torch.equal(a, b)
    c = AR.patched_graph_layer("gelu")(x, W, p, 4, bias, kpm, pre_ln)
    assert torch.equal(a, c)
    d = AR.graph_layer(x, W, p, 4, bias, kpm, pre_ln, activation="relu")
    assert not torch.equal(a, d) and bool(torch.isfinite(d).all())
