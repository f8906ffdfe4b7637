"""The Graphormer FFN activation kinds on the GPU (csrc/activation.hip, engine.transformer_block(act=...), --activation-fn):
mdt_act_fwd against the fp64 reference of tests/activation_reference.py with per-element bounds, its dropout masks, the
two-launch GELU against the fused fc1 epilogue, a Graphormer layer and the Tiny model against the restated oracle layer,
and the launcher.

On a tree without the feature every kernel test fails on the missing mdt_act_fwd, every layer, model and launcher test on the
layer's NotImplementedError."""
import math
from argparse import Namespace  # noqa: F401

import numpy as np
import pytest
import torch

import tests.activation_reference as AR
import tests.gemm_reference as GR
from oracle import mdt_ref_cpu as R
from oracle import structure as S
from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2, BF16_LOGIT_ABS
from tests.util_model import fill_hash_weights, model_args, named_canonical_params, split_qkv_grad

pytestmark = pytest.mark.gpu

KINDS = ["gelu", "relu", "gelu_accurate", "tanh", "linear"]
DTYPES = [torch.float32, torch.bfloat16]
# (rows, N, ld) of the issue; the last one is this file's: mdt_act_fwd launches up to 8 workgroups of 256 lanes per compute
# unit, so 257 x 3080 is one grid pass on a 256-CU device — 1031 x 4104 is more than one for both vector widths
SHAPES = [(1, 8, 8), (3, 24, 24), (5, 20, 20), (4, 6, 6), (257, 3080, 3080), (1031, 4104, 4104)]
STRIDED = (7, 96, 104)
SPECIAL = [0.0, -0.0, 65504.0, -65504.0, float("inf"), -float("inf"), float("nan")]
C = 0x9E3779B97F4A7C15
M63 = 0x7FFFFFFFFFFFFFFF
_INPUTS, _MEASURED = {}, {}


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from multimodaldiscussiontransformer_amd import _lib
    return _lib


def inputs(rows, N, dtype):
    """N(0, 2) values with exact 0, -0, ±65504, ±inf and NaN mixed in (every 97th element, and the front of the buffer),
    stored as ``dtype``; made once per shape."""
    key = (rows, N, dtype)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * rows + N)
        x = (torch.randn(rows * N, generator=g) * 2.0)
        sp = torch.tensor(SPECIAL)
        k = min(len(SPECIAL), rows * N - 1)
        x[:k] = sp[:k]
        at = torch.arange(11, max(rows * N, 12), 97)[:max(0, (rows * N - 11 + 96) // 97)]
        x[at] = sp[torch.arange(at.numel()) % len(SPECIAL)]
        _INPUTS[key] = x.view(rows, N).to(dtype)
    return _INPUTS[key]


def expect_route(N, lds, dtype):
    vn = 8 if dtype == torch.bfloat16 else 4
    return "act_vec" if N % vn == 0 and all(ld % vn == 0 for ld in lds) else "act_scalar"


def note_measured(kind, x, h, u, p, seed):
    if kind in ("gelu", "gelu_accurate") and h.dtype == torch.float32:
        k = AR.measured_constant(kind, x, h, u, p, seed)
        _MEASURED[kind] = max(_MEASURED.get(kind, 0.0), k)


# ------------------------------------------------------------------------------------------------ kernel against fp64
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_act_fwd_against_fp64(ops, L, kind, dtype):
    worst = 0.0
    for rows, N, ld in SHAPES:
        xs = inputs(rows, N, dtype)
        big = rows == 1031                                # this file's own shape: once, with dropout, no repeats
        for p, seed in ((0.0, 0), (0.3, 4711 + rows)):
            if big and p == 0.0:
                continue
            ref = AR.reference(kind, xs, p, seed)
            x = xs.cuda()
            h, u = ops.act_fwd(x, kind, drop_p=p, drop_seed=seed)
            assert L.last_route() == expect_route(N, (ld,), dtype), (L.last_route(), rows, N)
            assert torch.equal(x.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               xs.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))        # input left alone
            what = f"{kind} {dtype} {rows}x{N} p={p}"
            note_measured(kind, xs, h, u, p, seed)           # printed before anything is asserted
            if kind in _MEASURED and dtype == torch.float32:
                print(f"[act measured] {kind} {rows}x{N} p={p}: worst err / (u32 S) so far {_MEASURED[kind]:.4f} "
                      f"(bound constant {AR.K_GELU if kind == 'gelu' else AR.K_GELU_ACCURATE})")
            worst = max(worst, AR.compare(h, ref["h"], what=what + " h"), AR.compare(u, ref["u"], what=what + " u"))
            if big:
                continue
            # h aliased to pre, and forward without a tape: the same bits
            xa = x.clone()
            ha, ua = ops.act_fwd(xa, kind, drop_p=p, drop_seed=seed, out=xa)
            assert ha.data_ptr() == xa.data_ptr()
            bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
            assert torch.equal(ha.view(bits), h.view(bits)) and torch.equal(ua.view(bits), u.view(bits)), what + " aliased"
            hn, un = ops.act_fwd(x, kind, drop_p=p, drop_seed=seed, want_u=False)
            assert un is None and torch.equal(hn.view(bits), h.view(bits)), what + " u = None"
    print(f"[act fwd] {kind} {dtype}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_act_fwd_strided_buffers_keep_their_padding(ops, L, kind, dtype):
    """pre, h and u each at its own row stride inside poisoned buffers: nothing outside the [rows, N] views is written."""
    rows, N, ld = STRIDED
    xs = inputs(rows, N, dtype)
    for p, seed in ((0.0, 0), (0.5, 99)):
        ref = AR.reference(kind, xs, p, seed)
        gp = GR.Guarded(rows, N, dtype, "cuda", ld=ld, init=xs.cuda())
        gh = GR.Guarded(rows, N, dtype, "cuda", ld=ld + 8)
        gu = GR.Guarded(rows, N, dtype, "cuda", ld=ld + 16)
        h, u = ops.act_fwd(gp.view, kind, drop_p=p, drop_seed=seed, out=gh.view, u=gu.view)
        assert L.last_route() == "act_vec"
        torch.cuda.synchronize()
        assert gp.untouched() and gh.untouched() and gu.untouched(), f"{kind} {dtype}: wrote outside its views"
        what = f"{kind} {dtype} strided p={p}"
        AR.compare(h, ref["h"], what=what + " h")
        AR.compare(u, ref["u"], what=what + " u")
        # in place in the strided buffer, without u
        ops.act_fwd(gp.view, kind, drop_p=p, drop_seed=seed, out=gp.view, want_u=False)
        assert gp.untouched()
        AR.compare(gp.view, ref["h"], what=what + " in place")
    # an odd stride takes the scalar kernel, with the same result
    gp = GR.Guarded(rows, N, dtype, "cuda", ld=ld + 1, init=xs.cuda())
    h, u = ops.act_fwd(gp.view, kind)
    assert L.last_route() == "act_scalar" and gp.untouched()
    ref = AR.reference(kind, xs)
    AR.compare(h, ref["h"], what=f"{kind} {dtype} odd stride h")
    AR.compare(u, ref["u"], what=f"{kind} {dtype} odd stride u")


def test_act_fwd_nonfinite_inputs_as_torch(ops):
    """NaN and ±inf through every kind: h has torch's NaNs and infinities (relu keeps a NaN: the optimiser's guard sees it)."""
    import torch.nn.functional as F
    fns = {"relu": F.relu, "tanh": torch.tanh, "gelu_accurate": lambda t: F.gelu(t, approximate="tanh"), "gelu": F.gelu,
           "linear": lambda t: t * 1.0}
    x = torch.tensor([SPECIAL + [1.5]], dtype=torch.float32)
    for kind, fn in fns.items():
        for dtype in DTYPES:
            h, u = ops.act_fwd(x.to(dtype).cuda(), kind)
            want = fn(x.double())
            got = h.float().cpu().double()
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (kind, dtype, got, want)
            assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.equal(got[torch.isinf(got)], want[torch.isinf(want)]), (kind, dtype)
    h, u = ops.act_fwd(x.cuda(), "relu")
    assert math.isnan(float(h[0, 6])) and float(h[0, 0]) == 0.0 and float(u[0, 0]) == 0.0 and float(h[0, 5]) == 0.0


def test_act_fwd_bad_arguments(ops, L):
    x = torch.zeros(4, 8).cuda()
    st = L.stream()
    call = lambda kind, dt, ldp, ldh, p=0.0: L.lib.mdt_act_fwd(st, dt, kind, 4, 8, L.ptr(x), ldp, L.ptr(x), ldh, None, 0, p, 0)  # noqa: E731
    assert call(5, 0, 8, 8) == -1 and "kind" in L.lib.mdt_last_error_string().decode()
    assert call(-1, 0, 8, 8) == -1
    assert call(1, 2, 8, 8) == -1 and "dtype" in L.lib.mdt_last_error_string().decode()
    assert call(1, 0, 7, 8) == -1 and call(1, 0, 8, 4) == -1
    assert call(1, 0, 8, 8, p=1.0) == -1
    assert L.lib.mdt_act_fwd(st, 0, 1, 0, 8, None, 8, None, 8, None, 0, 0.0, 0) == 0          # rows == 0: nothing to do
    assert call(1, 0, 8, 8) == 0
    with pytest.raises(KeyError):
        ops.act_fwd(x, "swish")


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.3, 0.5])
def test_act_fwd_dropout_is_the_mask_of_mdt_dropout(ops, p, dtype):
    rows, N, seed = 37, 40, 2024
    g = torch.Generator().manual_seed(3)
    xs = (0.5 + 1.5 * torch.rand(rows, N, generator=g)).to(dtype)            # bounded away from 0: act and act' are non-zero
    keep = ops.dropout_mask(rows * N, p, seed).view(rows, N).bool()
    assert torch.equal(keep.cpu(), GR.drop_scale(rows, N, p, seed) != 0)
    inv_keep = GR.drop_params(p)[1]
    for kind in KINDS:
        h, u = ops.act_fwd(xs.cuda(), kind, drop_p=p, drop_seed=seed)
        assert torch.equal(h == 0, ~keep), kind
        assert torch.equal(u == 0, ~keep), kind
        h1, u1 = ops.act_fwd(xs.cuda(), kind)
        # the kept elements carry 1 / (1 - p): the fp32 product of the unscaled result, up to the roundings of the two stores
        tol = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22
        for a, b in ((h, h1), (u, u1)):
            r = (a.double() / (b.double() * inv_keep))[keep]
            assert float((r - 1.0).abs().max()) <= tol, (kind, float((r - 1.0).abs().max()))
        ref = AR.reference(kind, xs, p, seed)
        AR.compare(h, ref["h"], what=f"{kind} p={p} h")
        AR.compare(u, ref["u"], what=f"{kind} p={p} u")
        assert not torch.equal(ops.act_fwd(xs.cuda(), kind, drop_p=p, drop_seed=seed + 1)[0] == 0, ~keep)


# ------------------------------------------------------------------------------------------------ two launches against the fused epilogue
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_two_launch_gelu_against_fused_epilogue_fp32(ops, p):
    """fc1 with MDT_EPI_GELU | MDT_EPI_AUX_GRAD (what the benchmark runs) against the plain bias GEMM followed by
    mdt_act_fwd(GELU) on the same operands: both within the fp64 bound of the stored pre-activation, so within twice that
    of each other."""
    M, K, N, seed = 33, 64, 96, 515
    a = GR.gen((M, K), 1, 1.0, torch.float32).cuda()
    w = GR.gen((N, K), 2, 2.0 * GR.b_scale(K), torch.float32).cuda()
    b = GR.gen((N,), 3, 0.5, torch.float32).cuda()
    u1 = torch.empty(M, N).cuda()
    h1 = ops.gemm(a, w, bias=b, aux=u1, epilogue=ops.EPI_GELU | ops.EPI_AUX_GRAD, drop_p=p, drop_seed=seed)
    pre = ops.gemm(a, w, bias=b)
    pre0 = pre.clone()
    h2, u2 = ops.act_fwd(pre, "gelu", drop_p=p, drop_seed=seed, out=pre)
    ref = AR.reference("gelu", pre0.cpu(), p, seed)
    for name, fused, two in (("h", h1, h2), ("u", u1, u2)):
        AR.compare(two, ref[name], what=f"two-launch {name}")
        AR.compare(fused, ref[name], what=f"fused {name}")
        v, d, _ = ref[name]
        bnd = GR.bound(v, d, torch.float32)
        assert bool(((fused.cpu().double() - two.cpu().double()).abs() <= 2.0 * bnd).all()), name
        assert torch.equal(fused == 0, two == 0) or p == 0.0
    assert float(h2.abs().max()) > 0.5        # the operands reach the range where GELU bends


# ------------------------------------------------------------------------------------------------ layer
LAYER = dict(D=64, Fg=96, H=4, T=9, B=3)
PFX = "layers.0.layers.0."


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def build_layer(kind, pre_ln, dtype, p_act=0.0):
    from multimodaldiscussiontransformer_amd.modules import GraphormerGraphEncoderLayer
    c = LAYER
    layer = GraphormerGraphEncoderLayer(c["D"], c["Fg"], c["H"], dropout=0.0, attention_dropout=0.0, activation_dropout=p_act,
                                        activation_fn=kind, pre_layernorm=pre_ln)
    with torch.no_grad():
        for i, prm in enumerate(layer.parameters()):
            prm.copy_(rnd(*prm.shape, seed=100 + i, scale=0.25) + (1.0 if prm.dim() == 1 and i % 2 == 0 else 0.0))
    return layer.cuda().to(dtype)


def layer_run(layer, dtype):
    """forward + backward through the public forward → (y, dx, {oracle name: gradient}), the operands as stored"""
    c = LAYER
    x = rnd(c["T"], c["B"], c["D"], seed=1).to(dtype).cuda().requires_grad_(True)
    bias = rnd(c["B"], c["H"], c["T"], c["T"], seed=2).cuda()
    kpm = torch.zeros(c["B"], c["T"], dtype=torch.bool)
    kpm[1, c["T"] - 2:] = True
    cot = rnd(c["T"], c["B"], c["D"], seed=3).to(dtype).cuda()
    y, attn = layer(x, self_attn_bias=bias, self_attn_padding_mask=kpm.cuda())
    assert attn is None
    (y.float() * cot.float()).sum().backward()
    grads = {PFX + k: prm.grad for k, prm in layer.named_parameters()}
    return y.detach(), x, bias, kpm, cot, grads


def layer_reference(layer, kind, pre_ln, x, bias, kpm, cot, act_scale=None):
    """the restated oracle layer in fp64 on the layer's stored weights and operands"""
    W = {PFX + k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.state_dict().items()}
    xr = x.detach().cpu().double().requires_grad_(True)
    # the key projection's output is kept so that its gradient dK can be read: the key bias gradient is the column sum of dK,
    # which cancels to zero (a key bias shifts every score of a row alike) — its error is measured against what is summed
    kw, kept, linear = W[PFX + "self_attn.k_proj.weight"], {}, torch.nn.functional.linear

    def keeping(inp, weight, b=None):
        out = linear(inp, weight, b)
        if weight is kw:
            out.retain_grad()
            kept["k"] = out
        return out

    torch.nn.functional.linear = keeping
    try:
        y = AR.graph_layer(xr, W, PFX[:-1], LAYER["H"], bias.cpu().double(), kpm, pre_ln, activation=kind, act_scale=act_scale)
    finally:
        torch.nn.functional.linear = linear
    (y * cot.cpu().double()).sum().backward()
    layer_reference.summed = {PFX + "self_attn.k_proj.bias": float(kept["k"].grad.abs().sum((0, 1)).norm())}
    return y.detach(), xr.grad, {n: w.grad for n, w in W.items()}


def check_layer_fp32(tag, y, x, grads, yr, dxr, gref):
    gate = lambda ref: 1e-3 * max(1.0, float(ref.abs().max()))  # noqa: E731
    rows = [("out", float((y.cpu().double() - yr).abs().max()), gate(yr)), ("dx", float((x.grad.cpu().double() - dxr).abs().max()), gate(dxr))]
    for name, ref in gref.items():
        gr = split_qkv_grad(name, grads)
        assert gr is not None, name
        rows.append((name, float((gr.cpu().double() - ref).abs().max()), gate(ref)))
    w = max(rows, key=lambda r: r[1] / r[2])
    print(f"[{tag}] {len(rows)} tensors, worst |err| / gate {w[1] / w[2]:.3e} ({w[0]})")
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, bad
    assert len(rows) == 2 + 16


@pytest.mark.parametrize("pre_ln", [False, True], ids=["post_ln", "pre_ln"])
@pytest.mark.parametrize("kind", KINDS + ["gelu_fast"])
def test_layer_fp32_against_fp64_restatement(kind, pre_ln):
    layer = build_layer(kind, pre_ln, torch.float32).eval()
    y, x, bias, kpm, cot, grads = layer_run(layer, torch.float32)
    yr, dxr, gref = layer_reference(layer, kind, pre_ln, x, bias, kpm, cot)
    check_layer_fp32(f"layer fp32 {kind} {'pre' if pre_ln else 'post'}-LN", y, x, grads, yr, dxr, gref)


@pytest.mark.parametrize("pre_ln", [False, True], ids=["post_ln", "pre_ln"])
@pytest.mark.parametrize("kind", KINDS)
def test_layer_bf16_against_fp64_restatement(kind, pre_ln):
    layer = build_layer(kind, pre_ln, torch.bfloat16).eval()
    y, x, bias, kpm, cot, grads = layer_run(layer, torch.bfloat16)
    yr, dxr, gref = layer_reference(layer, kind, pre_ln, x, bias, kpm, cot)          # on the bf16-rounded weights and operands
    err = (y.float().cpu().double() - yr).abs()
    assert bool((err <= 0.03 + 2e-2 * yr.abs()).all()), float((err - 2e-2 * yr.abs()).max())
    rows = []
    for name, ref in list(gref.items()) + [("dx", dxr)]:
        gr = x.grad if name == "dx" else split_qkv_grad(name, grads)
        assert gr is not None, name
        # the key bias gradient is a sum of T * B rows of dK that cancels to zero: as for the classifier bias of the model
        # tests, its error is taken relative to the scale of what is summed (|| sum_rows |dK| ||), not to the cancelled result
        rn = max(float(ref.norm()), layer_reference.summed.get(name, 0.0))
        rows.append((float((gr.float().cpu().double() - ref).norm()) / rn, name))
    rows.sort(reverse=True)
    print(f"[layer bf16 {kind} {'pre' if pre_ln else 'post'}-LN] worst rel-L2: " + "; ".join(f"{n} {r:.3e}" for r, n in rows[:4]))
    bad = [(n, r) for r, n in rows if r > BF16_GRAD_REL_L2]
    assert not bad, bad


@pytest.mark.parametrize("kind,pre_ln", [(k, False) for k in KINDS] + [("relu", True), ("gelu_accurate", True)])
def test_layer_activation_dropout_training_against_restatement(ops, kind, pre_ln):
    """activation_dropout = 0.5 in train(): the site seeds follow the CPU generator (base + C * counter, the third site of
    the block), the mask is regenerated with ops.dropout_mask and put behind the restated activation line."""
    p = 0.5
    layer = build_layer(kind, pre_ln, torch.float32, p_act=p).train()
    torch.manual_seed(31337)
    y, x, bias, kpm, cot, grads = layer_run(layer, torch.float32)
    torch.manual_seed(31337)
    base = int(torch.randint(0, 2 ** 62, (1,)).item())
    s_act = (base + C * 3) & M63
    c = LAYER
    m = ops.dropout_mask(c["T"] * c["B"] * c["Fg"], p, s_act).view(c["T"], c["B"], c["Fg"])
    assert 0.3 < float(m.float().mean()) < 0.7
    scale = m.cpu().double() * GR.drop_params(p)[1]
    yr, dxr, gref = layer_reference(layer, kind, pre_ln, x, bias, kpm, cot, act_scale=scale)
    check_layer_fp32(f"layer fp32 {kind} act-dropout {'pre' if pre_ln else 'post'}-LN", y, x, grads, yr, dxr, gref)
    y0, _, _ = layer_reference(layer, kind, pre_ln, x, bias, kpm, cot)
    assert float((y0 - yr).abs().max()) > 1e-2         # the mask matters: without it the gate is missed by far


# ------------------------------------------------------------------------------------------------ full model
_ORACLE, _PRODUCT = {}, {}


def tiny_case():
    """The Tiny shape — D 128, 8 graph heads of 16, 2 encoder heads of 64 — on four 12-comment trees, every comment labelled
    (the construction of tests/test_wide_heads_model_gpu.py)."""
    from multimodaldiscussiontransformer_amd import synthetic
    hp = R.hparams(dim=128, enc_heads=2, graph_heads=8, enc_ffn=256, graph_ffn=128, text_layers=4, vit_layers=4, num_fusion_layers=1,
                   num_fusion_stack=1, num_graph_stack=1, num_bottleneck=4, vocab_size=600, max_pos=64, image_size=32, patch=16,
                   pos_weight=1.5, neg_weight=1.0)
    rng = np.random.Generator(np.random.PCG64(1016))
    trees = [synthetic.make_tree(12, rng, seq_len=16, vocab_size=hp.vocab_size, image_frac=0.0, image_size=hp.image_size, min_len=3)
             for _ in range(4)]
    for i, t in enumerate(trees):
        n = len(t["parent"])
        t["y_mask"][:] = True
        t["y"] = np.asarray([(k + i) % 2 for k in range(n)], dtype=np.float32)
    return hp, trees


def model_oracle(kind, rounded):
    """fp32 oracle forward + backward with oracle.mdt_ref_cpu.graph_layer replaced by the restated layer (graph_stack looks
    it up at call time); once per (kind, weights rounded to bf16 or not)."""
    if (kind, rounded) not in _ORACLE:
        hp, trees = tiny_case()
        W = R.make_weights(hp)
        if rounded:
            W = {n: w.detach().bfloat16().float().requires_grad_(not R.is_frozen(hp, n)) for n, w in W.items()}
        batch = R.to_torch_batch(S.collate(trees, 5))
        saved = R.graph_layer
        R.graph_layer = AR.patched_graph_layer(kind)
        try:
            logits, _ = R.model_forward(W, hp, batch)
        finally:
            R.graph_layer = saved
        loss, counters = R.node_cross_entropy(logits, batch["y"], batch["y_mask"], hp)
        loss.backward()
        _ORACLE[(kind, rounded)] = dict(logits=logits.detach(), loss=float(loss.detach()), counters=counters,
                                        grads={n: (None if w.grad is None else w.grad.detach()) for n, w in W.items()})
    return _ORACLE[(kind, rounded)]


def model_product(kind, dtype, backward=True):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    hp, trees = tiny_case()
    args = model_args(hp)
    args.activation_fn = kind
    model = fill_hash_weights(GraphormerModel.build_model(args, task=None)).cuda().to(dtype).train()
    if dtype == torch.bfloat16:
        model.prepare_main_grads()
    pb = pack_batch(trees, 5)
    loss, log = 0.0, None
    if backward:
        crit = GraphPredictionNodeCrossEntropy(None, positive_weight=hp.pos_weight, negative_weight=hp.neg_weight)
        loss, _, log = crit(model, {"nsamples": len(trees), "net_input": {"batched_data": pb.batched_data}})
        loss.backward()
        loss = float(loss.detach())
    with torch.no_grad():
        logits, _ = model(pb.batched_data)
    torch.cuda.synchronize()
    return model, loss, log, logits.float().cpu()


def gelu_logits_fp32():
    if "gelu" not in _PRODUCT:
        _PRODUCT["gelu"] = model_product("gelu", torch.float32, backward=False)[3]
    return _PRODUCT["gelu"]


@pytest.mark.parametrize("kind", ["relu", "gelu_accurate"])
def test_tiny_model_fp32_vs_restated_oracle(kind):
    o = model_oracle(kind, rounded=False)
    model, loss, log, logits = model_product(kind, torch.float32)
    d_logit = float((logits - o["logits"]).abs().max())
    grads = {k: p.grad for k, p in named_canonical_params(model).items()}
    worst, n = (0.0, ""), 0
    for name, ref in o["grads"].items():
        if ref is None:
            continue
        gr = split_qkv_grad(name, grads)
        assert gr is not None, name
        n += 1
        err = float((gr.float().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        worst = max(worst, (err, name))
    print(f"[tiny {kind} fp32] logits |err| {d_logit:.3e}; {n} gradients, worst |err| / max(1, |g|max) {worst[0]:.3e} ({worst[1]})")
    assert d_logit < 1e-3
    for k in ("ncorrect", "total_positive"):
        assert int(log[k]) == o["counters"][k], k
    assert worst[0] <= 1e-3, worst
    assert n > 40
    if kind == "relu":      # the flag reaches the kernel: relu is not gelu by far more than the gate
        d = float((logits - gelu_logits_fp32()).abs().max())
        print(f"[tiny relu fp32] max |relu logits - gelu logits| = {d:.3e}")
        assert d > 1e-3


@pytest.mark.parametrize("kind", ["relu", "gelu_accurate"])
def test_tiny_model_bf16_vs_restated_fp32_oracle(kind):
    o = model_oracle(kind, rounded=True)
    model, loss, log, lg = model_product(kind, torch.bfloat16)
    d_logit = float((lg - o["logits"]).abs().max())
    grads = {n: getattr(p, "main_grad", None) for n, p in named_canonical_params(model).items()}
    rows, tiny = [], []
    for name, ref in o["grads"].items():
        if ref is None:
            continue
        gr = split_qkv_grad(name, grads)
        assert gr is not None, name
        rn = float(ref.double().norm())
        if rn < 1e-6:
            tiny.append((name, float(gr.float().norm())))
            continue
        floor = 0.5 if name == "node_classifier.bias" else 0.0
        rel = float((gr.float().cpu().double() - ref.double()).norm()) / max(rn, floor)
        rows.append((rel, name, rn, ref.numel()))
    rows.sort(reverse=True)
    print(f"[tiny {kind} bf16] logits |err| {d_logit:.3e}; loss {loss:.4f} vs {o['loss']:.4f}; {len(rows)} gradients; worst rel-L2: "
          + "; ".join(f"{n} {r:.3e} (|g| {rn:.2e}, {ne} el)" for r, n, rn, ne in rows[:6]))
    assert d_logit < BF16_LOGIT_ABS, d_logit
    assert abs(loss - o["loss"]) < 0.15 + 0.01 * abs(o["loss"])
    margin = (o["logits"][:, 1] - o["logits"][:, 0])
    pred_ref, pred = margin > 0, (lg[:, 1] - lg[:, 0]) > 0
    clear = margin.abs() > 2 * BF16_LOGIT_ABS
    assert bool((pred_ref[clear] == pred[clear]).all())
    assert int(log["total_positive"]) == o["counters"]["total_positive"]
    for name, nrm in tiny:
        assert nrm < 5e-3, name
    bad = [(n, r) for r, n, _, _ in rows if r > BF16_GRAD_REL_L2]
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ launcher
def test_launcher_trains_with_relu():
    """three updates of train.py on the synthetic task with --activation-fn relu (the sizes of the smallest case of
    tests/test_train_gpu.py); two synthetic batches and --update-freq 2, so every update sees the same trees and a small
    step along the gradient has to lower their loss"""
    from multimodaldiscussiontransformer_amd import train
    argv = ["--task", "node_prediction", "--arch", "multi_graphormer_base", "--criterion", "node_cross_entropy",
            "--dataset-name", "synthetic", "--batch-size", "8", "--update-freq", "2", "--lr", "5e-4", "--end-learning-rate", "1e-5",
            "--warmup-updates", "3", "--total-num-update", "8", "--encoder-embed-dim", "128", "--encoder-ffn-embed-dim", "128",
            "--encoder-attention-heads", "2", "--num_fusion_layers", "0", "--num_bottleneck_tokens", "2",
            "--attention-dropout", "0", "--act-dropout", "0", "--dropout", "0", "--spatial-pos-max", "5", "--log-interval", "1",
            "--synthetic-nodes", "6", "--synthetic-seq-len", "12", "--synthetic-batches", "2", "--seed", "5",
            "--bert-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "vocab": 512, "max_pos": 64}',
            "--vit-config", '{"dim": 128, "layers": 2, "heads": 2, "intermediate": 128, "image_size": 32, "patch": 16}',
            "--activation-fn", "relu", "--max-update", "3", "--no-save"]
    hist = train.main(argv)
    assert [h["num_updates"] for h in hist] == [1, 2, 3]
    print("[launcher relu] losses " + ", ".join(f"{h['loss']:.5f}" for h in hist))
    assert all(math.isfinite(h["loss"]) for h in hist)
    assert hist[2]["loss"] < hist[0]["loss"]
    layers = train.main.last_run["model"].encoder.graph_encoder.layers
    assert all(m.activation_fn == "relu" for st in layers for m in st.layers)


def test_enable_fp8_with_relu_raises():
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    hp, _ = tiny_case()
    for kind in ("relu", "gelu"):
        args = model_args(hp)
        args.activation_fn = kind
        model = GraphormerModel.build_model(args, task=None).cuda()
        if kind == "relu":
            with pytest.raises(NotImplementedError, match="fp8.*relu|relu.*fp8"):
                model.enable_fp8(True)
            assert model.enable_fp8(False) is None
        else:
            try:
                assert model.enable_fp8(True) is not None
            finally:
                model.enable_fp8(False)
