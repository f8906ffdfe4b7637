"""Full models whose graph heads are 128 and 96 wide, against the oracle: D 256 with 2 graph heads (128; encoder heads of 64)
and D 384 with 4 graph heads (96; encoder heads of 64).  2 + 2 text layers, one fusion layer, text only, four 12-comment trees
with every comment labelled.  Before the wide attention kernels existed the first graph layer raised MdtUnsupported.

fp32: logits and every parameter gradient within 1e-3 (<= 1e-3 * max(1, |g|max)), counters equal — the gate of
tests/test_real_shapes_gpu.py::test_sequences_beyond_272_tokens_fp32_vs_oracle.
bf16: the assertions of tests/test_tiny_bf16_gpu.py — logits within BF16_LOGIT_ABS, every parameter gradient within
BF16_GRAD_REL_L2 in relative L2 of the fp32 oracle on the bf16-rounded weights."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import mdt_ref_cpu as R
from oracle import structure as S
from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2, BF16_LOGIT_ABS
from tests.util_model import fill_hash_weights, model_args, named_canonical_params, split_qkv_grad

SHAPES = {128: dict(dim=256, enc_heads=4, graph_heads=2), 96: dict(dim=384, enc_heads=6, graph_heads=4)}
_ORACLE = {}


def test_registered_architecture_defaults_to_128_wide_heads():
    """Why the width matters: multi_graphormer, as registered, is 1024 / 8."""
    import multimodaldiscussiontransformer_amd.models  # noqa: F401
    from multimodaldiscussiontransformer_amd.registry import ARCH_CONFIG_REGISTRY
    args = Namespace()
    ARCH_CONFIG_REGISTRY["multi_graphormer"](args)
    assert args.encoder_embed_dim // args.encoder_attention_heads == 128


def case(hd):
    from multimodaldiscussiontransformer_amd import synthetic
    s = SHAPES[hd]
    hp = R.hparams(enc_ffn=2 * s["dim"], graph_ffn=s["dim"], text_layers=4, vit_layers=4, num_fusion_layers=1, num_fusion_stack=1,
                   num_graph_stack=1, num_bottleneck=4, vocab_size=600, max_pos=64, image_size=32, patch=16, pos_weight=1.5,
                   neg_weight=1.0, **s)
    assert hp.dim // hp.graph_heads == hd and hp.dim // hp.enc_heads == 64
    rng = np.random.Generator(np.random.PCG64(1000 + hd))
    trees = [synthetic.make_tree(12, rng, seq_len=16, vocab_size=hp.vocab_size, image_frac=0.0, image_size=hp.image_size, min_len=3)
             for _ in range(4)]
    for i, t in enumerate(trees):
        n = len(t["parent"])
        t["y_mask"][:] = True
        t["y"] = np.asarray([(k + i) % 2 for k in range(n)], dtype=np.float32)
    return hp, trees


def oracle_run(hd, rounded):
    """fp32 oracle forward + backward, once per (width, weights rounded to bf16 or not)."""
    if (hd, rounded) not in _ORACLE:
        hp, trees = case(hd)
        W = R.make_weights(hp)
        if rounded:
            W = {n: w.detach().bfloat16().float().requires_grad_(not R.is_frozen(hp, n)) for n, w in W.items()}
        batch = R.to_torch_batch(S.collate(trees, 5))
        logits, _ = R.model_forward(W, hp, batch)
        loss, counters = R.node_cross_entropy(logits, batch["y"], batch["y_mask"], hp)
        loss.backward()
        _ORACLE[(hd, rounded)] = dict(logits=logits.detach(), loss=float(loss.detach()), counters=counters,
                                      grads={n: (None if w.grad is None else w.grad.detach()) for n, w in W.items()})
    return _ORACLE[(hd, rounded)]


def product_run(hd, dtype):
    from multimodaldiscussiontransformer_amd.criterions import GraphPredictionNodeCrossEntropy
    from multimodaldiscussiontransformer_amd.data.packer import pack_batch
    from multimodaldiscussiontransformer_amd.models import GraphormerModel
    hp, trees = case(hd)
    model = fill_hash_weights(GraphormerModel.build_model(model_args(hp), task=None)).cuda().to(dtype).train()
    if dtype == torch.bfloat16:
        model.prepare_main_grads()
    pb = pack_batch(trees, 5)
    crit = GraphPredictionNodeCrossEntropy(None, positive_weight=hp.pos_weight, negative_weight=hp.neg_weight)
    loss, _, log = crit(model, {"nsamples": len(trees), "net_input": {"batched_data": pb.batched_data}})
    loss.backward()
    with torch.no_grad():
        logits, _ = model(pb.batched_data)
    torch.cuda.synchronize()
    return model, float(loss.detach()), log, logits.float().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [128, 96])
def test_wide_graph_heads_fp32_vs_oracle(hd):
    o = oracle_run(hd, rounded=False)
    model, loss, log, logits = product_run(hd, torch.float32)
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
    print(f"[hd{hd} model fp32] logits |err| {d_logit:.3e}; {n} gradients, worst |err| / max(1, |g|max) {worst[0]:.3e} ({worst[1]})")
    assert d_logit < 1e-3
    for k in ("ncorrect", "total_positive"):
        assert int(log[k]) == o["counters"][k], k
    assert worst[0] <= 1e-3, worst
    assert n > 40


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [128, 96])
def test_wide_graph_heads_bf16_vs_fp32_oracle(hd):
    o = oracle_run(hd, rounded=True)
    model, loss, log, lg = product_run(hd, torch.bfloat16)
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
            # mathematically zero (a key bias shifts every score of a row alike): what is left is rounding noise
            tiny.append((name, float(gr.float().norm())))
            continue
        # the classifier bias gradient is a sum of ~n_labels terms of magnitude ~0.5 that cancel: its error is measured
        # against the scale of what is summed, not against the cancelled result
        floor = 0.5 if name == "node_classifier.bias" else 0.0
        rel = float((gr.float().cpu().double() - ref.double()).norm()) / max(rn, floor)
        rows.append((rel, name, rn, ref.numel()))
    rows.sort(reverse=True)
    print(f"[hd{hd} model bf16] logits |err| {d_logit:.3e}; loss {loss:.4f} vs {o['loss']:.4f}; {len(rows)} gradients; worst rel-L2: "
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
