"""BASELINE.json configs[0] — Tiny mDT: D 128, BERT-mini split 2 + 2 (2 heads of 64), 2 executed graph layers with 8 heads of
16, eight 16-comment trees — in the production dtype.  The 16-wide graph heads run the bf16 MFMA attention kernels
(csrc/attention_v2.hip, head_dim 16); before those existed the first graph layer raised MdtUnsupported.

The assertions are those of tests/test_real_shapes_gpu.py::test_bf16_real_shapes_vs_fp32_oracle, which lists M, C2, C4 and
LAUNCH: logits within BF16_LOGIT_ABS of the fp32 oracle on the same bf16-rounded weights, the loss, predictions wherever the
fp32 margin is clear, total_positive, and every parameter gradient within BF16_GRAD_REL_L2 in relative L2."""
import pytest
import torch

from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2, BF16_LOGIT_ABS, oracle_run, product_run
from tests.util_model import named_canonical_params, split_qkv_grad

pytestmark = pytest.mark.gpu


def test_tiny_mdt_bf16_vs_fp32_oracle():
    kind = "C1"
    o = oracle_run(kind, rounded=True)
    model, pb, loss, sample_size, log, logits, glob = product_run(kind, torch.bfloat16, True, main_grad=True)
    lg = logits.float().cpu()
    d_logit = float((lg - o["logits"]).abs().max())
    grads = {n: getattr(p, "main_grad", None) for n, p in named_canonical_params(model).items()}
    rows = []
    tiny = []
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
        # the classifier bias gradient is a sum of ~n_labels terms of magnitude ~0.5 that cancel to ~0.1: its error is
        # measured against the scale of what is summed, not against the cancelled result
        floor = 0.5 if name == "node_classifier.bias" else 0.0
        rel = float((gr.float().cpu().double() - ref.double()).norm()) / max(rn, floor)
        rows.append((rel, name, rn, ref.numel()))
    rows.sort(reverse=True)
    print(f"[{kind} bf16] logits |err| {d_logit:.3e}; loss {loss:.4f} vs {o['loss']:.4f}; {len(rows)} gradients; worst rel-L2: "
          + "; ".join(f"{n} {r:.3e} (|g| {rn:.2e}, {ne} el)" for r, n, rn, ne in rows[:8]))
    assert d_logit < BF16_LOGIT_ABS, d_logit
    assert abs(loss - o["loss"]) < 0.15 + 0.01 * abs(o["loss"])
    # predictions may differ only where the fp32 margin is inside the bf16 logit tolerance
    margin = (o["logits"][:, 1] - o["logits"][:, 0])
    pred_ref, pred = margin > 0, (lg[:, 1] - lg[:, 0]) > 0
    clear = margin.abs() > 2 * BF16_LOGIT_ABS
    assert bool((pred_ref[clear] == pred[clear]).all())
    assert int(log["total_positive"]) == o["counters"]["total_positive"]
    for name, nrm in tiny:
        assert nrm < 5e-3, name
    bad = [(n, r) for r, n, _, _ in rows if r > BF16_GRAD_REL_L2]
    assert not bad, bad[:10]
