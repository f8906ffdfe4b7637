"""Drop-in for mDT/src/criterions/hatespeech_loss.py (criterion ``node_cross_entropy``).

The weighted two-class cross entropy, the fp16 rounding of logits / class weights the
reference applies whatever the model dtype (``.type(torch.HalfTensor)``, :58-64, :95) and the
TP / FP / FN counters are one HIP kernel (``mdt_node_ce``); labelled rows come from the
packer's CSR index instead of a boolean-mask gather.  ``reduce_metrics`` reproduces the
reference's accuracy / precision / recall / F1 with its zero guards (:133-173).

Not in the reference: ``label_smoothing`` and ``focal_gamma``.  With either one non-zero the loss is the label-smoothed / focal
objective of ``mdt_node_objective`` and the logging output carries ``nll_loss``, the plain weighted NLL of the
same launch; with both at 0 nothing differs from the reference's criterion.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Dict, List

import torch

from .. import ops
from ..data.packer import packed_from_batched_data
from ..registry import FairseqCriterion, FairseqDataclass, register_criterion


@dataclass
class GraphPredictionNodeCrossEntropyConfig(FairseqDataclass):
    positive_weight: float = field(default=1.0, metadata={"help": "Weight to associate to the positive class"})
    negative_weight: float = field(default=1.0, metadata={"help": "Weight to associate to the negative class"})
    # not reference fields: with either one non-zero the loss is ops.node_objective (csrc/node_objective.hip)
    # ("opt_in": the launcher's derived flag stays None until given, train.py build_parser)
    label_smoothing: float = field(default=0.0, metadata={"opt_in": True, "help": "FairSeq's epsilon in [0, 1): the target distribution "
                                                                                  "is (1 - eps) one-hot + eps / 2 uniform"})
    focal_gamma: float = field(default=0.0, metadata={"opt_in": True, "help": "focal loss exponent >= 0: the hard-target term of a row "
                                                                              "is scaled by (1 - p_target)^gamma"})


def check_objective(label_smoothing: float, focal_gamma: float) -> None:
    """The ranges mdt_node_objective accepts (a NaN fails both comparisons)."""
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
    if not (focal_gamma >= 0.0 and math.isfinite(focal_gamma)):
        raise ValueError(f"focal_gamma must be finite and >= 0, got {focal_gamma!r}")


class _NodeObjective(torch.autograd.Function):
    """→ (objective f32[1], plain weighted NLL f32[1], counters); the gradient flows through the objective only."""

    @staticmethod
    def forward(ctx, logits, rows, targets, w_neg, w_pos, fp16_loss, label_smoothing, focal_gamma):
        out, counters, dlogits = ops.node_objective(logits.contiguous(), rows, targets, w_neg, w_pos, label_smoothing=label_smoothing,
                                                    focal_gamma=focal_gamma, fp16_loss=fp16_loss)
        ctx.save_for_backward(dlogits)
        loss, nll = out[0:1], out[1:2]
        ctx.mark_non_differentiable(nll, counters)
        return loss, nll, counters

    @staticmethod
    def backward(ctx, gloss, _gn, _gc):
        (dlogits,) = ctx.saved_tensors
        return dlogits * gloss.to(dlogits.dtype), None, None, None, None, None, None, None


class _NodeCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, rows, targets, w_neg, w_pos, fp16_loss):
        loss, counters, dlogits = ops.node_ce(logits.contiguous(), rows, targets, w_neg, w_pos, fp16_loss=fp16_loss)
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(counters)
        return loss, counters

    @staticmethod
    def backward(ctx, gloss, _gc):
        (dlogits,) = ctx.saved_tensors
        return dlogits * gloss.to(dlogits.dtype), None, None, None, None, None


@register_criterion("node_cross_entropy", dataclass=GraphPredictionNodeCrossEntropyConfig)
class GraphPredictionNodeCrossEntropy(FairseqCriterion):
    """Node cross-entropy loss for graph node classification."""

    def __init__(self, task, positive_weight: float = 1.0, negative_weight: float = 1.0, fp16_loss: bool = True, *,
                 label_smoothing: float = 0.0, focal_gamma: float = 0.0) -> None:
        super().__init__(task)
        self.positive_weight = float(positive_weight)
        self.negative_weight = float(negative_weight)
        self.fp16_loss = fp16_loss
        self.label_smoothing, self.focal_gamma = float(label_smoothing or 0.0), float(focal_gamma or 0.0)
        check_objective(self.label_smoothing, self.focal_gamma)
        # the reference keeps the weights as a half tensor [negative, positive]
        self.weight = torch.tensor([negative_weight, positive_weight], dtype=torch.half)

    def forward(self, model, sample: Dict[str, Any], reduce=True):
        """→ (loss, sample_size, logging_output) exactly as the reference (:66-131)."""
        if not reduce:
            raise NotImplementedError("reduce=False is never used by the reference trainer")
        bd = sample["net_input"]["batched_data"]
        num_comments = bd["x"].shape[1]
        comment_logits, _ = model(**sample["net_input"])
        pb = packed_from_batched_data(bd)
        nll = None
        if self.label_smoothing == 0.0 and self.focal_gamma == 0.0:
            loss, counters = _NodeCE.apply(comment_logits, pb.label_rows, pb.targets, self.negative_weight,
                                           self.positive_weight, self.fp16_loss)
        else:
            loss, nll, counters = _NodeObjective.apply(comment_logits, pb.label_rows, pb.targets, self.negative_weight,
                                                       self.positive_weight, self.fp16_loss, self.label_smoothing, self.focal_gamma)
        loss = loss.squeeze(0)
        sample_size = pb.n_labels
        logging_output = {
            "loss": loss.data, "sample_size": sample_size, "nsentences": sample_size, "ntokens": num_comments,
            "ncorrect": counters[0], "num_positive_correct": counters[1], "total_positive": counters[2],
            "num_pred_positive": counters[3],
        }
        if nll is not None:
            logging_output["nll_loss"] = nll.squeeze(0)      # the plain weighted NLL: comparable between objectives
        return loss, sample_size, logging_output

    @staticmethod
    def compute_metrics(logging_outputs: List[Dict[str, Any]]) -> Dict[str, float]:
        def tot(k):
            return sum(float(log.get(k, 0)) for log in logging_outputs)

        loss_sum, sample_size = tot("loss"), tot("sample_size")
        out = {"loss": loss_sum / sample_size if sample_size else 0.0}
        if any("nll_loss" in log for log in logging_outputs):
            out["nll_loss"] = tot("nll_loss") / sample_size if sample_size else 0.0
        if len(logging_outputs) > 0 and "ncorrect" in logging_outputs[0]:
            ncorrect, tp, total_pos, pred_pos = tot("ncorrect"), tot("num_positive_correct"), tot("total_positive"), tot("num_pred_positive")
            recall = 0 if total_pos == 0 else tp / total_pos
            precision = 0 if pred_pos == 0 else tp / pred_pos
            f1 = 0 if (precision == 0 and recall == 0) else 2 * ((precision * recall) / (precision + recall))
            out.update(accuracy=ncorrect / sample_size, recall=recall, precision=precision, f1=f1)
        return out

    @staticmethod
    def reduce_metrics(logging_outputs) -> None:
        """Aggregate logging outputs from data parallel training; logs through fairseq.metrics when
        fairseq is installed, otherwise keeps the values in ``last_metrics``."""
        m = GraphPredictionNodeCrossEntropy.compute_metrics(logging_outputs)
        GraphPredictionNodeCrossEntropy.last_metrics = m
        try:
            from fairseq import metrics
        except ImportError:
            return
        sample_size = sum(float(log.get("sample_size", 0)) for log in logging_outputs)
        for k, v in m.items():
            metrics.log_scalar(k, v, sample_size, round=3)

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True
