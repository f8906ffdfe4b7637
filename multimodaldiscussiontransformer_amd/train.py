"""Minimal ``fairseq-train``-compatible launcher for the HIP-backed mDT (fairseq itself is optional).

Accepts the flags of mDT/experiments/hateful_discussions/run_train.sh:28-65 with the same
spellings (flags it does not implement are refused; the few it accepts without effect —
--wandb-project, --num-workers, --required-batch-size-multiple — say so on stderr), resolves --task / --arch / --criterion / --dataset-name through
``registry.py``, and runs the reference recipe: Adam(0.9, 0.999, eps 1e-8, wd 0.01),
polynomial-decay LR with warm-up, --update-freq gradient accumulation, gradient scaling by
1 / (global) sample size, ``--clip-norm`` / the ``gnorm`` meter / the non-finite-update guard computed on the
device (optim.py), bf16 (``--fp16`` in the reference) with fp32 master weights, RCCL
data parallelism when launched under ``torch.distributed.run``.

Without a registered dataset (the HatefulDiscussions graphs are private) ``--dataset-name
synthetic`` trains on generated discussion trees whose label depends on the labelled comment's
text, which is what the smoke test uses.

  python -m multimodaldiscussiontransformer_amd.train --task node_prediction --arch multi_graphormer_base \\
      --criterion node_cross_entropy --dataset-name synthetic --batch-size 12 --max-update 50 ...
"""
from __future__ import annotations

import argparse
import ast
import json
import math
import os
import sys
import time

import numpy as np
import torch

from . import synthetic
from .registry import ARCH_CONFIG_REGISTRY, ARCH_MODEL_REGISTRY, CRITERION_REGISTRY, MODEL_REGISTRY, TASK_REGISTRY


def build_parser():
    from . import criterions, models, tasks  # noqa: F401  (registration side effects)
    # argument_default=SUPPRESS: model flags that are not given stay absent, so the architecture functions
    # fill their defaults exactly as under fairseq-train
    p = argparse.ArgumentParser(allow_abbrev=False, argument_default=argparse.SUPPRESS)
    p.add_argument("--user-dir", default=None)
    p.add_argument("--num-workers", type=int, default=0)
    p.add_argument("--task", default="node_prediction")
    p.add_argument("--criterion", default="node_cross_entropy")
    p.add_argument("--arch", default="multi_graphormer_base")
    p.add_argument("--optimizer", default="adam")
    p.add_argument("--adam-betas", default="(0.9, 0.999)")
    p.add_argument("--adam-eps", type=float, default=1e-8)
    p.add_argument("--weight-decay", type=float, default=0.01)
    p.add_argument("--lr-scheduler", default="polynomial_decay")
    p.add_argument("--power", type=float, default=1.0)
    p.add_argument("--warmup-updates", type=int, default=0)
    p.add_argument("--total-num-update", type=int, default=10820)
    p.add_argument("--lr", type=float, default=3e-5)
    p.add_argument("--end-learning-rate", type=float, default=3e-7)
    p.add_argument("--batch-size", type=int, default=12)
    p.add_argument("--update-freq", type=int, default=1)
    p.add_argument("--max-epoch", type=int, default=0)
    p.add_argument("--max-update", type=int, default=0)
    p.add_argument("--fp16", action="store_true", default=False, help="the reference's half precision; runs as bf16 here")
    p.add_argument("--bf16", action="store_true", default=False)
    p.add_argument("--fp8", action="store_true", default=False,
                   help="BASELINE.json configs[4] (not a reference flag): bf16 run with per-tensor-scaled fp8 operands in the blocks' big GEMMs (fp8.py)")
    p.add_argument("--fp8-sites", default=None, help="preset (all | fast4 | grads) or comma list of fp8 sites (fp8.PRESETS); default all")
    p.add_argument("--deterministic", action="store_true", default=False,
                   help="not a reference flag: ordered gradient reductions instead of fp32 atomics (engine.set_deterministic) — loss, "
                        "gradients and parameters are bit-for-bit reproducible in one process on one GPU; bf16 / fp32 only, not with --fp8")
    p.add_argument("--checkpoint-activations", action="store_true", default=False,
                   help="FairSeq's flag: recompute the activations of the pretrained BERT / ViT blocks in backward instead of keeping them "
                        "(engine.set_recompute) — the same loss and gradients from a fraction of the activation memory, for one more "
                        "forward of those blocks; bf16 / fp32 only, not with --fp8")
    p.add_argument("--checkpoint-policy", choices=("block", "ffn"), default=None,
                   help="with --checkpoint-activations: block (default) keeps only each block's input and output and replays its forward; "
                        "ffn keeps everything but the two F-wide FFN tensors and repeats one fc1 GEMM per block")
    # FairSeq's EMA flags (fairseq/dataclass/configs.py EMAConfig); defaults are filled in main() so that a flag given without
    # --store-ema can be told from one left alone
    p.add_argument("--store-ema", action="store_true", default=False,
                   help="keep an fp32 exponential moving average of the trainable weights (updated inside the fused Adam launch) and "
                        "store it in checkpoints as extra_state['ema']")
    p.add_argument("--ema-decay", type=float, default=None, help="FairSeq's default: 0.9999")
    p.add_argument("--ema-start-update", type=int, default=None, help="the average is a copy of the weights before this update (default 0)")
    p.add_argument("--ema-update-freq", type=int, default=None, help="update the average every N updates (default 1)")
    p.add_argument("--ema-fp32", action="store_true", default=None, help="accepted: the average here is always fp32, built from the fp32 masters")
    p.add_argument("--validate-with-ema", action="store_true", default=None,
                   help="not a FairSeq flag: run the validation passes with the averaged weights (FusedAdam.ema_weights) — the validation "
                        "log line then carries \"weights\": \"ema\"")
    # parameter groups of the fused Adam step (not reference flags): GraphormerModel.optimizer_groups
    p.add_argument("--encoder-lr-scale", type=float, default=1.0,
                   help="not a reference flag: learning-rate scale of the pretrained BERT / ViT embeddings and blocks (finite, >= 0; 0 freezes "
                        "them while their Adam moments advance)")
    p.add_argument("--encoder-layer-decay", type=float, default=1.0,
                   help="not a reference flag: layer-wise rate decay G in (0, 1] down the pretrained stacks — the block with original index i "
                        "of a depth-L encoder runs at --encoder-lr-scale * G^(L - i), its embeddings at G^(L + 1)")
    p.add_argument("--no-decay-bias-norm", action="store_true", default=False,
                   help="not a reference flag: weight decay 0 for biases and LayerNorm weights (every parameter with ndim <= 1)")
    # parameter-efficient fine-tuning (not reference flags): GraphormerModel.add_lora
    p.add_argument("--lora-rank", type=int, default=0,
                   help="not a reference flag: freeze the pretrained BERT / ViT embeddings and blocks and train rank-N adapters (8, 16, 32 "
                        "or 64) beside the --lora-targets layers of every pretrained block (with --freeze_initial_encoders: of the fusion "
                        "blocks); 0: off")
    p.add_argument("--lora-alpha", type=float, default=None, help="adapter scale numerator: the adapter sum is scaled by alpha / rank "
                   "(finite, > 0; default 2 * rank)")
    p.add_argument("--lora-targets", default=None, help="comma list out of q,k,v,out,fc1,fc2 (out: the attention output "
                   "projection; fc1 / fc2: the FFN's two dense layers), or all: the layers that get adapters (default q,v)")
    p.add_argument("--lora-dropout", type=float, default=None, help="with --lora-rank: PEFT's lora_dropout — in training every adapter "
                   "reads dropout(x) with this probability (0 <= P < 1; default 0: off); the masks are made inside the adapter kernels")
    p.add_argument("--save-merged", default="", help="with --lora-rank: also write, at the end, a plain checkpoint with the adapters "
                   "folded into the projections (GraphormerModel.merge_lora) — it loads into a model built without --lora-rank")
    p.add_argument("--log-interval", type=int, default=10)
    # criterion flags: every field of every registered criterion's config dataclass (FairSeq derives them the same way)
    from .registry import CRITERION_REGISTRY as _CR
    for _cls, _dc in _CR.values():
        for f in getattr(_dc, "__dataclass_fields__", {}).values():
            if f.name.startswith("_"):
                continue
            flag = "--" + f.name.replace("_", "-")
            if f.type in (bool, "bool"):
                p.add_argument(flag, type=lambda v: str(v).lower() in ("1", "true", "yes"), nargs="?", const=True, default=f.default)
            else:
                # an opt-in field (--label-smoothing, --focal-gamma) stays None until given: main() keeps it out of the
                # checkpoint cfg of a run without it and can tell "not given" from "given as 0" when it restores
                p.add_argument(flag, type=type(f.default), default=None if f.metadata.get("opt_in") else f.default)
    p.add_argument("--distributed-world-size", type=int, default=1)
    p.add_argument("--save-checkpoint", default="", help="write a FairSeq-layout checkpoint here at the end")
    p.add_argument("--save-dir", default="", help="FairSeq: checkpoint_last.pt (and checkpoint<epoch>.pt) are written here")
    p.add_argument("--save-interval-updates", type=int, default=0)
    p.add_argument("--no-save", action="store_true", default=False)
    p.add_argument("--restore-file", default="", help="FairSeq checkpoint to start from (run_train.sh:58)")
    p.add_argument("--reset-optimizer", action="store_true", default=False)
    p.add_argument("--reset-lr-scheduler", action="store_true", default=False)
    p.add_argument("--reset-meters", action="store_true", default=False)
    p.add_argument("--reset-dataloader", action="store_true", default=False)
    p.add_argument("--clip-norm", type=float, default=0.0)
    p.add_argument("--required-batch-size-multiple", type=int, default=1)
    p.add_argument("--validate-interval-updates", type=int, default=0,
                   help="run_train.sh:42 — every N updates (and after the last one) an eval-mode pass over --valid-subset")
    p.add_argument("--valid-subset", default="valid")
    p.add_argument("--disable-validation", action="store_true", default=False)
    p.add_argument("--synthetic-valid-batches", type=int, default=2)
    p.add_argument("--wandb-project", default=None)
    # synthetic data controls
    p.add_argument("--synthetic-nodes", type=int, default=16)
    p.add_argument("--synthetic-seq-len", type=int, default=32)
    p.add_argument("--synthetic-image-frac", type=float, default=0.0)
    p.add_argument("--synthetic-batches", type=int, default=8)
    p.add_argument("--bert-config", type=json.loads, default=None, help="JSON overrides of the BERT shape (tests)")
    p.add_argument("--vit-config", type=json.loads, default=None)
    # task flags (mDT/src/tasks/task.py:29-113)
    from .tasks import TaskConfig
    for f in TaskConfig.__dataclass_fields__.values():
        flag = "--" + f.name.replace("_", "-")
        if f.type in (bool, "bool"):
            p.add_argument(flag, action="store_true", default=False)
        else:
            p.add_argument(flag, type=type(f.default), default=f.default)
    MODEL_REGISTRY["multi_graphormer"].add_args(p)
    return p


def synthetic_batches(args, task, rank):
    """Discussion trees whose labelled comment is hateful iff its second token id is in the upper half of
    the vocabulary — learnable from the text encoder alone, so a few dozen updates move the loss."""
    vocab = (args.bert_config or {}).get("vocab", 30522)
    img = (args.vit_config or {}).get("image_size", 224)
    out = []
    for i in range(args.synthetic_batches):
        trees = synthetic.make_trees(args.batch_size, args.synthetic_nodes, seed=args.seed * 7919 + rank * 1000 + i,
                                     seq_len=args.synthetic_seq_len, vocab_size=vocab, image_frac=args.synthetic_image_frac,
                                     image_size=img, min_len=4)
        for t in trees:
            m = int(np.nonzero(t["y_mask"])[0][0])
            t["y"] = np.asarray([1.0 if t["input_ids"][m, 1] >= vocab // 2 else 0.0], dtype=np.float32)
        out.append(task.collate(trees))
    return out


def main(argv=None):
    """Train; → the logged metrics.  The activation-recomputation policy is a process-wide switch that ``_main`` sets before
    it builds the model: it is put back however the run ends, so a later run in this process starts as this one found it."""
    from . import engine
    was_recompute = engine.recompute()
    try:
        return _main(argv)
    finally:
        engine.set_recompute(was_recompute)


def _main(argv):
    parser = build_parser()
    args, unknown = parser.parse_known_args(argv)
    if unknown:
        # a flag this launcher does not know may change what is trained: refuse instead of training something else
        raise SystemExit(f"[mdt-train] unsupported FairSeq flag(s): {' '.join(unknown)} — this launcher implements the flags of "
                         "mDT/experiments/hateful_discussions/run_train.sh; run fairseq-train --user-dir <repo>/src for the rest")
    if args.clip_norm < 0:
        raise SystemExit("[mdt-train] --clip-norm must be >= 0 (0: measure gnorm and guard against non-finite updates, no clipping)")
    if args.fp16:
        print("[mdt-train] --fp16: runs as bf16 with fp32 master weights and NO loss scaling; an update whose gradient norm is "
              "not finite is skipped and counted (skipped_updates), there is no scale to lower", file=sys.stderr)
    if args.wandb_project:
        print("[mdt-train] --wandb-project: metrics are printed as JSON lines, nothing is sent to wandb", file=sys.stderr)
    # accepted for launch-script compatibility, without effect here — said, not silent
    if args.num_workers:
        print("[mdt-train] --num-workers: ignored — batches are packed by the native packer in ONE prefetch thread (data/prefetch.py)", file=sys.stderr)
    if args.required_batch_size_multiple != 1:
        print("[mdt-train] --required-batch-size-multiple: ignored — batches hold exactly --batch-size trees (the last one of an epoch may be smaller)",
              file=sys.stderr)
    ema_names = ["ema_decay", "ema_start_update", "ema_update_freq", "ema_fp32", "validate_with_ema"]
    ema_flags = [f for f in ema_names if getattr(args, f) is not None]
    if ema_flags and not args.store_ema:
        raise SystemExit("[mdt-train] " + ", ".join("--" + f.replace("_", "-") for f in ema_flags) + " without --store-ema: there is no "
                         "weight average to configure, evaluate or store — add --store-ema")
    if args.store_ema:
        if args.ema_fp32:
            print("[mdt-train] --ema-fp32: the average is always fp32 here, built from the fp32 master weights", file=sys.stderr)
        args.ema_decay = 0.9999 if args.ema_decay is None else args.ema_decay
        args.ema_start_update = args.ema_start_update or 0
        args.ema_update_freq = args.ema_update_freq or 1
        if not 0.0 <= args.ema_decay <= 1.0 or args.ema_update_freq < 1:
            raise SystemExit("[mdt-train] --ema-decay must lie in [0, 1] and --ema-update-freq be >= 1")
    store_ema, validate_with_ema = args.store_ema, bool(args.validate_with_ema)
    args.ema_fp32, args.validate_with_ema = bool(args.ema_fp32), validate_with_ema
    if not store_ema:
        for f in ["store_ema"] + ema_names:      # a run without the average writes the checkpoint (its cfg included) it always wrote
            delattr(args, f)
    if not (math.isfinite(args.encoder_lr_scale) and args.encoder_lr_scale >= 0.0):
        raise SystemExit("[mdt-train] --encoder-lr-scale must be finite and >= 0")
    if not (math.isfinite(args.encoder_layer_decay) and 0.0 < args.encoder_layer_decay <= 1.0):
        raise SystemExit("[mdt-train] --encoder-layer-decay must be finite and lie in (0, 1]")
    group_flags = dict(encoder_lr_scale=args.encoder_lr_scale, encoder_layer_decay=args.encoder_layer_decay,
                       no_decay_bias_norm=bool(args.no_decay_bias_norm))
    use_groups = group_flags != dict(encoder_lr_scale=1.0, encoder_layer_decay=1.0, no_decay_bias_norm=False)
    if not use_groups:
        for f in group_flags:                    # flags left at their defaults: the optimiser, the log lines and the checkpoint cfg of a run without them
            delattr(args, f)
    lora_rank, save_merged = int(args.lora_rank or 0), args.save_merged
    lora_flags = [f for f in ("lora_alpha", "lora_targets", "lora_dropout") if getattr(args, f) is not None] + (["save_merged"] if save_merged else [])
    if lora_flags and not lora_rank:
        raise SystemExit("[mdt-train] " + ", ".join("--" + f.replace("_", "-") for f in lora_flags) + " without --lora-rank: there are no "
                         "adapters to configure or merge — add --lora-rank")
    delattr(args, "save_merged")                 # where a file goes is no property of the model: not part of a checkpoint's cfg
    if lora_rank:
        from .modules._fused import LORA_RANKS, parse_lora_targets
        if lora_rank not in LORA_RANKS:
            raise SystemExit(f"[mdt-train] --lora-rank must be one of {', '.join(map(str, LORA_RANKS))} (0: off)")
        args.lora_alpha = 2.0 * lora_rank if args.lora_alpha is None else args.lora_alpha
        if not (math.isfinite(args.lora_alpha) and args.lora_alpha > 0.0):
            raise SystemExit("[mdt-train] --lora-alpha must be finite and > 0")
        try:
            args.lora_targets = ",".join(parse_lora_targets(args.lora_targets or "q,v"))
        except ValueError as e:
            raise SystemExit(f"[mdt-train] --lora-targets: {e}")
        if args.lora_dropout is not None and not 0.0 <= args.lora_dropout < 1.0:      # NaN fails both comparisons
            raise SystemExit("[mdt-train] --lora-dropout must be in [0, 1)")
        if not args.lora_dropout:                # not given, or 0: the log line and the checkpoint cfg of a run without the flag
            delattr(args, "lora_dropout")
        if args.fp8:
            raise SystemExit("[mdt-train] --fp8 with --lora-rank: low-rank adapters with fp8 GEMMs are not supported (the adapter sum "
                             "enters the bf16 qkv buffer only) — train the adapters in bf16")
    else:
        for f in ("lora_rank", "lora_alpha", "lora_targets", "lora_dropout"):      # a run without adapters writes the checkpoint cfg it always wrote
            delattr(args, f)
    # --label-smoothing / --focal-gamma (criterions/hatespeech_loss.py): None until given.  Left alone, a restored run takes
    # them from its checkpoint's cfg (below, after the restore); a run without them keeps the cfg, the log keys and the
    # six-wide scalar vectors it always had.
    objective_names = ("label_smoothing", "focal_gamma")
    objective_given = [f for f in objective_names if getattr(args, f) is not None]
    if objective_given and args.criterion != "node_cross_entropy":
        raise SystemExit("[mdt-train] " + ", ".join("--" + f.replace("_", "-") for f in objective_given) + f" with --criterion "
                         f"{args.criterion}: only node_cross_entropy has a label-smoothed / focal objective")

    def set_objective(eps, gamma):
        """The two values into ``args`` where the objective is on, out of it where it is off; → on."""
        from .criterions.hatespeech_loss import check_objective
        eps, gamma = float(eps or 0.0), float(gamma or 0.0)
        try:
            check_objective(eps, gamma)
        except ValueError as e:
            raise SystemExit(f"[mdt-train] --label-smoothing must be in [0, 1) and --focal-gamma finite and >= 0 ({e})")
        on = eps != 0.0 or gamma != 0.0
        for f, v in zip(objective_names, (eps, gamma)):
            if on:
                setattr(args, f, v)
            elif hasattr(args, f):
                delattr(args, f)
        return on

    objective_on = set_objective(args.label_smoothing, args.focal_gamma)
    from . import engine
    was_deterministic = engine.deterministic()
    if args.deterministic:
        if args.fp8:
            raise SystemExit("[mdt-train] --deterministic with --fp8: the fp8 path has no ordered reductions")
        engine.set_deterministic(True)
        print("[mdt-train] --deterministic: ordered gradient reductions, no float atomics, one stream (one process, one GPU: "
              "the all-reduce order of several ranks is not fixed)", file=sys.stderr)
    ckpt_act, ckpt_policy = bool(args.checkpoint_activations), args.checkpoint_policy
    if ckpt_policy is not None and not ckpt_act:
        raise SystemExit("[mdt-train] --checkpoint-policy without --checkpoint-activations: there is nothing to recompute — add "
                         "--checkpoint-activations")
    if ckpt_act and args.fp8:
        raise SystemExit(f"[mdt-train] --checkpoint-activations with --fp8: {engine.RECOMPUTE_FP8_WHY}")
    for f in ("checkpoint_activations", "checkpoint_policy"):      # how activations are kept is no property of the model: the
        delattr(args, f)                                           # checkpoint cfg is that of a run without the flag
    if ckpt_act:
        engine.set_recompute(ckpt_policy or "block")               # before the model is built; main() puts it back
    import torch.distributed as dist
    from .ddp import DataParallel
    from .optim import FusedAdam, PolynomialDecayLR
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl")
    torch.manual_seed(args.seed)

    task_cls, task_cfg_cls = TASK_REGISTRY[args.task]
    cfg = task_cfg_cls(**{k: getattr(args, k) for k in task_cfg_cls.__dataclass_fields__})
    task = task_cls.setup_task(cfg)
    ARCH_CONFIG_REGISTRY[args.arch](args)
    assert ARCH_MODEL_REGISTRY[args.arch] in MODEL_REGISTRY
    # the reference's encoders come from from_pretrained() (multigraphormer_graph_encoder.py:236-245): build_model loads the same
    # HuggingFace weights from LOCAL files (--pretrained-bert / --pretrained-vit) unless the run starts from a checkpoint,
    # opts out (--random-init-encoders) or uses custom encoder shapes — a recipe that silently trained from random weights
    # would not be the reference's recipe
    args._skip_pretrained = bool(args.restore_file)
    try:
        model = task.build_model(args)
    except FileNotFoundError as e:
        raise SystemExit(f"[mdt-train] {e}\n[mdt-train] give --pretrained-bert / --pretrained-vit a local path, start from a "
                         f"checkpoint (--restore-file), or pass --random-init-encoders to train from random weights")
    if lora_rank and rank == 0:
        n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
        n_frozen = sum(p.numel() for p in model.parameters() if not p.requires_grad)
        n_dense = len(model.lora_dense_modules())
        print(f"[mdt-train] --lora-rank {lora_rank}: {len(model.lora_modules())} adapted QKV projections"
              f"{f' and {n_dense} adapted dense layers' if n_dense else ''} (targets {args.lora_targets}, "
              f"alpha {args.lora_alpha:g}{f', dropout {args.lora_dropout:g}' if getattr(args, 'lora_dropout', 0) else ''}), {n_train} trainable / {n_frozen} frozen parameter elements", file=sys.stderr)
    if engine.recompute() != "none" and rank == 0:
        ge = model.encoder.graph_encoder
        tm, vm = ge.text_model, ge.vit_model

        def live(*mods):        # a prefix without a trainable parameter runs without a tape: nothing is kept there anyway
            return any(p.requires_grad for m in mods for p in m.parameters())

        n_blocks = (len(model.pretrained_blocks()[1]) + (len(tm.encoder.layer) if live(tm.embeddings, tm.encoder) else 0)
                    + (len(vm.encoder.layer) if live(vm.embeddings, vm.encoder, vm.layernorm) else 0))
        what = dict(block="input and output kept, forward replayed in backward", ffn="u and h recomputed from the FFN input")
        print(f"[mdt-train] activation recomputation: policy {engine.recompute()} ({what[engine.recompute()]}) on {n_blocks} "
              "pretrained BERT / ViT blocks; the graph layers keep their activations", file=sys.stderr)
    model = model.cuda()
    half = args.fp16 or args.bf16 or args.fp8
    if half:
        model = model.bfloat16()
    model.train()
    fp8_state = model.enable_fp8(sites=args.fp8_sites) if args.fp8 else None      # the optimiser tells it when the weight copies go stale
    dp = DataParallel(model)
    dp.broadcast_parameters()
    crit_cls, _ = CRITERION_REGISTRY[args.criterion]
    crit = crit_cls.build_criterion(args, task)      # constructor arguments by name from the flags, as FairSeq does
    betas = ast.literal_eval(args.adam_betas) if isinstance(args.adam_betas, str) else args.adam_betas
    opt_params = [p for p in model.parameters() if hasattr(p, "main_grad")]
    if use_groups:
        opt_params = [dict(g, params=[p for p in g["params"] if hasattr(p, "main_grad")])
                      for g in model.optimizer_groups(weight_decay=args.weight_decay, **group_flags)]
        opt_params = [g for g in opt_params if g["params"]]
    opt = FusedAdam(opt_params, lr=args.lr, betas=betas, eps=args.adam_eps,
                    weight_decay=args.weight_decay, clip_norm=args.clip_norm,     # the norm pass and the guard are always on, as in FairSeq
                    **(dict(ema_decay=args.ema_decay, ema_start_update=args.ema_start_update, ema_update_freq=args.ema_update_freq)
                       if store_ema else {}))
    min_scale = None
    if use_groups:
        min_scale = min(g["lr_scale"] for g in opt.param_groups)
        if rank == 0:
            print(json.dumps(dict(optimizer_groups=[dict(tensors=len(g["params"]), elements=sum(p.numel() for p in g["params"]),
                                                         lr_scale=g["lr_scale"], weight_decay=g["weight_decay"])
                                                    for g in opt.param_groups])), flush=True)
    sched = PolynomialDecayLR(args.lr, args.end_learning_rate, args.warmup_updates, args.total_num_update, args.power)
    from . import checkpoint as ckpt
    start_update, epoch0 = 0, 1
    if args.restore_file:
        if not os.path.exists(args.restore_file):
            raise SystemExit(f"[mdt-train] --restore-file {args.restore_file} does not exist")
        info = ckpt.load_checkpoint(args.restore_file, model, optimizer=opt, reset_optimizer=args.reset_optimizer,
                                    reset_lr_scheduler=args.reset_lr_scheduler, reset_meters=args.reset_meters,
                                    reset_dataloader=args.reset_dataloader, allow_missing_prefixes=("node_encoder_stack.",))
        start_update, epoch0 = info["num_updates"], info["epoch"]
        stored = (info.get("cfg") or {}).get("model") or {}
        if not objective_given and args.criterion == "node_cross_entropy" and any(stored.get(f) for f in objective_names):
            # the objective the checkpoint was trained with goes on, as its cfg records it; either flag on the command line
            # (0 included) says otherwise
            objective_on = set_objective(stored.get("label_smoothing"), stored.get("focal_gamma"))
            crit.label_smoothing, crit.focal_gamma = args.label_smoothing, args.focal_gamma
            print(f"[mdt-train] {args.restore_file} was trained with --label-smoothing {args.label_smoothing:g} --focal-gamma "
                  f"{args.focal_gamma:g}: continuing with them", file=sys.stderr)
        if rank == 0:
            print(json.dumps(dict(restored=args.restore_file, num_updates=start_update, optimizer=info["loaded_optimizer"],
                                  missing=len(info["missing"]), unexpected=len(info["unexpected"]))), flush=True)
        if store_ema:
            # the average is model state, not optimiser state: --reset-optimizer does not drop it
            if info.get("ema") is not None:
                opt.load_ema_state_dict(model, info["ema"])
            else:
                opt.seed_ema_from_weights()
                print(f"[mdt-train] --store-ema: {args.restore_file} holds no extra_state['ema'] — the average starts as a copy of the "
                      "restored weights", file=sys.stderr)
        dp.broadcast_parameters()

    skip_batches = 0          # batches of the running epoch that the restored checkpoint had already consumed
    if args.restore_file and not args.reset_dataloader:
        skip_batches = int(info.get("iterations_in_epoch", 0))      # (not read from extra_state: --reset-meters empties that, and must not rewind the data)
    valid_batches = None      # callable → iterable of packed batches of the held-out split (this rank's share)
    if args.dataset_name == "synthetic":
        batches = synthetic_batches(args, task, rank)
        n_batches = len(batches)

        def batch_stream():
            while True:
                yield from batches

        if not args.disable_validation and args.synthetic_valid_batches > 0:
            import copy
            va = copy.copy(args)
            va.seed, va.synthetic_batches = args.seed + 104729, args.synthetic_valid_batches     # trees the training stream never shows
            held_out = synthetic_batches(va, task, rank)
            valid_batches = lambda: held_out      # noqa: E731
    elif task.dm is None:
        raise SystemExit(f"[mdt-train] dataset {args.dataset_name!r} is not registered: pass --user-data-dir <package whose "
                         "modules call register_dataset> (mDT/src/tasks/task.py:123-137) or --dataset-name synthetic")
    else:
        # a registered dataset (mDT/src/tasks/task.py:168-204): rank r takes every world-th batch of the epoch order;
        # batches are packed, uploaded and indexed one step ahead by the prefetch thread.  FairSeq keeps the last,
        # partial batch of an epoch (no drop-last): the number of batches per epoch is the CEILING, which is also what
        # --max-epoch turns into a number of updates.
        from .data.prefetch import Prefetcher
        task.collate_device = "cuda"
        ds = task.load_dataset("train")
        per_step = args.batch_size * world
        n_batches = max(1, (len(ds) + per_step - 1) // per_step)

        def index_stream():
            epoch, first = epoch0, skip_batches % n_batches
            while True:
                if hasattr(ds, "set_epoch"):
                    ds.set_epoch(epoch)
                order = list(ds.ordered_indices())
                for b in range(first, n_batches):
                    lo = (b * world + rank) * args.batch_size
                    idx = [int(i) for i in order[lo:lo + args.batch_size]]
                    # the tail batch of an epoch may leave the last ranks without trees; collectives must stay matched, so such
                    # a rank takes the tail batch's first tree again (at most world - 1 trees per epoch are seen twice)
                    yield idx if idx else [int(order[min(b * per_step, len(order) - 1)])]
                epoch, first = epoch + 1, 0

        ge = model.encoder.graph_encoder

        def make(idx):
            sample = ds.collater([ds[i] for i in idx])
            return sample["net_input"]["batched_data"]["_packed"]

        def warm(pb):
            ix = ge._indices(pb)
            if ge.prune_last_layer:
                ge._prune_indices(pb, ix)

        batch_stream = lambda: Prefetcher(index_stream(), make, depth=2, warm=warm)   # noqa: E731
        if not args.disable_validation:
            try:
                vds = task.load_dataset(args.valid_subset)
            except (KeyError, ValueError, AttributeError, FileNotFoundError):
                vds = None
            if vds is not None and len(vds) > 0:
                def valid_batches():
                    order = list(range(len(vds)))
                    nb_ = (len(order) + per_step - 1) // per_step
                    for b in range(nb_):
                        lo = (b * world + rank) * args.batch_size
                        idx = order[lo:lo + args.batch_size]
                        if idx:                         # held-out trees are counted once: a rank without a share sits the batch out
                            yield vds.collater([vds[i] for i in idx])["net_input"]["batched_data"]["_packed"]
    stream = iter(batch_stream())
    if args.dataset_name == "synthetic" and start_update and not args.reset_dataloader:
        for _ in range(start_update * args.update_freq):        # resume the batch order where the checkpoint left it
            next(stream)
    max_update = args.max_update or (args.max_epoch * n_batches // max(1, args.update_freq)) or 50
    # loss, sample size and the criterion's four counters; with the label-smoothed / focal objective one more slot: nll_loss
    n_scal = 7 if objective_on else 6
    not_counters = ("loss", "sample_size", "nsentences", "ntokens", "nll_loss")
    scal = torch.zeros(n_scal, dtype=torch.float32, device="cuda")
    history = []
    it = 0
    t0 = time.time()
    lr_for = sched.for_update        # FairSeq's timing: update k runs with the rate of num_updates = k - 1

    best = {"value": None}
    meter = {"upd": start_update, "clipped": 0, "checked": start_update}      # state of the clip meter / guard at the last log line

    def check_guard(upd, g=None):
        """FairSeq's answer to a non-finite gradient: under --fp16 the update is skipped and counted (its overflow skip,
        without a scale to lower); in every other precision the run stops.  The optimiser has skipped the update on the
        device — weights and moments are intact — and the host learns of it here, at a synchronisation it makes anyway."""
        g = opt.guard_host() if g is None else g
        if g["skipped"] > 0 and not args.fp16:
            raise FloatingPointError(f"[mdt-train] non-finite gradient norm in an update between {meter['checked'] + 1} and {upd} "
                                     f"({g['skipped']} skipped; weights and optimiser moments are those before it): "
                                     "lower the learning rate or pass --clip-norm")
        meter["checked"] = upd
        return g

    # --lora-dropout: every step's site seeds come from torch's CPU generator (engine.Tape.next_seed).  So that a resumed run
    # continues the masks of the uninterrupted one, the generator's state rides in the checkpoint's extra_state and a validation
    # pass (whose forward-only tapes draw from it too) leaves it as it found it.  Without the flag none of this happens: the
    # checkpoint bytes and the generator's sequence are those of a run before the flag existed.
    keep_rng = bool(getattr(args, "lora_dropout", 0))

    def save(path, upd):
        check_guard(upd)
        done = skip_batches + it                     # batches consumed since the restored epoch began
        ckpt.save_checkpoint(path, model, args, optimizer=opt, num_updates=upd, criterion_name=crit_cls.__name__,
                             lr_scheduler_state={"best": best["value"]}, epoch=epoch0 + done // max(1, n_batches),
                             training_time=time.time() - t0,
                             extra_state={"train_iterator": {"version": 2, "epoch": epoch0 + done // max(1, n_batches),
                                                             "iterations_in_epoch": done % max(1, n_batches), "shuffle": True},
                                          "val_loss": best["value"], **({"ema": opt.ema_state_dict(model)} if store_ema else {}),
                                          **({"rng_state": torch.get_rng_state()} if keep_rng else {})})

    valid_history = []
    main.valid_history = valid_history

    def validate(upd):
        """FairSeq's ``validate``: eval mode, no gradients, the summed logging outputs of every held-out batch (all ranks) go
        through the criterion's own ``reduce_metrics`` arithmetic (criterions/hatespeech_loss.py:133-173: accuracy,
        precision, recall, F1 with its zero guards)."""
        if valid_batches is None:
            return None
        check_guard(upd)
        was = model.training
        rng = torch.get_rng_state() if keep_rng else None
        model.eval()
        tot = torch.zeros(n_scal, dtype=torch.float32, device="cuda")
        keys = None
        import contextlib
        with (opt.ema_weights() if validate_with_ema else contextlib.nullcontext()), torch.no_grad():
            for pb in valid_batches():
                loss, sample_size, log = crit(model, {"nsamples": pb.B, "net_input": {"batched_data": pb.batched_data}})
                keys = [k for k in log if k not in not_counters]
                tot[0] += loss.detach().float()
                tot[1] += float(sample_size)
                tot[2:6] += torch.stack([log[k] for k in keys]).float()
                if objective_on:
                    tot[6] += log["nll_loss"].float()
        model.train(was)
        if rng is not None:
            torch.set_rng_state(rng)
        if world > 1:
            dist.all_reduce(tot)
        if keys is None:
            keys = ["ncorrect", "num_positive_correct", "total_positive", "num_pred_positive"]
        s_ = tot.tolist()
        summed = dict(loss=s_[0], sample_size=s_[1], **dict(zip(keys, s_[2:6])), **(dict(nll_loss=s_[6]) if objective_on else {}))
        crit_cls.reduce_metrics([summed])            # logs through fairseq.metrics when fairseq is there
        m = {("valid_" + k): v for k, v in crit_cls.compute_metrics([summed]).items()}
        m.update(valid_counters=summed, num_updates=upd, subset=args.valid_subset)
        if validate_with_ema:
            m["weights"] = "ema"
        if best["value"] is None or m["valid_loss"] < best["value"]:
            best["value"] = m["valid_loss"]
        m["valid_best_loss"] = best["value"]
        valid_history.append(m)
        if rank == 0:
            print(json.dumps(m), flush=True)
        return m

    if keep_rng and args.restore_file and info["extra_state"].get("rng_state") is not None:
        torch.set_rng_state(info["extra_state"]["rng_state"])
    for upd in range(start_update + 1, max_update + 1):
        dp.zero_grad()
        acc = torch.zeros(n_scal, dtype=torch.float32, device="cuda")
        for micro in range(args.update_freq):
            dp.accumulate(micro == args.update_freq - 1)
            pb = next(stream)
            it += 1
            loss, sample_size, log = crit(model, {"nsamples": pb.B, "net_input": {"batched_data": pb.batched_data}})
            loss.backward()
            counter_keys = [k for k in log if k not in not_counters]   # 4 per criterion
            acc[0] += loss.detach().float()
            acc[1] += float(sample_size)
            acc[2:6] += torch.stack([log[k] for k in counter_keys]).float()
            if objective_on:
                acc[6] += log["nll_loss"].float()
        scal.copy_(acc)
        gscale = dp.finish_backward(scal, fold_scale=True)     # all-reduce (world > 1); 1 / global sample size is applied by the optimiser
        opt.step(lr=lr_for(upd), grad_scale=gscale, num_updates=upd)
        if upd % args.log_interval == 0 or upd == max_update:
            s = torch.cat([scal.double(), opt.guard_log_vector()]).tolist()     # the only host sync, once per log interval
            gw = s[n_scal:]
            g = check_guard(upd, dict(gnorm=gw[0], applied=int(gw[1]), clipped=int(gw[2]), skipped=int(gw[3])))
            m = crit_cls.compute_metrics([dict(loss=s[0], sample_size=s[1], **dict(zip(counter_keys, s[2:6])),
                                               **(dict(nll_loss=s[6]) if objective_on else {}))])
            # FairSeq's meters: gnorm of this update, clip = per cent of the updates since the previous line that were clipped
            m.update(num_updates=upd, lr=lr_for(upd), gnorm=g["gnorm"], clip=100.0 * (g["clipped"] - meter["clipped"]) / (upd - meter["upd"]),
                     skipped_updates=g["skipped"], wall=round(time.time() - t0, 2))
            if min_scale is not None:
                m["lr_min"] = lr_for(upd) * min_scale              # the smallest group rate of this update
            meter.update(upd=upd, clipped=g["clipped"])
            history.append(m)
            if rank == 0:
                print(json.dumps(m), flush=True)
        if args.validate_interval_updates > 0 and upd % args.validate_interval_updates == 0 and upd != max_update:
            validate(upd)
        if rank == 0 and args.save_dir and not args.no_save and args.save_interval_updates > 0 and upd % args.save_interval_updates == 0:
            for path in ckpt.checkpoint_paths(args.save_dir, epoch0, upd):
                save(path, upd)
    if max_update > start_update:
        validate(max_update)                         # FairSeq validates at the end of training as well
    if rank == 0 and args.save_checkpoint:
        save(args.save_checkpoint, max_update)
    if rank == 0 and args.save_dir and not args.no_save:
        save(os.path.join(args.save_dir, "checkpoint_last.pt"), max_update)
    if rank == 0 and save_merged:
        # the adapters folded into the projections, under the cfg of a run without --lora-rank: a plain mDT checkpoint
        check_guard(max_update)
        plain = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in ("lora_rank", "lora_alpha", "lora_targets", "lora_dropout")})
        ckpt.save_checkpoint(save_merged, model, plain, model_state=ckpt.merged_model_state(model, opt), num_updates=max_update,
                             criterion_name=crit_cls.__name__, training_time=time.time() - t0)
    main.last_run = dict(model=model, criterion=crit, valid_batches=valid_batches, optimizer=opt, fp8=fp8_state)     # for tests / notebooks
    if fp8_state is not None:
        from . import fp8 as _fp8
        _fp8.ACTIVE = None                           # process-wide switch: a later model in this process starts in bf16
    if args.deterministic:
        engine.set_deterministic(was_deterministic)  # the same: a later run in this process starts as this one found the switch
    if world > 1:
        dist.destroy_process_group()
    return history


if __name__ == "__main__":
    main()
