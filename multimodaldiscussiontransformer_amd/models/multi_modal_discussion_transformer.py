"""Drop-in for mDT/src/models/multi_modal_discussion_transformer.py: model ``multi_graphormer``
with architectures ``multi_graphormer`` / ``multi_graphormer_base``, the reference's CLI flags
(underscore flags included) and the classifier head — pooler → dropout → classifier applied to
both the text [CLS] and bottleneck token 0 with the *same* weights, averaged (:265-274).

Encoder, head and their backward run as ONE tape (one autograd node); with
``prepare_main_grads`` parameter gradients accumulate in persistent fp32 buffers laid out in a
single flat arena, which is what the RCCL data-parallel hook all-reduces.
"""
from __future__ import annotations

import logging

import torch
import torch.nn as nn

from .. import engine as E
from ..data.packer import packed_from_batched_data
from ..modules import MultiGraphormerGraphEncoder, init_graphormer_params
from ..registry import FairseqEncoder, FairseqEncoderModel, register_model, register_model_architecture

logger = logging.getLogger(__name__)


def _slot(n: int) -> int:
    """arena slot size: 256-byte aligned so every main_grad view is vector-addressable"""
    return (n + 63) // 64 * 64


def safe_hasattr(obj, k):
    return getattr(obj, k, None) is not None


@register_model("multi_graphormer")
class GraphormerModel(FairseqEncoderModel):
    """mDT/src/models/multi_modal_discussion_transformer.py:22-178 (extends FairseqEncoderModel there as here)."""

    def __init__(self, args, encoder):
        super().__init__(encoder)
        self.args = args
        if getattr(args, "apply_graphormer_init", False):
            self.apply(init_graphormer_params)
        self.encoder_embed_dim = args.encoder_embed_dim

    @staticmethod
    def add_args(parser):
        """Model-specific arguments, names identical to the reference (:33-158)."""
        parser.add_argument("--dropout", type=float, metavar="D", help="dropout probability")
        parser.add_argument("--attention-dropout", type=float, metavar="D", help="dropout probability for attention weights")
        parser.add_argument("--act-dropout", type=float, metavar="D", help="dropout probability after activation in FFN")
        parser.add_argument("--encoder-ffn-embed-dim", type=int, metavar="N", help="encoder embedding dimension for FFN")
        parser.add_argument("--encoder-layers", type=int, metavar="N", help="num encoder layers")
        parser.add_argument("--encoder-attention-heads", type=int, metavar="N", help="num encoder attention heads")
        parser.add_argument("--num_fusion_layers", type=int, metavar="N", help="num fusion layers")
        parser.add_argument("--num_graph_stack", type=int, metavar="N", help="num graph layers per fusion layer")
        parser.add_argument("--num_fusion_stack", type=int, metavar="N", help="num fusion layers per graph layer")
        parser.add_argument("--num_bottleneck_tokens", type=int, metavar="N", help="num bottleneck tokens")
        parser.add_argument("--encoder-embed-dim", type=int, metavar="N", help="encoder embedding dimension")
        parser.add_argument("--split", type=int, metavar="N", help="dataset split to use (not used in code)")
        parser.add_argument("--share-encoder-input-output-embed", action="store_true",
                            help="share encoder input and output embeddings")
        parser.add_argument("--encoder-learned-pos", action="store_true",
                            help="use learned positional embeddings in the encoder")
        parser.add_argument("--no-token-positional-embeddings", action="store_true",
                            help="if set, disables positional embeddings (outside self attention)")
        parser.add_argument("--max-positions", type=int, help="number of positional embeddings to learn")
        parser.add_argument("--apply-graphormer-init", action="store_true",
                            help="use custom param initialization for Graphormer")
        parser.add_argument("--activation-fn", choices=["relu", "gelu", "gelu_fast", "gelu_accurate", "tanh", "linear"],
                            help="activation function to use")
        parser.add_argument("--encoder-normalize-before", action="store_true",
                            help="apply layernorm before each encoder block")
        parser.add_argument("--pre-layernorm", action="store_true",
                            help="apply layernorm before self-attention and ffn. Without this, post layernorm will used")
        parser.add_argument("--freeze_initial_encoders", action="store_true", help="freezes the initial layers ")
        # not in the reference, which hard-codes the hub names and downloads (multigraphormer_graph_encoder.py:236-245):
        parser.add_argument("--pretrained-bert", default=None, help="HuggingFace BERT weights for the text stack: local directory / "
                            "file or a name in the LOCAL HF cache (default bert-base-uncased); never downloaded")
        parser.add_argument("--pretrained-vit", default=None, help="same for the image stack (default google/vit-base-patch16-224)")
        parser.add_argument("--random-init-encoders", action="store_true", default=False,
                            help="build the BERT / ViT stacks from random weights instead")

    def max_nodes(self):
        return self.encoder.max_nodes

    @classmethod
    def build_model(cls, args, task):
        base_architecture(args)
        if not safe_hasattr(args, "max_nodes"):
            args.max_nodes = getattr(args, "tokens_per_sample", 10000)
        logger.info(args)
        encoder = GraphormerEncoder(args)
        model = cls(args, encoder)
        # A parser that went through add_args (FairSeq's, or train.py's) carries --random-init-encoders: such a run gets the
        # reference's pretrained encoders unless it opts out or runs custom BERT / ViT shapes; programmatic construction
        # (tests, bench.py: a bare namespace) never touches the disk.
        custom = getattr(args, "bert_config", None) is not None or getattr(args, "vit_config", None) is not None
        if hasattr(args, "random_init_encoders") and not args.random_init_encoders and not custom and \
                not getattr(args, "_skip_pretrained", False):
            from .. import hf_weights
            info = hf_weights.load_pretrained_encoders(encoder.graph_encoder,
                                                       bert=getattr(args, "pretrained_bert", None) or hf_weights.BERT_NAME,
                                                       vit=getattr(args, "pretrained_vit", None) or hf_weights.VIT_NAME)
            logger.info("pretrained encoders: %s", info)
        if getattr(args, "lora_rank", 0):          # after the pretrained weights: the adapters sit beside them
            model.add_lora(int(args.lora_rank), getattr(args, "lora_alpha", None), getattr(args, "lora_targets", None) or "q,v",
                           dropout=float(getattr(args, "lora_dropout", None) or 0.0))
        return model

    def forward(self, batched_data, **kwargs):
        return self.encoder(batched_data, **kwargs)

    # ---- optimiser parameter groups -----------------------------------------------------------
    def encoder_layer_ids(self):
        """{id(parameter): (layer id, L)} for the parameters of the two PRETRAINED encoders.  Per encoder of full depth L
        (``bert_config["layers"]`` / ``vit_config["layers"]``): its embeddings (ViT: patch projection, [CLS], position table)
        have id 0 and the block with original index i has id i + 1, whether it stayed in the truncated ``text_model`` /
        ``vit_model`` prefix or was sliced out into a GraphFusionStack.  Poolers and ViT's final LayerNorm are not listed."""
        ge = self.encoder.graph_encoder
        out = {}
        for enc, cfg, side in ((ge.text_model, ge.bert_config, "bert_encoder"), (ge.vit_model, ge.vit_config, "vit_encoder")):
            depth = int(cfg["layers"])
            blocks = list(enc.encoder.layer) + [getattr(fl, side) for st in ge.fusion_layers for fl in st.fusion_layers]
            assert len(blocks) == depth, f"{side}: {len(blocks)} blocks found, the encoder has {depth}"
            for p in enc.embeddings.parameters():
                out[id(p)] = (0, depth)
            for i, blk in enumerate(blocks):
                for p in blk.parameters():
                    out[id(p)] = (i + 1, depth)
        return out

    def optimizer_groups(self, encoder_lr_scale=1.0, encoder_layer_decay=1.0, no_decay_bias_norm=False, weight_decay=0.01):
        """The parameter groups for FusedAdam: ``[{"params", "lr_scale", "weight_decay"}]``, one per distinct pair in
        ``parameters()`` order of first appearance, every trainable parameter exactly once (frozen ones in none).
        A pretrained-encoder parameter of layer id ``k`` (encoder_layer_ids) gets lr_scale =
        ``encoder_lr_scale * encoder_layer_decay ** (L + 1 - k)``: the last block runs at scale x decay, the embeddings at
        scale x decay^(L + 1).  Everything else — poolers, ViT's final LayerNorm, graph stacks, structural-bias tables, bottleneck
        tokens, fusion projections, classifier, the dead head parameters — has scale 1.  ``no_decay_bias_norm``: weight decay 0 for
        parameters with ``ndim <= 1``.  Reads module structure only: runs on the CPU."""
        ids = self.encoder_layer_ids()
        groups = {}
        for p in self.parameters():
            if not p.requires_grad:
                continue
            scale = 1.0
            if id(p) in ids:
                k, depth = ids[id(p)]
                scale = float(encoder_lr_scale) * float(encoder_layer_decay) ** (depth + 1 - k)
            wd = 0.0 if (no_decay_bias_norm and p.ndim <= 1) else float(weight_decay)
            groups.setdefault((scale, wd), {"params": [], "lr_scale": scale, "weight_decay": wd})["params"].append(p)
        return list(groups.values())

    # ---- low-rank adapters ---------------------------------------------------------------------
    def pretrained_blocks(self):
        """The BertLayer / ViTLayer blocks of the two pretrained encoders: the truncated prefixes first, then the fusion stacks."""
        ge = self.encoder.graph_encoder
        prefix = list(ge.text_model.encoder.layer) + list(ge.vit_model.encoder.layer)
        fusion = [blk for st in ge.fusion_layers for fl in st.fusion_layers for blk in (fl.bert_encoder, fl.vit_encoder)]
        return prefix, fusion

    def lora_modules(self):
        """The QKV projections that carry adapters."""
        prefix, fusion = self.pretrained_blocks()
        return [b.qkv_params() for b in prefix + fusion if b.qkv_params().lora_A is not None]

    def lora_dense_modules(self):
        """The dense layers (attention output projection, fc1, fc2: modules/_fused.py AdaptedLinear) that carry an adapter."""
        prefix, fusion = self.pretrained_blocks()
        return [m for b in prefix + fusion for m in b.dense_lora_layers().values() if m.lora_A is not None]

    def add_lora(self, rank: int, alpha=None, targets=("q", "v"), dropout: float = 0.0):
        """Parameter-efficient fine-tuning: every parameter of the two pretrained encoders (``encoder_layer_ids``: embeddings and
        blocks) is frozen and rank-``rank`` adapters are trained beside the targets of every pretrained block — q / k / v of the
        fused QKV projection, ``out`` (attention output projection), ``fc1``, ``fc2``; "all": the six —
        of the fusion blocks only when the prefixes are frozen by --freeze_initial_encoders, which then keep running without a
        tape.  Poolers, ViT's final LayerNorm, the graph stacks, bottleneck tokens and the head stay as they are.  ``alpha``
        defaults to 2 * rank; the adapter sum is scaled by alpha / rank.  ``dropout`` (PEFT's lora_dropout, 0 <= p < 1): in training
        mode every adapter of an adapted block reads dropout(x), one probability for all of them (the fused q / k / v adapters
        share one mask); it adds no parameter and no state-dict key, and ``merge_lora`` is unaffected.  Call it after the
        pretrained weights are loaded and before ``prepare_main_grads`` / FusedAdam.  → the number of adapted blocks."""
        import math
        from .. import fp8
        from ..modules._fused import LORA_RANKS, LORA_TARGETS, parse_lora_targets
        if getattr(self, "main_grad_flat", None) is not None:
            raise RuntimeError("add_lora after prepare_main_grads: the gradient arena was laid out without the adapters")
        if fp8.ACTIVE is not None:
            raise NotImplementedError("low-rank adapters with fp8 GEMMs enabled are not supported (the adapter sum enters the bf16 "
                                      "qkv buffer only): disable fp8 first")
        if self.lora_modules() or self.lora_dense_modules():
            raise RuntimeError("add_lora: the model already has adapters")
        if rank not in LORA_RANKS:
            raise ValueError(f"add_lora: rank {rank} is not one of {LORA_RANKS}")
        alpha = 2.0 * rank if alpha is None else float(alpha)
        if not (math.isfinite(alpha) and alpha > 0):
            raise ValueError(f"add_lora: alpha {alpha} is not a finite positive number")
        dropout = float(dropout)
        if not 0.0 <= dropout < 1.0:           # NaN fails both comparisons
            raise ValueError(f"add_lora: dropout {dropout} is not in [0, 1)")
        targets = parse_lora_targets(targets)
        ids = self.encoder_layer_ids()
        for p in self.parameters():
            if id(p) in ids:
                p.requires_grad = False
        prefix, fusion = self.pretrained_blocks()
        blocks = fusion if getattr(self.args, "freeze_initial_encoders", False) else prefix + fusion
        qkv = tuple(t for t in targets if t in LORA_TARGETS)
        for b in blocks:
            b.lora_dropout_p = dropout
            if qkv:
                b.qkv_params().add_lora(rank, alpha, qkv)
            for name, m in b.dense_lora_layers().items():
                if name in targets:
                    m.add_lora(rank, alpha)
        return len(blocks)

    def merge_lora(self):
        """Fold every adapter into its projection (W_j += s B_j A_j, fp32, one rounding) and remove it: ``state_dict()`` then has
        exactly the keys of a model built without adapters.  → the number of layers merged (QKV projections and dense layers)."""
        mods = self.lora_modules() + self.lora_dense_modules()
        for m in mods:
            m.merge_lora()
        for b in sum(self.pretrained_blocks(), []):
            b.lora_dropout_p = 0.0
        if mods:
            E.weights_changed()
        return len(mods)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """As nn.Module's, with one allowance: a checkpoint WITHOUT adapter keys loads into an adapted model (fine-tuning from a
        full checkpoint) — the adapters keep their values and their keys are reported in the returned ``missing_keys``."""
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        for m in self.lora_modules() + self.lora_dense_modules():
            res.missing_keys.extend(m._lora_missing)
            m._lora_missing = []
        return res

    # ---- fp32 gradient arena ----------------------------------------------------------------
    def prepare_main_grads(self):
        """Give every trainable parameter an fp32 ``main_grad`` view into one flat buffer (reverse
        registration order ≈ the order gradients become final in backward, so data-parallel buckets
        are contiguous slices).  Returns the flat buffer."""
        params = [p for p in self.encoder.graph_encoder.live_parameters() if p.requires_grad]
        extra = [p for p in self.parameters() if p.requires_grad and all(p is not q for q in params)]
        params = params + extra
        total = sum(_slot(p.numel()) for p in params)
        flat = torch.zeros(total, dtype=torch.float32, device=params[0].device)
        off = 0
        for p in reversed(params):
            p.main_grad = flat[off:off + p.numel()].view(p.shape)
            off += _slot(p.numel())
        self.main_grad_flat = flat
        self.encoder.graph_encoder.use_main_grad = True
        return flat

    def zero_main_grads(self):
        self.main_grad_flat.zero_()

    def enable_fp8(self, on: bool = True, sites=None):
        """BASELINE.json configs[4]: per-tensor-scaled fp8 operands (e4m3 activations / weights, e5m2 gradients, delayed
        scaling) for the encoder blocks' big GEMMs.  ``sites``: a preset of fp8.PRESETS ("all" — the default —, "fast4",
        "grads") or a comma list of site names (fp8.py says which GEMMs and what each choice costs in accuracy)."""
        from .. import fp8
        act = getattr(self.args, "activation_fn", "gelu")
        if on and act != "gelu":
            raise NotImplementedError(f"enable_fp8 with --activation-fn {act}: the fp8 path quantises h inside fc1's fused gelu "
                                      "epilogue, which the other activations do not go through")
        if on and (self.lora_modules() or self.lora_dense_modules()):
            raise NotImplementedError("enable_fp8 on a model with low-rank adapters is not supported: the adapter sum enters the "
                                      "bf16 qkv buffer only (train the adapters in bf16, or merge_lora() first)")
        from .. import engine
        if on and engine.deterministic():
            raise NotImplementedError("enable_fp8 in deterministic mode: the fp8 path has no ordered reductions "
                                      "(engine.set_deterministic(False) first)")
        if on and engine.recompute() != "none":
            raise NotImplementedError(f"enable_fp8 with activation recomputation ({engine.recompute()}): {engine.RECOMPUTE_FP8_WHY} "
                                      "(engine.set_recompute(\"none\") first)")
        fp8.ACTIVE = fp8.Fp8State(next(self.parameters()).device, sites=sites) if on else None
        return fp8.ACTIVE


class GraphormerEncoder(FairseqEncoder):
    def __init__(self, args):
        super().__init__(dictionary=None)
        self.max_nodes = args.max_nodes
        extra = {}
        if getattr(args, "bert_config", None) is not None:
            extra["bert_config"] = args.bert_config
        if getattr(args, "vit_config", None) is not None:
            extra["vit_config"] = args.vit_config
        self.graph_encoder = MultiGraphormerGraphEncoder(
            num_atoms=args.num_atoms, num_in_degree=args.num_in_degree, num_out_degree=args.num_out_degree,
            num_edges=args.num_edges, num_spatial=args.num_spatial, num_edge_dis=args.num_edge_dis,
            edge_type=args.edge_type, multi_hop_max_dist=args.multi_hop_max_dist,
            num_bottle_neck=args.num_bottleneck_tokens, num_fusion_layers=args.num_fusion_layers,
            num_fusion_stack=args.num_fusion_stack, num_graph_stack=args.num_graph_stack,
            num_encoder_layers=args.encoder_layers, embedding_dim=args.encoder_embed_dim,
            ffn_embedding_dim=args.encoder_ffn_embed_dim, num_attention_heads=args.encoder_attention_heads,
            dropout=args.dropout, attention_dropout=args.attention_dropout, activation_dropout=args.act_dropout,
            encoder_normalize_before=args.encoder_normalize_before, pre_layernorm=args.pre_layernorm,
            apply_graphormer_init=args.apply_graphormer_init, activation_fn=args.activation_fn,
            freeze_initial_encoders=args.freeze_initial_encoders, **extra)
        ge = self.graph_encoder
        # the same module objects under a second name, exactly as the reference registers them (:215-221)
        self.node_encoder_stack = nn.ModuleList([ge.text_pooler, ge.text_dropout, ge.node_classifier])
        self.share_input_output_embed = args.share_encoder_input_output_embed
        self.embed_out = None
        self.lm_output_learned_bias = None
        self.load_softmax = not getattr(args, "remove_head", False)
        # dead parameters of the reference head (:231-247), kept for checkpoint compatibility
        self.masked_lm_pooler = nn.Linear(args.encoder_embed_dim, args.encoder_embed_dim)
        self.lm_head_transform_weight = nn.Linear(args.encoder_embed_dim, args.encoder_embed_dim)
        self.layer_norm = nn.LayerNorm(args.encoder_embed_dim)
        if self.load_softmax:
            self.lm_output_learned_bias = nn.Parameter(torch.zeros(1))
            if not self.share_input_output_embed:
                self.embed_out = nn.Linear(args.encoder_embed_dim, args.num_classes, bias=False)
            else:
                raise NotImplementedError

    def forward(self, batched_data, **unused):
        """→ (logits [M, 2], global_embedding [B, D])."""
        ge = self.graph_encoder
        pb = packed_from_batched_data(batched_data)
        p_head = ge.text_dropout.p if self.training else 0.0
        nb = ge.num_bottle_neck

        def run(tape):
            text, glob, rows = ge._fwd(tape, pb, prune_last=ge.prune_last_layer)
            logits = E.classifier_head(tape, text, pb.M, rows["cls_rows"], rows["bn0_rows"], ge.text_pooler.dense.weight,
                                       ge.text_pooler.dense.bias, ge.node_classifier.weight, ge.node_classifier.bias,
                                       p_drop=p_head)
            return logits, glob

        logits, glob = E.run_tape(run, [], ge.live_parameters(), use_main_grad=ge.use_main_grad, hook=ge.grad_ready_hook)
        return logits, glob

    def upgrade_state_dict_named(self, state_dict, name):
        if not self.load_softmax:
            for k in list(state_dict.keys()):
                if "embed_out.weight" in k or "lm_output_learned_bias" in k:
                    del state_dict[k]
        return state_dict


@register_model_architecture("multi_graphormer", "multi_graphormer")
def base_architecture(args):
    args.dropout = getattr(args, "dropout", 0.1)
    args.attention_dropout = getattr(args, "attention_dropout", 0.1)
    args.act_dropout = getattr(args, "act_dropout", 0.0)
    args.encoder_ffn_embed_dim = getattr(args, "encoder_ffn_embed_dim", 4096)
    args.encoder_layers = getattr(args, "encoder_layers", 6)
    args.encoder_attention_heads = getattr(args, "encoder_attention_heads", 8)
    args.split = getattr(args, "split", 0)
    args.encoder_embed_dim = getattr(args, "encoder_embed_dim", 1024)
    args.share_encoder_input_output_embed = getattr(args, "share_encoder_input_output_embed", False)
    args.no_token_positional_embeddings = getattr(args, "no_token_positional_embeddings", False)
    args.num_bottleneck_tokens = getattr(args, "num_bottleneck_tokens", 4)
    args.num_fusion_layers = getattr(args, "num_fusion_layers", 4)
    args.num_graph_stack = getattr(args, "num_graph_stack", 1)
    args.num_fusion_stack = getattr(args, "num_fusion_stack", 1)
    args.apply_graphormer_init = getattr(args, "apply_graphormer_init", False)
    args.activation_fn = getattr(args, "activation_fn", "gelu")
    args.encoder_normalize_before = getattr(args, "encoder_normalize_before", True)
    # task-level defaults (mDT/src/tasks/task.py:29-113) for callers that build the model directly
    for k, v in dict(num_atoms=512 * 9, num_in_degree=512, num_out_degree=512, num_edges=512 * 3, num_spatial=512,
                     num_edge_dis=128, edge_type="multi_hop", multi_hop_max_dist=5, num_classes=1, pre_layernorm=False,
                     freeze_initial_encoders=False).items():
        if not hasattr(args, k):
            setattr(args, k, v)


@register_model_architecture("multi_graphormer", "multi_graphormer_base")
def graphormer_base_architecture(args):
    args.encoder_embed_dim = getattr(args, "encoder_embed_dim", 80)
    args.split = getattr(args, "split", 0)
    args.encoder_layers = getattr(args, "encoder_layers", 12)
    args.encoder_attention_heads = getattr(args, "encoder_attention_heads", 8)
    args.encoder_ffn_embed_dim = getattr(args, "encoder_ffn_embed_dim", 80)
    args.activation_fn = getattr(args, "activation_fn", "gelu")
    args.freeze_initial_encoders = getattr(args, "freeze_initial_encoders", False)
    args.encoder_normalize_before = getattr(args, "encoder_normalize_before", True)
    args.apply_graphormer_init = getattr(args, "apply_graphormer_init", False)
    args.share_encoder_input_output_embed = getattr(args, "share_encoder_input_output_embed", False)
    args.no_token_positional_embeddings = getattr(args, "no_token_positional_embeddings", False)
    args.pre_layernorm = getattr(args, "pre_layernorm", False)
    base_architecture(args)
