"""Shared building blocks of the drop-in modules: fused Q/K/V parameter storage with
reference-compatible state-dict names, HF-style encoder layers, parameter containers.

The kernels want one [3D, D] projection; checkpoints of the reference hold three D x D
matrices (``q_proj/k_proj/v_proj`` in modules/multihead_attention.py:54-62,
``attention.self.{query,key,value}`` in HF BertLayer, ``attention.attention.{...}`` in HF
ViTLayer, transformers 4.x).  ``QKVFusedMixin`` keeps the fused tensor as the live
``nn.Parameter`` and splits / merges on ``state_dict`` / ``load_state_dict``.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import torch
import torch.nn as nn

from ..engine import BlockParams, LoraSlot


class QKVFusedMixin:
    """Mixin for an ``nn.Module`` that owns ``qkv_weight [3D, D]`` and ``qkv_bias [3D]``.
    ``_qkv_names`` are the three sub-prefixes (relative to this module) used in checkpoints."""
    _qkv_names = ("q_proj", "k_proj", "v_proj")

    def _init_qkv(self, dim: int, bias: bool = True):
        self.qkv_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.qkv_bias = nn.Parameter(torch.zeros(3 * dim)) if bias else None
        self._qkv_dim = dim

    def _qkv_view(self, i: int):
        d = self._qkv_dim
        return SimpleNamespace(weight=self.qkv_weight[i * d:(i + 1) * d],
                               bias=None if self.qkv_bias is None else self.qkv_bias[i * d:(i + 1) * d])

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        d = self._qkv_dim
        w = destination.pop(prefix + "qkv_weight")
        b = destination.pop(prefix + "qkv_bias", None)
        for i, n in enumerate(self._qkv_names):
            destination[f"{prefix}{n}.weight"] = w[i * d:(i + 1) * d]
            if b is not None:
                destination[f"{prefix}{n}.bias"] = b[i * d:(i + 1) * d]

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        names = [f"{prefix}{n}.weight" for n in self._qkv_names]
        if all(k in state_dict for k in names):
            state_dict[prefix + "qkv_weight"] = torch.cat([state_dict.pop(k) for k in names], dim=0)
            bnames = [f"{prefix}{n}.bias" for n in self._qkv_names]
            if all(k in state_dict for k in bnames):
                state_dict[prefix + "qkv_bias"] = torch.cat([state_dict.pop(k) for k in bnames], dim=0)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def _hf_init_linear(lin: nn.Linear, std: float = 0.02):
    nn.init.normal_(lin.weight, 0.0, std)
    if lin.bias is not None:
        nn.init.zeros_(lin.bias)


LORA_RANKS = (8, 16, 32, 64)
LORA_TARGETS = ("q", "k", "v")                      # the thirds of the fused QKV projection
LORA_DENSE_TARGETS = ("out", "fc1", "fc2")          # attention.output.dense, intermediate.dense, output.dense
LORA_ALL_TARGETS = LORA_TARGETS + LORA_DENSE_TARGETS


def parse_lora_targets(targets) -> tuple:
    """("q", "v") from "q,v" or a sequence: distinct names of q / k / v / out / fc1 / fc2, returned in that (canonical) order;
    "all" stands for the six of them."""
    names = [t.strip() for t in targets.split(",")] if isinstance(targets, str) else list(targets)
    names = [u for t in names for u in (LORA_ALL_TARGETS if t == "all" else (t,))]
    if not names or any(t not in LORA_ALL_TARGETS for t in names) or len(set(names)) != len(names):
        raise ValueError(f"LoRA targets {targets!r}: a non-empty list of distinct names out of q, k, v, out, fc1, fc2 (or all)")
    return tuple(t for t in LORA_ALL_TARGETS if t in names)


class AdaptedLinear(nn.Linear):
    """An ``nn.Linear`` of a pretrained block (attention.output.dense, intermediate.dense, output.dense) that may carry a low-rank
    adapter: live parameters ``lora_A`` [r, in] and ``lora_Bt`` [r, out] (the rows of B^T — the operand layout of the kernels),
    saved under PEFT's names ``lora_A.weight`` [r, in] / ``lora_B.weight`` [out, r].  Without an adapter it is an nn.Linear."""

    def __init__(self, d_in, d_out):
        super().__init__(d_in, d_out)
        self.lora_A = self.lora_Bt = None
        self.lora_rank, self.lora_alpha = 0, 0.0
        self._lora_missing = []

    def add_lora(self, rank: int, alpha: float):
        if self.lora_A is not None:
            raise RuntimeError("add_lora: this layer already has an adapter")
        if rank not in LORA_RANKS:
            raise ValueError(f"LoRA rank {rank}: one of {LORA_RANKS}")
        w = self.weight
        a = torch.empty(rank, self.in_features, dtype=torch.float32)
        nn.init.kaiming_uniform_(a, a=math.sqrt(5))         # as an nn.Linear(in, r) weight; B = 0: the adapted layer starts as the base
        self.lora_A = nn.Parameter(a.to(device=w.device, dtype=w.dtype))
        self.lora_Bt = nn.Parameter(torch.zeros(rank, self.out_features, device=w.device, dtype=w.dtype))
        self.lora_rank, self.lora_alpha = int(rank), float(alpha)

    def lora_slot(self):
        """The engine.LoraSlot of this layer, None without an adapter."""
        return None if self.lora_A is None else LoraSlot(self.lora_A, self.lora_Bt, self.lora_alpha / self.lora_rank)

    def merge_lora(self):
        """W += s Bt^T A in fp32, rounded once to the parameter's dtype; the adapter is removed."""
        if self.lora_A is None:
            return
        s = self.lora_alpha / self.lora_rank
        with torch.no_grad():
            self.weight.copy_((self.weight.float() + s * (self.lora_Bt.float().t() @ self.lora_A.float())).to(self.weight.dtype))
        self.lora_A = self.lora_Bt = None
        self.lora_rank, self.lora_alpha = 0, 0.0

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self.lora_A is None:
            return
        destination[prefix + "lora_A.weight"] = destination.pop(prefix + "lora_A")
        destination[prefix + "lora_B.weight"] = destination.pop(prefix + "lora_Bt").t()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        self._lora_missing = []
        if self.lora_A is not None:
            ka, kb = prefix + "lora_A.weight", prefix + "lora_B.weight"
            if ka not in state_dict and kb not in state_dict:
                # a checkpoint of the full model: the adapter keeps its values; GraphormerModel.load_state_dict reports the keys
                self._lora_missing = [ka, kb]
                state_dict[prefix + "lora_A"], state_dict[prefix + "lora_Bt"] = self.lora_A.data, self.lora_Bt.data
            elif ka in state_dict and kb in state_dict:
                state_dict[prefix + "lora_A"] = state_dict.pop(ka)
                state_dict[prefix + "lora_Bt"] = state_dict.pop(kb).t()
            # one of the two: the strict loader names the absent one
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def _dense_lora_fields(out_dense, fc1_dense, fc2_dense) -> dict:
    """The dense-adapter fields of engine.BlockParams of a block's three AdaptedLinear layers ({} without adapters)."""
    slots = dict(lora_o=out_dense.lora_slot(), lora_fc1=fc1_dense.lora_slot(), lora_fc2=fc2_dense.lora_slot())
    return {k: v for k, v in slots.items() if v is not None}


class _SelfAttentionParams(QKVFusedMixin, nn.Module):
    """The fused QKV projection of a pretrained block and, after ``add_lora``, the low-rank adapters beside it: live parameters
    ``lora_A`` / ``lora_Bt`` [|J| r, D] (rows of A_j and of B_j^T, target-major — one operand layout for every kernel), saved per
    target under PEFT's names ``{query,key,value}.lora_A.weight`` [r, D] / ``.lora_B.weight`` [D, r] next to the split q/k/v keys."""

    def __init__(self, dim, names):
        super().__init__()
        self._qkv_names = names
        self._init_qkv(dim)
        nn.init.normal_(self.qkv_weight, 0.0, 0.02)
        self.lora_A = self.lora_Bt = None
        self.lora_targets, self.lora_rank, self.lora_alpha = (), 0, 0.0
        self._lora_missing = []

    # ---- adapters
    def add_lora(self, rank: int, alpha: float, targets):
        if self.lora_A is not None:
            raise RuntimeError("add_lora: this projection already has adapters")
        targets = parse_lora_targets(targets)
        if any(t not in LORA_TARGETS for t in targets):
            raise ValueError(f"LoRA targets {targets!r}: the fused QKV projection takes q, k, v only")
        if rank not in LORA_RANKS:
            raise ValueError(f"LoRA rank {rank}: one of {LORA_RANKS}")
        w = self.qkv_weight
        n = len(targets) * rank
        a = torch.empty(n, self._qkv_dim, dtype=torch.float32)
        for j in range(len(targets)):               # every A_j as an nn.Linear(D, r) weight; B = 0: the adapted model starts as the base
            nn.init.kaiming_uniform_(a[j * rank:(j + 1) * rank], a=math.sqrt(5))
        self.lora_A = nn.Parameter(a.to(device=w.device, dtype=w.dtype))
        self.lora_Bt = nn.Parameter(torch.zeros(n, self._qkv_dim, device=w.device, dtype=w.dtype))
        self.lora_targets, self.lora_rank, self.lora_alpha = targets, int(rank), float(alpha)

    def lora_fields(self) -> dict:
        """The adapter fields of engine.BlockParams ({} without adapters)."""
        if self.lora_A is None:
            return {}
        return dict(lora_A=self.lora_A, lora_Bt=self.lora_Bt, lora_cols=tuple(LORA_TARGETS.index(t) for t in self.lora_targets),
                    lora_scale=self.lora_alpha / self.lora_rank)

    def merge_lora(self):
        """W_j += s Bt_j^T A_j in fp32, rounded once to the parameter's dtype; the adapters are removed."""
        if self.lora_A is None:
            return
        d, r, s = self._qkv_dim, self.lora_rank, self.lora_alpha / self.lora_rank
        with torch.no_grad():
            for j, t in enumerate(self.lora_targets):
                c = LORA_TARGETS.index(t) * d
                a, bt = self.lora_A[j * r:(j + 1) * r].float(), self.lora_Bt[j * r:(j + 1) * r].float()
                wj = self.qkv_weight[c:c + d]
                wj.copy_((wj.float() + s * (bt.t() @ a)).to(wj.dtype))
        self.lora_A = self.lora_Bt = None
        self.lora_targets, self.lora_rank, self.lora_alpha = (), 0, 0.0

    def _lora_key(self, prefix, target, which):
        return f"{prefix}{self._qkv_names[LORA_TARGETS.index(target)]}.lora_{which}.weight"

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self.lora_A is None:
            return
        a, bt, r = destination.pop(prefix + "lora_A"), destination.pop(prefix + "lora_Bt"), self.lora_rank
        for j, t in enumerate(self.lora_targets):
            destination[self._lora_key(prefix, t, "A")] = a[j * r:(j + 1) * r]
            destination[self._lora_key(prefix, t, "B")] = bt[j * r:(j + 1) * r].t()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        self._lora_missing = []
        if self.lora_A is not None:
            keys = [self._lora_key(prefix, t, w) for t in self.lora_targets for w in ("A", "B")]
            have = [k for k in keys if k in state_dict]
            if not have:
                # a checkpoint of the full model: the adapters keep their values; GraphormerModel.load_state_dict reports the keys
                self._lora_missing = keys
                state_dict[prefix + "lora_A"], state_dict[prefix + "lora_Bt"] = self.lora_A.data, self.lora_Bt.data
            elif len(have) == len(keys):
                state_dict[prefix + "lora_A"] = torch.cat([state_dict.pop(self._lora_key(prefix, t, "A")) for t in self.lora_targets], dim=0)
                state_dict[prefix + "lora_Bt"] = torch.cat([state_dict.pop(self._lora_key(prefix, t, "B")).t() for t in self.lora_targets], dim=0)
            # some but not all: the strict loader names the absent ones (lora_A / lora_Bt missing, the rest unexpected)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


class _DenseLN(nn.Module):
    def __init__(self, d_in, d_out, eps, with_ln=True):
        super().__init__()
        self.dense = AdaptedLinear(d_in, d_out)
        _hf_init_linear(self.dense)
        if with_ln:
            self.LayerNorm = nn.LayerNorm(d_out, eps=eps)


class _Dense(nn.Module):
    def __init__(self, d_in, d_out):
        super().__init__()
        self.dense = AdaptedLinear(d_in, d_out)
        _hf_init_linear(self.dense)


class _BertAttention(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.self = _SelfAttentionParams(dim, ("query", "key", "value"))
        self.output = _DenseLN(dim, dim, eps)


class BertLayer(nn.Module):
    """Parameter layout of HF ``BertLayer`` (transformers 4.x names); post-LN block, eps 1e-12."""
    pre_ln = False

    def __init__(self, dim=768, heads=12, intermediate=3072, eps=1e-12):
        super().__init__()
        self.dim, self.heads, self.eps = dim, heads, eps
        self.hidden_dropout_p, self.attention_dropout_p = 0.0, 0.0     # hidden_dropout_prob / attention_probs_dropout_prob
        self.lora_dropout_p = 0.0       # PEFT's lora_dropout, set by the model's add_lora
        self.attention = _BertAttention(dim, eps)
        self.intermediate = _Dense(dim, intermediate)
        self.output = _DenseLN(intermediate, dim, eps)

    def drop_kwargs(self):
        t = self.training
        kw = dict(p_hidden=self.hidden_dropout_p if t else 0.0, p_attn=self.attention_dropout_p if t else 0.0)
        if t and self.lora_dropout_p > 0:      # adapter-input dropout (add_lora(dropout=...)): training only, like the two above
            kw["p_lora"] = self.lora_dropout_p
        return kw

    def qkv_params(self) -> "_SelfAttentionParams":
        return self.attention.self

    def dense_lora_layers(self) -> dict:
        """{target name: AdaptedLinear} of the block's three dense layers"""
        return {"out": self.attention.output.dense, "fc1": self.intermediate.dense, "fc2": self.output.dense}

    def block_params(self) -> BlockParams:
        a, o = self.attention, self.output
        return BlockParams(a.self.qkv_weight, a.self.qkv_bias, a.output.dense.weight, a.output.dense.bias,
                           a.output.LayerNorm.weight, a.output.LayerNorm.bias, self.intermediate.dense.weight,
                           self.intermediate.dense.bias, o.dense.weight, o.dense.bias, o.LayerNorm.weight, o.LayerNorm.bias,
                           **a.self.lora_fields(), **_dense_lora_fields(*self.dense_lora_layers().values()))


class _ViTAttention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.attention = _SelfAttentionParams(dim, ("query", "key", "value"))
        self.output = _DenseLN(dim, dim, 0.0, with_ln=False)


class ViTLayer(nn.Module):
    """Parameter layout of HF ``ViTLayer`` (transformers 4.x names); pre-LN block, eps 1e-12."""
    pre_ln = True

    def __init__(self, dim=768, heads=12, intermediate=3072, eps=1e-12):
        super().__init__()
        self.dim, self.heads, self.eps = dim, heads, eps
        self.hidden_dropout_p, self.attention_dropout_p = 0.0, 0.0
        self.lora_dropout_p = 0.0
        self.attention = _ViTAttention(dim)
        self.intermediate = _Dense(dim, intermediate)
        self.output = _Dense(intermediate, dim)
        self.layernorm_before = nn.LayerNorm(dim, eps=eps)
        self.layernorm_after = nn.LayerNorm(dim, eps=eps)

    def drop_kwargs(self):
        t = self.training
        kw = dict(p_hidden=self.hidden_dropout_p if t else 0.0, p_attn=self.attention_dropout_p if t else 0.0)
        if t and self.lora_dropout_p > 0:      # adapter-input dropout (add_lora(dropout=...)): training only, like the two above
            kw["p_lora"] = self.lora_dropout_p
        return kw

    def qkv_params(self) -> "_SelfAttentionParams":
        return self.attention.attention

    def dense_lora_layers(self) -> dict:
        """{target name: AdaptedLinear} of the block's three dense layers"""
        return {"out": self.attention.output.dense, "fc1": self.intermediate.dense, "fc2": self.output.dense}

    def block_params(self) -> BlockParams:
        a = self.attention
        return BlockParams(a.attention.qkv_weight, a.attention.qkv_bias, a.output.dense.weight, a.output.dense.bias,
                           self.layernorm_before.weight, self.layernorm_before.bias, self.intermediate.dense.weight,
                           self.intermediate.dense.bias, self.output.dense.weight, self.output.dense.bias,
                           self.layernorm_after.weight, self.layernorm_after.bias, **a.attention.lora_fields(),
                           **_dense_lora_fields(*self.dense_lora_layers().values()))


class _Pooler(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dense = nn.Linear(dim, dim)
        _hf_init_linear(self.dense)


class _LayerList(nn.Module):
    """``encoder.layer.{i}`` container."""
    def __init__(self, layers):
        super().__init__()
        self.layer = nn.ModuleList(layers)


class _BertEmbeddings(nn.Module):
    def __init__(self, vocab, max_pos, type_vocab, dim, eps):
        super().__init__()
        self.word_embeddings = nn.Embedding(vocab, dim)
        self.position_embeddings = nn.Embedding(max_pos, dim)
        self.token_type_embeddings = nn.Embedding(type_vocab, dim)
        self.LayerNorm = nn.LayerNorm(dim, eps=eps)
        for e in (self.word_embeddings, self.position_embeddings, self.token_type_embeddings):
            nn.init.normal_(e.weight, 0.0, 0.02)


class BertModel(nn.Module):
    """``text_model``: embeddings + the first layers of BERT + pooler (parameters only — the
    compute is scheduled by MultiGraphormerGraphEncoder)."""
    def __init__(self, dim=768, layers=12, heads=12, intermediate=3072, vocab=30522, max_pos=512, type_vocab=2, eps=1e-12):
        super().__init__()
        self.dim, self.heads, self.eps = dim, heads, eps
        self.embeddings = _BertEmbeddings(vocab, max_pos, type_vocab, dim, eps)
        self.encoder = _LayerList([BertLayer(dim, heads, intermediate, eps) for _ in range(layers)])
        self.pooler = _Pooler(dim)


class _PatchEmbeddings(nn.Module):
    def __init__(self, dim, patch, channels=3):
        super().__init__()
        self.projection = nn.Conv2d(channels, dim, kernel_size=patch, stride=patch)
        nn.init.trunc_normal_(self.projection.weight, std=0.02)
        nn.init.zeros_(self.projection.bias)


class _ViTEmbeddings(nn.Module):
    def __init__(self, dim, image_size, patch):
        super().__init__()
        n = (image_size // patch) ** 2
        self.cls_token = nn.Parameter(torch.empty(1, 1, dim))
        self.position_embeddings = nn.Parameter(torch.empty(1, n + 1, dim))
        self.patch_embeddings = _PatchEmbeddings(dim, patch)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        nn.init.trunc_normal_(self.position_embeddings, std=0.02)


class ViTModel(nn.Module):
    """``vit_model``: patch embeddings + first layers + the final LayerNorm (applied mid-network
    by the reference, quirk 5) + pooler."""
    def __init__(self, dim=768, layers=12, heads=12, intermediate=3072, image_size=224, patch=16, eps=1e-12):
        super().__init__()
        self.dim, self.heads, self.eps, self.image_size, self.patch = dim, heads, eps, image_size, patch
        self.embeddings = _ViTEmbeddings(dim, image_size, patch)
        self.encoder = _LayerList([ViTLayer(dim, heads, intermediate, eps) for _ in range(layers)])
        self.layernorm = nn.LayerNorm(dim, eps=eps)
        self.pooler = _Pooler(dim)


def xavier_uniform_(t: torch.Tensor, gain: float = 1.0):
    fan_out, fan_in = t.shape[0], t.shape[1]
    a = gain * math.sqrt(6.0 / (fan_in + fan_out))
    with torch.no_grad():
        t.uniform_(-a, a)
