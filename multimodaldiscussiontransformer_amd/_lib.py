"""ctypes binding of libmdt_hip.so (the C ABI in include/mdt_hip.h).

The library is the product: there is no Python / eager fallback.  Importing this module
on a machine where the shared object is missing raises; calling an op with CPU tensors
raises.  PyTorch only provides device memory and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdt_hip.so")

MDT_F32, MDT_BF16 = 0, 1
EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_DGELU, EPI_ACCUM, EPI_ATOMIC, EPI_DROPOUT, EPI_COLSUM = 1, 2, 4, 8, 16, 32, 64, 128
EPI_AUX_GRAD, EPI_MULAUX, EPI_ASUM = 256, 512, 1024
ACT_GELU, ACT_RELU, ACT_GELU_ACCURATE, ACT_TANH, ACT_LINEAR = 0, 1, 2, 3, 4

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float


class AttnFwdArgs(C.Structure):
    _fields_ = [
        ("dtype", _i), ("nseq", _i), ("S", _i), ("H", _i), ("hd", _i),
        ("seq_stride", _i64), ("pos_stride", _i64), ("scale", _f),
        ("qkv", _vp), ("ld_qkv", _i64), ("out", _vp), ("ld_out", _i64), ("lse", _vp),
        ("key_mask", _vp), ("dense_bias", _vp), ("attn_bias", _vp), ("spatial_pos", _vp),
        ("sp_table", _vp), ("virt", _vp), ("key_pad", _vp), ("num_spatial", _i),
        ("drop_p", _f), ("drop_seed", C.c_uint64), ("seq_offsets", _vp), ("q_limit", _i),
        ("seq_ids", _vp), ("s_cap", _i), ("nseq_total", _i),
    ]


class AttnBwdArgs(C.Structure):
    _fields_ = [
        ("f", AttnFwdArgs), ("dout", _vp), ("ld_dout", _i64), ("dqkv", _vp), ("ld_dqkv", _i64),
        ("d_dense_bias", _vp), ("d_sp_table", _vp), ("d_virt", _vp),
    ]


_SIGS = {
    "mdt_abi_version": ([], _i),
    "mdt_last_error_string": ([], C.c_char_p),
    "mdt_last_route": ([], C.c_char_p),
    "mdt_source_hash": ([], C.c_char_p),
    "mdt_gemm": ([_vp, _i, _i, _i, _i, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _f, _vp, _vp, _i64,
                  _vp, _i64, _i, _f, C.c_uint64, _vp], _i),
    "mdt_gemm_tile_queue_bytes": ([], C.c_size_t),
    "mdt_gemm_set_tile_queue": ([_vp, C.c_size_t], _i),
    "mdt_reload_env": ([], None),
    "mdt_dropout": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _i64, _f, C.c_uint64], _i),
    "mdt_dropout_mask": ([_vp, _i64, _f, C.c_uint64, _vp], _i),
    "mdt_act_fwd": ([_vp, _i, _i, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f, C.c_uint64], _i),
    "mdt_colsum": ([_vp, _i, _i64, _i64, _vp, _i64, _vp, _vp], _i),
    "mdt_layernorm_fwd": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _vp, _f, _vp, _i64, _vp, _vp], _i),
    "mdt_layernorm_fwd_q8": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _vp, _f, _vp, _i64, _vp, _vp, _vp, _i64, _i, _vp, _vp], _i),
    "mdt_layernorm_bwd": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp,
                           _vp, _i64, _f, C.c_uint64, _vp], _i),
    "mdt_attention_fwd": ([_vp, C.POINTER(AttnFwdArgs)], _i),
    "mdt_attention_bwd": ([_vp, C.POINTER(AttnBwdArgs)], _i),
    "mdt_attention_route": ([C.POINTER(AttnBwdArgs), _i, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)], _i),
    "mdt_attention_mean_probs": ([_vp, C.POINTER(AttnFwdArgs), _vp], _i),
    "mdt_attention_head_weights": ([_vp, C.POINTER(AttnFwdArgs), _i, _vp], _i),
    "mdt_graph_attn_bias": ([_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "mdt_row_axpby": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _f,
                       _vp, _i64, _vp, _i64, _i64, _i64, _f, _i], _i),
    "mdt_row_scatter_add_f32": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _vp, _i64, _i64, _i64], _i),
    "mdt_sum_slices_f32": ([_vp, _i64, _i64, _i, _vp, _i64, _i64, _vp, _i64, _i], _i),
    "mdt_gemm_splitk_ordered_workspace_bytes": ([_i64, _i64, _i], C.c_size_t),
    "mdt_gemm_splitk_ordered": ([_vp, _i, _i, _i, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _f, _i, _vp, C.c_size_t], _i),
    "mdt_colsum_ordered_workspace_bytes": ([_i64, _i64], C.c_size_t),
    "mdt_colsum_ordered": ([_vp, _i, _i64, _i64, _vp, _i64, _vp, _vp, _vp, C.c_size_t], _i),
    "mdt_layernorm_bwd_ordered_workspace_bytes": ([_i64, _i], C.c_size_t),
    "mdt_layernorm_bwd_ordered": ([_vp, _i, _i64, _i, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp,
                                   _vp, _i64, _f, C.c_uint64, _vp, _vp, C.c_size_t], _i),
    "mdt_row_segment_sum_f32": ([_vp, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i64], _i),
    "mdt_attn_bias_grad_ordered_workspace_bytes": ([_i, _i, _i], C.c_size_t),
    "mdt_attn_bias_grad_ordered": ([_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_size_t], _i),
    "mdt_float_atomic_launches": ([_i], _i64),
    "mdt_lora_down": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f], _i),
    "mdt_lora_up_add": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f], _i),
    "mdt_lora_up_add_drop": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f, _f, C.c_uint64], _i),
    "mdt_lora_up_add_mul": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _f], _i),
    "mdt_lora_up_act": ([_vp, _i, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _f, _f, C.c_uint64], _i),
    "mdt_lora_wgrad_slab_rows": ([], _i),
    "mdt_lora_wgrad_workspace_bytes": ([_i64, _i, _i], C.c_size_t),
    "mdt_lora_wgrad": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f, _vp, C.c_size_t], _i),
    "mdt_lora_down_drop": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f, _f, C.c_uint64], _i),
    "mdt_lora_wgrad_drop": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _f, _f, C.c_uint64, _vp, C.c_size_t], _i),
    "mdt_lora_up_add_mul_drop": ([_vp, _i, _i64, _i, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _f, _f, C.c_uint64], _i),
    "mdt_bert_embed_sum": ([_vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i64, _i64, _i64], _i),
    "mdt_bert_embed_rows": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i64], _i),
    "mdt_bert_embed_ln_rows": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _f, _vp, _i64, _vp, _i64, _vp, _vp], _i),
    "mdt_vit_patchify": ([_vp, _i, _i, _i, _i, _i, _vp, _vp, _i64], _i),
    "mdt_vit_assemble": ([_vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64], _i),
    "mdt_vit_patch_embed": ([_vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _vp, _vp, _i, _vp, _i64, _i64, _i64], _i),
    "mdt_graph_node_feature": ([_vp, _i, _i, _i, _i, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64], _i),
    "mdt_tanh_fwd": ([_vp, _i, _i64, _vp, _vp], _i),
    "mdt_tanh_bwd": ([_vp, _i, _i64, _vp, _vp, _vp], _i),
    "mdt_node_ce": ([_vp, _i, _i64, _i, _vp, _vp, _vp, _f, _f, _i, _f, _vp, _vp, _vp], _i),
    "mdt_node_objective": ([_vp, _i, _i64, _i, _vp, _vp, _vp, _f, _f, _i, _f, _f, _f, _vp, _vp, _vp], _i),
    "mdt_gemm_fp8": ([_vp, _i, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f,
                      C.c_uint64, _vp], _i),
    "mdt_gemm_fp8_q8": ([_vp, _i, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f,
                         C.c_uint64, _vp, _vp, _i64, _i, _vp, _vp], _i),
    "mdt_fp8_quantize": ([_vp, _i, _i, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp], _i),
    "mdt_fp8_scale_update": ([_vp, _i, _vp, _vp, _vp, _vp, _f], _i),
    "mdt_contrastive_loss_workspace_bytes": ([_i, _i], C.c_size_t),
    "mdt_contrastive_loss": ([_vp, _i, _i, _i, _vp, _i64, _vp, _vp, _f, _f, _i, _vp, _f, _vp, _vp, _vp, _i64], _i),
    "mdt_adam_step_multi": ([_vp, _i, _i, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp], _i),
    "mdt_cast": ([_vp, _i, _i, _i64, _vp, _vp], _i),
    "mdt_transpose2d": ([_vp, _i, _i, _i64, _i64, _vp, _i64, _vp, _i64], _i),
    "mdt_adam_step": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _vp], _i),
    "mdt_grad_sumsq_multi": ([_vp, _i, _vp, _vp, _i64, _vp], _i),
    "mdt_grad_sumsq": ([_vp, _i64, _vp, _vp], _i),
    "mdt_grad_norm_finalize": ([_vp, _vp, _i64, _f, _vp, _f, _f, _f, _i, _i, _vp], _i),
    "mdt_adam_step_guarded": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _vp], _i),
    "mdt_adam_step_multi_guarded": ([_vp, _i, _i, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp], _i),
    "mdt_adam_step_ema": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _vp, _vp, _f], _i),
    "mdt_adam_step_multi_ema": ([_vp, _i, _i, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp, _vp, _f], _i),
    "mdt_adam_step_ema_guarded": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i, _vp, _vp, _f], _i),
    "mdt_adam_step_multi_ema_guarded": ([_vp, _i, _i, _vp, _vp, _i64, _f, _f, _f, _f, _f, _i, _vp, _vp, _f], _i),
    "mdt_adam_step_multi_groups": ([_vp, _i, _i, _vp, _vp, _i64, _f, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _f], _i),
    "mdt_adam_step_group": ([_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i, _f, _f, _vp, _vp, _vp, _f], _i),
    "mdt_ema_swap_multi": ([_vp, _i, _i, _vp, _vp, _vp, _i64, _i], _i),
    "mdt_resize_plan_ksize": ([_i, _i], _i),
    "mdt_resize_plan": ([_i, _i, _vp, _vp, _i], _i),
    "mdt_image_norm_lut": ([C.c_double, _vp, _vp, _vp], _i),
    "mdt_image_preprocess": ([_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i], _i),
    "mdt_pack_structure": ([_i, _vp, _vp, _i, _i, _vp, _vp, _vp], _i),
    "mdt_pack_structure_ud": ([_i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp], _i),
}

EXPORTS = tuple(_SIGS)


class MdtError(RuntimeError):
    status = 0


class MdtUnsupported(MdtError):
    """MDT_ERR_UNSUPPORTED: a valid request this build has no kernel for (callers may choose another route); every other
    status is a contract violation or a launch failure and is never to be retried silently."""
    status = -2


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension is the product path and has no fallback. "
            "Build it with `python -m multimodaldiscussiontransformer_amd.build` (hipcc, gfx950).")
    lib = C.CDLL(LIB_PATH)
    for name, (args, res) in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    if lib.mdt_abi_version() != 1:
        raise ImportError("libmdt_hip.so ABI version mismatch")
    # the .so is git-ignored and travels to the GPU box prebuilt: it must be the build of the csrc/ next to it
    skip = os.environ.get("MDT_SKIP_SOURCE_HASH") == "1"
    if skip and ("pytest" in sys.modules or os.environ.get("MDT_BENCH_OFFICIAL") == "1"):
        # the override exists for in-call A/B runs of two builds (tools/ab_libs.sh): a test run or a bench line of record
        # must never inherit it
        raise ImportError("MDT_SKIP_SOURCE_HASH=1 is refused under pytest and bench.py (bench.py --foreign-library for an A/B arm)")
    from .build import source_hash, hash_inputs_present
    if not skip and hash_inputs_present():      # an installed copy without csrc/ or include/ has nothing to compare against
        built, here = lib.mdt_source_hash().decode(), source_hash()
        if built != here:
            raise ImportError(f"{LIB_PATH} was built from other sources (library {built[:16]}, csrc/ {here[:16]}): rebuild with "
                              "`python -m multimodaldiscussiontransformer_amd.build` (MDT_SKIP_SOURCE_HASH=1 overrides, for A/B runs of two builds)")
    return lib


lib = _load()


def reload_env():
    """The library reads its MDT_* environment switches once; call this after changing them (tests, A/B tools)."""
    lib.mdt_reload_env()


def last_route() -> str:
    """The route of this thread's last successful GEMM / attention launch ("w4p", "v4x", ...; include/mdt_hip.h)."""
    return lib.mdt_last_route().decode()


_TILE_QUEUE = None


def enable_dynamic_tile_queue(device="cuda"):
    """Hand the persistent GEMM a zeroed device buffer for its dynamic tile queue (used when MDT_GEMM_DYNAMIC=1)."""
    global _TILE_QUEUE
    if _TILE_QUEUE is None:
        _TILE_QUEUE = torch.zeros(lib.mdt_gemm_tile_queue_bytes() // 4, dtype=torch.int32, device=device)
        check(lib.mdt_gemm_set_tile_queue(_TILE_QUEUE.data_ptr(), _TILE_QUEUE.numel() * 4), "mdt_gemm_set_tile_queue")
    return _TILE_QUEUE


def check(status: int, what: str = ""):
    if status != 0:
        e = (MdtUnsupported if status == -2 else MdtError)(f"{what}: status {status}: {lib.mdt_last_error_string().decode()}")
        e.status = status
        raise e


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return MDT_F32
    if t.dtype == torch.bfloat16:
        return MDT_BF16
    raise MdtError(f"unsupported dtype {t.dtype} (fp32 and bf16 only)")


def ptr(t) -> int:
    if t is None:
        return None
    if not t.is_cuda:
        raise MdtError("libmdt_hip operates on device tensors only (no CPU path)")
    return t.data_ptr()


def stream() -> int:
    if not torch.cuda.is_available():
        raise MdtError("no GPU visible: libmdt_hip is the only compute path (there is no CPU fallback)")
    return torch.cuda.current_stream().cuda_stream
