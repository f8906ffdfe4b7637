"""Tape engine: the host-side scheduler of the fused forward / backward.

The reference runs eager PyTorch autograd over ~1000 small ops per step.  Here a step is a
short *tape* of coarse ops (one per transformer block, exchange, embedding, head), each
of which launches hand-written HIP kernels through the C ABI and knows its own adjoint.
The tape owns activation gradients explicitly, which is what lets the bottleneck-token
exchanges (in-place row writes in the reference: modules/multigraphormer_graph_encoder.py:
371,425,435; modules/multi_graphormer_fusion_layer.py:63-66) stay sparse row updates in
backward too, instead of dense zero-filled gradient tensors.

``TapeFunction`` is the single bridge to ``torch.autograd``: a module's public
``forward`` (same signature as the reference module) wraps its tape-level ``_fwd`` in
one autograd node.  Parameter gradients are accumulated in fp32 — into ``param.main_grad``
(persistent, what the RCCL data-parallel hook all-reduces) when present, otherwise into
temporaries that are handed back to autograd as ordinary ``.grad``s.
"""
from __future__ import annotations

import os

import contextlib
import threading
import weakref
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch

from . import fp8 as F8
from . import ops


# ------------------------------------------------------------------------------------------
# deterministic (ordered) mode: a process-wide switch.  On, every gradient reduction of the backward pass takes its
# fixed-order form (ops.gemm_splitk_ordered, colsum_ordered, layernorm_bwd_ordered, row_segment_sum, attn_bias_grad_ordered:
# plain stores of partials + one sequential reducer instead of fp32 atomics), so loss, gradients and the parameters after
# the optimiser step are bit-for-bit functions of weights, batch, seeds and library build — in ONE process on ONE GPU, bf16
# or fp32 (DESIGN.md §4 "ordered mode").  Off (the default), nothing changes.
_DETERMINISTIC = os.environ.get("MDT_DETERMINISTIC", "0") == "1"


def set_deterministic(on: bool) -> None:
    global _DETERMINISTIC
    if on and F8.ACTIVE is not None:
        raise NotImplementedError("deterministic mode with fp8 GEMMs: the fp8 path has no ordered reductions (disable fp8 first)")
    _DETERMINISTIC = bool(on)


def deterministic() -> bool:
    return _DETERMINISTIC


# ------------------------------------------------------------------------------------------
# activation recomputation: a process-wide policy, read by the modules when they record a pretrained BERT / ViT block and handed
# to transformer_block, which captures it in the block's adjoint.  "none" (the default): the tape keeps every activation of
# every block until backward reaches it.  "ffn": u, h and the fc1 / fc2 adapters' t are dropped after the forward and made
# again from the kept FFN input right before the FFN's adjoint (one more fc1 GEMM per block).  "block": nothing of a block is
# kept but its input and output; the adjoint first runs the block's forward again from the same seeds.  The forward has no float
# atomics and dropout masks are functions of the seeds, so a replay writes the bits the first pass wrote.
RECOMPUTE_POLICIES = ("none", "ffn", "block")


def _checked_policy(policy) -> str:
    if policy not in RECOMPUTE_POLICIES:
        raise ValueError(f"activation recomputation policy {policy!r} is not one of {', '.join(RECOMPUTE_POLICIES)}")
    return policy


RECOMPUTE_FP8_WHY = ("a replayed forward would record the step's amax a second time and take the fp8 producer slots again, so the "
                     "delayed scales of the next step would differ from a run without recomputation")
_RECOMPUTE = _checked_policy(os.environ.get("MDT_RECOMPUTE", "none") or "none")


def set_recompute(policy: str) -> None:
    global _RECOMPUTE
    _checked_policy(policy)
    if policy != "none" and F8.ACTIVE is not None:
        raise NotImplementedError(f"activation recomputation with fp8 GEMMs: {RECOMPUTE_FP8_WHY} (disable fp8 first)")
    _RECOMPUTE = policy


def recompute() -> str:
    return _RECOMPUTE


_ORDERED_WS: dict = {}


def ordered_workspace(nbytes: int, device) -> torch.Tensor:
    """The ordered kernels' workspace of the CURRENT stream: one byte buffer per (device, stream) that only grows.  A call's
    partials are consumed by the reducer enqueued right behind it on the same stream, so consecutive calls share it; a
    buffer that is outgrown goes back to the stream-ordered caching allocator."""
    key = (torch.device(device).index, torch.cuda.current_stream().cuda_stream)
    ws = _ORDERED_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes) * 5 // 4, 1 << 20), dtype=torch.uint8, device=device)
        _ORDERED_WS[key] = ws
    return ws


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None, row_weight=None) -> torch.Tensor:
    """ops.colsum, or its ordered form in deterministic mode."""
    if not _DETERMINISTIC:
        return ops.colsum(x, out=out, row_weight=row_weight)
    ws = ordered_workspace(ops.lib.mdt_colsum_ordered_workspace_bytes(x.shape[0], x.shape[1]), x.device)
    return ops.colsum_ordered(x, out=out, row_weight=row_weight, ws=ws)


def scatter_add(table_f32: torch.Tensor, idx: torch.Tensor, src: torch.Tensor, nrows: int) -> torch.Tensor:
    """ops.row_scatter_add (embedding gradients); deterministic mode: the segment sum over a stable sort of ``idx``."""
    if not _DETERMINISTIC:
        return ops.row_scatter_add(table_f32, idx, src, nrows)
    seg_row, seg_off, order = ops.segments_of(idx.reshape(-1)[:nrows], table_f32.shape[0])
    return ops.row_segment_sum(table_f32, seg_row, seg_off, order, src)


def layernorm_bwd(dy, x, gamma, mean, rstd, **kw):
    """ops.layernorm_bwd, or its ordered form in deterministic mode."""
    if not _DETERMINISTIC:
        return ops.layernorm_bwd(dy, x, gamma, mean, rstd, **kw)
    ws = ordered_workspace(ops.lib.mdt_layernorm_bwd_ordered_workspace_bytes(x.shape[0], x.shape[1]), x.device)
    return ops.layernorm_bwd_ordered(dy, x, gamma, mean, rstd, ws=ws, **kw)


def wgrad_gemm(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, asum=None) -> None:
    """out[N, K] (fp32) += dY^T X over the rows, split-K: fp32 atomics, or in deterministic mode the slabs in ascending order."""
    split = _split_k(dy.shape[1], x.shape[1], dy.shape[0])
    if not _DETERMINISTIC:
        ops.gemm(dy, x, trans_a=True, trans_b=True, out=out, epilogue=ops.EPI_ATOMIC, split_k=split, asum=asum)
        return
    assert asum is None, "deterministic mode: no bias sum rides on the weight-gradient GEMM"
    ws = ordered_workspace(ops.lib.mdt_gemm_splitk_ordered_workspace_bytes(out.shape[0], out.shape[1], split), dy.device)
    ops.gemm_splitk_ordered(dy, x, out, trans_a=True, trans_b=True, split_k=split, ws=ws)


class _StreamState(threading.local):
    """Which branch the calling thread is enqueuing for (autograd runs a tape's backward on its own thread)."""
    side_active = False


_SS = _StreamState()
_SIDE_STREAMS = {}


def side_stream(device) -> "torch.cuda.Stream":
    """The second HIP stream of ``device`` (one per process and device): the image branch of a two-stream tape."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return _SIDE_STREAMS[key]


class Var:
    """An activation on the tape: data + lazily created gradient buffer."""
    __slots__ = ("data", "grad", "needs_grad", "side")

    def __init__(self, data: torch.Tensor, needs_grad: bool = True):
        self.data = data
        self.grad: Optional[torch.Tensor] = None
        self.needs_grad = needs_grad
        self.side = _SS.side_active            # produced (and consumed) by the image branch of a two-stream tape

    @property
    def rows(self):
        return self.data.shape[0]


class Tape:
    def __init__(self, use_main_grad: bool = False, on_params_ready: Optional[Callable] = None, inference: bool = False):
        self.ops: List[Callable[[], None]] = []
        self.inference = inference                 # forward only (torch.no_grad): adjoints and what they hold are dropped
        self.use_main_grad = use_main_grad
        self.tmp_grads = {}
        self.on_params_ready = on_params_ready     # DDP hook: called with the params an op just finished
        self._seed_base = None
        self._seed_ctr = 0
        self.side: Optional[torch.cuda.Stream] = None
        self._main: Optional[torch.cuda.Stream] = None

    # -- two HIP streams ------------------------------------------------------------------
    # The text and image branches of mDT are independent between bottleneck exchanges (the 6 + 6 pre-fusion layers,
    # and the two blocks of every fusion layer).  A two-stream tape enqueues the image branch on a second stream, so
    # the last partially filled wave of one branch's GEMM tiles and its small kernels run beside the other branch's
    # work.  The discipline that keeps this race-free:
    #   * ``fork()``  — side waits for everything main has enqueued; ``join()`` — main waits for side.  In backward
    #     the tape is walked in reverse, so a fork acts as a join and vice versa (both are recorded on the tape).
    #   * only ops inside ``on_side()`` run on the side stream, and they touch nothing but image-branch tensors
    #     (allocated there, by the stream-aware caching allocator), parameters, parameter gradients and index
    #     vectors (all persistent).  Exchange ops run on main strictly between a join and the next fork.
    #   * the one tensor class that crosses the other way — a gradient buffer that a main-stream adjoint creates for
    #     an image-branch activation — is allocated from the side stream's pool (``grad_buf``), so the allocator
    #     recycles it in side-stream order; a dense gradient handed over by an op (``add_grad``) falls back to
    #     ``record_stream``.
    #   * buffer lifetime: the buffer of a Var is written only between the op that made it and the forward of the first block
    #     that reads it (``rows_mix`` is the only in-place writer, and every exchange sits in front of its reader); afterwards
    #     nothing writes it until the tape is dropped.  Adjoints read ``x.data`` at backward time, and a block recorded under the
    #     "block" recomputation policy replays its whole forward from it — on the stream its adjoint runs on, so the replay of
    #     an image-branch block allocates and frees on the side stream inside the recorded ``on_side`` region.
    def enable_side(self, device):
        # Deterministic mode runs the tape on ONE stream.  Both branch streams accumulate (read-modify-write) into shared
        # destinations — the bottleneck exchanges' gradient buffers (rows_mix, take_rows, scatter_rows, graph_node_features
        # with accumulate=True) and the workspace of the ordered reducers — and the order of those updates is fixed by
        # fork / join events only where an exchange sits strictly between a join and the next fork; that has not been shown
        # for every accumulate, so the mode does not rely on it.
        if _DETERMINISTIC:
            return
        if self.side is None:
            self.side = side_stream(device)

    def fork(self):
        if self.side is None:
            return
        self.side.wait_stream(torch.cuda.current_stream())
        self.record(lambda: torch.cuda.current_stream().wait_stream(self.side))

    def join(self):
        if self.side is None:
            return
        torch.cuda.current_stream().wait_stream(self.side)
        self.record(lambda: self.side.wait_stream(torch.cuda.current_stream()))

    def _enter_side(self):
        self._main = torch.cuda.current_stream()
        torch.cuda.set_stream(self.side)
        _SS.side_active = True

    def _leave_side(self):
        if _SS.side_active:
            torch.cuda.set_stream(self._main)
            _SS.side_active = False

    @contextlib.contextmanager
    def on_side(self):
        """Ops issued inside run on the side stream, forward and backward (no-op on a single-stream tape)."""
        if self.side is None:
            yield
            return
        self.record(self._leave_side)             # backward reaches the region's first op last
        self._enter_side()
        try:
            yield
        finally:
            self._leave_side()
            self.record(self._enter_side)

    def _crossing(self, v: "Var", t: torch.Tensor):
        """``t`` was just allocated on the current stream as a gradient of ``v``: tell the allocator when the other
        branch is the one that will read it."""
        if self.side is not None and v.side != _SS.side_active:
            t.record_stream(self.side if v.side else self._main)

    def next_seed(self) -> int:
        """A fresh 63-bit dropout-site seed (CPU generator: follows torch.manual_seed, no device sync)."""
        if self._seed_base is None:
            self._seed_base = int(torch.randint(0, 2 ** 62, (1,)).item())
        self._seed_ctr += 1
        return (self._seed_base + 0x9E3779B97F4A7C15 * self._seed_ctr) & 0x7FFFFFFFFFFFFFFF

    # -- gradient plumbing ------------------------------------------------------------
    def record(self, bwd: Callable[[], None]):
        if not self.inference:                     # the closure keeps every saved activation alive
            self.ops.append(bwd)

    def adjoint(self, o: "Var", bwd: Callable[[torch.Tensor], None], take: bool = True):
        """Record ``bwd(g)`` as the adjoint of the op that made ``o``.  The backward pass calls it with ``g = o.grad``, taken
        out of ``o`` first (``take=False``: left there), and skips it when nothing contributed a gradient to ``o``."""
        def run():
            g = o.grad
            if take:
                o.grad = None
            if g is not None:
                bwd(g)

        self.record(run)

    def pgrad(self, p: torch.nn.Parameter) -> Optional[torch.Tensor]:
        """fp32 accumulation buffer of a parameter, or None when it is frozen."""
        if p is None or not p.requires_grad:
            return None
        if self.use_main_grad:
            g = getattr(p, "main_grad", None)
            if g is None:
                raise RuntimeError("use_main_grad=True but a trainable parameter has no .main_grad buffer")
            return g
        g = self.tmp_grads.get(id(p))
        if g is None:
            g = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            self.tmp_grads[id(p)] = g
        return g

    def grad_buf(self, v: Var) -> torch.Tensor:
        """Gradient buffer of ``v`` for sparse (row-wise) accumulation; zero-created on first use."""
        if v.grad is None:
            if self.side is not None and v.side and not _SS.side_active:
                # an exchange adjoint (main stream) creates the gradient of an image-branch activation: take the
                # buffer from the side stream's pool, where its reader will run and where it is freed.  The side
                # stream is idle here (between a join and the next fork), so waiting for its zero-fill costs nothing;
                # record_stream instead would park the block behind an event on every free, and a host that runs
                # steps ahead of the GPU then falls back to hipMalloc
                with torch.cuda.stream(self.side):
                    v.grad = torch.zeros_like(v.data)
                torch.cuda.current_stream().wait_stream(self.side)
            else:
                v.grad = torch.zeros_like(v.data)
                self._crossing(v, v.grad)
        return v.grad

    def add_grad(self, v: Var, g: torch.Tensor):
        """Dense contribution: take ownership of ``g`` or accumulate it."""
        if not v.needs_grad:
            return
        if v.grad is None:
            v.grad = g
            self._crossing(v, g)
        else:
            ops.row_axpby(v.grad, v.grad.shape[0], a=g, accumulate=True)

    def backward(self):
        try:
            while self.ops:
                self.ops.pop()()
        finally:
            self._leave_side()
        self.ops = []
        self.sync_streams()
        if F8.ACTIVE is not None:
            F8.ACTIVE.end_of_step()          # this step's |x| maxima become the next step's scales (one launch)

    def sync_streams(self):
        """End of a pass: whatever follows on the main stream sees the side stream's work."""
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)


# ------------------------------------------------------------------------------------------
# parameter bundles
@dataclass
class LoraSlot:
    """A low-rank adapter beside one dense layer [out, in] of a block: ``A`` [r, in], ``Bt`` [r, out] (the rows of B^T),
    ``scale`` = alpha / r.  The layer computes x W^T + b + scale (x A^T) Bt."""
    A: torch.nn.Parameter
    Bt: torch.nn.Parameter
    scale: float = 1.0


@dataclass
class BlockParams:
    """One transformer block.  ``qkv_w`` is the row-concatenation [Wq; Wk; Wv] (3D x D)."""
    qkv_w: torch.nn.Parameter
    qkv_b: torch.nn.Parameter
    o_w: torch.nn.Parameter
    o_b: torch.nn.Parameter
    ln1_w: torch.nn.Parameter
    ln1_b: torch.nn.Parameter
    fc1_w: torch.nn.Parameter
    fc1_b: torch.nn.Parameter
    fc2_w: torch.nn.Parameter
    fc2_b: torch.nn.Parameter
    ln2_w: torch.nn.Parameter
    ln2_b: torch.nn.Parameter
    # low-rank adapters beside the (frozen) QKV projection, or None: lora_A / lora_Bt [|J| r, D] hold the rows of A_j / B_j^T
    # target-major, lora_cols the thirds of the qkv buffer they add to (0 = q, 1 = k, 2 = v), lora_scale = alpha / r
    lora_A: Optional[torch.nn.Parameter] = None
    lora_Bt: Optional[torch.nn.Parameter] = None
    lora_cols: Optional[tuple] = None
    lora_scale: float = 1.0
    # adapters beside the attention output projection (A [r, D], Bt [r, D]), fc1 (A [r, D], Bt [r, F]) and fc2 (A [r, F], Bt [r, D])
    lora_o: Optional[LoraSlot] = None
    lora_fc1: Optional[LoraSlot] = None
    lora_fc2: Optional[LoraSlot] = None

    def dense_lora(self):
        return [s for s in (self.lora_o, self.lora_fc1, self.lora_fc2) if s is not None]

    def all(self):
        base = [self.qkv_w, self.qkv_b, self.o_w, self.o_b, self.ln1_w, self.ln1_b, self.fc1_w, self.fc1_b,
                self.fc2_w, self.fc2_b, self.ln2_w, self.ln2_b]
        if self.lora_A is not None:
            base = base + [self.lora_A, self.lora_Bt]
        return base + [p for s in self.dense_lora() for p in (s.A, s.Bt)]


@dataclass
class AttnSpec:
    nseq: int
    S: int
    H: int
    seq_stride: Optional[int] = None
    pos_stride: int = 1
    scale: Optional[float] = None
    key_mask: Optional[torch.Tensor] = None        # u8[nseq,S]
    dense_bias: Optional[torch.Tensor] = None      # f32[nseq,H,S,S]
    dense_bias_var: Optional[Var] = None           # gradient sink for dense_bias (module-level API)
    attn_bias: Optional[torch.Tensor] = None       # f32[nseq,S,S]   structural: {0,-inf} mask
    spatial_pos: Optional[torch.Tensor] = None     # i32[nseq,S-1,S-1]
    sp_table: Optional[torch.nn.Parameter] = None  # [num_spatial,H]
    virt: Optional[torch.nn.Parameter] = None      # [1,H]
    key_pad: Optional[torch.Tensor] = None         # u8[nseq,S]
    seq_offsets: Optional[torch.Tensor] = None     # i32[nseq+1]: ragged sequences of at most S rows (no masks / biases)
    q_limit: int = 0                               # > 0: only the first q_limit rows of every sequence are needed as queries
    bins: Optional[list] = None                    # ragged: [(sequence ids i32[n], cap), ...] — one launch per length bin

    def kwargs(self):
        return dict(seq_stride=self.seq_stride, pos_stride=self.pos_stride, scale=self.scale, key_mask=self.key_mask,
                    seq_offsets=self.seq_offsets, q_limit=self.q_limit, bins=self.bins,
                    dense_bias=self.dense_bias, attn_bias=self.attn_bias, spatial_pos=self.spatial_pos,
                    sp_table=None if self.sp_table is None else self.sp_table.data,
                    virt=None if self.virt is None else self.virt.data.view(-1), key_pad=self.key_pad)


# ------------------------------------------------------------------------------------------
# helpers
def _split_k(n_out: int, k_out: int, red: int) -> int:
    tiles = ((n_out + 127) // 128) * ((k_out + 127) // 128)
    s = max(1, 1024 // max(1, tiles))
    return int(max(1, min(s, red // 1024 if red >= 1024 else 1)))


_WGRAD_ASUM = os.environ.get("MDT_WGRAD_ASUM", "1") != "0"     # 0: separate column-sum launches (A/B runs)


def wgrad(tape: Tape, dy: torch.Tensor, x: torch.Tensor, w: torch.nn.Parameter, b: Optional[torch.nn.Parameter]):
    """dW[N,K] += dY^T X (fp32, split-K atomics) and db[N] += colsum(dY)."""
    gw = tape.pgrad(w)
    gb = tape.pgrad(b) if b is not None else None
    if gw is not None:
        # the bias gradient rides on the weight-gradient GEMM, which streams dY anyway (MDT_EPI_ASUM; bf16 operands) — not in
        # deterministic mode, where it is a column sum of its own
        ride = gb is not None and dy.dtype == torch.bfloat16 and _WGRAD_ASUM and not _DETERMINISTIC
        wgrad_gemm(dy, x, gw.view(dy.shape[1], x.shape[1]), asum=gb.view(-1) if ride else None)
        if ride:
            return
    if gb is not None:
        colsum(dy, out=gb.view(-1))


_LN_BIAS_RIDE = os.environ.get("MDT_LN_BIAS_RIDE", "1") != "0"    # 0: those sums stay in the LayerNorm backward (A/B runs)


# ------------------------------------------------------------------------------------------
# A/B switches of the embedding ops, and the epoch of weights rewritten behind torch's back
EMBED_LN_FUSED = os.environ.get("MDT_EMBED_LN_FUSED", "1") != "0"         # 0: embedding sum and its LayerNorm as two launches (A/B runs, tests)
PATCH_K_PAD = os.environ.get("MDT_PATCH_K_PAD", "1") != "0"               # 0: ViT-L/14's K = 588 patch GEMMs stay on the any-shape kernel (A/B runs)
PATCH_EMBED_FUSED = os.environ.get("MDT_PATCH_EMBED_FUSED", "1") != "0"   # 0: patch gather, GEMM and assembly as three launches (A/B runs, tests)
WEIGHT_EPOCH = 0            # bumped by whoever rewrites weights behind torch's back (FusedAdam's step and swap, a restore, a broadcast)


def weights_changed():
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1


def weight_stamp(w: torch.nn.Parameter) -> tuple:
    """What a copy derived from ``w`` (zero-padded here, 8-bit in fp8.Fp8State) is stamped with; the copy is stale once the
    stamp differs: torch-side in-place writes bump ``_version``, writes behind torch's back bump WEIGHT_EPOCH, a new storage moves
    ``data_ptr``."""
    return (w._version, WEIGHT_EPOCH, w.data_ptr())


_KP_CACHE: dict = {}


def _k_padded(w: torch.nn.Parameter, wmat: torch.Tensor, kp: int) -> torch.Tensor:
    """[out, kp] copy of a weight viewed as [out, k] with zero columns behind k, cached until the weight's stamp changes."""
    key = (id(w), kp)
    ver = weight_stamp(w)
    hit = _KP_CACHE.get(key)
    if hit is not None and hit[0]() is w and hit[1] == ver:
        return hit[2]
    wp = torch.zeros(wmat.shape[0], kp, dtype=wmat.dtype, device=wmat.device)
    wp[:, :wmat.shape[1]].copy_(wmat)
    _KP_CACHE[key] = (weakref.ref(w), ver, wp)
    return wp


def dgrad(dy: torch.Tensor, w: torch.nn.Parameter, **kw) -> torch.Tensor:
    """dX[M, in] = dY[M, out] @ W[out, in] (+ epilogue).  W is read in place as the k-major operand: since the 4-wave
    kernel reads k-major fragments with asm ds_read_b64_tr_b16 pairs (gemm.hip, w4_frag) that form runs as fast as the
    k-contiguous one through a cached transposed copy of W (tools/gemm_ab.py --nn-dgrad; whole step 137.9 / 138.0 ms
    either way in one call), so no copy is kept."""
    return ops.gemm(dy, w.data, trans_b=True, **kw)


def linear(f8, x: torch.Tensor, w: torch.nn.Parameter, tag: str, *, grad=False, x8=None, q8_site=None, q8_grad=False, **kw):
    """One 8-bit-capable GEMM of a block: x @ W^T, or with ``grad`` the input gradient x @ W.  The 8-bit kernel where ``f8``
    (fp8.ACTIVE as the block read it; None: bf16 everywhere) takes the site (tag, id(w)), else the bf16 GEMM with the same
    epilogue keywords ``kw``.  ``x8``: x already quantised by its producer; ``q8_site`` / ``q8_grad``: the site (and format)
    of the GEMM that consumes the output.  → (out, (out8, inv scale) or None)"""
    r = None if f8 is None else f8.linear(x, w, (tag, id(w)), transposed_weight=grad, grad=grad, x8=x8, q8_site=q8_site,
                                          q8_grad=q8_grad, **kw)
    if r is None:
        return (dgrad(x, w, **kw) if grad else ops.gemm(x, w.data, **kw)), None
    return r if q8_site is not None else (r, None)


def dyd_rides(g: torch.Tensor) -> bool:
    """bias gradients of the dense layers behind a LayerNorm ride on their weight-gradient GEMM (MDT_EPI_ASUM) when that
    GEMM takes the 256 x 256 kernel (bf16, enough rows); small problems keep the sums inside the LayerNorm backward"""
    return _LN_BIAS_RIDE and g.dtype == torch.bfloat16 and g.shape[0] >= 8192 and not _DETERMINISTIC


def _ln_bwd(tape, dy, x, w, b, mean, rstd, add=None):
    return layernorm_bwd(dy, x, w.data, mean, rstd, add=add, dgamma=tape.pgrad(w), dbeta=tape.pgrad(b))


def _ln_bwd_dense(tape, dy, x, w, b, mean, rstd, bias_param, p_drop, seed, add=None):
    """LayerNorm backward + the fused tail for the dense layer that feeds it: returns (dx, dxd) where dxd is dx
    through that layer's hidden-dropout mask, and accumulates the layer's bias gradient (column sums of dxd)."""
    gb = tape.pgrad(bias_param) if bias_param is not None else None
    return layernorm_bwd(dy, x, w.data, mean, rstd, add=add, dgamma=tape.pgrad(w), dbeta=tape.pgrad(b),
                         drop_p=p_drop, drop_seed=seed, colsum=None if gb is None else gb.view(-1),
                         want_dropped=True)


def lora_down_site(src: torch.Tensor, A: torch.Tensor, p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """t = dropout_p(src) A^T of one adapter site: the mask is made inside the kernel from ``seed`` (counters row * width + col of
    ``src`` as passed) and no dropped copy of ``src`` exists; p = 0 is the plain ``ops.lora_down`` launch."""
    return ops.lora_down_drop(src, A, drop_p=p, drop_seed=seed) if p > 0 else ops.lora_down(src, A)


def lora_site_bwd(dt: torch.Tensor, src: torch.Tensor, A: torch.Tensor, gA, dx, ws, p: float, seed: int) -> None:
    """What a site's input dropout changes in the adjoint: dA += dt^T dropout_p(src) and dx += s o (dt A) under the same mask."""
    if gA is not None:
        if p > 0:
            ops.lora_wgrad_drop(dt, src, gA, drop_p=p, drop_seed=seed, ws=ws)
        else:
            ops.lora_wgrad(dt, src, gA, ws=ws)
    if dx is not None:
        if p > 0:
            ops.lora_up_add_drop(dt, A, dx, drop_p=p, drop_seed=seed)
        else:
            ops.lora_up_add(dt, A, dx)


def lora_fwd(P: BlockParams, src: torch.Tensor, qkv: torch.Tensor, p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """Adapters of the QKV projection, forward: t = dropout_p(src) A^T (stored in the working dtype; one site: the q, k and v
    adapters read the same dropped source), then qkv[:, c_j : c_j + D] += s t_j Bt_j for every target, in place and before
    attention reads qkv.  → t"""
    D = src.shape[1]
    r = P.lora_A.shape[0] // len(P.lora_cols)
    t = lora_down_site(src, P.lora_A.data, p, seed)
    for j, c in enumerate(P.lora_cols):
        ops.lora_up_add(t[:, j * r:(j + 1) * r], P.lora_Bt.data[j * r:(j + 1) * r], qkv[:, c * D:(c + 1) * D], alpha=P.lora_scale)
    return t


def lora_bwd(tape: Tape, P: BlockParams, src: torch.Tensor, t: torch.Tensor, dqkv: torch.Tensor, dx: Optional[torch.Tensor],
             p: float = 0.0, seed: int = 0) -> None:
    """Adjoint of lora_fwd: dBt_j += s t_j^T dqkv_j, dt_j = s dqkv_j Bt_j^T, dA += dt^T src and, where the block wants its input
    gradient, dx += dt A on the output of the frozen projection's dgrad.  The weight gradients are sums in a fixed order
    (ops.lora_wgrad): the same launches in the default and in the deterministic mode; a frozen adapter costs nothing.  ``p``,
    ``seed``: the site's input dropout (lora_site_bwd)."""
    D = src.shape[1]
    n = P.lora_A.shape[0]
    r = n // len(P.lora_cols)
    s = P.lora_scale
    gA, gBt = tape.pgrad(P.lora_A), tape.pgrad(P.lora_Bt)
    want_dt = gA is not None or dx is not None
    dt = torch.empty(src.shape[0], n, dtype=src.dtype, device=src.device) if want_dt else None
    ws = None
    if gA is not None or gBt is not None:
        ws = ordered_workspace(ops.lib.mdt_lora_wgrad_workspace_bytes(src.shape[0], n, D), src.device)
    for j, c in enumerate(P.lora_cols):
        rows, dq = slice(j * r, (j + 1) * r), dqkv[:, c * D:(c + 1) * D]
        if gBt is not None:
            ops.lora_wgrad(t[:, rows], dq, gBt.view(n, D)[rows], alpha=s, ws=ws)
        if want_dt:
            ops.lora_down(dq, P.lora_Bt.data[rows], out=dt[:, rows], alpha=s)
    if want_dt:
        lora_site_bwd(dt, src, P.lora_A.data, None if gA is None else gA.view(n, D), dx, ws, p, seed)


def lora_dense_bwd(tape: Tape, L: LoraSlot, src: torch.Tensor, t: torch.Tensor, g: torch.Tensor, dx: Optional[torch.Tensor],
                   p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """Adjoint of a dense layer's adapter y += s (src A^T) Bt, ``g`` the gradient of that sum [R, out], ``t`` the stored src A^T:
    dBt += s t^T g, dt = s g Bt^T, dA += dt^T src, and dx += dt A where ``dx`` (the output of the base layer's dgrad) is given.
    → dt, for the caller whose dx takes another epilogue (fc2: times u).  Fixed-order weight gradients as in lora_bwd; a frozen
    adapter launches nothing for them.  ``p``, ``seed``: the site's input dropout (``t`` was made from dropout_p(src))."""
    r = L.A.shape[0]
    gA, gBt = tape.pgrad(L.A), tape.pgrad(L.Bt)
    ws = None
    if gA is not None or gBt is not None:
        wide = max(src.shape[1], g.shape[1])
        ws = ordered_workspace(ops.lib.mdt_lora_wgrad_workspace_bytes(src.shape[0], r, wide), src.device)
    if gBt is not None:
        ops.lora_wgrad(t, g, gBt.view(r, g.shape[1]), alpha=L.scale, ws=ws)
    dt = ops.lora_down(g, L.Bt.data, alpha=L.scale)
    lora_site_bwd(dt, src, L.A.data, None if gA is None else gA.view(r, src.shape[1]), dx, ws, p, seed)
    return dt


# ------------------------------------------------------------------------------------------
# ops
def transformer_block(tape: Tape, x: Var, P: BlockParams, spec: AttnSpec, *, pre_ln: bool, eps: float,
                      p_hidden: float = 0.0, p_attn: float = 0.0, p_act: float = 0.0, keep_rows=None, act: str = "gelu",
                      recompute: str = "none", p_lora: float = 0.0) -> Var:
    """One encoder block (post-LN: HF BertLayer / Graphormer layer; pre-LN: HF ViTLayer or
    Graphormer with --pre-layernorm).  7 GEMM-class launches + attention + 2 LayerNorms
    forward; the adjoint mirrors it with the residual adds folded into epilogues.  The attention half
    (``attn_fwd`` / ``attn_bwd``) and the FFN half (``ffn_fwd`` / ``ffn_bwd``) are written once; the two placements
    differ in what each LayerNorm normalises, what the FFN's residual is, and the tails of ``bwd``.
    Dropout (training): ``p_attn`` on attention probabilities (inside the attention kernel),
    ``p_hidden`` on the two dense outputs before their residual adds and ``p_act`` after GELU
    (both in the GEMM epilogue); masks are regenerated in backward from per-site seeds.  The FFN
    saves ``u`` = d h / d pre-activation (GELU' times the activation-dropout scale) rather than
    the pre-activation itself, so the backward epilogue is a single multiply.  ``act``: the FFN activation, a name of
    ``ops.ACT_KINDS``.  "gelu" (erf form) is fused into fc1's epilogue; every other kind runs fc1 as a plain bias GEMM and
    ``ops.act_fwd`` then turns the pre-activation into h (in place) and u — the adjoint is the same for all of them.

    Low-rank adapters (``P.lora_A`` on QKV; ``P.lora_o`` / ``P.lora_fc1`` / ``P.lora_fc2`` on the dense layers): t = x A^T by
    ``ops.lora_down``, then the sum s t Bt joins the base GEMM's output in one pass — under the hidden-dropout mask the GEMM's
    epilogue applied (``lora_up_add_drop``: o, fc2) or in front of the non-linearity (``lora_up_act``: fc1, which then runs as
    a plain bias GEMM for every ``act``).  Backward: ``lora_dense_bwd``; fc2's share of du takes the multiply by u in
    ``lora_up_add_mul``.  The block still takes exactly four dropout seeds.

    ``p_lora`` (PEFT's lora_dropout, one probability for all adapters of the block): every adapter reads dropout(x), t =
    dropout(x) A^T.  The mask is made inside the adapter kernels (``lora_down_drop`` forward, ``lora_wgrad_drop`` for dA,
    ``lora_up_add_drop`` for dx += s o (dt A), ``lora_up_add_mul_drop`` for fc2's share of du) from one further seed per adapter
    site present, drawn after the four above in the order qkv, out, fc1, fc2; the fused QKV adapters are ONE site.  0 draws
    no seed and launches what the block launched before.

    ``keep_rows`` (i32[R]): only these token rows of the block's OUTPUT are needed downstream (the last fusion
    layer feeds nothing but bottleneck token 0 and [CLS] of every comment to the graph / the head).  Keys and
    values still come from every row, but the output projection, both LayerNorms and the FFN — three quarters of
    the block's GEMM work — run on the R kept rows only, and the block returns [R, D] in ``keep_rows`` order.
    Exact: the dropped rows' outputs are dead values in the reference too.

    ``recompute`` (a name of RECOMPUTE_POLICIES; ignored by a forward-only tape): "ffn" drops u, h and the fc1 / fc2 adapters' t
    after the forward and makes them again from the kept FFN input in front of ``ffn_bwd``; "block" keeps nothing but ``x`` and
    the output, and the adjoint runs ``run`` — the same launches, seeds, ``keep_rows`` and ``spec`` — a second time before the
    unchanged ``bwd``.  Neither draws a seed, so every dropout site of the tape keeps its seed under every policy."""
    xd = x.data
    s_attn, s_o, s_act, s_f2 = (tape.next_seed() for _ in range(4))
    if not 0.0 <= p_lora < 1.0:
        raise ValueError(f"transformer_block: p_lora={p_lora} is not in [0, 1)")
    # adapter-input dropout: drawn here, outside run(), so that the "block" replay and the "ffn" re-run see the same masks
    sl_qkv = sl_o = sl_f1 = sl_f2 = 0
    if p_lora > 0:
        sl_qkv = tape.next_seed() if P.lora_A is not None else 0
        sl_o = tape.next_seed() if P.lora_o is not None else 0
        sl_f1 = tape.next_seed() if P.lora_fc1 is not None else 0
        sl_f2 = tape.next_seed() if P.lora_fc2 is not None else 0
    kw = dict(spec.kwargs(), drop_p=p_attn, drop_seed=s_attn)
    R = None if keep_rows is None else int(keep_rows.numel())
    f8 = F8.ACTIVE
    if act not in ops.ACT_KINDS:
        raise ValueError(f"transformer_block: unknown activation {act!r} (one of {sorted(ops.ACT_KINDS)})")
    if act != "gelu" and f8 is not None:
        raise NotImplementedError(f"fp8 GEMMs with the {act} activation: the fused fp8 producer of h is fc1's erf-GELU epilogue")
    if P.lora_A is not None and f8 is not None:
        raise NotImplementedError("fp8 GEMMs on a block with low-rank adapters: the adapter sum enters the bf16 qkv buffer only "
                                  "(run adapters in bf16, or fp8 without --lora-rank)")
    Lo, L1, L2 = P.lora_o, P.lora_fc1, P.lora_fc2
    if P.dense_lora() and f8 is not None:
        raise NotImplementedError("fp8 GEMMs on a block with low-rank adapters: the adapter sums of the output projection, fc1 and "
                                  "fc2 enter bf16 buffers only (run adapters in bf16, or fp8 without --lora-rank)")
    # read here, once, and captured by the adjoint: autograd runs the backward on another thread, after the caller may have
    # switched the process-wide policy.  A forward-only tape (or region of one) keeps nothing, so there is nothing to recompute
    policy = "none" if tape.inference else _checked_policy(recompute)
    if policy != "none" and f8 is not None:
        raise NotImplementedError(f"transformer_block(recompute={policy!r}) with fp8 GEMMs: {RECOMPUTE_FP8_WHY}")

    def gather(src):
        """rows ``keep_rows`` of src (identity when the block keeps everything)"""
        if keep_rows is None:
            return src
        out_ = torch.empty(R, src.shape[1], dtype=src.dtype, device=src.device)
        ops.row_axpby(out_, R, a=src, ai=keep_rows)
        return out_

    def spread(g_):
        """adjoint of gather: a tensor of the block input's rows that is zero except g_ at ``keep_rows``"""
        if keep_rows is None:
            return g_
        full = torch.zeros(xd.shape[0], g_.shape[1], dtype=g_.dtype, device=g_.device)
        ops.row_axpby(full, R, di=keep_rows, a=g_)
        return full

    def ln8(x_, lw, lb, w_, tag):
        """LayerNorm whose output feeds the 8-bit GEMM (tag, w_): the fp8 copy leaves the LayerNorm kernel itself when that site
        has a scale (fp8.py producer_slot).  → (y, mean, rstd, (y8, inv scale) or None)"""
        slot = None if (f8 is None or x_.dtype != torch.bfloat16) else f8.producer_slot(x_.shape[0], w_, (tag, id(w_)))
        if slot is None:
            return (*ops.layernorm_fwd(x_, lw.data, lb.data, eps), None)
        return (*ops.layernorm_fwd(x_, lw.data, lb.data, eps, q8=slot[:4]), (slot[0], slot[4]))

    def run():
        """The block's forward from ``xd`` with the seeds drawn above → (output, adjoint).  The adjoint's closure is what keeps
        the activations: a caller that drops it keeps nothing of the block, and a second call makes the same tensors again."""
        def attn_fwd(src, src8):
            """attention half: QKV of ``src`` (all rows), attention, output projection + residual x on the kept rows"""
            qkv_, _ = linear(f8, src, P.qkv_w, "qkv", x8=src8, bias=P.qkv_b.data)
            lt_ = None
            if P.lora_A is not None:           # the adapters' sum joins qkv before attention reads it; t is kept for backward only
                lt_ = lora_fwd(P, src, qkv_, p_lora, sl_qkv)
                if tape.inference:
                    lt_ = None
            ctx_full_, lse_ = ops.attention_fwd(qkv_, spec.nseq, spec.S, spec.H, **kw)
            ctx_, xk = gather(ctx_full_), gather(xd)
            t_ = ops.gemm(ctx_, P.o_w.data, bias=P.o_b.data, residual=xk, drop_p=p_hidden, drop_seed=s_o)
            if Lo is not None:                 # the adapter's sum joins under the mask the GEMM's epilogue applied
                lto = lora_down_site(ctx_, Lo.A.data, p_lora, sl_o)
                ops.lora_up_add_drop(lto, Lo.Bt.data, t_, alpha=Lo.scale, drop_p=p_hidden, drop_seed=s_o)
                if not tape.inference:
                    lts["o"] = lto
            return qkv_, lt_, ctx_full_, lse_, ctx_, t_

        def fc2_fwd(h_, h8, res):
            y_ = linear(f8, h_, P.fc2_w, "fc2", x8=h8, bias=P.fc2_b.data, residual=res, drop_p=p_hidden, drop_seed=s_f2)[0]
            if L2 is not None:
                lt2 = lora_down_site(h_, L2.A.data, p_lora, sl_f2)
                ops.lora_up_add_drop(lt2, L2.Bt.data, y_, alpha=L2.scale, drop_p=p_hidden, drop_seed=s_f2)
                if not tape.inference:
                    lts["fc2"] = lt2
            return y_

        def fc1_fwd(src, src8):
            """fc1 and the activation: → (u, h, the 8-bit h or None).  The "ffn" policy's adjoint calls it a second time."""
            if L1 is not None:      # the adapter's sum joins the stored pre-activation in front of the non-linearity, whatever its kind
                pre_ = ops.gemm(src, P.fc1_w.data, bias=P.fc1_b.data)
                lt1 = lora_down_site(src, L1.A.data, p_lora, sl_f1)
                h_, u_ = ops.lora_up_act(lt1, L1.Bt.data, pre_, act, alpha=L1.scale, drop_p=p_act, drop_seed=s_act, out=pre_,
                                         want_u=not tape.inference)
                if not tape.inference:
                    lts["fc1"] = lt1
                return u_, h_, None
            if act != "gelu":       # fc1 leaves the pre-activation; one more launch makes h (in place) and u of it
                pre_ = ops.gemm(src, P.fc1_w.data, bias=P.fc1_b.data)
                h_, u_ = ops.act_fwd(pre_, act, drop_p=p_act, drop_seed=s_act, out=pre_, want_u=not tape.inference)
                return u_, h_, None
            u_ = torch.empty(src.shape[0], P.fc1_w.shape[0], dtype=src.dtype, device=src.device)
            h_, h8 = linear(f8, src, P.fc1_w, "fc1", x8=src8, q8_site=("fc2", id(P.fc2_w)), bias=P.fc1_b.data, aux=u_,
                            epilogue=ops.EPI_GELU | ops.EPI_AUX_GRAD, drop_p=p_act, drop_seed=s_act)
            return u_, h_, h8

        def ffn_fwd(src, src8, res):
            """FFN half: fc1 writes h and u (and, 8-bit, the quantised h that fc2 then reads), fc2 adds ``res``"""
            u_, h_, h8 = fc1_fwd(src, src8)
            return u_, h_, fc2_fwd(h_, h8, res)

        lts = {}        # the stored t = x A^T of the dense adapters, for backward only
        # a_in / f_in: what the attention / FFN half reads; t: the attention half's output (its residual is always x)
        if not pre_ln:
            a_in = xd
            qkv, lt, ctx_full, lse, ctx, t = attn_fwd(a_in, None)
            f_in, m1, r1, f_in8 = ln8(t, P.ln1_w, P.ln1_b, P.fc1_w, "fc1")
            u, h, y = ffn_fwd(f_in, f_in8, f_in)
            out, m2, r2 = ops.layernorm_fwd(y, P.ln2_w.data, P.ln2_b.data, eps)
        else:
            a_in, m1, r1, a_in8 = ln8(xd, P.ln1_w, P.ln1_b, P.qkv_w, "qkv")
            qkv, lt, ctx_full, lse, ctx, t = attn_fwd(a_in, a_in8)
            f_in, m2, r2, f_in8 = ln8(t, P.ln2_w, P.ln2_b, P.fc1_w, "fc1")
            u, h, out = ffn_fwd(f_in, f_in8, t)
        if policy == "ffn":     # fc2 has been enqueued behind h: u, h and the FFN adapters' t are made again from f_in in ffn_bwd
            u = h = None
            lts.pop("fc1", None)
            lts.pop("fc2", None)

        def ffn_bwd(gd, fc2_b, dres):
            """FFN half: ``gd`` = gradient of fc2's output behind its dropout; ``fc2_b``: the bias whose gradient rides on the
            weight-gradient GEMM (None: summed elsewhere).  → gradient of the half's input (+ ``dres``)"""
            nonlocal u, h
            if policy == "ffn":     # the fc1 path the forward took, from the same seed: the same bits
                u, h, _ = fc1_fwd(f_in, None)
                if L2 is not None:
                    lts["fc2"] = lora_down_site(h, L2.A.data, p_lora, sl_f2)
            wgrad(tape, gd, h, P.fc2_w, fc2_b)
            gb1 = tape.pgrad(P.fc1_b)           # fc1 bias gradient = colsum(du): fused into the GEMM epilogue
            det = _DETERMINISTIC                # ... or, in deterministic mode, summed from the stored du in a fixed order
            # an fc2 adapter adds its share of du behind the GEMM, so the bias sum cannot ride on that GEMM's epilogue either
            late = det or L2 is not None
            dt2 = lora_dense_bwd(tape, L2, h, lts["fc2"], gd, None, p_lora, sl_f2) if L2 is not None else None
            du, du8 = linear(f8, gd, P.fc2_w, "d_fc2", grad=True, q8_site=("d_fc1", id(P.fc1_w)), q8_grad=True, aux=u,
                             epilogue=ops.EPI_MULAUX, colsum=None if (gb1 is None or late) else gb1.view(-1))
            if L2 is not None:                  # dh is never materialised: the adapter's share takes the same multiply by u
                if p_lora > 0:                  # ... under the mask the adapter read h through
                    ops.lora_up_add_mul_drop(dt2, L2.A.data, du, u, drop_p=p_lora, drop_seed=sl_f2)
                else:
                    ops.lora_up_add_mul(dt2, L2.A.data, du, u)
            if late and gb1 is not None:
                colsum(du, out=gb1.view(-1))
            wgrad(tape, du, f_in, P.fc1_w, None)
            df = linear(f8, du, P.fc1_w, "d_fc1", grad=True, x8=du8, residual=dres)[0]     # 8-bit when the GEMM above handed over the quantised du
            if L1 is not None:
                lora_dense_bwd(tape, L1, f_in, lts["fc1"], du, df, p_lora, sl_f1)
            if policy == "ffn":
                u = h = None
            return df

        def attn_bwd(dtd, o_b, want_dx, dres=None):
            """attention half: ``dtd`` = gradient of the output projection behind its dropout (R rows; attention backward and the
            QKV weight gradient see all rows).  → gradient of the half's input (+ ``dres`` at the kept rows), None unless wanted"""
            wgrad(tape, dtd, ctx, P.o_w, o_b)
            dctx = ops.gemm(dtd, P.o_w.data, trans_b=True)
            if Lo is not None:
                lora_dense_bwd(tape, Lo, ctx, lts["o"], dtd, dctx, p_lora, sl_o)
            dqkv = _attention_bwd(tape, spec, kw, dctx, qkv, ctx_full, lse, spread)
            wgrad(tape, dqkv, a_in, P.qkv_w, P.qkv_b)
            dx_ = dgrad(dqkv, P.qkv_w, residual=None if dres is None else spread(dres)) if want_dx else None
            if P.lora_A is not None:
                lora_bwd(tape, P, a_in, lt, dqkv, dx_, p_lora, sl_qkv)
            return dx_

        def bwd(g):
            ride = _WGRAD_ASUM and dyd_rides(g)     # bias gradients ride on the weight-gradient GEMMs (wgrad) where they can
            if not pre_ln:
                dy, dyd = _ln_bwd_dense(tape, g, y, P.ln2_w, P.ln2_b, m2, r2, None if ride else P.fc2_b, p_hidden, s_f2)
                df = ffn_bwd(dyd, P.fc2_b if ride else None, dy)
                dt_, dtd = _ln_bwd_dense(tape, df, t, P.ln1_w, P.ln1_b, m1, r1, None if ride else P.o_b, p_hidden, s_o)
                dx = attn_bwd(dtd, P.o_b if ride else None, x.needs_grad, dt_)
                if x.needs_grad:
                    tape.add_grad(x, dx)
            else:
                gd = ops.dropout(g, p_hidden, s_f2) if p_hidden > 0 else g     # fc2's output went through hidden dropout
                df = ffn_bwd(gd, P.fc2_b, None)
                dt_, dtd = _ln_bwd_dense(tape, df, t, P.ln2_w, P.ln2_b, m2, r2, None if ride else P.o_b, p_hidden, s_o, add=g)
                da = attn_bwd(dtd, P.o_b if ride else None, True)
                if x.needs_grad:
                    tape.add_grad(x, _ln_bwd(tape, da, xd, P.ln1_w, P.ln1_b, m1, r1, add=spread(dt_)))
                else:   # LayerNorm parameters still need their gradients
                    _ln_bwd(tape, da, xd, P.ln1_w, P.ln1_b, m1, r1)
            if tape.on_params_ready:
                tape.on_params_ready(P.all())

        return out, bwd

    if policy == "block":
        out = run()[0]          # the adjoint of this pass, and with it everything it would have kept, is dropped here

        def bwd(g):
            # on the stream the adjoint runs on (an image-branch block: the side stream, inside the recorded on_side region);
            # reads x.data, which nothing has written since this block's forward (the buffer-lifetime rule)
            replayed = run()[1]
            replayed(g)
    else:
        out, bwd = run()
    o = Var(out)
    tape.adjoint(o, bwd)
    return o


def _attention_bwd(tape: Tape, spec: AttnSpec, kw: dict, dctx, qkv, ctx, lse, spread=lambda g: g):
    """ops.attention_bwd (``kw``: spec.kwargs() and the dropout site, as forward) with its bias gradients: the structural
    tables' go to their parameters, a dense bias' to ``spec.dense_bias_var``.  ``spread``: takes ``dctx`` to all rows of
    ``qkv`` (a block with keep_rows).  → dqkv"""
    extra = {}
    if spec.sp_table is not None and _DETERMINISTIC:
        return _attention_bwd_ordered(tape, spec, kw, dctx, qkv, ctx, lse, spread)
    if spec.sp_table is not None:
        extra = dict(d_sp_table=tape.pgrad(spec.sp_table),
                     d_virt=None if tape.pgrad(spec.virt) is None else tape.pgrad(spec.virt).view(-1))
    want_dense = spec.dense_bias_var is not None and spec.dense_bias_var.needs_grad
    dqkv, dbias = ops.attention_bwd(spread(dctx), qkv, ctx, lse, spec.nseq, spec.S, spec.H, **kw, want_dense_dbias=want_dense,
                                    **extra)
    if want_dense:
        tape.add_grad(spec.dense_bias_var, dbias)
    return dqkv


def _attention_bwd_ordered(tape: Tape, spec: AttnSpec, kw: dict, dctx, qkv, ctx, lse, spread):
    """Deterministic mode, structural bias: the backward stores dS densely (the whole-row kernels do, for every route a
    structural launch takes) with the table gradients switched off, and ops.attn_bias_grad_ordered reduces it in a fixed
    order.  The key-chunked long path (more than 272 tokens) is refused: its dS image is S^2 * H * 4 bytes per tree."""
    if spec.S > 272:
        raise NotImplementedError(f"deterministic mode: a structural attention bias over {spec.S} tokens takes the long path "
                                  "(S > 272), whose bias gradient exists with float atomics only")
    dqkv, dS = ops.attention_bwd(spread(dctx), qkv, ctx, lse, spec.nseq, spec.S, spec.H, **kw, want_dense_dbias=True)
    gt, gv = tape.pgrad(spec.sp_table), tape.pgrad(spec.virt)
    if gt is not None:
        ws = ordered_workspace(ops.lib.mdt_attn_bias_grad_ordered_workspace_bytes(spec.nseq, spec.H, gt.shape[0]), dS.device)
        ops.attn_bias_grad_ordered(dS, spec.spatial_pos, gt, None if gv is None else gv.view(-1), ws=ws)
    if spec.dense_bias_var is not None and spec.dense_bias_var.needs_grad:
        tape.add_grad(spec.dense_bias_var, dS)
    return dqkv


def attention_layer(tape: Tape, x: Var, qkv_w, qkv_b, o_w, o_b, spec: AttnSpec, p_attn: float = 0.0, stash: Optional[dict] = None) -> Var:
    """Bare multi-head self-attention + output projection (modules/multihead_attention.py:91-214).  ``stash``: receives
    the qkv buffer and the log-sum-exp (what the need_weights=True path recomputes the probabilities from)."""
    xd = x.data
    kw = dict(spec.kwargs(), drop_p=p_attn, drop_seed=tape.next_seed())
    qkv = ops.gemm(xd, qkv_w.data, bias=None if qkv_b is None else qkv_b.data)
    ctx, lse = ops.attention_fwd(qkv, spec.nseq, spec.S, spec.H, **kw)
    if stash is not None:
        stash.update(qkv=qkv, lse=lse, kw=spec.kwargs())
    out = ops.gemm(ctx, o_w.data, bias=None if o_b is None else o_b.data)
    o = Var(out)

    def bwd(g):
        wgrad(tape, g, ctx, o_w, o_b)
        dqkv = _attention_bwd(tape, spec, kw, ops.gemm(g, o_w.data, trans_b=True), qkv, ctx, lse)
        wgrad(tape, dqkv, xd, qkv_w, qkv_b)
        if x.needs_grad:
            tape.add_grad(x, ops.gemm(dqkv, qkv_w.data, trans_b=True))

    tape.adjoint(o, bwd)
    return o


def layernorm(tape: Tape, x: Var, w, b, eps: float) -> Var:
    y, mean, rstd = ops.layernorm_fwd(x.data, w.data, b.data, eps)
    o = Var(y)

    def bwd(g):
        dx = _ln_bwd(tape, g, x.data, w, b, mean, rstd)
        tape.add_grad(x, dx)

    tape.adjoint(o, bwd)
    return o


def dropout(tape: Tape, x: Var, p: float) -> Var:
    """Stand-alone inverted dropout (embedding / pooler dropouts); identity when p == 0."""
    if p <= 0.0:
        return x
    seed = tape.next_seed()
    o = Var(ops.dropout(x.data, p, seed))

    def bwd(g):
        tape.add_grad(x, ops.dropout(g, p, seed))

    tape.adjoint(o, bwd)
    return o


def bert_embeddings(tape: Tape, ids, types, word, pos, typ) -> Var:
    """word + position + token-type sum (HF BertEmbeddings before its LayerNorm)."""
    M, Lq = ids.shape
    D = word.shape[1]
    out = torch.empty(M * Lq, D, dtype=word.dtype, device=word.device)
    ops.bert_embed_sum(ids, types, word.data, pos.data, typ.data, out, out_seq_stride=Lq, out_off=0)
    o = Var(out)

    def bwd(g):
        gw, gp = tape.pgrad(word), tape.pgrad(pos)
        if gw is not None:
            scatter_add(gw, ids.view(-1), g, M * Lq)
        if gp is not None:
            colsum(g.view(M, Lq * D), out=gp[:Lq].view(-1))
        _type_emb_grad(tape, g, types.view(-1), typ)

    tape.adjoint(o, bwd)
    return o


def _type_emb_grad(tape: Tape, g, types, typ):
    """Token-type embedding gradient of the rows ``g`` (``types`` i32[rows], two types): row 1 gets the column sums of the
    type-1 rows, row 0 the column sums of all rows minus those."""
    gt = tape.pgrad(typ)
    if gt is None:
        return
    assert typ.shape[0] == 2, "token-type gradient is implemented for type_vocab_size == 2"
    D = g.shape[1]
    tot = colsum(g)
    one = colsum(g, row_weight=types)
    ops.row_axpby(gt, 1, d_off=1, a=one.view(1, D), accumulate=True)
    ops.row_axpby(gt, 1, d_off=0, a=tot.view(1, D), b=one.view(1, D), beta=-1.0, accumulate=True)


def _embed_rows_grads(tape: Tape, g, rows, ids, types, pos_ids, word, pos, typ):
    gw, gp = tape.pgrad(word), tape.pgrad(pos)
    if gw is not None:
        scatter_add(gw, ids, g, rows)
    if gp is not None:
        scatter_add(gp, pos_ids, g, rows)
    _type_emb_grad(tape, g, types, typ)


def bert_embeddings_rows(tape: Tape, ids, types, pos_ids, word, pos, typ) -> Var:
    """Ragged form of ``bert_embeddings``: one row per VALID token (ids / types / pos_ids i32[rows])."""
    rows = ids.numel()
    D = word.shape[1]
    out = torch.empty(rows, D, dtype=word.dtype, device=word.device)
    ops.bert_embed_rows(ids, types, pos_ids, word.data, pos.data, typ.data, out)
    o = Var(out)

    def bwd(g):
        _embed_rows_grads(tape, g, rows, ids, types, pos_ids, word, pos, typ)

    tape.adjoint(o, bwd)
    return o


def bert_embeddings_ln_rows(tape: Tape, ids, types, pos_ids, word, pos, typ, w, b, eps: float) -> Var:
    """``layernorm(bert_embeddings_rows(...))`` in one pass (ops.bert_embed_ln_rows): same bits; the summed rows are
    written out only when a backward pass will read them."""
    rows = ids.numel()
    y, mean, rstd, xs = ops.bert_embed_ln_rows(ids, types, pos_ids, word.data, pos.data, typ.data, w.data, b.data, eps,
                                               keep_sum=not tape.inference)
    o = Var(y)

    def bwd(g):
        dx = _ln_bwd(tape, g, xs, w, b, mean, rstd)
        _embed_rows_grads(tape, dx, rows, ids, types, pos_ids, word, pos, typ)

    tape.adjoint(o, bwd)
    return o


def vit_embeddings(tape: Tape, images, proj_w, proj_b, cls, pos, patch: int) -> Var:
    """Conv2d(k = s = patch) as a patch gather + one GEMM, then [CLS] and position add."""
    I = images.shape[0]
    D = proj_w.shape[0]
    g_ = images.shape[-1] // patch
    npatch = g_ * g_
    wmat = proj_w.data.view(D, -1)
    tokens = torch.empty(I * (npatch + 1), D, dtype=proj_w.dtype, device=proj_w.device)
    # One launch (the GEMM's A loader gathers from the pixels, ops.vit_patch_embed) when nothing downstream needs the gathered
    # matrix: inference, or a frozen projection (the shipped launch freezes the ViT embeddings).  A trainable projection's
    # weight gradient contracts over that matrix, so it is made once here and kept.
    fused = (PATCH_EMBED_FUSED and proj_w.dtype == torch.bfloat16 and patch == 16 and D % 128 == 0
             and (tape.inference or not (proj_w.requires_grad or proj_b.requires_grad)))
    cols = patches = None
    if fused:
        ops.vit_patch_embed(images, patch, wmat, proj_b.data, cls.data.view(-1), pos.data.view(npatch + 1, D), tokens,
                            seq_stride=npatch + 1, off=0)
    else:
        # K = C * patch^2 is 588 for ViT-L/14: zero-padded to a multiple of 128, the projection and its weight gradient run on
        # the MFMA tile kernels instead of the any-shape fp32 one (large config: 1.3 + 1.7 ms per step -> 0.4 + 0.4)
        kin = wmat.shape[1]
        kp = kin if (kin % 128 == 0 or proj_w.dtype != torch.bfloat16 or not PATCH_K_PAD) else (kin + 127) // 128 * 128
        cols = ops.vit_patchify(images, patch, proj_w.dtype, k_pad=kp)
        patches = ops.gemm(cols, _k_padded(proj_w, wmat, kp) if kp != kin else wmat, bias=proj_b.data)
        ops.vit_assemble(patches, cls.data.view(-1), pos.data.view(npatch + 1, D), tokens, I, npatch,
                         seq_stride=npatch + 1, off=0)
    o = Var(tokens)

    def bwd(g):
        gw, gb, gc, gp = tape.pgrad(proj_w), tape.pgrad(proj_b), tape.pgrad(cls), tape.pgrad(pos)
        if gw is not None or gb is not None:
            dpatch = torch.empty(I * npatch, D, dtype=g.dtype, device=g.device)
            ops.row_axpby(dpatch, I * npatch, a=g, a_inner=npatch, a_stride=npatch + 1, a_off=1)
            if gw is not None:
                kin_, kp_ = gw.view(D, -1).shape[1], cols.shape[1]
                acc = gw.view(D, -1) if kp_ == kin_ else torch.zeros(D, kp_, dtype=torch.float32, device=g.device)
                wgrad_gemm(dpatch, cols, acc)
                if kp_ != kin_:
                    gw.view(D, -1).add_(acc[:, :kin_])
            if gb is not None:
                colsum(dpatch, out=gb)
        if gp is not None:
            colsum(g.view(I, (npatch + 1) * D), out=gp.view(-1))
        if gc is not None:
            colsum(g.view(I, (npatch + 1) * D)[:, :D], out=gc.view(-1))

    tape.adjoint(o, bwd)
    return o


def expand_sequences(tape: Tape, x: Var, nseq: int, s_in: int, n_front: int, front: Optional[torch.nn.Parameter]) -> Var:
    """[nseq*s_in, D] → [nseq*(n_front+s_in), D] with ``n_front`` rows prepended to every sequence:
    the learned bottleneck tokens (``front`` = bottle_neck.weight, modules/multigraphormer_graph_encoder.py:339)
    or zeros (image sequences, whose bottleneck rows are refreshed before every fusion layer)."""
    D = x.data.shape[1]
    S = n_front + s_in
    out = torch.empty(nseq * S, D, dtype=x.data.dtype, device=x.data.device)
    ops.row_axpby(out, nseq * s_in, d_inner=s_in, d_stride=S, d_off=n_front, a=x.data)
    if front is not None:
        ops.row_axpby(out, nseq * n_front, d_inner=n_front, d_stride=S, d_off=0, a=front.data, a_inner=n_front,
                      a_stride=0, a_off=0)
    else:
        ops.row_axpby(out, nseq * n_front, d_inner=n_front, d_stride=S, d_off=0)
    o = Var(out)

    def bwd(g):
        if front is not None and tape.pgrad(front) is not None:
            colsum(g.view(nseq, S * D)[:, : n_front * D], out=tape.pgrad(front).view(-1))
        if x.needs_grad:
            dx = torch.empty_like(x.data)
            ops.row_axpby(dx, nseq * s_in, a=g, a_inner=s_in, a_stride=S, a_off=n_front)
            tape.add_grad(x, dx)

    tape.adjoint(o, bwd)
    return o


def expand_rows(tape: Tape, x: Var, rows_out: int, body_idx, front_idx, n_front: int, front: torch.nn.Parameter) -> Var:
    """Index-driven ``expand_sequences`` for the text side (padded or ragged layout alike): row r of ``x`` goes to
    row ``body_idx[r]`` of the [rows_out, D] result, and row ``front_idx[k]`` receives learned bottleneck token
    ``k % n_front`` (modules/multigraphormer_graph_encoder.py:339)."""
    D = x.data.shape[1]
    rows_in = x.data.shape[0]
    nfront = front_idx.numel()
    assert rows_in + nfront == rows_out, "expand_rows: body and front rows must tile the output exactly"
    out = torch.empty(rows_out, D, dtype=x.data.dtype, device=x.data.device)
    ops.row_axpby(out, rows_in, di=body_idx, a=x.data)
    ops.row_axpby(out, nfront, di=front_idx, a=front.data, a_inner=n_front, a_stride=0, a_off=0)
    o = Var(out)

    def bwd(g):
        gf = tape.pgrad(front)
        if gf is not None:
            fr = torch.empty(nfront, D, dtype=g.dtype, device=g.device)
            ops.row_axpby(fr, nfront, a=g, ai=front_idx)
            colsum(fr.view(nfront // n_front, n_front * D), out=gf.view(-1))
        if x.needs_grad:
            dx = torch.empty_like(x.data)
            ops.row_axpby(dx, rows_in, a=g, ai=body_idx)
            tape.add_grad(x, dx)

    tape.adjoint(o, bwd)
    return o


def rows_mix(tape: Tape, dst: Var, src: Var, nrows: int, *, alpha: float, beta: float, d_idx=None, d_map=(1, 1, 0),
             s_idx=None, s_map=(1, 1, 0)) -> Var:
    """In place: dst[dr] = alpha * src[sr] + beta * dst[dr] for ``nrows`` row pairs.
    alpha=1, beta=0 is the reference's ``dst[index] = src[index2]`` assignment; alpha=beta=0.5 the
    image/text bottleneck average (modules/multi_graphormer_fusion_layer.py:63-66).
    Adjoint (also in place on the gradient buffers): g_src[sr] += alpha * g_dst[dr]; g_dst[dr] *= beta."""
    di, ds_, do = d_map
    si, ss, so = s_map
    ops.row_axpby(dst.data, nrows, di=d_idx, d_inner=di, d_stride=ds_, d_off=do,
                  a=src.data, ai=s_idx, a_inner=si, a_stride=ss, a_off=so, alpha=alpha,
                  b=dst.data if beta != 0.0 else None, bi=d_idx, b_inner=di, b_stride=ds_, b_off=do, beta=beta)

    def bwd(g):
        if src.needs_grad:
            gs = tape.grad_buf(src)
            ops.row_axpby(gs, nrows, di=s_idx, d_inner=si, d_stride=ss, d_off=so,
                          a=g, ai=d_idx, a_inner=di, a_stride=ds_, a_off=do, alpha=alpha, accumulate=True)
        ops.row_axpby(g, nrows, di=d_idx, d_inner=di, d_stride=ds_, d_off=do,
                      a=g if beta != 0.0 else None, ai=d_idx, a_inner=di, a_stride=ds_, a_off=do, alpha=beta)

    tape.adjoint(dst, bwd, take=False)      # in place: dst's gradient stays where it is, for the ops before this one
    return dst


def graph_node_features(tape: Tape, text: Var, text_row_of_node, in_degree, out_degree, in_emb, out_emb, graph_token,
                        B: int, T: int, src_rows_of_comment, graph_rows_of_comment, M: int, in_scatter_idx,
                        out_scatter_idx) -> Var:
    """modules/graphormer_layers.py:39-50 fused with the masked scatter that builds graph_data
    (modules/multigraphormer_graph_encoder.py:363-371): node n of tree b reads bottleneck token 0
    of its comment (row ``text_row_of_node``, -1 = padding node → zeros), both add the degree
    embeddings.  ``*_scatter_idx`` i32[B*T]: embedding row that graph row r feeds in backward,
    -1 for the graph token and for padding_idx (degree 0) rows."""
    x = ops.graph_node_feature(text.data, text_row_of_node, in_degree, out_degree, in_emb.data, out_emb.data,
                               graph_token.data.view(-1), B, T)
    o = Var(x)
    D = x.shape[1]

    def bwd(g):
        if text.needs_grad:
            gt = tape.grad_buf(text)
            ops.row_axpby(gt, M, di=src_rows_of_comment, a=g, ai=graph_rows_of_comment, accumulate=True)
        gi, go, gk = tape.pgrad(in_emb), tape.pgrad(out_emb), tape.pgrad(graph_token)
        if gi is not None:
            scatter_add(gi, in_scatter_idx, g, B * T)
        if go is not None:
            scatter_add(go, out_scatter_idx, g, B * T)
        if gk is not None:
            colsum(g.view(B, T * D)[:, :D], out=gk.view(-1))

    tape.adjoint(o, bwd)
    return o


def classifier_head(tape: Tape, text: Var, M: int, cls_rows, bn0_rows, pool_w, pool_b, cls_w, cls_b, p_drop: float = 0.0) -> Var:
    """models/multi_modal_discussion_transformer.py:265-274: the SAME pooler (dense + tanh on
    token 0) and classifier are applied to the text sequence ([CLS], row nb of each comment)
    and to the bottleneck sequence (bottleneck token 0, row 0); logits are their mean.
    ``cls_rows`` / ``bn0_rows``: i32[M] rows of [CLS] / bottleneck token 0 of every comment in ``text``."""
    D = text.data.shape[1]
    rows = torch.empty(2 * M, D, dtype=text.data.dtype, device=text.data.device)
    ops.row_axpby(rows, M, d_off=0, a=text.data, ai=cls_rows)
    ops.row_axpby(rows, M, d_off=M, a=text.data, ai=bn0_rows)
    pre = ops.gemm(rows, pool_w.data, bias=pool_b.data)
    pooled = ops.tanh_fwd(pre)
    seed = tape.next_seed()
    pooled_d = ops.dropout(pooled, p_drop, seed) if p_drop > 0 else pooled   # text_dropout, independent masks per branch
    l2 = ops.gemm(pooled_d, cls_w.data, bias=cls_b.data)                     # [2M, C]
    C = l2.shape[1]
    logits = torch.empty(M, C, dtype=l2.dtype, device=l2.device)
    ops.row_axpby(logits, M, a=l2, alpha=0.5, b=l2, b_off=M, beta=0.5)
    o = Var(logits)

    def bwd(g):
        dl2 = torch.empty_like(l2)
        ops.row_axpby(dl2, M, d_off=0, a=g, alpha=0.5)
        ops.row_axpby(dl2, M, d_off=M, a=g, alpha=0.5)
        wgrad(tape, dl2, pooled_d, cls_w, cls_b)
        dpooled = ops.gemm(dl2, cls_w.data, trans_b=True)
        if p_drop > 0:
            dpooled = ops.dropout(dpooled, p_drop, seed)
        dpre = ops.tanh_bwd(pooled, dpooled)
        wgrad(tape, dpre, rows, pool_w, pool_b)
        if text.needs_grad:
            drows = ops.gemm(dpre, pool_w.data, trans_b=True)
            gt = tape.grad_buf(text)
            ops.row_axpby(gt, M, di=cls_rows, a=drows, a_off=0, accumulate=True)
            ops.row_axpby(gt, M, di=bn0_rows, a=drows, a_off=M, accumulate=True)
        if tape.on_params_ready:
            tape.on_params_ready([pool_w, pool_b, cls_w, cls_b])

    tape.adjoint(o, bwd)
    return o


def take_rows(tape: Tape, src: Var, nrows: int, s_map=(1, 1, 0), s_idx=None) -> Var:
    """out[r] = src[row(r)] (e.g. the global embedding = graph-token row of every tree)."""
    si, ss, so = s_map
    out = torch.empty(nrows, src.data.shape[1], dtype=src.data.dtype, device=src.data.device)
    ops.row_axpby(out, nrows, a=src.data, ai=s_idx, a_inner=si, a_stride=ss, a_off=so)
    o = Var(out)

    def bwd(g):
        if not src.needs_grad:
            return
        gs = tape.grad_buf(src)
        ops.row_axpby(gs, nrows, di=s_idx, d_inner=si, d_stride=ss, d_off=so, a=g, accumulate=True)

    tape.adjoint(o, bwd)
    return o


def scatter_rows(tape: Tape, src: Var, rows_out: int, d_idx, s_idx) -> Var:
    """out = zeros[rows_out, D]; out[d_idx[r]] = src[s_idx[r]] (ragged rows back into the reference's padded shape)."""
    n = d_idx.numel()
    out = torch.zeros(rows_out, src.data.shape[1], dtype=src.data.dtype, device=src.data.device)
    ops.row_axpby(out, n, di=d_idx, a=src.data, ai=s_idx)
    o = Var(out)

    def bwd(g):
        if not src.needs_grad:
            return
        gs = tape.grad_buf(src)
        ops.row_axpby(gs, n, di=s_idx, a=g, ai=d_idx, accumulate=True)

    tape.adjoint(o, bwd)
    return o


# ------------------------------------------------------------------------------------------
# autograd bridge
class TapeFunction(torch.autograd.Function):
    """One autograd node around a whole tape.

    ``TapeFunction.apply(run, use_main_grad, hook, inference, n_in, *tensors)`` where ``tensors`` are the
    ``n_in`` differentiable tensor inputs followed by every parameter the tape may touch;
    ``run(tape, *input_vars) -> tuple[Var]``."""

    @staticmethod
    def forward(ctx, run, use_main_grad, hook, inference, n_in, *tensors):
        ctx.set_materialize_grads(False)
        tape = Tape(use_main_grad=use_main_grad, on_params_ready=hook, inference=inference)
        ins = [Var(t, needs_grad=t.requires_grad) for t in tensors[:n_in]]
        try:
            outs = run(tape, *ins)
        finally:
            tape._leave_side()
        tape.sync_streams()
        if inference and F8.ACTIVE is not None:
            F8.ACTIVE.end_of_step()      # no backward will close this pass: its |x| maxima become the next scales here (and are reset)
        ctx.tape, ctx.ins, ctx.outs = tape, ins, outs
        ctx.params = tensors[n_in:]
        ctx.n_in = n_in
        return tuple(o.data for o in outs)

    @staticmethod
    def backward(ctx, *gouts):
        tape = ctx.tape
        for o, g in zip(ctx.outs, gouts):
            if g is not None:
                g = g.contiguous()
                o.grad = g if o.grad is None else o.grad + g
        tape.backward()
        gin = [v.grad if v.needs_grad else None for v in ctx.ins]
        if tape.use_main_grad:
            gp = [None] * len(ctx.params)
        else:
            gp = []
            for p in ctx.params:
                g = tape.tmp_grads.get(id(p))
                gp.append(None if g is None else (g if p.dtype == torch.float32 else ops.cast(g, p.dtype)))
        ctx.tape = ctx.ins = ctx.outs = None
        return (None, None, None, None, None, *gin, *gp)


def run_tape(run, inputs: Sequence[torch.Tensor], params: Sequence[torch.nn.Parameter], *, use_main_grad=False, hook=None):
    """Execute ``run`` under the autograd bridge; returns a tuple of output tensors."""
    probe = inputs[0] if len(inputs) else params[0]
    if not probe.is_cuda:
        raise RuntimeError("the mDT HIP path has no CPU fallback: move the module and its inputs to the GPU")
    # grad mode is read HERE: inside Function.forward it is always off
    inference = not torch.is_grad_enabled()
    return TapeFunction.apply(run, use_main_grad, hook, inference, len(inputs), *inputs, *params)
