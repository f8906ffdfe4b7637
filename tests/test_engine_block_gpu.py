"""engine.transformer_block and engine.attention_layer on a bare Tape, launch by launch (multimodaldiscussiontransformer_amd/engine.py).

A recorder wraps every ``ops`` entry point the block calls.  The real kernels run; after a synchronise it keeps host copies of
what each launch read, what it wrote, what the buffers it accumulates into held before, and its scalar keywords.  The run —
launches, inputs, parameters, the tape's four site seeds, output, dx and the gradient buffers — is a *trace*, and three layers
of checks are pure functions of a trace (host tensors only: tests/test_engine_block_reference_cpu.py runs them on a torch model
of the block and on its mutants):

  (a) ``check_launches``   every launch against the fp64 reference of its kernel family, from the operands it read: the
                           per-element bounds of tests/gemm_reference.py, layernorm_reference.py, attention_reference.py,
                           activation_reference.py, rowops_reference.py.  No error compounds through the block.
  (b) ``check_wiring``     every launch has a role (which parameter it reads or writes, its transposition flags, forward or
                           backward); the roles a configuration must launch are written down here from the documented structure
                           of the block (``expected_roles``), each occurs once and nothing else runs.  Then bit equality:
                           every consumer reads its producer's output, every backward launch of a dropout site carries the
                           forward's (p, seed), the seeds are the tape's first four, every parameter's gradient buffer is the
                           output of the launch that owns it — each bias gradient has ONE owner, the one the switches
                           prescribe — and on_params_ready fires once, with all twelve buffers final.
  (c) ``check_end_to_end`` y, dx, the twelve parameter gradients and the bias-source gradients against the fp64 autograd
                           restatement of tests/block_reference.py on the stored operands.  fp32: 1e-3 max(1, max|ref|) per
                           tensor (tests/test_activation_gpu.py check_layer_fp32); bf16: relative L2 per tensor within
                           bf16_gate(shape) (below).  This layer is the wiring gate; precision is carried by (a).

Shapes.  S: 3 sequences of 20 tokens, D 128, 2 heads of 64, F 192, batch-major, the last 5 keys of sequence 1 masked.
S-ragged: lengths (20, 7, 13).  G: 3 trees of 9 nodes, D 64, 4 heads of 16, F 96, time-major rows, the structural bias
(attn_bias in {0, -inf}, spatial_pos, an 8-row table, virt, key_pad on the last two nodes of tree 2).  R: bf16, D 128, 2 heads,
F 192 at 64 x 128 = 8192 padded rows and at 63 x 128 + 127 = 8191 ragged rows, the two sides of engine.dyd_rides' threshold.
Dropout "on": p_hidden 0.25, p_attn 0.25, p_act 0.5.  Inputs and cotangents differ from row to row; the cotangent carries a
per-column offset of varying sign and size (at the R shapes x does too), so that no column sum of a gradient cancels (a
cancelling sum of 8192 fp32 terms has a bound that says nothing; the CPU companion shows that every cap — median bound / |ref|
<= 2^-7 — holds for the reference alone at these operands).  One case freezes the four dense biases.
fp8 GEMMs are out of scope: every run asserts fp8.ACTIVE is None."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

import tests.activation_reference as ACT
import tests.attention_reference as AR
import tests.block_reference as BR
import tests.gemm_reference as GR
import tests.layernorm_reference as LR
import tests.rowops_reference as RR
from tests.rowops_reference import bf16, f32
from tests.test_engine_embeddings_gpu import check_dropout, check_total
from tests.test_real_shapes_gpu import BF16_GRAD_REL_L2

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 97531
GOLDEN = 0x9E3779B97F4A7C15
M63 = 0x7FFFFFFFFFFFFFFF
P_ON = dict(p_hidden=0.25, p_attn=0.25, p_act=0.5)
P_OFF = dict(p_hidden=0.0, p_attn=0.0, p_act=0.0)
WEIGHTS = ("qkv", "o", "fc1", "fc2")
WORST = {}                       # launch kind -> worst err / bound over the session
CASE_WORST = {}                  # the same for the trace being checked (reset by check_trace)

# bf16, layer (c): relative L2 per tensor against the fp64 restatement on the bf16-stored operands.  The limit is 4 x the largest
# value the CPU torch model of tests/test_engine_block_reference_cpu.py (bf16 rounding at every store the kernels make, fp32
# arithmetic, the dropout masks of the CPU ports) reaches against the same restatement at the same shapes — the model reproduces
# neither the kernels' summation order nor the bf16 probabilities inside the attention kernels — and never more than
# BF16_GRAD_REL_L2.  Measured with dropout on (test_model_is_accepted prints and re-asserts them; worst tensor of each trace):
#   S  (60 rows, D 128, F 192)    post-LN 3.9e-3 (dx), pre-LN 5.1e-3 (ln1_w); keep_rows + q_limit 5.2e-3 (qkv_w) / 5.8e-3 (dx);
#                                 ragged (40 rows) pre-LN 4.9e-3 (dx); pre-filled main_grad 3.9e-3 (dx)
#   G  (27 rows, D 64, F 96)      relu, structural bias: post-LN 3.7e-3 (dx), pre-LN 2.0e-2 (sp_table; fc1_w 1.8e-2: relu kinks)
#   R  (8192 / 8191 rows, D 128)  post-LN 3.8e-3 (dx), pre-LN 4.0e-3 (dx)
# The kernels on an MI355X, same cases: S at most 6.1e-3 (ln1_w, pre-LN with keep_rows), G post-LN 3.9e-3 (dx), R at most 4.0e-3 (dx).
BF16_E2E_MEASURED = {"S": 5.9e-3, "G": 2.0e-2, "R": 4.0e-3}


def bf16_gate(shape):
    return min(4.0 * BF16_E2E_MEASURED[shape[0]], BF16_GRAD_REL_L2)


SHAPES = {
    "S": dict(nseq=3, S=20, D=128, H=2, F=192, eps=1e-12),
    "Sr": dict(nseq=3, S=20, D=128, H=2, F=192, eps=1e-12, lens=(20, 7, 13)),
    "G": dict(nseq=3, S=9, D=64, H=4, F=96, eps=1e-5, time_major=True, struct=True),
    "R8192": dict(nseq=64, S=128, D=128, H=2, F=192, eps=1e-12),
    "R8191": dict(nseq=64, S=128, D=128, H=2, F=192, eps=1e-12, lens=(128,) * 63 + (127,)),
}


@pytest.fixture(scope="module")
def E():
    from multimodaldiscussiontransformer_amd import engine
    assert torch.cuda.is_available(), "GPU tests need a device"
    return engine


@pytest.fixture(scope="module")
def ops():
    from multimodaldiscussiontransformer_amd import ops as o
    return o


@pytest.fixture
def restore_mode(E):
    was = E.deterministic()
    yield
    E.set_deterministic(was)


def dev(t):
    return t.to(DEV).contiguous()


def host(t):
    return None if t is None else t.detach().cpu().clone()


# ------------------------------------------------------------------------------------------------ the cases (CPU; shared with the CPU companion)
def make_case(shape, dtype, pre_ln, *, drop=True, keep=False, act="gelu", x_needs_grad=True, main_grad=False, deterministic=False,
              inference=False, ln_bias_ride=True, wgrad_asum=True, frozen=(), torch_seed=4321):
    """Host operands and settings of one run of the block: everything but the device."""
    g = SHAPES[shape]
    nseq, S, D, H, F = g["nseq"], g["S"], g["D"], g["H"], g["F"]
    lens = g.get("lens")
    rows = sum(lens) if lens else nseq * S
    spec = dict(nseq=nseq, S=S, H=H, seq_stride=None, pos_stride=1, q_limit=0)
    if lens:
        off = torch.zeros(nseq + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(torch.tensor(lens), 0)
        spec["seq_offsets"] = off
    elif g.get("time_major"):
        spec.update(seq_stride=1, pos_stride=nseq)
    if shape == "S":
        km = torch.ones(nseq, S, dtype=torch.uint8)
        km[1, S - 5:] = 0
        spec["key_mask"] = km
    s = SEED + 1000 * sorted(SHAPES).index(shape)
    w = lambda shp, k, scale: RR.values(shp, s + k, scale, dtype)                   # noqa: E731
    ln_w = lambda k: (1.0 + 0.5 * RR.values((D,), s + k, 1.0, f32)).to(dtype)         # noqa: E731
    params = dict(qkv_w=w((3 * D, D), 1, 1.5 * GR.b_scale(D)), qkv_b=w((3 * D,), 2, 0.6), o_w=w((D, D), 3, 1.5 * GR.b_scale(D)),
                  o_b=w((D,), 4, 0.6), ln1_w=ln_w(5), ln1_b=w((D,), 6, 0.6), fc1_w=w((F, D), 7, 1.5 * GR.b_scale(D)), fc1_b=w((F,), 8, 0.6),
                  fc2_w=w((D, F), 9, 1.5 * GR.b_scale(F)), fc2_b=w((D,), 10, 0.6), ln2_w=ln_w(11), ln2_b=w((D,), 12, 0.6))
    if g.get("struct"):
        gen = torch.Generator().manual_seed(s + 20)
        ab = torch.zeros(nseq, S, S)
        cut = torch.rand(nseq, S - 1, S - 1, generator=gen) < 0.15
        cut &= ~torch.eye(S - 1, dtype=torch.bool)[None]                           # every node keeps itself and the graph token
        ab[:, 1:, 1:][cut] = float("-inf")
        kp = torch.zeros(nseq, S, dtype=torch.uint8)
        kp[2, S - 2:] = 1
        spec.update(attn_bias=ab, spatial_pos=torch.randint(0, 8, (nseq, S - 1, S - 1), generator=gen, dtype=torch.int32), key_pad=kp)
        params.update(sp_table=w((8, H), 21, 1.0), virt=w((1, H), 22, 1.0))
    keep_rows = None
    if keep:
        assert not lens and not g.get("time_major")
        keep_rows = torch.tensor([2 * S + 4, 0, S + 4, 2 * S, 4, S], dtype=torch.int64)    # tokens 0 and 4 of every sequence, not monotone
        spec["q_limit"] = 5
    rows_out = rows if keep_rows is None else int(keep_rows.numel())
    # per-column offsets of varying sign and size in the cotangent: no column sum of the adjoint is a cancelling sum.  The 8192-row
    # shapes carry them in x too: Σ_rows dy xh of the pre-LN LayerNorm 1 needs a column mean in both factors to stay clear of the cap
    def offsets(k):
        o = RR.values((D,), s + k, 1.0, f32)
        return (torch.sign(o) * (0.35 + 0.65 * o.abs()))[None]

    cot = (0.5 * RR.values((rows_out, D), s + 32, 1.0, f32) + offsets(31)).to(dtype)
    x = (RR.values((rows, D), s + 30, 1.5, f32) + offsets(33)).to(dtype) if shape[0] == "R" else w((rows, D), 30, 2.0)
    p = P_ON if drop else P_OFF
    cfg = dict(shape=shape, dtype=dtype, pre_ln=pre_ln, eps=g["eps"], act=act, keep_rows=keep_rows, spec=spec, rows=rows, rows_out=rows_out, D=D, F=F,
               x=x, cot=cot, params=params, x_needs_grad=x_needs_grad, main_grad=main_grad, deterministic=deterministic,
               inference=inference, ln_bias_ride=ln_bias_ride, wgrad_asum=wgrad_asum, frozen=tuple(frozen), torch_seed=torch_seed, lens=lens, **p)
    cfg["grads0"] = {n: (RR.values(tuple(t.shape), s + 40 + i, 2.0, f32) if main_grad else torch.zeros(t.shape)) for i, (n, t) in enumerate(params.items())}
    return cfg


def tape_seeds(base, n=4):
    """What Tape.next_seed hands out: base + golden * counter, 63 bits."""
    return [(base + GOLDEN * i) & M63 for i in range(1, n + 1)]


def split_k(n_out, k_out, red):
    """engine._split_k restated: the slabs a weight-gradient GEMM over ``red`` rows is cut into."""
    tiles = ((n_out + 127) // 128) * ((k_out + 127) // 128)
    return max(1, min(max(1, 1024 // max(1, tiles)), red // 1024 if red >= 1024 else 1))


# ------------------------------------------------------------------------------------------------ the recorder
class BlockRecorder:
    """Wraps the ops the block calls; ``launches`` receives one dict per launch (host copies, scalars as they were passed)."""
    OPS = ("gemm", "gemm_splitk_ordered", "attention_fwd", "attention_bwd", "attn_bias_grad_ordered", "layernorm_fwd", "layernorm_bwd",
           "layernorm_bwd_ordered", "act_fwd", "dropout", "row_axpby", "colsum", "colsum_ordered")

    def __init__(self, ops, mp):
        self.launches = []
        for name in self.OPS:
            mp.setattr(ops, name, getattr(self, "_" + name)(getattr(ops, name)))

    def _add(self, op, **fields):
        torch.cuda.synchronize()
        self.launches.append(dict(op=op, **{k: (host(v) if torch.is_tensor(v) else v) for k, v in fields.items()}))

    def _gemm(self, real):
        def gemm(a, b, **kw):
            assert not (set(kw) - {"trans_a", "trans_b", "out", "bias", "residual", "aux", "epilogue", "split_k", "drop_p", "drop_seed", "colsum", "asum"}), kw.keys()
            before = {k + "0": host(kw.get(k)) for k in ("out", "aux", "colsum", "asum")}
            out = real(a, b, **kw)
            self._add("gemm", a=a, b=b, out=out, c_old=before["out0"], aux0=before["aux0"], aux=kw.get("aux"), colsum0=before["colsum0"],
                      colsum=kw.get("colsum"), asum0=before["asum0"], asum=kw.get("asum"), bias=kw.get("bias"), residual=kw.get("residual"),
                      trans_a=bool(kw.get("trans_a", False)), trans_b=bool(kw.get("trans_b", False)), epilogue=int(kw.get("epilogue", 0)),
                      split_k=int(kw.get("split_k", 1)), drop_p=float(kw.get("drop_p", 0.0)), drop_seed=int(kw.get("drop_seed", 0)))
            return out
        return gemm

    def _gemm_splitk_ordered(self, real):
        def gemm_splitk_ordered(a, b, out, *, trans_a=False, trans_b=False, split_k=1, ws=None):
            c_old = host(out)
            r = real(a, b, out, trans_a=trans_a, trans_b=trans_b, split_k=split_k, ws=ws)
            self._add("gemm_splitk_ordered", a=a, b=b, out=out, c_old=c_old, trans_a=bool(trans_a), trans_b=bool(trans_b), split_k=int(split_k))
            return r
        return gemm_splitk_ordered

    @staticmethod
    def _attn_kw(kw):
        bins = kw.get("bins")
        return dict({k: v for k, v in kw.items() if k not in ("bins", "d_sp_table", "d_virt")},
                    bins=None if bins is None else [(host(i), int(c)) for i, c in bins])

    def _attention_fwd(self, real):
        def attention_fwd(qkv, nseq, S, H, **kw):
            out, lse = real(qkv, nseq, S, H, **kw)
            self._add("attention_fwd", qkv=qkv, nseq=nseq, S=S, H=H, out=out, lse=lse, **self._attn_kw(kw))
            return out, lse
        return attention_fwd

    def _attention_bwd(self, real):
        def attention_bwd(dout, qkv, out, lse, nseq, S, H, **kw):
            t0, v0 = host(kw.get("d_sp_table")), host(kw.get("d_virt"))
            dqkv, dbias = real(dout, qkv, out, lse, nseq, S, H, **kw)
            self._add("attention_bwd", dout=dout, qkv=qkv, out=out, lse=lse, nseq=nseq, S=S, H=H, dqkv=dqkv, dbias=dbias, d_sp_table0=t0,
                      d_sp_table=kw.get("d_sp_table"), d_virt0=v0, d_virt=kw.get("d_virt"), **self._attn_kw(kw))
            return dqkv, dbias
        return attention_bwd

    def _attn_bias_grad_ordered(self, real):
        def attn_bias_grad_ordered(dS, spatial_pos, d_sp_table=None, d_virt=None, ws=None):
            t0, v0 = host(d_sp_table), host(d_virt)
            r = real(dS, spatial_pos, d_sp_table, d_virt, ws=ws)
            self._add("attn_bias_grad_ordered", dS=dS, spatial_pos=spatial_pos, d_sp_table0=t0, d_sp_table=d_sp_table, d_virt0=v0, d_virt=d_virt)
            return r
        return attn_bias_grad_ordered

    def _layernorm_fwd(self, real):
        def layernorm_fwd(x, gamma, beta, eps, out=None, q8=None):
            assert out is None and q8 is None, "the fp8 producer is out of scope here"
            y, mean, rstd = real(x, gamma, beta, eps)
            self._add("layernorm_fwd", x=x, gamma=gamma, beta=beta, eps=float(eps), y=y, mean=mean, rstd=rstd)
            return y, mean, rstd
        return layernorm_fwd

    def _ln_bwd(self, real, op):
        def layernorm_bwd(dy, x, gamma, mean, rstd, **kw):
            assert not (set(kw) - {"add", "dgamma", "dbeta", "drop_p", "drop_seed", "colsum", "want_dropped", "ws"}), kw.keys()
            before = {k: host(kw.get(k)) for k in ("dgamma", "dbeta", "colsum")}
            r = real(dy, x, gamma, mean, rstd, **kw)
            dx, dxd = r if kw.get("want_dropped") else (r, None)
            self._add(op, dy=dy, x=x, gamma=gamma, mean=mean, rstd=rstd, add=kw.get("add"), dgamma0=before["dgamma"], dgamma=kw.get("dgamma"),
                      dbeta0=before["dbeta"], dbeta=kw.get("dbeta"), colsum0=before["colsum"], colsum=kw.get("colsum"), dx=dx, dxd=None if dxd is dx else dxd,
                      drop_p=float(kw.get("drop_p", 0.0)), drop_seed=int(kw.get("drop_seed", 0)), want_dropped=bool(kw.get("want_dropped", False)))
            return r
        return layernorm_bwd

    def _layernorm_bwd(self, real):
        return self._ln_bwd(real, "layernorm_bwd")

    def _layernorm_bwd_ordered(self, real):
        return self._ln_bwd(real, "layernorm_bwd_ordered")

    def _act_fwd(self, real):
        def act_fwd(pre, kind, *, drop_p=0.0, drop_seed=0, want_u=True, out=None, u=None):
            pre0 = host(pre)
            h, uu = real(pre, kind, drop_p=drop_p, drop_seed=drop_seed, want_u=want_u, out=out, u=u)
            self._add("act_fwd", pre=pre0, kind=kind, drop_p=float(drop_p), drop_seed=int(drop_seed), want_u=bool(want_u), h=h, u=uu)
            return h, uu
        return act_fwd

    def _dropout(self, real):
        def dropout(x, p, seed, out=None):
            assert out is None
            y = real(x, p, seed)
            self._add("dropout", x=x, p=float(p), seed=int(seed), out=y)
            return y
        return dropout

    def _row_axpby(self, real):
        def row_axpby(dst, nrows, **kw):
            assert not (set(kw) - {"di", "a", "ai", "accumulate"}), f"the block moves whole rows by index only: {sorted(kw)}"
            dst0 = host(dst)
            r = real(dst, nrows, **kw)
            self._add("row_axpby", dst0=dst0, dst=dst, nrows=int(nrows), di=kw.get("di"), a=kw.get("a"), ai=kw.get("ai"), accumulate=bool(kw.get("accumulate", False)))
            return r
        return row_axpby

    def _colsum_any(self, real, op):
        def colsum(x, out=None, row_weight=None, **kw):
            assert row_weight is None and out is not None
            out0 = host(out)
            r = real(x, out=out, row_weight=row_weight, **kw)
            self._add(op, x=x, out0=out0, out=out)
            return r
        return colsum

    def _colsum(self, real):
        return self._colsum_any(real, "colsum")

    def _colsum_ordered(self, real):
        return self._colsum_any(real, "colsum_ordered")


# ------------------------------------------------------------------------------------------------ running the block
@contextlib.contextmanager
def switches(E, mp, cfg):
    was = E.deterministic()
    mp.setattr(E, "_LN_BIAS_RIDE", cfg["ln_bias_ride"])
    mp.setattr(E, "_WGRAD_ASUM", cfg["wgrad_asum"])
    E.set_deterministic(cfg["deterministic"])
    try:
        yield
    finally:
        E.set_deterministic(was)


def device_spec(E, cfg, P, dense_var=None):
    sp = cfg["spec"]
    u8 = lambda t: None if t is None else dev(t)                                                 # noqa: E731
    bins = None
    if cfg["lens"]:                       # the encoder's default length bins (data/packer.py RaggedText.length_bins), where they cut anything
        from multimodaldiscussiontransformer_amd.data.packer import RaggedText
        lens = torch.tensor(cfg["lens"])
        order = torch.argsort(lens, stable=True)
        rt = SimpleNamespace(order=dev(order.to(torch.int32)), sorted_lens=lens[order].numpy(), max_len=int(lens.max()))
        bins = RaggedText.length_bins(rt, 0)
    return E.AttnSpec(nseq=sp["nseq"], S=sp["S"], H=sp["H"], seq_stride=sp["seq_stride"], pos_stride=sp["pos_stride"], key_mask=u8(sp.get("key_mask")),
                      dense_bias=None if sp.get("dense_bias") is None else dev(sp["dense_bias"]), dense_bias_var=dense_var,
                      attn_bias=None if sp.get("attn_bias") is None else dev(sp["attn_bias"]),
                      spatial_pos=None if sp.get("spatial_pos") is None else dev(sp["spatial_pos"]), sp_table=P.get("sp_table"), virt=P.get("virt"),
                      key_pad=u8(sp.get("key_pad")), seq_offsets=None if sp.get("seq_offsets") is None else dev(sp["seq_offsets"]), q_limit=sp["q_limit"], bins=bins)


def run_block(E, ops, monkeypatch, cfg):
    """One forward (+ backward) of engine.transformer_block under the recorder → the trace."""
    from multimodaldiscussiontransformer_amd import fp8 as F8
    assert F8.ACTIVE is None, "fp8 GEMMs inside the block are out of scope: these cases run with fp8.ACTIVE None"
    P = {n: torch.nn.Parameter(dev(t), requires_grad=n not in cfg["frozen"]) for n, t in cfg["params"].items()}
    if cfg["main_grad"]:
        for n, p in P.items():
            p.main_grad = dev(cfg["grads0"][n])
    BP = E.BlockParams(**{n: P[n] for n in BR.PARAMS})
    hook = []

    def buf(n):
        return P[n].main_grad if cfg["main_grad"] else tape.tmp_grads.get(id(P[n]))

    def on_ready(params):
        torch.cuda.synchronize()
        hook.append(dict(all_params=len(params) == 12 and all(a is b for a, b in zip(params, BP.all())), snap={n: host(buf(n)) for n in BR.PARAMS}))

    with monkeypatch.context() as mp, switches(E, mp, cfg):
        rec = BlockRecorder(ops, mp)
        tape = E.Tape(use_main_grad=cfg["main_grad"], on_params_ready=on_ready, inference=cfg["inference"])
        torch.manual_seed(cfg["torch_seed"])
        xv = E.Var(dev(cfg["x"]), needs_grad=cfg["x_needs_grad"])
        keep = None if cfg["keep_rows"] is None else dev(cfg["keep_rows"].to(torch.int32))
        o = E.transformer_block(tape, xv, BP, device_spec(E, cfg, P), pre_ln=cfg["pre_ln"], eps=cfg["eps"], p_hidden=cfg["p_hidden"],
                                p_attn=cfg["p_attn"], p_act=cfg["p_act"], keep_rows=keep, act=cfg["act"])
        assert tape._seed_ctr == 4, "the block takes exactly four site seeds"
        atomics = None
        if cfg["inference"]:
            assert tape.ops == [] and tape.tmp_grads == {}
        else:
            o.grad = dev(cfg["cot"])
            before = ops.float_atomic_launches()
            tape.backward()
            atomics = ops.float_atomic_launches() - before
        torch.cuda.synchronize()
        assert F8.ACTIVE is None
    torch.manual_seed(cfg["torch_seed"])
    assert tape._seed_base == int(torch.randint(0, 2 ** 62, (1,)).item()), "the tape's seed base does not follow torch.manual_seed"
    grads = {} if cfg["inference"] else {n: host(buf(n)) for n in P}
    return dict(cfg=cfg, launches=rec.launches, tape_seeds=tape_seeds(tape._seed_base), y=host(o.data), dx=host(xv.grad), grads=grads, hook=hook,
                atomics=atomics)


# ------------------------------------------------------------------------------------------------ (a) every launch against its own reference
@contextlib.contextmanager
def captured(worst, kind):
    """Runs a reference module's check with its WORST dict emptied, files what it noted under ``kind`` and puts the dict back."""
    saved = dict(worst)
    worst.clear()
    try:
        yield
    finally:
        for v in worst.values():
            note(kind, v)
        for k, v in saved.items():
            worst[k] = max(worst.get(k, 0.0), v)


def note(kind, ratio):
    r = ratio if ratio == ratio else float("inf")
    for d in (WORST, CASE_WORST):
        d[kind] = max(d.get(kind, 0.0), r)


def ratio(got, v, d, dt):
    fin = torch.isfinite(v)
    r = torch.where(fin, (got.double() - v).abs() / GR.bound(v, d, dt).clamp(min=1e-300), torch.zeros_like(v))
    return float(r.max()) if r.numel() else 0.0


def check_gemm(r, what):
    ordered = r["op"] == "gemm_splitk_ordered"
    ep = GR.EPI_ATOMIC if ordered else r["epilogue"]
    got, aux = {"out": r["out"]}, None
    if not ordered:
        ep |= (GR.EPI_BIAS if r["bias"] is not None else 0) | (GR.EPI_RESIDUAL if r["residual"] is not None else 0) | (GR.EPI_DROPOUT if r["drop_p"] > 0 else 0)
        ep |= (GR.EPI_COLSUM if r["colsum"] is not None else 0) | (GR.EPI_ASUM if r["asum"] is not None else 0)
        if ep & GR.EPI_AUX_GRAD:
            aux, got["aux"] = r["aux"], r["aux"]
        elif ep & GR.EPI_MULAUX:
            aux = r["aux0"]
        if r["colsum"] is not None:
            got["colsum"] = r["colsum"]
        if r["asum"] is not None:
            got["asum"] = r["asum"]
    g = lambda k: None if ordered else r[k]                                                  # noqa: E731
    sum0 = g("colsum0") if g("colsum0") is not None else g("asum0")
    ref = GR.reference(r["a"], r["b"], trans_a=r["trans_a"], trans_b=r["trans_b"], epilogue=ep, bias=g("bias"), residual=g("residual"), aux=aux,
                       c_old=r["c_old"], colsum0=sum0, drop_p=0.0 if ordered else r["drop_p"], drop_seed=0 if ordered else r["drop_seed"], split_k=r["split_k"])
    dts = {"out": r["out"].dtype, "aux": r["a"].dtype, "colsum": f32, "asum": f32}
    for k, t in got.items():
        note(r["op"] + (" sum" if k in ("colsum", "asum") else ""), ratio(t, *ref[k], dts[k]))
    GR.check(got, ref, dts, what=what)


def check_layernorm_fwd(r, what):
    dt = r["x"].dtype
    with captured(LR.WORST, "layernorm_fwd"):
        LR.check({"y": r["y"], "mean": r["mean"], "rstd": r["rstd"]}, LR.reference_fwd(r["x"], r["gamma"], r["beta"], r["eps"]), {"y": dt, "mean": f32, "rstd": f32}, what=what)


def check_layernorm_bwd(r, what):
    dt = r["x"].dtype
    dropped = r["want_dropped"] and r["drop_p"] > 0
    assert (r["dxd"] is not None) == dropped, f"{what}: a dropped copy exactly when a mask is asked for"
    ref = LR.reference_bwd(r["dy"], r["x"], r["gamma"], r["mean"], r["rstd"], add=r["add"], drop_p=r["drop_p"], drop_seed=r["drop_seed"], dgamma0=r["dgamma0"],
                           dbeta0=r["dbeta0"], colsum0=r["colsum0"], want_dropped=dropped, want_colsum=r["colsum"] is not None, dx_stored=r["dx"], dxd_stored=r["dxd"])
    got = {k: r[k] for k in ("dx", "dxd", "dgamma", "dbeta", "colsum") if r[k] is not None}
    with captured(LR.WORST, r["op"]):
        LR.check(got, ref, {"dx": dt, "dxd": dt}, what=what)


def attn_operands(r):
    m, lens = BR.row_map(r["nseq"], r["S"], r.get("seq_stride"), r.get("pos_stride", 1), r.get("seq_offsets"))
    assert int(m.max()) < r["qkv"].shape[0], "attention: the launch geometry addresses rows past the buffer"
    hd = r["qkv"].shape[1] // 3 // r["H"]
    kw = dict(key_mask=r.get("key_mask"), key_pad=r.get("key_pad"), dense_bias=r.get("dense_bias"), attn_bias=r.get("attn_bias"), spatial_pos=r.get("spatial_pos"),
              sp_table=r.get("sp_table"), virt=r.get("virt"), drop_p=r.get("drop_p", 0.0), drop_seed=r.get("drop_seed", 0), lens=None if lens is None else lens.tolist(),
              q_limit=r.get("q_limit", 0))
    return m, r.get("scale") or hd ** -0.5, kw


def check_attention(r, what):
    """Forward or backward launch: the strides are undone on the host, rows outside ``valid`` are not compared."""
    dt = r["qkv"].dtype
    m, scale, kw = attn_operands(r)
    bwd = r["op"] == "attention_bwd"
    qkv = BR.to_logical(r["qkv"], m)
    dout = BR.to_logical(r["dout"], m) if bwd else torch.zeros(qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3, dtype=dt)
    ref = AR.reference(qkv, dout, r["H"], scale, dt, want_bwd=bwd, **kw)
    if not bwd:
        got = {"out": BR.to_logical(r["out"], m), "lse": r["lse"]}
    else:
        got = {"dqkv": BR.to_logical(r["dqkv"], m)}
        if r["dbias"] is not None:
            got["dbias"] = r["dbias"]
        for k in ("d_sp_table", "d_virt"):
            if r[k] is not None:
                assert float(r[k + "0"].abs().max()) == 0.0, f"{what}: {k} is accumulated onto a fresh buffer in every case of this file"
                got[k] = r[k].view(ref[k][0].shape)
        if r.get("q_limit", 0):
            D = r["qkv"].shape[1] // 3
            past = got["dqkv"][:, r["q_limit"]:, :D]
            assert int((past != 0).sum()) == 0, f"{what}: dQ of the rows past q_limit is not exactly zero"
    for k, v in AR.check(got, ref, dt, what=what).items():
        note(r["op"] + (" bias grad" if k in ("d_sp_table", "d_virt") else ""), v)


def check_bias_grad_ordered(r, what):
    """d_sp_table / d_virt += the bins of the stored dS (exact fp32 terms) summed in any order."""
    dS = r["dS"].double()
    nseq, H, S, _ = dS.shape
    ns = r["d_sp_table"].shape[0]
    idx = r["spatial_pos"].long().reshape(-1)
    pick = dS[:, :, 1:, 1:].permute(0, 2, 3, 1).reshape(-1, H)
    tab = r["d_sp_table0"].double().index_add(0, idx, pick)
    mag = r["d_sp_table0"].double().abs().index_add(0, idx, pick.abs())
    cnt = torch.zeros(ns, dtype=torch.float64).index_add(0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    d = GR._gamma(cnt + 1)[:, None] * mag
    tab[0], d[0] = r["d_sp_table0"].double()[0], 0.0
    RR.check("attn_bias_grad_ordered", r["d_sp_table"], (tab, d, d == 0), what=what + " d_sp_table", dtype=f32, nonvacuous=True)
    note("attn_bias_grad_ordered", ratio(r["d_sp_table"], tab, d, f32))
    if r["d_virt"] is not None:
        edge = torch.cat([dS[:, :, 0, :], dS[:, :, 1:, 0]], 2).permute(0, 2, 1).reshape(-1, H)
        check_total("attn_bias_grad_ordered", r["d_virt"], r["d_virt0"], edge, what + " d_virt")


def check_act_fwd(r, what):
    ref = ACT.reference(r["kind"], r["pre"], r["drop_p"], r["drop_seed"])
    note("act_fwd", ACT.compare(r["h"], ref["h"], what=what + " h"))
    assert (r["u"] is not None) == r["want_u"], f"{what}: u is stored exactly when the backward will read it"
    if r["u"] is not None:
        note("act_fwd", ACT.compare(r["u"], ref["u"], what=what + " u"))


def check_row_axpby(r, what):
    m = lambda i: (None if i is None else i.long(), 1, 1, 0)                             # noqa: E731
    ref = RR.reference_row_axpby(r["dst0"], r["nrows"], d=m(r["di"]), a=r["a"], am=m(r["ai"]), accumulate=r["accumulate"])
    if not r["accumulate"]:
        assert bool(ref[2].all()), f"{what}: a row copy is bit-determined"
    with captured(RR.WORST, "row_axpby"):
        RR.check("row_axpby", r["dst"], ref, what=what)


def check_launch(r, what):
    op = r["op"]
    if op in ("gemm", "gemm_splitk_ordered"):
        check_gemm(r, what)
    elif op == "layernorm_fwd":
        check_layernorm_fwd(r, what)
    elif op in ("layernorm_bwd", "layernorm_bwd_ordered"):
        check_layernorm_bwd(r, what)
    elif op in ("attention_fwd", "attention_bwd"):
        check_attention(r, what)
    elif op == "attn_bias_grad_ordered":
        with captured(RR.WORST, op):
            check_bias_grad_ordered(r, what)
    elif op == "act_fwd":
        check_act_fwd(r, what)
    elif op == "dropout":
        with captured(RR.WORST, "dropout"):
            check_dropout("dropout", r["out"], r["x"], r["p"], r["seed"], what)
    elif op == "row_axpby":
        check_row_axpby(r, what)
    elif op in ("colsum", "colsum_ordered"):
        with captured(RR.WORST, op):
            check_total(op, r["out"], r["out0"], r["x"].double(), what)
    else:
        raise AssertionError(f"{what}: no reference for a launch of {op}")


def check_launches(trace, roles=None):
    """Layer (a).  → the number of launches verified."""
    names = {id(r): k for k, r in (roles or {}).items()}
    for i, r in enumerate(trace["launches"]):
        check_launch(r, f"[launch {i}: {names.get(id(r), r['op'])}]")
    return len(trace["launches"])


# ------------------------------------------------------------------------------------------------ (b) roles and wiring
def bits(a, b):
    """Same shape, type and bits (a NaN equals itself: rows a kernel leaves unspecified are compared as stored)."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = {2: torch.int16, 4: torch.int32, 1: torch.uint8, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def classify(trace):
    """{role: launch}.  The role follows from which parameter a launch reads (or, for a gradient, writes), its transposition flags
    and forward / backward; a second launch of a role, or a launch without one, is an error."""
    P = trace["cfg"]["params"]
    roles, late = {}, []

    def put(role, r):
        assert role not in roles, f"role {role} launched twice"
        roles[role] = r

    def weight(t, by_shape=False):
        hit = [n for n in WEIGHTS if n + "_w" in P and (tuple(t.shape) == tuple(P[n + "_w"].shape) if by_shape else bits(t, P[n + "_w"]))]
        assert len(hit) == 1, f"a GEMM operand [{tuple(t.shape)}] is {'no' if not hit else 'more than one'} weight of the block"
        return hit[0]

    for r in trace["launches"]:
        op = r["op"]
        if op in ("gemm", "gemm_splitk_ordered"):
            if r["trans_a"] and r["trans_b"]:
                put("wgrad_" + weight(r["out"], by_shape=True), r)
            elif r["trans_b"]:
                put("dgrad_" + weight(r["b"]), r)
            else:
                assert not r["trans_a"]
                put("fwd_" + weight(r["b"]), r)
        elif op == "layernorm_fwd":
            put(("ln1" if bits(r["gamma"], P["ln1_w"]) else "ln2" if bits(r["gamma"], P["ln2_w"]) else "ln?") + "_fwd", r)
        elif op in ("layernorm_bwd", "layernorm_bwd_ordered"):
            put(("ln1" if bits(r["gamma"], P["ln1_w"]) else "ln2" if bits(r["gamma"], P["ln2_w"]) else "ln?") + "_bwd", r)
        elif op in ("attention_fwd", "attention_bwd"):
            put("attn_" + op[-3:], r)
        elif op == "attn_bias_grad_ordered":
            put("bias_grad", r)
        elif op == "act_fwd":
            put("act_fwd", r)
        elif op == "dropout":
            put("drop_g", r)
        elif op in ("colsum", "colsum_ordered"):
            hit = [n for n in WEIGHTS if n + "_b" in P and r["out"].numel() == P[n + "_b"].numel()]
            if "fc2" in hit and "o" in hit:       # both D wide: inside a block o_b is never a column-sum launch (a LayerNorm backward sits behind it)
                hit.remove("o")
            assert len(hit) == 1, f"a column sum of {r['out'].numel()} columns belongs to no bias of the block"
            put(f"colsum_{hit[0]}_b", r)
        else:
            late.append(r)
    for r in late:
        assert r["op"] == "row_axpby" and not r["accumulate"], f"unexpected launch {r['op']}"
        if r["ai"] is not None:
            put("gather_x" if bits(r["a"], trace["cfg"]["x"]) else "gather_ctx", r)
        else:
            assert r["di"] is not None
            put("spread_dctx" if "dgrad_o" in roles and bits(r["a"], roles["dgrad_o"]["out"]) else "spread_dt", r)
    return roles


def attn_ln(cfg):
    """The LayerNorm whose backward carries the output projection's dropout mask and bias sum: it normalises t."""
    return "ln2" if cfg["pre_ln"] else "ln1"


def expected_roles(cfg):
    """({role: op}, {bias: (role, field)}) a configuration must launch, from the documented structure of the block: QKV, attention,
    output projection, two LayerNorms, fc1 (+ a separate activation unless erf-GELU), fc2 forward; the mirrored adjoint with two
    GEMMs per dense layer.  Bias gradients: o_b / fc2_b ride on their weight-gradient GEMM (asum) where engine.dyd_rides says so —
    bf16, at least 8192 gradient rows, both switches on, not deterministic — else they are column sums of the LayerNorm backward
    behind them (pre-LN fc2 has none behind it: asum in bf16 with _WGRAD_ASUM, else a column-sum launch, as for qkv_b); fc1_b is
    the column sum in fc2's input-gradient GEMM, in deterministic mode an ordered column sum of the stored du."""
    det, bf, pre = cfg["deterministic"], cfg["dtype"] == bf16, cfg["pre_ln"]
    keep = cfg["keep_rows"] is not None
    R = {"fwd_" + n: "gemm" for n in WEIGHTS}
    R.update(attn_fwd="attention_fwd", ln1_fwd="layernorm_fwd", ln2_fwd="layernorm_fwd")
    if cfg["act"] != "gelu":
        R["act_fwd"] = "act_fwd"
    if keep:
        R.update(gather_ctx="row_axpby", gather_x="row_axpby")
    if cfg["inference"]:
        return R, {}
    lnb, cs = ("layernorm_bwd_ordered", "colsum_ordered") if det else ("layernorm_bwd", "colsum")
    R.update({"wgrad_" + n: "gemm_splitk_ordered" if det else "gemm" for n in WEIGHTS})
    R.update(dgrad_fc2="gemm", dgrad_fc1="gemm", dgrad_o="gemm", attn_bwd="attention_bwd", ln1_bwd=lnb, ln2_bwd=lnb)
    if pre or cfg["x_needs_grad"]:
        R["dgrad_qkv"] = "gemm"
    if pre and cfg["p_hidden"] > 0:
        R["drop_g"] = "dropout"
    if keep:
        R["spread_dctx"] = "row_axpby"
        if cfg["x_needs_grad"]:
            R["spread_dt"] = "row_axpby"
    if det and cfg["spec"].get("attn_bias") is not None:
        R["bias_grad"] = "attn_bias_grad_ordered"
    asum = bf and cfg["wgrad_asum"] and not det
    rides = asum and cfg["ln_bias_ride"] and cfg["rows_out"] >= 8192
    own = {"o_b": ("wgrad_o", "asum") if rides else (attn_ln(cfg) + "_bwd", "colsum"), "qkv_b": ("wgrad_qkv", "asum") if asum else ("colsum_qkv_b", "out"),
           "fc1_b": ("colsum_fc1_b", "out") if det else ("dgrad_fc2", "colsum")}
    if pre:
        own["fc2_b"] = ("wgrad_fc2", "asum") if asum else ("colsum_fc2_b", "out")
    else:
        own["fc2_b"] = ("wgrad_fc2", "asum") if rides else ("ln2_bwd", "colsum")
    own = {n: o for n, o in own.items() if n not in cfg["frozen"]}          # a frozen bias: no owner, no launch of its own
    for role, _ in own.values():
        if role.startswith("colsum_"):
            R[role] = cs
    return R, own


BEFORE = {"out": "c_old", "asum": "asum0", "colsum": "colsum0", "dgamma": "dgamma0", "dbeta": "dbeta0"}


def check_wiring(trace):
    """Layer (b).  → {role: launch}."""
    cfg, P, seeds = trace["cfg"], trace["cfg"]["params"], trace["tape_seeds"]
    pre, keep = cfg["pre_ln"], cfg["keep_rows"]
    want, own = expected_roles(cfg)
    roles = classify(trace)
    assert {k: r["op"] for k, r in roles.items()} == want, (f"roles launched differ from the block's structure: missing {sorted(set(want) - set(roles))}, "
                                                            f"unexpected {sorted(set(roles) - set(want))}, other entry point "
                                                            f"{sorted(k for k in set(want) & set(roles) if roles[k]['op'] != want[k])}")
    L = SimpleNamespace(**roles)

    def eq(a, b, what):
        assert bits(a, b), f"wiring: {what}"

    # ---- seeds: the tape's first four, pairwise distinct, one per site, forward and backward alike
    assert len(set(seeds)) == 4, "wiring: the four site seeds are not pairwise distinct"
    s_attn, s_o, s_act, s_f2 = seeds
    x, g = cfg["x"], cfg["cot"]
    # ---- forward
    ln_a, ln_f = ("ln1_fwd", "ln2_fwd") if pre else (None, "ln1_fwd")
    a_in = x
    if pre:
        eq(L.ln1_fwd["x"], x, "pre-LN: LayerNorm 1 does not read x")
        a_in = L.ln1_fwd["y"]
    eq(L.fwd_qkv["a"], a_in, "the QKV projection does not read " + ("LayerNorm 1's output" if pre else "x"))
    eq(L.fwd_qkv["bias"], P["qkv_b"], "QKV bias")
    eq(L.attn_fwd["qkv"], L.fwd_qkv["out"], "attention does not read the QKV projection's output")
    assert (L.attn_fwd["drop_p"], L.attn_fwd["drop_seed"]) == (cfg["p_attn"], s_attn), "wiring: attention forward (p, seed) is not the first site's"
    sp = cfg["spec"]
    for k in ("seq_stride", "pos_stride", "q_limit"):
        assert L.attn_fwd.get(k) == sp.get(k), f"wiring: attention {k}"
    for k in ("key_mask", "key_pad", "attn_bias", "spatial_pos", "seq_offsets", "dense_bias"):
        eq(L.attn_fwd.get(k), sp.get(k), f"attention {k} is not the spec's")
    if sp.get("attn_bias") is not None:
        eq(L.attn_fwd["sp_table"], P["sp_table"], "attention sp_table")
        eq(L.attn_fwd["virt"], P["virt"].view(-1), "attention virt")
    ctx_full = L.attn_fwd["out"]
    ctx_k, x_k = ctx_full, x
    if keep is not None:
        for role, src, name in (("gather_ctx", ctx_full, "ctx"), ("gather_x", x, "x")):
            r = roles[role]
            eq(r["a"], src, f"gather({name}) does not read {name}")
            assert r["di"] is None and torch.equal(r["ai"].long(), keep), f"wiring: gather({name}) does not index with keep_rows"
            eq(r["dst"], src[keep], f"gather({name}) is not {name}[keep_rows]")
        ctx_k, x_k = L.gather_ctx["dst"], L.gather_x["dst"]
    eq(L.fwd_o["a"], ctx_k, "the output projection does not read the (gathered) context")
    eq(L.fwd_o["residual"], x_k, "the output projection's residual is not gather(x)")
    eq(L.fwd_o["bias"], P["o_b"], "output projection bias")
    assert (L.fwd_o["drop_p"], L.fwd_o["drop_seed"]) == (cfg["p_hidden"], s_o), "wiring: output projection (p, seed) is not the second site's"
    t = L.fwd_o["out"]
    eq(roles[ln_f]["x"], t, f"{ln_f} does not read t, the attention half's output")
    f_in = roles[ln_f]["y"]
    eq(L.fwd_fc1["a"], f_in, "fc1 does not read f_in")
    eq(L.fwd_fc1["bias"], P["fc1_b"], "fc1 bias")
    if cfg["act"] == "gelu":
        assert L.fwd_fc1["epilogue"] == GR.EPI_GELU | GR.EPI_AUX_GRAD, "wiring: fc1's epilogue is not GELU | AUX_GRAD"
        assert (L.fwd_fc1["drop_p"], L.fwd_fc1["drop_seed"]) == (cfg["p_act"], s_act), "wiring: fc1 (p, seed) is not the third site's"
        h, u = L.fwd_fc1["out"], L.fwd_fc1["aux"]
    else:
        assert L.fwd_fc1["epilogue"] == 0 and L.fwd_fc1["drop_p"] == 0.0 and L.fwd_fc1["aux"] is None, "wiring: fc1 is not a plain bias GEMM"
        eq(L.act_fwd["pre"], L.fwd_fc1["out"], "act_fwd does not read fc1's pre-activation")
        assert (L.act_fwd["kind"], L.act_fwd["drop_p"], L.act_fwd["drop_seed"]) == (cfg["act"], cfg["p_act"], s_act), "wiring: act_fwd (kind, p, seed)"
        assert L.act_fwd["want_u"] == (not cfg["inference"])
        h, u = L.act_fwd["h"], L.act_fwd["u"]
    eq(L.fwd_fc2["a"], h, "fc2 does not read fc1's h")
    eq(L.fwd_fc2["residual"], t if pre else f_in, "fc2's residual is not " + ("t" if pre else "f_in"))
    eq(L.fwd_fc2["bias"], P["fc2_b"], "fc2 bias")
    assert (L.fwd_fc2["drop_p"], L.fwd_fc2["drop_seed"]) == (cfg["p_hidden"], s_f2), "wiring: fc2 (p, seed) is not the fourth site's"
    if pre:
        eq(trace["y"], L.fwd_fc2["out"], "the block's output is not fc2's")
    else:
        eq(L.ln2_fwd["x"], L.fwd_fc2["out"], "LayerNorm 2 does not read fc2's output")
        eq(trace["y"], L.ln2_fwd["y"], "the block's output is not LayerNorm 2's")
    if cfg["inference"]:
        assert trace["hook"] == [] and trace["grads"] == {} and trace["dx"] is None
        return roles
    # ---- backward
    def ln_bwd(role, dy, xin, fwd, add, p, seed, what):
        r = roles[role]
        eq(r["dy"], dy, f"{what}: dy")
        eq(r["x"], xin, f"{what}: x is not what the forward normalised")
        eq(r["mean"], roles[fwd]["mean"], f"{what}: mean")
        eq(r["rstd"], roles[fwd]["rstd"], f"{what}: rstd")
        eq(r["add"], add, f"{what}: the residual gradient (add)")
        if p is not None:
            assert r["want_dropped"] and (r["drop_p"], r["drop_seed"]) == (p, seed), f"wiring: {what}: (p, seed) of the tail is not the forward site's"
        else:
            assert not r["want_dropped"] and r["drop_p"] == 0.0 and r["colsum"] is None, f"wiring: {what}: a plain LayerNorm backward has no tail"
        return r["dx"], (r["dx"] if r["dxd"] is None else r["dxd"])

    if pre:
        gd = g
        if cfg["p_hidden"] > 0:
            eq(L.drop_g["x"], g, "pre-LN: dropout(g) does not read the upstream gradient")
            assert (L.drop_g["p"], L.drop_g["seed"]) == (cfg["p_hidden"], s_f2), "wiring: pre-LN dropout(g) (p, seed) is not fc2's site"
            gd = L.drop_g["out"]
        dres = None
    else:
        dres, gd = ln_bwd("ln2_bwd", g, L.fwd_fc2["out"], "ln2_fwd", None, cfg["p_hidden"], s_f2, "LayerNorm 2 backward")
    eq(L.wgrad_fc2["a"], gd, "the fc2 weight gradient does not read fc2's output gradient behind the dropout mask")
    eq(L.wgrad_fc2["b"], h, "the fc2 weight gradient does not read h")
    eq(L.dgrad_fc2["a"], gd, "fc2's input gradient does not read gd")
    assert L.dgrad_fc2["epilogue"] == GR.EPI_MULAUX, "wiring: fc2's input gradient is not a MULAUX GEMM"
    eq(L.dgrad_fc2["aux0"], u, "the MULAUX aux is not the u the forward stored")
    du = L.dgrad_fc2["out"]
    eq(L.wgrad_fc1["a"], du, "the fc1 weight gradient does not read du")
    eq(L.wgrad_fc1["b"], f_in, "the fc1 weight gradient does not read f_in")
    eq(L.dgrad_fc1["a"], du, "fc1's input gradient does not read du")
    eq(L.dgrad_fc1["residual"], dres, "fc1's input gradient: the residual gradient (post-LN: LayerNorm 2's dx; pre-LN: none)")
    df = L.dgrad_fc1["out"]
    dt_, dtd = ln_bwd(attn_ln(cfg) + "_bwd", df, t, attn_ln(cfg) + "_fwd", g if pre else None, cfg["p_hidden"], s_o, "the LayerNorm backward over t")
    eq(L.wgrad_o["a"], dtd, "the o weight gradient does not read dtd, the gradient behind the dropout mask")
    eq(L.wgrad_o["b"], ctx_k, "the o weight gradient does not read the (gathered) context")
    eq(L.dgrad_o["a"], dtd, "the context gradient does not read dtd")
    assert L.dgrad_o["epilogue"] == 0 and L.dgrad_o["residual"] is None
    dctx = L.dgrad_o["out"]

    def spread(role, src, what):
        if keep is None:
            return src
        r = roles[role]
        eq(r["a"], src, f"spread({what}) does not read {what}")
        assert r["ai"] is None and torch.equal(r["di"].long(), keep), f"wiring: spread({what}) does not index with keep_rows"
        assert float(r["dst0"].float().abs().max()) == 0.0 and r["dst"].shape[0] == cfg["rows"], f"wiring: spread({what}) does not start from zero rows of x"
        eq(r["dst"], torch.zeros_like(r["dst"]).index_copy(0, keep, src), f"spread({what}) is not zero except {what} at keep_rows")
        return r["dst"]

    eq(L.attn_bwd["dout"], spread("spread_dctx", dctx, "dctx"), "attention backward does not read the (spread) context gradient")
    eq(L.attn_bwd["qkv"], L.fwd_qkv["out"], "attention backward does not read the forward's qkv")
    eq(L.attn_bwd["out"], ctx_full, "attention backward does not read the forward's full-row ctx")
    eq(L.attn_bwd["lse"], L.attn_fwd["lse"], "attention backward does not read the forward's lse")
    for k in ("drop_p", "drop_seed", "seq_stride", "pos_stride", "q_limit", "scale"):
        assert L.attn_bwd.get(k) == L.attn_fwd.get(k), f"wiring: attention backward {k} differs from the forward's"
    for k in ("key_mask", "key_pad", "attn_bias", "spatial_pos", "seq_offsets", "dense_bias", "sp_table", "virt"):
        eq(L.attn_bwd.get(k), L.attn_fwd.get(k), f"attention backward {k} differs from the forward's")
    assert L.attn_fwd.get("bins") is None and L.attn_bwd.get("bins") is None, "wiring: no ragged set of this file is long enough for the encoder's length bins to cut"
    dqkv = L.attn_bwd["dqkv"]
    eq(L.wgrad_qkv["a"], dqkv, "the qkv weight gradient does not read dqkv")
    eq(L.wgrad_qkv["b"], a_in, "the qkv weight gradient does not read a_in" + (" (LayerNorm 1's output, not x)" if pre else ""))
    for n in WEIGHTS:
        r = roles["wgrad_" + n]
        assert r["split_k"] == split_k(r["out"].shape[0], r["out"].shape[1], r["a"].shape[0]), f"wiring: split_k of the {n} weight gradient"
    dx = None
    if "dgrad_qkv" in roles:
        eq(L.dgrad_qkv["a"], dqkv, "the input gradient does not read dqkv")
        want_res = spread("spread_dt", dt_, "dt") if (not pre and cfg["x_needs_grad"]) else None
        eq(L.dgrad_qkv["residual"], want_res, "the input gradient's residual (post-LN: the spread dt; pre-LN: none)")
        dx = L.dgrad_qkv["out"]
    if pre:
        add = spread("spread_dt", dt_, "dt") if cfg["x_needs_grad"] else None
        dx, _ = ln_bwd("ln1_bwd", dx, x, "ln1_fwd", add, None, None, "LayerNorm 1 backward")
    if cfg["x_needs_grad"]:
        eq(trace["dx"], dx, "x.grad is not the block's last input gradient")
    else:
        assert trace["dx"] is None, "wiring: x needs no gradient and got one"
    # ---- gradient buffers: every parameter's buffer is the output of the ONE launch that owns it, which started from the buffer's content
    owners = {n + "_w": ("wgrad_" + n, "out") for n in WEIGHTS}
    owners.update(ln1_w=("ln1_bwd", "dgamma"), ln1_b=("ln1_bwd", "dbeta"), ln2_w=("ln2_bwd", "dgamma"), ln2_b=("ln2_bwd", "dbeta"), **own)
    writers = {n: [] for n in ("qkv_b", "o_b", "fc1_b", "fc2_b")}
    for n in WEIGHTS:
        if roles["wgrad_" + n].get("asum") is not None:
            writers[n + "_b"].append(("wgrad_" + n, "asum"))
        if f"colsum_{n}_b" in roles:
            writers[n + "_b"].append((f"colsum_{n}_b", "out"))
    if L.dgrad_fc2["colsum"] is not None:
        writers["fc1_b"].append(("dgrad_fc2", "colsum"))
    for role, bias in ((attn_ln(cfg) + "_bwd", "o_b"), ("ln2_bwd", None if pre else "fc2_b")):
        if roles[role]["colsum"] is not None and bias is not None:
            writers[bias].append((role, "colsum"))
    if pre:
        assert L.ln1_bwd["colsum"] is None
    assert all(n.endswith("_b") and n[:-2] in WEIGHTS for n in cfg["frozen"]), "this file freezes dense biases only"
    for n, w in writers.items():
        if n in cfg["frozen"]:
            assert not w and trace["grads"][n] is None, f"wiring: the frozen {n} has a gradient buffer or a launch that writes one ({w})"
            continue
        assert len(w) == 1, f"wiring: the gradient of {n} has {len(w)} owners ({w}): never both, never neither"
        assert w[0] == own[n], f"wiring: the gradient of {n} is owned by {w[0]}, the switches prescribe {own[n]}"
    for n, (role, field) in owners.items():
        eq(roles[role]["out0" if role.startswith("colsum_") else BEFORE[field]], cfg["grads0"][n].view(roles[role][field].shape), f"the launch that owns the gradient of {n} did not start from the buffer's content")
        eq(trace["grads"][n], roles[role][field].view(trace["grads"][n].shape), f"the gradient buffer of {n} is not the output of {role}.{field}")
    # ---- the hook: once, with P.all(), every buffer final
    assert len(trace["hook"]) == 1, f"hook: on_params_ready was called {len(trace['hook'])} times"
    assert trace["hook"][0]["all_params"], "hook: on_params_ready was not called with P.all()"
    for n in BR.PARAMS:
        eq(trace["hook"][0]["snap"][n], trace["grads"][n], f"hook: the gradient of {n} changed after on_params_ready")
    return roles


# ------------------------------------------------------------------------------------------------ (c) end to end
def e2e_rows(trace, ref):
    """[(tensor, error, gate)]: fp32 max |Δ| against 1e-3 max(1, max|ref|); bf16 relative L2 against bf16_gate(shape), the key bias
    relative to what is summed."""
    cfg = trace["cfg"]
    D = cfg["D"]
    pairs = [("y", trace["y"], ref["y"], 0.0)]
    if not cfg["inference"]:
        if cfg.get("x_needs_grad", True):
            pairs.append(("dx", trace["dx"], ref["dx"], 0.0))
        for n, r in ref["grads"].items():
            if n in cfg.get("frozen", ()):
                continue
            got = trace["grads"][n].double().view(r.shape) - cfg["grads0"][n].double().view(r.shape)
            if n == "qkv_b":
                pairs += [("qkv_b." + k, got[i * D:(i + 1) * D], r[i * D:(i + 1) * D], ref["summed"].get("qkv_b." + k, 0.0)) for i, k in enumerate("qkv")]
            else:
                pairs.append((n, got, r, 0.0))
    rows = []
    for name, got, r, floor in pairs:
        assert got is not None and tuple(got.shape) == tuple(r.shape), f"end to end: {name} is missing or has another shape"
        if cfg["dtype"] == f32:
            rows.append((name, float((got.double() - r).abs().max()), 1e-3 * max(1.0, float(r.abs().max()))))
        else:
            rows.append((name, BR.rel_l2(got, r, floor), bf16_gate(cfg["shape"])))
    return rows


def block_reference(trace):
    cfg = trace["cfg"]
    return BR.reference(cfg["x"], cfg["params"], cfg["cot"], cfg, trace["tape_seeds"])


def check_end_to_end(trace, ref=None, tag=""):
    """Layer (c).  → the rows, worst first."""
    rows = e2e_rows(trace, ref or block_reference(trace))
    rows.sort(key=lambda r: -r[1] / r[2])
    print(f"[{tag}] end to end, {len(rows)} tensors, worst error / gate: " + "; ".join(f"{n} {e:.3e} / {g:.1e}" for n, e, g in rows[:3]))
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, f"end to end: {bad}"
    return rows


def check_trace(trace, tag):
    """All three layers; every launch recorded has a role and was verified against its reference."""
    CASE_WORST.clear()
    roles = check_wiring(trace)
    n = check_launches(trace, roles)
    assert n == len(trace["launches"]) == len(roles), f"{tag}: {len(trace['launches'])} launches recorded, {len(roles)} with a role, {n} verified"
    print(f"\n[{tag}] {n} launches verified; worst err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(CASE_WORST.items())))
    check_end_to_end(trace, tag=tag)
    return roles


# ------------------------------------------------------------------------------------------------ the cases
def tag_of(cfg):
    return f"{cfg['shape']} {'bf16' if cfg['dtype'] == bf16 else 'fp32'} {'pre' if cfg['pre_ln'] else 'post'}-LN"


DT = pytest.mark.parametrize("dtype", (f32, bf16), ids=("fp32", "bf16"))
PLACE = pytest.mark.parametrize("pre_ln", (False, True), ids=("post", "pre"))


@PLACE
@DT
@pytest.mark.parametrize("drop", (False, True), ids=("nodrop", "drop"))
def test_block_base_wiring_and_dropout_sites(E, ops, monkeypatch, dtype, pre_ln, drop):
    """Cases 1-8, shape S: the base wiring with dropout off, the four sites and their backward counterparts with dropout on."""
    cfg = make_case("S", dtype, pre_ln, drop=drop)
    check_trace(run_block(E, ops, monkeypatch, cfg), tag_of(cfg) + (" dropout" if drop else ""))


@PLACE
def test_block_keep_rows_with_q_limit(E, ops, monkeypatch, pre_ln):
    """Cases 9-10: the pruned last fusion layer — six kept rows in a non-monotone order, q_limit 5, dropout on: gather, spread, the
    compact dropout counters of the R-row GEMMs, dQ exactly zero past the limit."""
    cfg = make_case("S", bf16, pre_ln, keep=True)
    roles = check_trace(run_block(E, ops, monkeypatch, cfg), tag_of(cfg) + " keep_rows")
    assert roles["fwd_o"]["out"].shape[0] == 6 and roles["attn_bwd"]["q_limit"] == 5


def test_block_input_without_gradient_pre_ln(E, ops, monkeypatch):
    """Case 11: x.needs_grad False in a pre-LN block — no dx, LayerNorm 1 still gets its parameter gradients."""
    cfg = make_case("S", f32, True, x_needs_grad=False)
    trace = run_block(E, ops, monkeypatch, cfg)
    roles = check_trace(trace, tag_of(cfg) + " x frozen")
    assert trace["dx"] is None and roles["ln1_bwd"]["add"] is None and float(trace["grads"]["ln1_w"].abs().max()) > 0


def test_block_with_frozen_biases(E, ops, monkeypatch):
    """The four dense biases frozen: none gets a buffer, a column sum inside another launch or a launch of its own; the rest is unchanged."""
    cfg = make_case("S", f32, False, frozen=("qkv_b", "o_b", "fc1_b", "fc2_b"))
    trace = run_block(E, ops, monkeypatch, cfg)
    roles = check_trace(trace, tag_of(cfg) + " biases frozen")
    assert all(trace["grads"][n] is None for n in cfg["frozen"]) and roles["dgrad_fc2"]["colsum"] is None and "colsum_qkv_b" not in roles


def test_block_accumulates_into_main_grad(E, ops, monkeypatch):
    """Case 12: use_main_grad with pre-filled buffers — every owner starts from the buffer's content, the hook sees final values."""
    cfg = make_case("S", bf16, False, main_grad=True)
    check_trace(run_block(E, ops, monkeypatch, cfg), tag_of(cfg) + " main_grad")


@PLACE
def test_block_ragged_launch(E, ops, monkeypatch, pre_ln):
    """Cases 13-14: lengths (20, 7, 13) through seq_offsets, dropout on."""
    cfg = make_case("Sr", bf16, pre_ln)
    check_trace(run_block(E, ops, monkeypatch, cfg), tag_of(cfg) + " ragged")


@DT
def test_block_structural_bias_relu_time_major(E, ops, monkeypatch, dtype):
    """Cases 15-16, shape G: structural bias with table gradients, time-major rows, dropout on, act = relu — the separate act_fwd
    launch, whose u carries the activation-dropout scale."""
    cfg = make_case("G", dtype, False, act="relu")
    trace = run_block(E, ops, monkeypatch, cfg)
    roles = check_trace(trace, tag_of(cfg) + " relu")
    u = roles["act_fwd"]["u"].float()
    assert set(u.unique().tolist()) == {0.0, 2.0}, "u of relu at p_act = 0.5 is 0 or the dropout scale 2"
    assert float(trace["grads"]["sp_table"][0].abs().max()) == 0.0 and float(trace["grads"]["sp_table"][1:].abs().max()) > 0


def test_block_on_an_inference_tape(E, ops, monkeypatch):
    """Case 17: G, pre-LN, inference tape — want_u False, nothing recorded on the tape, the output of the training tape."""
    train = run_block(E, ops, monkeypatch, make_case("G", f32, True, act="relu"))
    cfg = make_case("G", f32, True, act="relu", inference=True)
    infer = run_block(E, ops, monkeypatch, cfg)
    roles = check_trace(infer, tag_of(cfg) + " inference")
    assert roles["act_fwd"]["u"] is None and bits(infer["y"], train["y"]), "the inference tape's output differs from the training tape's"


@pytest.mark.parametrize("shape", ("S", "G"))
def test_block_deterministic_mode(E, ops, monkeypatch, restore_mode, shape):
    """Cases 18-19: every reduction takes its ordered form (the role table asks for them by entry point), no float-atomic launch
    is counted, dx has the bits of the atomic run, every sum is within its bound."""
    kw = dict(act="relu") if shape == "G" else {}
    atomic = run_block(E, ops, monkeypatch, make_case(shape, f32, False, **kw))
    cfg = make_case(shape, f32, False, deterministic=True, **kw)
    det = run_block(E, ops, monkeypatch, cfg)
    assert atomic["atomics"] > 0 and det["atomics"] == 0, f"float-atomic launches: {atomic['atomics']} atomic, {det['atomics']} deterministic"
    assert not E.deterministic()
    check_trace(det, tag_of(cfg) + " deterministic")
    assert bits(det["dx"], atomic["dx"]) and bits(det["y"], atomic["y"]), "dx differs between deterministic and atomic mode"


RIDE_CASES = {   # case -> (shape, pre_ln, switches)
    "20-ride-post": ("R8192", False, {}), "21-ride-pre": ("R8192", True, {}), "22-below-threshold": ("R8191", False, {}),
    "23-ln-bias-ride-off": ("R8192", False, dict(ln_bias_ride=False)), "24-wgrad-asum-off": ("R8192", False, dict(wgrad_asum=False)),
}


@pytest.mark.parametrize("case", sorted(RIDE_CASES))
def test_block_bias_ride(E, ops, monkeypatch, case):
    """Cases 20-24, bf16, dropout on, either side of dyd_rides' threshold and with each switch off: who owns o_b and fc2_b is
    asserted by check_wiring from expected_roles; the values stay within the same bounds."""
    shape, pre_ln, sw = RIDE_CASES[case]
    cfg = make_case(shape, bf16, pre_ln, **sw)
    roles = check_trace(run_block(E, ops, monkeypatch, cfg), tag_of(cfg) + " " + case)
    rides = shape == "R8192" and not sw
    assert (roles["wgrad_o"]["asum"] is not None) == rides and (roles[attn_ln(cfg) + "_bwd"]["colsum"] is None) == rides
    assert (roles["wgrad_fc2"]["asum"] is not None) == (rides or (pre_ln and cfg["wgrad_asum"]))


# ------------------------------------------------------------------------------------------------ attention_layer
def run_attention_layer(E, ops, monkeypatch, cfg, *, biases=True, dense=False, stash=None):
    from multimodaldiscussiontransformer_amd import fp8 as F8
    assert F8.ACTIVE is None
    names = ("qkv_w", "o_w", "sp_table", "virt") + (("qkv_b", "o_b") if biases else ())
    cfg["params"] = {n: t for n, t in cfg["params"].items() if n in names}
    P = {n: torch.nn.Parameter(dev(t)) for n, t in cfg["params"].items()}
    dense_var = None
    if dense:
        sp = cfg["spec"]
        cfg["spec"]["dense_bias"] = RR.values((sp["nseq"], sp["H"], sp["S"], sp["S"]), SEED + 77, 2.0, f32)
        dense_var = E.Var(dev(cfg["spec"]["dense_bias"]), needs_grad=True)
    with monkeypatch.context() as mp, switches(E, mp, cfg):
        rec = BlockRecorder(ops, mp)
        tape = E.Tape()
        torch.manual_seed(cfg["torch_seed"])
        xv = E.Var(dev(cfg["x"]))
        o = E.attention_layer(tape, xv, P["qkv_w"], P.get("qkv_b"), P["o_w"], P.get("o_b"), device_spec(E, cfg, P, dense_var), p_attn=cfg["p_attn"], stash=stash)
        assert tape._seed_ctr == 1
        o.grad = dev(cfg["cot"])
        tape.backward()
        torch.cuda.synchronize()
    grads = {n: host(tape.tmp_grads[id(p)]) for n, p in P.items()}
    if dense:
        grads["dense_bias"] = host(dense_var.grad)
    return dict(cfg=cfg, launches=rec.launches, tape_seeds=tape_seeds(tape._seed_base, 1), y=host(o.data), dx=host(xv.grad), grads=grads)


def check_attention_layer(trace, tag):
    """The same three layers for engine.attention_layer: QKV, attention, output projection and their adjoints."""
    CASE_WORST.clear()
    cfg, P = trace["cfg"], trace["cfg"]["params"]
    roles = classify(trace)
    asum = cfg["dtype"] == bf16
    want = dict(fwd_qkv="gemm", attn_fwd="attention_fwd", fwd_o="gemm", wgrad_o="gemm", dgrad_o="gemm", attn_bwd="attention_bwd", wgrad_qkv="gemm", dgrad_qkv="gemm")
    own = {}
    for n in ("qkv", "o"):
        if n + "_b" in P:
            own[n + "_b"] = ("wgrad_" + n, "asum") if asum else (f"colsum_{n}_b", "out")
            if not asum:
                want[f"colsum_{n}_b"] = "colsum"
    assert {k: r["op"] for k, r in roles.items()} == want, f"attention_layer launched {sorted(roles)}, its structure is {sorted(want)}"
    L = SimpleNamespace(**roles)
    seed, = trace["tape_seeds"]
    for a, b, what in ((L.fwd_qkv["a"], cfg["x"], "QKV reads x"), (L.fwd_qkv["bias"], P.get("qkv_b"), "QKV bias"), (L.attn_fwd["qkv"], L.fwd_qkv["out"], "attention reads qkv"),
                       (L.fwd_o["a"], L.attn_fwd["out"], "the projection reads ctx"), (L.fwd_o["bias"], P.get("o_b"), "projection bias"), (trace["y"], L.fwd_o["out"], "output"),
                       (L.wgrad_o["a"], cfg["cot"], "o weight gradient reads g"), (L.wgrad_o["b"], L.attn_fwd["out"], "o weight gradient reads ctx"),
                       (L.dgrad_o["a"], cfg["cot"], "context gradient reads g"), (L.attn_bwd["dout"], L.dgrad_o["out"], "attention backward reads dctx"),
                       (L.attn_bwd["qkv"], L.fwd_qkv["out"], "attention backward reads qkv"), (L.attn_bwd["out"], L.attn_fwd["out"], "attention backward reads ctx"),
                       (L.attn_bwd["lse"], L.attn_fwd["lse"], "attention backward reads lse"), (L.wgrad_qkv["a"], L.attn_bwd["dqkv"], "qkv weight gradient reads dqkv"),
                       (L.wgrad_qkv["b"], cfg["x"], "qkv weight gradient reads x"), (L.dgrad_qkv["a"], L.attn_bwd["dqkv"], "dx reads dqkv"), (trace["dx"], L.dgrad_qkv["out"], "dx")):
        assert bits(a, b), f"wiring: attention_layer: {what}"
    assert L.fwd_o["residual"] is None and L.fwd_o["drop_p"] == 0.0 and L.dgrad_qkv["residual"] is None
    for r in (L.attn_fwd, L.attn_bwd):
        assert (r["drop_p"], r["drop_seed"]) == (cfg["p_attn"], seed), "wiring: attention_layer: (p, seed) is not the tape's first site"
    owners = dict(qkv_w=("wgrad_qkv", "out"), o_w=("wgrad_o", "out"), **own)
    for n, (role, field) in owners.items():
        assert bits(trace["grads"][n], roles[role][field].view(trace["grads"][n].shape)), f"wiring: the gradient of {n} is not {role}.{field}"
    for n in ("qkv", "o"):
        assert (roles["wgrad_" + n]["asum"] is not None) == (asum and n + "_b" in P), f"wiring: who owns {n}_b"
    if "sp_table" in P:
        assert bits(trace["grads"]["sp_table"], L.attn_bwd["d_sp_table"]) and bits(trace["grads"]["virt"].view(-1), L.attn_bwd["d_virt"])
    if "dense_bias" in trace["grads"]:
        assert bits(trace["grads"]["dense_bias"], L.attn_bwd["dbias"]), "wiring: the dense bias gradient is not the backward's dbias"
    n = check_launches(trace, roles)
    assert n == len(trace["launches"]) == len(roles)
    print(f"\n[{tag}] {n} launches verified; worst err / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(CASE_WORST.items())))
    params = dict(P, **({"dense_bias": cfg["spec"]["dense_bias"]} if "dense_bias" in trace["grads"] else {}))
    cfg["grads0"] = {k: torch.zeros(v.shape) for k, v in params.items()}
    ref = BR.attention_layer_reference(cfg["x"], params, cfg["cot"], cfg["spec"], cfg["p_attn"], seed)
    if "qkv_b" not in P:
        ref["summed"] = {}
    check_end_to_end(trace, ref, tag)
    return roles


def test_attention_layer_structural_tables(E, ops, monkeypatch):
    """Case 25: G fp32, the structural tables with gradients, attention dropout on."""
    trace = run_attention_layer(E, ops, monkeypatch, make_case("G", f32, False))
    check_attention_layer(trace, "attention_layer G fp32 structural")
    assert float(trace["grads"]["sp_table"][1:].abs().max()) > 0 and float(trace["grads"]["virt"].abs().max()) > 0


def test_attention_layer_dense_bias_var(E, ops, monkeypatch):
    """Case 26: G bf16, a dense bias whose Var needs a gradient: it takes the backward's dS."""
    cfg = make_case("G", bf16, False)
    for k in ("attn_bias", "spatial_pos"):
        cfg["spec"].pop(k)
    for k in ("sp_table", "virt"):
        cfg["params"].pop(k)
    trace = run_attention_layer(E, ops, monkeypatch, cfg, dense=True)
    roles = check_attention_layer(trace, "attention_layer G bf16 dense bias")
    assert roles["attn_bwd"]["dbias"] is not None and float(trace["grads"]["dense_bias"].abs().max()) > 0


def test_attention_layer_without_projection_biases(E, ops, monkeypatch):
    """Case 27: S bf16, bias-free projections, the stash filled with what need_weights recomputes the probabilities from."""
    stash = {}
    trace = run_attention_layer(E, ops, monkeypatch, make_case("S", bf16, False), biases=False, stash=stash)
    roles = check_attention_layer(trace, "attention_layer S bf16 no biases")
    assert bits(stash["qkv"].cpu(), roles["fwd_qkv"]["out"]) and bits(stash["lse"].cpu(), roles["attn_fwd"]["lse"])
    assert set(stash["kw"]) >= {"key_mask", "seq_stride", "pos_stride"} and roles["fwd_qkv"]["bias"] is None and roles["fwd_o"]["bias"] is None


def test_report_worst_error_over_bound():
    """Not a check of its own: prints the worst err / bound per launch kind over this run (pytest -s, or the log)."""
    print("\nengine block worst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
