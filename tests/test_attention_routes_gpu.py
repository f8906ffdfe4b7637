"""Every attention kernel and route against the fp64 reference of tests/attention_reference.py, element by element: the two
forward kernels and the key-chunked one, the backward routes v1, v2, v3, v4, v4x, v5 and long (the default route asserted, every
other route whose preconditions hold forced through MDT_ATTN_BWD), fp32 and bf16, no bias / key mask / dense bias /
structural bias, both row layouts, dropout, q_limit, ragged sequences and length bins, head widths 16, 64, 96 and 128, and
the non-training outputs (head weights, mean probabilities, the materialised structural bias).

nseq = 2, H = 3, independent data per (sequence, head); lengths on both sides of every tile-count rung.  Each case prints its
worst error over bound per output; tests/test_attention_reference_cpu.py proves on the CPU that the same bounds reject
subtly wrong kernels at every one of these cases.
"""
import pytest
import torch

import tests.attention_reference as A
from multimodaldiscussiontransformer_amd import _lib as L
from tests.attention_reference import BF, F32, Case
from tests.test_attention_head_dim_gpu import force_bwd, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

H, NSEQ = A.HEADS, A.NSEQ
TENSORS = ("key_mask", "key_pad", "dense_bias", "attn_bias", "spatial_pos", "sp_table", "virt")


def name_of(dtype):
    return "bf16" if dtype == BF else "fp32"


class Launch:
    """One case on the device: its operands laid out as the launch wants them, and the way back to logical tensors."""

    def __init__(self, c: Case, tm=False, want_bwd=True):
        self.c, self.tm = c, tm
        self.qkv, self.dout, self.kw, self.ref = A.case_reference(c, want_bwd)
        S, D = c.S, H * c.hd
        self.S, self.D = S, D
        self.lens = c.lens
        if c.lens:
            self.off = torch.tensor([0] + [sum(c.lens[:i + 1]) for i in range(NSEQ)], dtype=torch.int32)
            pack = lambda t: torch.cat([t[n, :l] for n, l in enumerate(c.lens)], 0)
            self.lay = dict(seq_offsets=self.off.cuda())
        elif tm:
            pack = lambda t: t.transpose(0, 1).reshape(S * NSEQ, -1)
            self.lay = dict(seq_stride=1, pos_stride=NSEQ)
        else:
            pack = lambda t: t.reshape(NSEQ * S, -1)
            self.lay = dict(seq_stride=S, pos_stride=1)
        self.q2 = pack(self.qkv).to(c.dtype).contiguous().cuda()
        self.d2 = pack(self.dout).to(c.dtype).contiguous().cuda()
        self.args = {k: (v if v.numel() else torch.zeros(1, dtype=v.dtype)).cuda() for k, v in self.kw.items() if k in TENSORS}   # S = 1: no (S-1)^2 distances
        self.args.update({k: v for k, v in self.kw.items() if k in ("drop_p", "drop_seed", "q_limit")})
        self.args["scale"] = c.hd ** -0.5

    def logical(self, t):
        t = t.float().cpu()
        if self.lens:
            out = torch.zeros(NSEQ, self.S, t.shape[1])
            for n, l in enumerate(self.lens):
                out[n, :l] = t[int(self.off[n]):int(self.off[n]) + l]
            return out
        if self.tm:
            return t.view(self.S, NSEQ, -1).transpose(0, 1)
        return t.view(NSEQ, self.S, -1)

    def forward(self, ops, bins=None):
        self.out, self.lse = ops.attention_fwd(self.q2, NSEQ, self.S, H, bins=bins, **self.lay, **self.args)
        route = L.last_route()
        want = A.fwd_route(self.c.dtype, self.c.hd, self.S, self.c.mode)
        assert route == want, f"forward took {route}, the dispatch says {want}"
        return {"out": self.logical(self.out), "lse": self.lse.cpu()}, route

    def backward(self, ops, want_route, bins=None):
        c = self.c
        extra = {}
        if c.mode == "struct":
            extra = dict(d_sp_table=torch.zeros(self.kw["sp_table"].shape[0], H, device="cuda"), d_virt=torch.zeros(H, device="cuda"))
        dqkv, dbias = ops.attention_bwd(self.d2, self.q2, self.out, self.lse, NSEQ, self.S, H, bins=bins, want_dense_dbias=c.mode == "dense",
                                        **self.lay, **self.args, **extra)
        route = L.last_route()
        assert route == want_route, f"backward took {route}, expected {want_route}"
        got = {"dqkv": self.logical(dqkv)}
        if dbias is not None:
            got["dbias"] = dbias.cpu()
        got.update({k: v.cpu() for k, v in extra.items()})
        return got


def show(tag, worst):
    print(f"[{tag}] err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def run_case(ops, force_bwd, c: Case, tm=False, routes=A.ROUTES, bins=None, cap=0):
    """Forward, default backward and every forced backward of one case, each output inside its bound."""
    tag = f"{name_of(c.dtype)} hd{c.hd} S={c.S} {c.mode} {c.family} p={c.p}" + (" tm" if tm else "") + (f" q{c.qlim}" if c.qlim else "") + \
        (f" len{c.lens}" if c.lens else "") + (" bins" if bins else "")
    want_bwd = c.family != "pointer"
    force_bwd(None)
    run = Launch(c, tm, want_bwd)
    got, route = run.forward(ops, bins)
    show(f"{tag} fwd {route}", A.check(got, run.ref, c.dtype, what=f"{tag} fwd {route}"))
    if not want_bwd:
        return
    default = A.bwd_route(c.dtype, c.hd, c.S, c.mode, c.p, c.qlim, cap)
    todo = [None]
    if c.dtype == BF and c.S <= 272 and default != "long":
        todo += [r for r in routes if r != default and A.bwd_ok(r, c.hd, c.S, c.mode, c.qlim, cap)]
    for forced in todo:
        force_bwd(forced)
        want = forced or default
        got = run.backward(ops, want, bins)
        show(f"{tag} bwd {want}", A.check(got, run.ref, c.dtype, what=f"{tag} bwd {want}"))
    force_bwd(None)


# ----------------------------------------------------------------------------- head width 64: the whole matrix
@pytest.mark.parametrize("S", A.SIZES)
@pytest.mark.parametrize("mode,tm", A.MODES)
@pytest.mark.parametrize("dtype", (F32, BF), ids=name_of)
def test_attention_matrix(ops, force_bwd, dtype, mode, tm, S):
    """Per (type, bias mode, layout, length): the "pointer" forward, the "soft" forward and backward without dropout, the
    "uniform" forward and backward with dropout 0.25; bf16: the default backward route and every route that can be forced."""
    for c in A.families(dtype, 64, S, mode):
        run_case(ops, force_bwd, c, tm)


@pytest.mark.parametrize("S", A.QLIM_SIZES)
@pytest.mark.parametrize("mode", ("none", "struct"))
def test_query_limit(ops, force_bwd, mode, S):
    """q_limit = 9 (bf16: the v2 forward and the v3 family honour it): out / lse of the first 9 rows, dK / dV of every row, dQ
    of the rows past the limit exactly 0; and the same launch without the limit."""
    run_case(ops, force_bwd, Case(BF, 64, S, mode, "soft", A.P_DROP, A.QLIM, None))
    run_case(ops, force_bwd, Case(BF, 64, S, mode, "soft", A.P_DROP, 0, None))


@pytest.mark.parametrize("S,lens", A.RAGGED)
@pytest.mark.parametrize("dtype", (F32, BF), ids=name_of)
def test_ragged_sequences(ops, force_bwd, dtype, S, lens):
    """seq_offsets: one sequence one row past a tile edge, the other ending on one; S stays the lse / dropout-counter bound."""
    run_case(ops, force_bwd, Case(dtype, 64, S, "none", "soft", A.P_DROP, 0, lens))


@pytest.mark.parametrize("S,lens,cap", A.BINS)
def test_length_bins(ops, force_bwd, S, lens, cap):
    """The same ragged set as two launches (seq_ids / s_cap): the short sequence with the kernels of its cap."""
    short = [i for i, n in enumerate(lens) if n <= cap]
    long_ = [i for i, n in enumerate(lens) if n > cap]
    bins = [(torch.tensor(short, dtype=torch.int32).cuda(), cap), (torch.tensor(long_, dtype=torch.int32).cuda(), S)]
    run_case(ops, force_bwd, Case(BF, 64, S, "none", "soft", A.P_DROP, 0, lens), bins=bins, cap=S, routes=("v3", "v4", "v5"))


# ----------------------------------------------------------------------------- key-chunked path, other widths
@pytest.mark.parametrize("dtype,hd,S,mode", A.LONG, ids=lambda v: name_of(v) if isinstance(v, torch.dtype) else str(v))
def test_key_chunked_path(ops, force_bwd, dtype, hd, S, mode):
    """S = 273 and 320 at head width 64 in every bias mode, and a dense bias on 128-wide heads of 209 tokens (bf16: the v1 images
    do not fit LDS there), without and with dropout."""
    for c in (Case(dtype, hd, S, mode, "soft", 0.0, 0, None), Case(dtype, hd, S, mode, "uniform", A.P_DROP, 0, None)):
        run_case(ops, force_bwd, c, tm=mode == "struct")


@pytest.mark.parametrize("hd,S,mode", A.WIDE)
@pytest.mark.parametrize("dtype", (F32, BF), ids=name_of)
def test_other_head_widths(ops, force_bwd, dtype, hd, S, mode):
    """Head widths 16, 96 and 128: one case per forward / backward route they reach, and the 256 | 257 step of the 128-wide v3."""
    for c in (Case(dtype, hd, S, mode, "soft", 0.0, 0, None), Case(dtype, hd, S, mode, "uniform", A.P_DROP, 0, None)):
        run_case(ops, force_bwd, c, tm=mode == "struct")


# ----------------------------------------------------------------------------- non-training outputs
@pytest.mark.parametrize("S", (33, 129))
@pytest.mark.parametrize("mode", ("struct", "mask"))
@pytest.mark.parametrize("dtype", (F32, BF), ids=name_of)
def test_non_training_outputs(ops, force_bwd, dtype, mode, S):
    """mdt_attention_head_weights (probabilities and raw scores), mdt_attention_mean_probs and mdt_graph_attn_bias."""
    force_bwd(None)
    c = Case(dtype, 64, S, mode, "soft", 0.0, 0, None)
    run = Launch(c, tm=mode == "struct", want_bwd=False)
    run.forward(ops)
    kw = {k: v for k, v in run.args.items() if k in TENSORS + ("scale",)}
    got = {"probs": ops.attention_head_weights(run.q2, run.lse, NSEQ, S, H, **run.lay, **kw).cpu(),
           "scores": ops.attention_head_weights(run.q2, None, NSEQ, S, H, raw_scores=True, **run.lay, **kw).cpu(),
           "mean_probs": ops.attention_mean_probs(run.q2, run.lse, NSEQ, S, H, **run.lay, **kw).cpu()}
    show(f"{name_of(dtype)} S={S} {mode} weights", A.check(got, run.ref, dtype, what=f"{name_of(dtype)} S={S} {mode}"))
    if mode == "struct":
        b = ops.graph_attn_bias(*(run.args[k] for k in ("attn_bias", "spatial_pos", "sp_table", "virt"))).cpu()
        v, d = A.reference_graph_bias(*(run.kw[k] for k in ("attn_bias", "spatial_pos", "sp_table", "virt")))
        assert bool(((b.double() == v) | torch.isfinite(v)).all()), "a -inf entry of the structural bias is not -inf"
        A.assert_within(b, v, A.bound(torch.nan_to_num(v, neginf=0.0), d, F32), what="graph_attn_bias", dtype=F32)


def test_worst_error_over_bound_report():
    """Runs last in this file: the worst error over bound per (output, type) that the cases above saw."""
    for (name, dtype), w in sorted(A.WORST.items(), key=str):
        print(f"[worst] {name_of(dtype)} {name}: {w:.3f}")
    assert all(w <= 1.0 for w in A.WORST.values())
