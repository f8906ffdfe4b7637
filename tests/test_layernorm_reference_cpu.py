"""The bounds of tests/layernorm_reference.py can fail: a CPU emulation of the LayerNorm kernels' arithmetic (fp32, one
rounding per operation, the kernels' order of operations, round-to-nearest-even to the storage type) is accepted at every
(dtype, D, form) of the GPU matrix (tests/test_layernorm_routes_gpu.py) in two summation orders — a lane's vectors in
turn and then a tree over the 64 lanes, as the kernels sum, and plain left to right — and each listed mutant of it, a
subtly wrong kernel, is rejected.  Operands come from the generator and scales the GPU matrix uses."""
import numpy as np
import pytest
import torch

import tests.layernorm_reference as LR

bf16, f32 = torch.bfloat16, torch.float32
ROWS = 9                 # rows_per_wave 4: two full waves and one with a single row
SEED = 4321
ORDERS = ("lanes", "ltr")


def _seq(v, axis):
    """fp32 left-to-right sum along ``axis`` (numpy's accumulate adds in turn, in the array's own type)."""
    return torch.from_numpy(np.ascontiguousarray(np.take(np.cumsum(v.numpy(), axis=axis, dtype=np.float32), -1, axis=axis)))


def row_sum(v, order, vn):
    """Σ over the columns of v [rows, D] in fp32: "ltr" left to right; "lanes" as a wave does it — lane l adds the
    elements of its vectors (column (i * 64 + l) * vn + j) in turn, then the 64 lanes combine in a tree."""
    if order == "ltr":
        return _seq(v, 1)
    rows, D = v.shape
    nv = -(-D // (64 * vn))
    p = torch.zeros(rows, nv * 64 * vn, dtype=f32)
    p[:, :D] = v                                      # absent vectors add nothing
    lanes = _seq(p.view(rows, nv, 64, vn).permute(0, 2, 1, 3).reshape(rows, 64, nv * vn).contiguous(), 2)
    n = 64
    while n > 1:
        n //= 2
        lanes = (lanes[:, :n] + lanes[:, n:2 * n]).to(f32)
    return lanes[:, 0]


def col_sum(terms, c0, order, skip_row=None, overwrite=False):
    """c0 + Σ over the rows of terms [rows, D] in fp32: "ltr" row after row; "lanes" as the kernels do — each wave its
    4 rows in turn, the 4 waves of a workgroup added, one atomic add per workgroup."""
    t = terms.clone()
    if skip_row is not None:
        t[skip_row] = 0
    acc = torch.zeros_like(c0) if overwrite else c0.clone()
    if order == "ltr":
        return (acc + _seq(torch.cat([torch.zeros(1, t.shape[1]), t]), 0)).to(f32) if overwrite else _seq(torch.cat([acc[None], t]), 0)
    for w0 in range(0, t.shape[0], 16):
        waves = [_seq(t[r:r + 4], 0) if r < t.shape[0] else torch.zeros(t.shape[1]) for r in range(w0, w0 + 16, 4)]
        acc = (acc + (((waves[0] + waves[1]).to(f32) + waves[2]).to(f32) + waves[3]).to(f32)).to(f32)
    return acc


def _store(v, dtype, mutant):
    if mutant == "truncate" and dtype == bf16:
        return (v.contiguous().view(torch.int32) & ~0xFFFF).view(f32).to(bf16)
    return v.to(dtype)


def emulate_fwd(x, gamma, beta, eps, order, mutant=None):
    T = x.dtype
    X, G, B = x.float(), gamma.float()[None], beta.float()[None]
    rows, D = X.shape
    vn = LR.vector_width(T, D)
    e = torch.tensor(eps, dtype=f32)
    n_mean = -(-D // (64 * vn)) * 64 * vn if mutant == "mean_over_padded_width" else D
    mu = (row_sum(X, order, vn) / torch.tensor(float(n_mean), dtype=f32)).to(f32)
    d = (X - mu[:, None]).to(f32)
    n_var = D - 1 if mutant == "variance_over_d_minus_1" else D
    var = (row_sum((d * d).to(f32), order, vn) / torch.tensor(float(n_var), dtype=f32)).to(f32)
    if mutant == "eps_after_sqrt":
        rs = (1.0 / (torch.sqrt(var) + e)).to(f32)
    else:
        rs = torch.rsqrt((var + e).to(f32))
    y = ((((d * rs[:, None]).to(f32) * G).to(f32)) + B).to(f32)
    if mutant == "last_vector_zero":
        y[:, (D - 1) // vn * vn:] = 0
    return {"y": _store(y, T, mutant), "mean": mu, "rstd": rs}


def emulate_bwd(o, mean, rstd, form, order, drop_p=LR.P_DROP, mutant=None, ldx=None):
    """mdt_layernorm_bwd on the operands ``o`` (LR.operands) in the form ``form``; the outputs it writes."""
    dy, x = o["dy"], o["x"]
    T = x.dtype
    has_add, has_cs, dropped = bool(form & 1), bool(form & 2), bool(form & 4)
    X, GY, G = x.float(), dy.float(), o["gamma"].float()[None]
    rows, D = X.shape
    vn = LR.vector_width(T, D)
    Df = torch.tensor(float(D), dtype=f32)
    mu, rs = mean[:, None], rstd[:, None]
    xh = ((X - mu).to(f32) * rs).to(f32)
    gg = (GY * G).to(f32)
    s1 = row_sum(GY if mutant == "s1_without_gamma" else gg, order, vn)
    s2 = row_sum(((GY if mutant == "m2_without_gamma" else gg) * xh).to(f32), order, vn)
    m1, m2 = (s1 / Df).to(f32)[:, None], (s2 / Df).to(f32)[:, None]
    v = (rs * ((gg - m1).to(f32) - (xh * m2).to(f32)).to(f32)).to(f32)
    A = o["add"].float() if has_add else None
    late_add = mutant == "add_after_dropout" and has_add and dropped
    if has_add and not late_add:
        v = (v + A).to(f32)
    if mutant == "last_vector_zero":
        v[:, (D - 1) // vn * vn:] = 0
    dx = _store(v, T, mutant)
    got = {"dx": _store((v + A).to(f32), T, mutant) if late_add else dx}
    tail = dx
    if dropped:
        if mutant == "counter_off_by_one":
            c = torch.arange(rows, dtype=torch.int64)[:, None] * D + torch.arange(D, dtype=torch.int64)[None] + 1
            s = (LR.R.keep_bits(c, drop_p, SEED).double() * LR.R.drop_params(drop_p)[1]).float()
        else:
            s = LR.drop_scale(rows, D, drop_p, SEED, counter_ld=ldx if mutant == "counter_uses_row_stride" else None).float()
        vd = ((v if mutant == "dxd_from_unrounded_dx" else dx.float()) * s).to(f32)
        if late_add:
            vd = (vd + A).to(f32)
        got["dxd"] = _store(vd, T, mutant)
        tail = dx if mutant == "colsum_of_dx_while_dropping" else got["dxd"]
    skip = 5 if mutant == "row_left_out_of_column_sums" else None
    over = mutant == "sums_overwrite"
    if has_cs:
        got["colsum"] = col_sum(tail.float(), o["colsum0"], order, skip, over)
    got["dgamma"] = col_sum((GY * xh).to(f32), o["dgamma0"], order, skip, over)
    got["dbeta"] = col_sum(GY, o["dbeta0"], order, skip, over)
    return got


def run_fwd(dtype, D, order, eps=1e-5, mutant=None, only=None, x_scale=2.0):
    o = LR.operands(ROWS, D, dtype, SEED, x_scale=x_scale)
    got = emulate_fwd(o["x"], o["gamma"], o["beta"], eps, order, mutant)
    ref = LR.reference_fwd(o["x"], o["gamma"], o["beta"], eps)
    if only:
        got = {k: got[k] for k in only}
    LR.check(got, ref, {"y": dtype, "mean": f32, "rstd": f32}, what=f"fwd {dtype} D={D} {order} {mutant}")


def run_bwd(dtype, D, form, order, mutant=None, drop_p=LR.P_DROP, only=None):
    o = LR.operands(ROWS, D, dtype, SEED)
    st = emulate_fwd(o["x"], o["gamma"], o["beta"], 1e-5, order)
    ldx = D + (64 if dtype == bf16 else 4)
    got = emulate_bwd(o, st["mean"], st["rstd"], form, order, drop_p, mutant, ldx)
    ref = LR.reference_bwd(o["dy"], o["x"], o["gamma"], st["mean"], st["rstd"], add=o["add"] if form & 1 else None,
                           drop_p=drop_p, drop_seed=SEED, dgamma0=o["dgamma0"], dbeta0=o["dbeta0"], colsum0=o["colsum0"],
                           want_dropped=bool(form & 4), want_colsum=bool(form & 2), dx_stored=got["dx"], dxd_stored=got.get("dxd"))
    if only:
        got = {k: got[k] for k in only}
    LR.check(got, ref, {"dx": dtype, "dxd": dtype}, what=f"bwd {dtype} D={D} form {form} {order} {mutant}")


FWD = [(t, D) for t in (bf16, f32) for D in LR.FWD_DIMS[t]]
BWD = [(t, D) for t in (bf16, f32) for D in LR.BWD_DIMS[t]]


def _id(v):
    if isinstance(v, dict):
        return "-".join(v) or "all"
    return "bf16" if v is bf16 else "f32" if v is f32 else str(v)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype,D", FWD, ids=_id)
def test_faithful_forward_is_accepted(dtype, D, order):
    for eps in (1e-5, 1e-12):
        run_fwd(dtype, D, order, eps)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype,D", BWD, ids=_id)
def test_faithful_backward_is_accepted_in_every_form(dtype, D, order):
    for form in LR.FORMS:
        run_bwd(dtype, D, form, order)
    run_bwd(dtype, D, 7, order, drop_p=0.0)           # a dropped copy with nothing dropped


def test_special_rows_are_bounded_and_accepted():
    """A constant row (every operation exact: y = beta, mean = the constant, rstd = eps^-1/2), a row of mean 1000 and
    spread 1 on a granule that keeps its sums exact, and bf16 rows at the largest power of two whose squares still sum
    to a finite fp32 number in any order."""
    for dtype, D in ((bf16, 768), (f32, 768), (bf16, 776), (f32, 132)):
        o = LR.operands(ROWS, D, dtype, SEED)
        x = o["x"]
        x[2] = 3.25
        x[4] = LR.far_mean_row(D, dtype, SEED)
        if dtype == bf16:
            x[6] = (x[6].float() * LR.largest_scale(D)).to(bf16)
        for order in ORDERS:
            for eps in (1e-5, 1e-12):
                got = emulate_fwd(x, o["gamma"], o["beta"], eps, order)
                ref = LR.reference_fwd(x, o["gamma"], o["beta"], eps)
                assert float(ref["y"][1][2].max()) == 0.0 and float(ref["mean"][1][2]) == 0.0     # the constant row is exact
                LR.check(got, ref, {"y": dtype, "mean": f32, "rstd": f32}, what=f"special rows {dtype} D={D} {order}")


def test_a_row_the_model_cannot_bound_is_refused():
    x = LR.gen((3, 768), 5, 1.0, f32)
    x[1] = 1000.0 + x[1] * 2.0 ** -12                 # fp32 noise on a large mean: δw > w / 2
    with pytest.raises(AssertionError, match="not bounded"):
        LR.reference_fwd(x, torch.ones(768), torch.zeros(768), 1e-12)


FWD_MUTANTS = [
    ("variance_over_d_minus_1", bf16, 768, dict(only=("rstd",))),
    ("variance_over_d_minus_1", f32, 768, dict(only=("rstd",))),
    ("variance_over_d_minus_1", bf16, 8, {}),
    ("mean_over_padded_width", bf16, 776, {}),
    ("mean_over_padded_width", f32, 132, {}),
    ("eps_after_sqrt", bf16, 768, dict(x_scale=2.0 ** -7)),
    ("eps_after_sqrt", f32, 128, dict(x_scale=2.0 ** -7)),
    ("last_vector_zero", bf16, 776, {}),
    ("last_vector_zero", f32, 132, {}),
    ("truncate", bf16, 768, {}),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mutant,dtype,D,kw", FWD_MUTANTS, ids=_id)
def test_forward_mutant_is_rejected(mutant, dtype, D, kw, order):
    run_fwd(dtype, D, order, **kw)                    # the faithful kernel passes the very same check
    with pytest.raises(AssertionError):
        run_fwd(dtype, D, order, mutant=mutant, **kw)


# (mutant, dtype, D, form, the one output that must reject it — None: any)
BWD_MUTANTS = [
    ("s1_without_gamma", bf16, 768, 0, "dx"),
    ("s1_without_gamma", f32, 128, 1, "dx"),
    ("m2_without_gamma", bf16, 768, 0, "dx"),
    ("m2_without_gamma", f32, 128, 1, "dx"),
    ("add_after_dropout", bf16, 768, 5, "dxd"),
    ("counter_uses_row_stride", bf16, 768, 4, "dxd"),
    ("counter_uses_row_stride", f32, 128, 7, "dxd"),
    ("counter_off_by_one", bf16, 1024, 4, "dxd"),
    ("dxd_from_unrounded_dx", bf16, 768, 5, "dxd"),
    ("colsum_of_dx_while_dropping", bf16, 768, 6, "colsum"),
    ("sums_overwrite", bf16, 768, 2, "colsum"),
    ("sums_overwrite", bf16, 768, 0, "dgamma"),
    ("sums_overwrite", f32, 128, 0, "dbeta"),
    ("row_left_out_of_column_sums", bf16, 768, 6, "colsum"),
    ("row_left_out_of_column_sums", bf16, 768, 0, "dgamma"),
    ("row_left_out_of_column_sums", f32, 128, 0, "dbeta"),
    ("last_vector_zero", bf16, 776, 1, "dx"),
    ("truncate", bf16, 768, 1, "dx"),
    ("truncate", bf16, 768, 4, "dxd"),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mutant,dtype,D,form,output", BWD_MUTANTS, ids=_id)
def test_backward_mutant_is_rejected(mutant, dtype, D, form, output, order):
    run_bwd(dtype, D, form, order)
    with pytest.raises(AssertionError, match=output):
        run_bwd(dtype, D, form, order, mutant=mutant, only=(output,))


def test_column_sums_with_a_vacuous_bound_are_refused():
    """40 000 rows of generated dy: the worst-case bound of dbeta is a large fraction of the sum itself, and check()
    refuses to call that a test; integer dy at the same row count is exact."""
    rows, D = 40_000, 8
    o = LR.operands(rows, D, f32, SEED)
    mean, rstd = torch.zeros(rows), torch.ones(rows)
    ref = LR.reference_bwd(o["dy"], o["x"], o["gamma"], mean, rstd)
    with pytest.raises(AssertionError, match="vacuous"):
        LR.check({"dbeta": ref["dbeta"][0].float()}, ref, {}, what="oversized")
    oi = LR.operands(rows, D, f32, SEED, int_dy=True)
    ref = LR.reference_bwd(oi["dy"], oi["x"], oi["gamma"], mean, rstd, dbeta0=oi["dbeta0"])
    assert float(ref["dbeta"][1].max()) == 0.0
    LR.check({"dbeta": ref["dbeta"][0].float()}, ref, {}, what="integer dy")


def test_embedding_sum_reference_rounds_twice():
    w, p, t = LR.gen((7, 8), 1, 1.0, f32), LR.gen((5, 8), 2, 1.0, f32), LR.gen((2, 8), 3, 1.0, f32)
    ids, pos, typ = torch.tensor([0, 6, 3]), torch.tensor([4, 0, 2]), torch.tensor([1, 0, 1])
    v, d = LR.reference_embed_sum(w, p, t, ids, typ, pos)
    got = ((w[ids] + t[typ]).to(f32) + p[pos]).to(f32)
    LR.assert_within(got, v, LR.bound(v, d, f32), what="embed sum")
    with pytest.raises(AssertionError):
        LR.assert_within(got + 2.0 ** -20, v, LR.bound(v, d, f32), what="embed sum")
