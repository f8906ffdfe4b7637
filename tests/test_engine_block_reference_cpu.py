"""The checks of tests/test_engine_block_gpu.py can fail.  engine.transformer_block is written once here as a small torch model:
fp32 arithmetic, a rounding to the storage type at every store the kernels make, the dropout masks of the CPU ports, the
gradient buffers accumulated in fp32 — and every step emits the record the GPU file's recorder would keep of that launch.  The
three layers of checks accept the model's trace at shapes S and G in both placements and both types with dropout on, at the
8192-row shape R in bf16, and with keep_rows, a frozen input and pre-filled main_grad buffers; they reject each mutant of
MUTANTS, a subtly wrong block, in the layer named there.  The references are the only judge.

Also shown here: the end-to-end gate discriminates (every mutant that changes values moves some tensor at least 10 x beyond
its gate), and for the chosen operands the references alone meet every non-vacuity cap of the sum checks (median bound /
|ref| <= 2^-7) — the caps are part of the checks the model's trace passes, the 8192-row bias sums of shape R included, which
is what the per-column offsets of the cotangent are for.  The relative L2 values printed by test_model_is_accepted are the
measurements behind BF16_E2E_MEASURED of the GPU file."""
import numpy as np
import pytest
import torch

import tests.activation_reference as ACT
import tests.attention_reference as AR
import tests.block_reference as BR
import tests.gemm_reference as GR
import tests.layernorm_reference as LR
import tests.rowops_reference as RR
import tests.test_engine_block_gpu as T
from tests.rowops_reference import bf16, f32

BASE = 0x2545F4914F6CDD1D >> 2          # a seed base as Tape.next_seed draws one: below 2^62


@pytest.fixture(autouse=True)
def _worst_ratios_are_left_alone():
    """The mutants' err / bound must not reach the reports of the GPU files that run in the same session."""
    saved = [(d, dict(d)) for d in (RR.WORST, LR.WORST, AR.WORST, T.WORST, T.CASE_WORST)]
    yield
    for d, was in saved:
        d.clear()
        d.update(was)


# ------------------------------------------------------------------------------------------------ the launches, modelled
class Model:
    """One method per entry point: the result in fp32 arithmetic, rounded where the kernel stores, and the recorder's record."""

    def __init__(self, cfg):
        self.cfg, self.T, self.launches = cfg, cfg["dtype"], []

    def rec(self, op, **fields):
        self.launches.append(dict(op=op, **{k: (v.clone() if torch.is_tensor(v) else v) for k, v in fields.items()}))

    def st(self, v):
        return v.float().to(self.T)

    def gemm(self, a, b, *, trans_a=False, trans_b=False, out=None, bias=None, residual=None, aux=None, epilogue=0, split_k=1, drop_p=0.0, drop_seed=0,
             colsum=None, asum=None):
        before = {k: (None if t is None else t.clone()) for k, t in (("out", out), ("aux", aux), ("colsum", colsum), ("asum", asum))}
        A = a.float().t() if trans_a else a.float()
        B = b.float() if trans_b else b.float().t()
        v = A @ B
        if bias is not None:
            v = v + bias.float()[None]
        s = GR.drop_scale(v.shape[0], v.shape[1], drop_p, drop_seed).float() if drop_p > 0 else None
        if epilogue & GR.EPI_GELU:
            sc = 1.0 if s is None else s
            aux = self.st(GR.gelu_grad(v.double()).float() * sc)                  # erf in fp64: 1 + erf cancels in fp32, a flaw of this model alone
            v = GR.gelu(v.double()).float() * sc
        elif s is not None:
            v = v * s
        if epilogue & GR.EPI_MULAUX:
            v = v * aux.float()
        if residual is not None:
            v = v + residual.float()
        if colsum is not None:
            colsum += v.sum(0)
        if asum is not None:
            asum += a.float().sum(0)
        if out is not None:
            out += v
            res = out
        else:
            res = self.st(v)
        self.rec("gemm", a=a, b=b, out=res, c_old=before["out"], aux0=before["aux"], aux=aux, colsum0=before["colsum"], colsum=colsum, asum0=before["asum"],
                 asum=asum, bias=bias, residual=residual, trans_a=trans_a, trans_b=trans_b, epilogue=int(epilogue), split_k=int(split_k), drop_p=float(drop_p),
                 drop_seed=int(drop_seed))
        return (res, aux) if epilogue & GR.EPI_GELU else res

    def ln_fwd(self, x, gamma, beta, eps):
        X = x.float()
        mean = X.mean(1)
        d = X - mean[:, None]
        rstd = ((d * d).mean(1) + float(np.float32(eps))).rsqrt()
        y = self.st((d * rstd[:, None]) * gamma.float() + beta.float())
        self.rec("layernorm_fwd", x=x, gamma=gamma, beta=beta, eps=float(eps), y=y, mean=mean, rstd=rstd)
        return y, mean, rstd

    def ln_bwd(self, dy, x, gamma, mean, rstd, *, add=None, dgamma=None, dbeta=None, drop_p=0.0, drop_seed=0, colsum=None, want_dropped=False):
        before = {k: (None if t is None else t.clone()) for k, t in (("dgamma", dgamma), ("dbeta", dbeta), ("colsum", colsum))}
        xh = (x.float() - mean[:, None]) * rstd[:, None]
        gg = dy.float() * gamma.float()
        v = rstd[:, None] * ((gg - gg.mean(1, keepdim=True)) - xh * (gg * xh).mean(1, keepdim=True))
        if add is not None:
            v = v + add.float()
        dx, dxd = self.st(v), None
        if want_dropped and drop_p > 0:
            dxd = self.st(dx.float() * GR.drop_scale(x.shape[0], x.shape[1], drop_p, drop_seed).float())
        tail = dx if dxd is None else dxd
        if colsum is not None:
            colsum += tail.float().sum(0)
        if dbeta is not None:
            dbeta += dy.float().sum(0)
        if dgamma is not None:
            dgamma += (dy.float() * xh).sum(0)
        self.rec("layernorm_bwd", dy=dy, x=x, gamma=gamma, mean=mean, rstd=rstd, add=add, dgamma0=before["dgamma"], dgamma=dgamma, dbeta0=before["dbeta"], dbeta=dbeta,
                 colsum0=before["colsum"], colsum=colsum, dx=dx, dxd=dxd, drop_p=float(drop_p), drop_seed=int(drop_seed), want_dropped=bool(want_dropped))
        return dx, tail

    # -- attention: the logical [nseq, H, S, hd] view in fp32, probabilities kept in fp32
    def _attn(self, qkv, drop_p, drop_seed):
        sp, P = self.cfg["spec"], self.cfg["params"]
        nseq, S, H = sp["nseq"], sp["S"], sp["H"]
        m, lens = BR.spec_geometry(sp)
        D = qkv.shape[1] // 3
        hd = D // H
        q, k, v = (BR.to_logical(qkv[:, i * D:(i + 1) * D].float(), m).view(nseq, S, H, hd).transpose(1, 2) for i in range(3))
        s = hd ** -0.5 * (q @ k.transpose(-1, -2))
        dead = torch.zeros(nseq, 1, 1, S, dtype=torch.bool)
        if lens is not None:
            dead = dead | (torch.arange(S)[None] >= lens[:, None])[:, None, None, :]
        if sp.get("key_mask") is not None:
            dead = dead | (sp["key_mask"] == 0)[:, None, None, :]
        if sp.get("key_pad") is not None:
            dead = dead | (sp["key_pad"] != 0)[:, None, None, :]
        if sp.get("attn_bias") is not None:
            s = s + AR.struct_bias(sp["attn_bias"], sp["spatial_pos"], P["sp_table"], P["virt"].view(-1))[0].float()
        s = torch.where(dead, torch.full_like(s, float("-inf")), s)
        ks = AR.drop_scale(nseq, H, S, drop_p, drop_seed).float()
        kw = dict(nseq=nseq, S=S, H=H, seq_stride=sp["seq_stride"], pos_stride=sp["pos_stride"], scale=None, key_mask=sp.get("key_mask"), dense_bias=None,
                  attn_bias=sp.get("attn_bias"), spatial_pos=sp.get("spatial_pos"), sp_table=P.get("sp_table"), virt=None if "virt" not in P else P["virt"].view(-1),
                  key_pad=sp.get("key_pad"), seq_offsets=sp.get("seq_offsets"), q_limit=sp["q_limit"], bins=None, drop_p=float(drop_p), drop_seed=int(drop_seed))
        return (q, k, v, s, ks, m, hd ** -0.5), kw

    def attn_fwd(self, qkv, drop_p, drop_seed):
        (q, k, v, s, ks, m, _), kw = self._attn(qkv, drop_p, drop_seed)
        lse = torch.logsumexp(s, -1)
        out = ((torch.exp(s - lse[..., None]) * ks) @ v).transpose(1, 2).reshape(s.shape[0], s.shape[2], -1)
        out = self.st(BR.from_logical(out, m, qkv.shape[0]))
        self.rec("attention_fwd", qkv=qkv, out=out, lse=lse, **kw)
        return out, lse

    def attn_bwd(self, dout, qkv, out, lse, drop_p, drop_seed, d_sp_table=None, d_virt=None):
        (q, k, v, s, ks, m, scale), kw = self._attn(qkv, drop_p, drop_seed)
        nseq, H, S, hd = q.shape
        t0, v0 = (None if t is None else t.clone() for t in (d_sp_table, d_virt))
        heads = lambda t: BR.to_logical(t.float(), m).view(nseq, S, H, hd).transpose(1, 2)          # noqa: E731
        dO, O = heads(dout), heads(out)
        P = torch.exp(s - lse[..., None])
        dPd = (dO @ v.transpose(-1, -2)) * ks
        dS = P * (dPd - (dO * O).sum(-1)[..., None])                   # delta = rowsum(dO . O_stored), the documented form
        parts = [scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), (P * ks).transpose(-1, -2) @ dO]
        dqkv = self.st(BR.from_logical(torch.cat([p.transpose(1, 2).reshape(nseq, S, H * hd) for p in parts], -1), m, qkv.shape[0]))
        if d_sp_table is not None:
            pick = dS[:, :, 1:, 1:].permute(0, 2, 3, 1).reshape(-1, H)
            add = torch.zeros_like(d_sp_table).index_add_(0, self.cfg["spec"]["spatial_pos"].long().reshape(-1), pick)
            add[0] = 0.0
            d_sp_table += add
            d_virt += dS[:, :, 0, :].sum((0, 2)) + dS[:, :, 1:, 0].sum((0, 2))
        self.rec("attention_bwd", dout=dout, qkv=qkv, out=out, lse=lse, dqkv=dqkv, dbias=None, d_sp_table0=t0, d_sp_table=d_sp_table, d_virt0=v0, d_virt=d_virt,
                 want_dense_dbias=False, **kw)
        return dqkv

    def act_fwd(self, pre, kind, drop_p, drop_seed, scale_u=True):
        s = ACT.drop_scale(pre.shape[0], pre.shape[1], drop_p, drop_seed).float()
        h = self.st(ACT.act(kind, pre.float()) * s)
        u = self.st(ACT.act_grad(kind, pre.float()) * (s if scale_u else 1.0))
        self.rec("act_fwd", pre=pre, kind=kind, drop_p=float(drop_p), drop_seed=int(drop_seed), want_u=True, h=h, u=u)
        return h, u

    def dropout(self, x, p, seed):
        y = self.st(x.float() * GR.drop_scale(x.shape[0], x.shape[1], p, seed).float())
        self.rec("dropout", x=x, p=float(p), seed=int(seed), out=y)
        return y

    def rows(self, dst, *, a, di=None, ai=None):
        dst0 = dst.clone()
        if ai is not None:
            dst[:] = a[ai.long()]
        else:
            dst[di.long()] = a
        self.rec("row_axpby", dst0=dst0, dst=dst, nrows=int((ai if ai is not None else di).numel()), di=di, a=a, ai=ai, accumulate=False)
        return dst

    def colsum(self, x, out):
        out0 = out.clone()
        out += x.float().sum(0)
        self.rec("colsum", x=x, out0=out0, out=out)


# ------------------------------------------------------------------------------------------------ the block, modelled
def model_block(cfg, mutant=None):
    """engine.transformer_block in atomic mode with both ride switches on → the trace the GPU file's run_block returns."""
    M, P, pre, bf = Model(cfg), cfg["params"], cfg["pre_ln"], cfg["dtype"] == bf16
    seeds = T.tape_seeds(BASE)
    if mutant == "s_o_equals_s_f2":
        seeds[1] = seeds[3]
    s_attn, s_o, s_act, s_f2 = seeds
    p_h, p_a, p_act, eps, x, g = cfg["p_hidden"], cfg["p_attn"], cfg["p_act"], cfg["eps"], cfg["x"], cfg["cot"]
    G = {n: (torch.zeros_like(t) if mutant == "main_grad_overwritten" else t.clone()) for n, t in cfg["grads0"].items() if n not in cfg["frozen"]}
    keep = cfg["keep_rows"]
    keep32 = None if keep is None else keep.to(torch.int32)
    hook = {}

    def gather(src, first_rows=False):
        if keep is None:
            return src
        idx = torch.arange(keep.numel(), dtype=torch.int32) if first_rows else keep32
        return M.rows(torch.zeros(keep.numel(), src.shape[1], dtype=src.dtype), a=src, ai=idx)

    def spread(g_):
        if keep is None:
            return g_
        idx = torch.sort(keep32).values if mutant == "spread_sorted_keep_rows" else keep32
        return M.rows(torch.zeros(cfg["rows"], g_.shape[1], dtype=g_.dtype), a=g_, di=idx)

    def ln(t, n):
        return M.ln_fwd(t, P[n + "_w"], P[n + "_b"], eps)

    # ---- forward
    if pre:
        a_in, m1, r1 = ln(x, "ln1")
    else:
        a_in = x
    qkv = M.gemm(a_in, P["qkv_w"], bias=P["qkv_b"])
    ctx_full, lse = M.attn_fwd(qkv, p_a, s_attn)
    ctx, xk = gather(ctx_full), gather(x, first_rows=mutant == "gather_x_first_rows")
    t = M.gemm(ctx, P["o_w"], bias=P["o_b"], residual=xk, drop_p=p_h, drop_seed=s_o)
    if pre:
        f_in, m2, r2 = ln(t, "ln2")
    else:
        f_in, m1, r1 = ln(t, "ln1")
    if cfg["act"] == "gelu":
        h, u = M.gemm(f_in, P["fc1_w"], bias=P["fc1_b"], aux=torch.zeros(f_in.shape[0], cfg["F"], dtype=cfg["dtype"]), epilogue=GR.EPI_GELU | GR.EPI_AUX_GRAD,
                      drop_p=p_act, drop_seed=s_act)
    else:
        h, u = M.act_fwd(M.gemm(f_in, P["fc1_w"], bias=P["fc1_b"]), cfg["act"], p_act, s_act, scale_u=mutant != "u_without_act_dropout_scale")
    y = M.gemm(h, P["fc2_w"], bias=P["fc2_b"], residual=t if pre else f_in, drop_p=p_h, drop_seed=s_f2)
    if pre:
        out = y
    else:
        out, m2, r2 = ln(y, "ln2")

    # ---- backward
    rides = bf and cfg["rows_out"] >= 8192

    def wgrad(dy, xin, n, bias):
        bias = bias if bias in G else None                      # a frozen bias has no buffer
        if n == "qkv" and mutant == "hook_before_last_grad":
            hook["snap"] = {k: v.clone() for k, v in G.items()}
        ride = bias is not None and bf
        M.gemm(dy, xin, trans_a=True, trans_b=True, out=G[n + "_w"], epilogue=GR.EPI_ATOMIC, split_k=T.split_k(dy.shape[1], xin.shape[1], dy.shape[0]),
               asum=G[bias] if ride else None)
        if bias is not None and not ride:
            M.colsum(dy, G[bias])

    def ln_bwd_dense(dy, xin, n, mean, rstd, bias, seed, add=None):
        return M.ln_bwd(dy, xin, P[n + "_w"], mean, rstd, add=add, dgamma=G[n + "_w"], dbeta=G[n + "_b"], drop_p=p_h, drop_seed=seed,
                        colsum=G.get(bias), want_dropped=True)

    def ffn_bwd(gd, fc2_b, dres):
        if mutant == "frozen_bias_still_summed":
            G["fc1_b"] = torch.zeros(cfg["F"])
        wgrad(gd, h, "fc2", fc2_b)
        du = M.gemm(gd, P["fc2_w"], trans_b=True, aux=u, epilogue=GR.EPI_MULAUX, colsum=G.get("fc1_b"))
        wgrad(du, t if mutant == "fc1_wgrad_reads_t" else f_in, "fc1", None)
        return M.gemm(du, P["fc1_w"], trans_b=True, residual=None if mutant == "post_ffn_bwd_without_dres" else dres)

    def attn_bwd(dt_, dtd, o_b, want_dx, dres=None):
        wgrad(dt_ if mutant == "o_wgrad_reads_dt" else dtd, ctx, "o", "o_b" if mutant == "bias_owned_twice" else o_b)
        dctx = M.gemm(dtd, P["o_w"], trans_b=True)
        saved = ctx_full
        if mutant == "attn_bwd_gets_gathered_ctx":
            saved = torch.zeros_like(ctx_full)
            saved[:ctx.shape[0]] = ctx
        tabs = dict(d_sp_table=G["sp_table"], d_virt=G["virt"].view(-1)) if "sp_table" in P else {}
        dqkv = M.attn_bwd(spread(dctx), qkv, saved, lse, p_a, s_attn, **tabs)
        wgrad(dqkv, x if mutant == "pre_qkv_wgrad_reads_x" else a_in, "qkv", "qkv_b")
        if not want_dx:
            return None
        return M.gemm(dqkv, P["qkv_w"], trans_b=True, residual=None if dres is None else spread(dres))

    o_owner = None if (rides or mutant == "bias_owned_by_nobody") else "o_b"
    dx = None
    if not pre:
        dy, dyd = ln_bwd_dense(g, y, "ln2", m2, r2, None if rides else "fc2_b", s_f2)
        df = ffn_bwd(dyd, "fc2_b" if rides else None, dy)
        dt_, dtd = ln_bwd_dense(df, t, "ln1", m1, r1, o_owner, s_f2 if mutant == "ln1_tail_uses_s_f2" else s_o)
        dx = attn_bwd(dt_, dtd, "o_b" if rides else None, cfg["x_needs_grad"], dt_)
    else:
        gd = M.dropout(g, p_h, s_f2) if (p_h > 0 and mutant != "pre_ln_skips_dropout_g") else g
        df = ffn_bwd(gd, "fc2_b", None)
        dt_, dtd = ln_bwd_dense(df, t, "ln2", m2, r2, o_owner, s_o, add=None if mutant == "pre_ln2_bwd_without_add" else g)
        da = attn_bwd(dt_, dtd, "o_b" if rides else None, True)
        add = spread(dt_) if cfg["x_needs_grad"] else None
        dx, _ = M.ln_bwd(da, x, P["ln1_w"], m1, r1, add=add, dgamma=G["ln1_w"], dbeta=G["ln1_b"])
        if not cfg["x_needs_grad"]:
            dx = None
    if mutant == "ln_params_in_each_others_buffers":
        for k in "wb":
            G["ln1_" + k], G["ln2_" + k] = G["ln2_" + k], G["ln1_" + k]
    snap = hook.get("snap", G)
    grads = {n: G.get(n) for n in P}
    return dict(cfg=cfg, launches=M.launches, tape_seeds=seeds, y=out, dx=dx, grads=grads, atomics=None,
                hook=[dict(all_params=True, snap={n: (snap[n].clone() if n in snap else None) for n in BR.PARAMS})])


# ------------------------------------------------------------------------------------------------ accepted
ACCEPTED = {   # name -> make_case arguments
    **{f"{shape}-{'bf16' if dt == bf16 else 'fp32'}-{'pre' if pre else 'post'}": ((shape, dt, pre), dict(act="relu") if shape == "G" else {})
       for shape in ("S", "G") for dt in (f32, bf16) for pre in (False, True)},
    "R8192-bf16-post": (("R8192", bf16, False), {}),
    "R8191-bf16-post": (("R8191", bf16, False), {}),
    "R8192-bf16-pre": (("R8192", bf16, True), {}),
    "S-bf16-post-keep_rows": (("S", bf16, False), dict(keep=True)),
    "S-bf16-pre-keep_rows": (("S", bf16, True), dict(keep=True)),
    "S-fp32-pre-x-frozen": (("S", f32, True), dict(x_needs_grad=False)),
    "S-bf16-post-main_grad": (("S", bf16, False), dict(main_grad=True)),
    "Sr-bf16-pre-ragged": (("Sr", bf16, True), {}),
    "S-fp32-post-no-dropout": (("S", f32, False), dict(drop=False)),
    "S-fp32-post-biases-frozen": (("S", f32, False), dict(frozen=("qkv_b", "o_b", "fc1_b", "fc2_b"))),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_model_is_accepted(name):
    """All three layers accept the model — with every non-vacuity cap of the sum checks in force — and every launch it records
    has a role and a reference.  Prints the worst end-to-end value: in bf16 the measurement behind BF16_E2E_MEASURED."""
    args, kw = ACCEPTED[name]
    trace = model_block(T.make_case(*args, **kw))
    roles = T.check_wiring(trace)
    assert T.check_launches(trace, roles) == len(trace["launches"]) == len(roles)
    rows = T.check_end_to_end(trace, tag="model " + name)
    print(f"accepted: {name} ({len(roles)} launches); worst end-to-end {rows[0][0]} {rows[0][1]:.3e} (gate {rows[0][2]:.1e})")
    if args[1] == bf16:
        assert rows[0][1] <= T.BF16_E2E_MEASURED[args[0][0]], f"{name}: the model itself reaches {rows[0][1]:.3e}: BF16_E2E_MEASURED is out of date"


# ------------------------------------------------------------------------------------------------ rejected
LAUNCH, WIRING, E2E = "launch", "wiring", "end_to_end"
MUTANTS = {   # mutant -> (make_case arguments, the layers that must reject it, whether it changes values)
    "bias_owned_twice": ((("S", bf16, False), {}), (WIRING, E2E), True),                    # LayerNorm colsum AND asum for o_b
    "bias_owned_by_nobody": ((("S", f32, False), {}), (WIRING, E2E), True),
    "ln1_tail_uses_s_f2": ((("S", f32, False), {}), (WIRING, E2E), True),
    "s_o_equals_s_f2": ((("S", f32, False), {}), (WIRING,), False),                         # consistent forward and backward: only the seeds tell
    "pre_ln_skips_dropout_g": ((("S", f32, True), {}), (WIRING, E2E), True),
    "u_without_act_dropout_scale": ((("G", f32, False), dict(act="relu")), (LAUNCH, E2E), True),
    "pre_ln2_bwd_without_add": ((("S", f32, True), {}), (WIRING, E2E), True),
    "post_ffn_bwd_without_dres": ((("S", f32, False), {}), (WIRING, E2E), True),
    "o_wgrad_reads_dt": ((("S", f32, False), {}), (WIRING, E2E), True),
    "fc1_wgrad_reads_t": ((("S", f32, True), {}), (WIRING, E2E), True),
    "pre_qkv_wgrad_reads_x": ((("S", f32, True), {}), (WIRING, E2E), True),
    "attn_bwd_gets_gathered_ctx": ((("S", bf16, False), dict(keep=True)), (LAUNCH, WIRING, E2E), True),
    "spread_sorted_keep_rows": ((("S", bf16, True), dict(keep=True)), (WIRING, E2E), True),
    "gather_x_first_rows": ((("S", bf16, False), dict(keep=True)), (WIRING, E2E), True),
    "ln_params_in_each_others_buffers": ((("S", f32, False), {}), (WIRING, E2E), True),
    "main_grad_overwritten": ((("S", bf16, False), dict(main_grad=True)), (WIRING, E2E), True),
    "hook_before_last_grad": ((("S", f32, False), {}), (WIRING,), False),
    "frozen_bias_still_summed": ((("S", f32, False), dict(frozen=("qkv_b", "o_b", "fc1_b", "fc2_b"))), (WIRING,), False),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_rejected(mutant):
    (args, kw), layers, changes_values = MUTANTS[mutant]
    trace = model_block(T.make_case(*args, **kw), mutant)
    said = {}
    for layer, run in ((WIRING, lambda: T.check_wiring(trace)), (LAUNCH, lambda: T.check_launches(trace)), (E2E, lambda: T.check_end_to_end(trace, tag=mutant))):
        try:
            run()
        except AssertionError as e:
            said[layer] = str(e).splitlines()[0][:160]
    print(f"rejected: {mutant} by " + "; ".join(f"{k} ({v})" for k, v in said.items()))
    assert set(layers) <= set(said), f"{mutant}: expected {layers} to reject it, {sorted(said)} did"
    if changes_values:
        worst = max(e / gate for _, e, gate in T.e2e_rows(trace, T.block_reference(trace)))
        assert worst >= 10.0, f"{mutant}: the worst tensor is only {worst:.2f} x its end-to-end gate"
