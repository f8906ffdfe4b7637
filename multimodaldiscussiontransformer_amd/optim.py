"""Optimiser + LR schedule of the reference launch (FairSeq `adam` + `polynomial_decay`,
mDT/experiments/hateful_discussions/run_train.sh:38-40), fused: one HIP kernel per parameter
tensor reads the fp32 gradient arena and updates moments, fp32 master weights and the
working-precision parameter in a single pass.

``clip_norm`` (FairSeq ``--clip-norm``) adds the global gradient norm on the device: one deterministic read of the
gradients (no atomics), a one-block finaliser that writes the guard state — gnorm, the effective gradient scale, the
skip flag of a non-finite update, running counters — and Adam kernels that read their scale from it.  Nothing of it
synchronises with the host."""
from __future__ import annotations

import torch

from ._lib import check, dt, lib, ptr, stream


class FusedAdam:
    def __init__(self, params, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, multi_tensor=True, clip_norm=None):
        """``clip_norm=None``: no norm pass, the unguarded kernels.  A number (0 included): the guarded path — gnorm is
        measured, a non-finite update is skipped, and gradients are clipped to that norm when it is > 0."""
        self.params = [p for p in params if p.requires_grad]
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.norm_launches = 0                    # sum-of-squares and finaliser launches issued so far (tests)
        self._guard = self._partials = None
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.step_count = 0
        self.multi_tensor = multi_tensor          # False: one launch per tensor (tests compare the two)
        self.state = {}
        for p in self.params:
            st = dict(m=torch.zeros(p.shape, dtype=torch.float32, device=p.device),
                      v=torch.zeros(p.shape, dtype=torch.float32, device=p.device))
            if p.dtype != torch.float32:
                st["master"] = p.detach().float().clone()
            self.state[id(p)] = st

    def _tables(self):
        """Device tables for the one-launch update, built once: parameters of one dtype whose gradients live in the
        fp32 ``main_grad`` arena (stable addresses).  Others fall back to one launch per tensor."""
        if not self.multi_tensor:
            return {}
        if getattr(self, "_tab", None) is not None:
            return self._tab
        import numpy as np
        groups = {}
        for p in self.params:
            g = getattr(p, "main_grad", None)
            if g is None or not g.is_contiguous() or not p.data.is_contiguous():
                continue
            groups.setdefault(p.dtype, []).append(p)
        tab = {}
        for dtype, ps in groups.items():
            rec = np.zeros((len(ps), 6), dtype=np.int64)
            first = np.zeros(len(ps) + 1, dtype=np.int64)
            for i, p in enumerate(ps):
                st = self.state[id(p)]
                rec[i] = (p.data.data_ptr(), st["master"].data_ptr() if "master" in st else 0, p.main_grad.data_ptr(),
                          st["m"].data_ptr(), st["v"].data_ptr(), p.numel())
                first[i + 1] = first[i] + (p.numel() + 4095) // 4096
            dev = ps[0].device
            tab[dtype] = (torch.from_numpy(rec).to(dev), torch.from_numpy(first).to(dev), len(ps), int(first[-1]),
                          {id(p) for p in ps}, ps, [p.main_grad.data_ptr() for p in ps])
        self._tab = tab
        return tab

    # -- guard state (include/mdt_hip.h: mdt_adam_guard — 8 words: scale, gnorm, step_size | skip, applied, clipped, skipped, -)
    def guard_buffers(self):
        """(guard state, partial sums) — allocated once, UNINITIALISED: the finaliser's first call starts the counters
        itself, and every partial the finaliser reads was written by that step's norm pass.  The partial buffer holds one
        slot per 4096-element chunk of every parameter, which no re-layout of the gradient arena changes."""
        if self._guard is None:
            dev = self.params[0].device
            self._guard = torch.empty(8, dtype=torch.float32, device=dev)
            self._partials = torch.empty(max(1, sum((p.numel() + 4095) // 4096 for p in self.params)), dtype=torch.float32, device=dev)
            self._guard_fresh = True
        return self._guard, self._partials

    def reset_guard(self):
        """The running counters restart from zero at the next step (a restored ``step_count`` counts applied updates)."""
        self._guard_fresh = True

    def _guard_word(self, i, as_int):
        if self.clip_norm is None:
            raise RuntimeError("FusedAdam(clip_norm=None) keeps no gradient norm: construct it with clip_norm=0 to measure without clipping")
        g = self.guard_buffers()[0]
        return (g.view(torch.int32) if as_int else g)[i]

    last_gnorm = property(lambda self: self._guard_word(1, False), doc="device scalar (fp32): gnorm of the last update")
    grad_scale_used = property(lambda self: self._guard_word(0, False), doc="device scalar (fp32): effective gradient scale of the last update")
    applied_steps = property(lambda self: self._guard_word(4, True), doc="device scalar (int32): updates applied")
    clipped = property(lambda self: self._guard_word(5, True), doc="device scalar (int32): updates clipped")
    skipped = property(lambda self: self._guard_word(6, True), doc="device scalar (int32): non-finite updates skipped")

    def guard_log_vector(self) -> torch.Tensor:
        """Device fp64 vector (gnorm, applied, clipped, skipped) for a caller that folds it into a sync of its own."""
        g = self.guard_buffers()[0]
        return torch.cat([g[1:2].double(), g.view(torch.int32)[4:7].double()])

    def guard_host(self) -> dict:
        """SYNCHRONISES with the device: gnorm of the last update and the running counters as Python numbers.  Before
        the first guarded step: the host's step count and zeros."""
        if self.clip_norm is None or self._guard is None or self._guard_fresh:
            return dict(gnorm=0.0, applied=self.step_count, clipped=0, skipped=0)
        v = self.guard_log_vector().tolist()
        return dict(gnorm=v[0], applied=int(v[1]), clipped=int(v[2]), skipped=int(v[3]))

    def applied_steps_host(self) -> int:
        """SYNCHRONISES with the device (guarded path): updates applied = attempts - skipped, Adam's ``step``."""
        return self.guard_host()["applied"]

    def _norm_pass(self, lr, grad_scale, tables, rest):
        """Sum of squares of every gradient the step will read → partials (table chunks first, then the per-tensor
        ones, in step order), then the one finaliser launch."""
        guard, partials = self.guard_buffers()
        n = 0
        for rec, first, nt, total, _, _, _ in tables.values():
            check(lib.mdt_grad_sumsq_multi(stream(), nt, ptr(rec), ptr(first), total, ptr(partials[n:])), "mdt_grad_sumsq_multi")
            n += total
            self.norm_launches += 1
        for p, g in rest:
            check(lib.mdt_grad_sumsq(stream(), g.numel(), ptr(g), ptr(partials[n:])), "mdt_grad_sumsq")
            n += (g.numel() + 4095) // 4096
            self.norm_launches += 1
        assert n <= partials.numel()
        check(lib.mdt_grad_norm_finalize(stream(), ptr(partials), n, self.clip_norm, ptr(grad_scale), float(lr), float(self.betas[0]),
                                         float(self.betas[1]), self.step_count, int(self._guard_fresh), ptr(guard)), "mdt_grad_norm_finalize")
        self.norm_launches += 1
        self._guard_fresh = False
        return guard

    def step(self, lr=None, grad_scale: torch.Tensor = None):
        """Gradients are read from ``p.main_grad`` (fp32 arena) or ``p.grad``; ``grad_scale`` is an optional
        fp32 device scalar multiplied into every gradient.  Never synchronises with the host."""
        self.step_count += 1
        lr = self.lr if lr is None else lr
        done = set()
        # main_grad views move when the DDP arena is re-laid-out after the first step: rebuild the tables then
        if getattr(self, "_tab", None) is not None and any(
                [p.main_grad.data_ptr() for p in ps] != gptrs for (_, _, _, _, _, ps, gptrs) in self._tab.values()):
            self._tab = None
        tables = self._tables()
        for (_, _, _, _, ids, _, _) in tables.values():
            done |= ids
        rest = list(self._rest(done))
        guard = self._norm_pass(lr, grad_scale, tables, rest) if self.clip_norm is not None else None
        for dtype, (rec, first, n, total, ids, _, _) in tables.items():
            head = (stream(), 0 if dtype == torch.float32 else 1, n, ptr(rec), ptr(first), total, float(lr), float(self.betas[0]),
                    float(self.betas[1]), float(self.eps), float(self.weight_decay), self.step_count)
            if guard is None:
                check(lib.mdt_adam_step_multi(*head, ptr(grad_scale)), "mdt_adam_step_multi")
            else:
                check(lib.mdt_adam_step_multi_guarded(*head, ptr(guard)), "mdt_adam_step_multi_guarded")
        self._step_rest(lr, grad_scale, rest, guard)
        from . import fp8
        if fp8.ACTIVE is not None:
            fp8.ACTIVE.optimizer_stepped()      # the cached 8-bit weight copies are stale now
        from . import engine
        engine.weights_changed()                # ... and the zero-padded copies the patch projection reads (engine._k_padded)

    def _rest(self, done):
        """(parameter, contiguous fp32 gradient) of every parameter the tables do not cover and that has a gradient."""
        for p in self.params:
            if id(p) in done:
                continue
            g = getattr(p, "main_grad", None)
            if g is None:
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32:
                    g = g.float()
            yield p, g.contiguous()

    def _step_rest(self, lr, grad_scale, rest, guard=None):
        for p, g in rest:
            st = self.state[id(p)]
            head = (stream(), dt(p), p.numel(), ptr(p.data), ptr(st.get("master")), ptr(g), ptr(st["m"]), ptr(st["v"]), float(lr),
                    float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay), self.step_count)
            if guard is None:
                check(lib.mdt_adam_step(*head, ptr(grad_scale)), "mdt_adam_step")
            else:
                check(lib.mdt_adam_step_guarded(*head, ptr(guard)), "mdt_adam_step_guarded")


class PolynomialDecayLR:
    """FairSeq ``polynomial_decay``: linear warm-up to ``lr`` over ``warmup_updates`` then
    (lr - end_lr) * (1 - progress)^power + end_lr until ``total_num_update``."""

    def __init__(self, lr=3e-5, end_lr=3e-7, warmup_updates=3246, total_num_update=10820, power=1.0):
        self.lr, self.end_lr, self.warmup, self.total, self.power = lr, end_lr, warmup_updates, total_num_update, power

    def for_update(self, k: int) -> float:
        """Learning rate update ``k`` (1-based) RUNS with under FairSeq's trainer.  FairSeq calls
        ``lr_scheduler.step_update(num_updates)`` after an update, so update k uses the rate of ``num_updates = k - 1``;
        before the first update the scheduler's constructor has set ``warmup_factor * lr`` with warmup_factor =
        1 / warmup_updates (fairseq/optim/lr_scheduler/polynomial_decay_schedule.py: __init__ and step_update)."""
        done = k - 1
        if done <= 0:
            return self.lr / self.warmup if self.warmup > 0 else self.lr
        return self(done)

    def __call__(self, num_updates: int) -> float:
        if self.warmup > 0 and num_updates <= self.warmup:
            return self.lr * num_updates / float(self.warmup)
        if num_updates >= self.total:
            return self.end_lr
        pct = 1 - (num_updates - self.warmup) / float(self.total - self.warmup)
        return (self.lr - self.end_lr) * pct ** self.power + self.end_lr
