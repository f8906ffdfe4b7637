"""Optimiser + LR schedule of the reference launch (FairSeq `adam` + `polynomial_decay`,
mDT/experiments/hateful_discussions/run_train.sh:38-40), fused: one HIP kernel per parameter
tensor reads the fp32 gradient arena and updates moments, fp32 master weights and the
working-precision parameter in a single pass.

``clip_norm`` (FairSeq ``--clip-norm``) adds the global gradient norm on the device: one deterministic read of the
gradients (no atomics), a one-block finaliser that writes the guard state — gnorm, the effective gradient scale, the
skip flag of a non-finite update, running counters — and Adam kernels that read their scale from it.  Nothing of it
synchronises with the host.

``ema_decay`` (FairSeq ``--store-ema``) keeps an fp32 exponential moving average of the weights in one flat arena.  The
average is updated by the Adam launch itself (the ``_ema`` entry points: the fresh fp32 value is in a register, a skipped
update leaves the average alone); ``ema_weights()`` swaps it into the working parameters for an evaluation and back.

Parameter groups (torch-style ``[{"params": [...], "lr_scale": 0.5, "weight_decay": 0.0}, ...]``) give a tensor its own rate
scale and weight decay inside the SAME launches: a float32 ``[n, 2]`` device array parallel to the table (include/mdt_hip.h:
mdt_adam_group) and the ``_groups`` / ``_group`` entry points.  The norm pass, the guard and the EMA arena are shared by all
groups; an optimiser whose parameters all have (1, the constructor's weight decay) issues exactly the entry points of one
without groups."""
from __future__ import annotations

import contextlib
from typing import NamedTuple, Optional

import numpy as np
import torch

from ._lib import check, dt, lib, ptr, stream


class Table(NamedTuple):
    """The parameters of one dtype as the one-launch kernels read them (include/mdt_hip.h: mdt_adam_tensor)."""
    rec: torch.Tensor                      # int64 [n, 6] on the device: param, master or 0, grad or 0, m, v, numel
    first: torch.Tensor                    # int64 [n + 1] on the device: first 4096-element chunk of each tensor, first[n] = total
    n: int
    total: int
    params: list
    grad_ptrs: list                        # the gradient address each record was built from (0: a table without gradients)
    ema_ptrs: Optional[torch.Tensor]       # int64 [n] on the device: the averages in table order (None: no average is kept)
    groups: Optional[torch.Tensor] = None  # float32 [n, 2] on the device: (lr_scale, weight_decay) per tensor (None: all trivial)


class FusedAdam:
    def __init__(self, params, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, multi_tensor=True, clip_norm=None,
                 ema_decay=None, ema_start_update=0, ema_update_freq=1):
        """``clip_norm=None``: no norm pass, the unguarded kernels.  A number (0 included): the guarded path — gnorm is
        measured, a non-finite update is skipped, and gradients are clipped to that norm when it is > 0.

        ``ema_decay=None``: no average, nothing allocated, the launches of a plain optimiser.  A number in [0, 1]: update
        ``k`` (``num_updates`` of ``step``, by default the count of ``step`` calls) with ``k % ema_update_freq == 0`` also
        does ``ema = d ema + (1 - d) p`` in the Adam kernel, d = 0 while ``k < ema_start_update`` (FairSeq: the average is
        a copy of the weights until then) and ``ema_decay`` afterwards; every other update is the plain launch."""
        params = list(params)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self._hyper = {}                          # id(parameter) -> (lr_scale, weight_decay) where a group was given
        self._has_groups = (None, False)          # (the weight decay it was worked out for, has_groups)
        if params and isinstance(params[0], dict):
            flat = []
            for k, g in enumerate(params):
                unknown = set(g) - {"params", "lr_scale", "weight_decay"}
                if unknown or "params" not in g:
                    raise ValueError(f"FusedAdam: group {k} has unknown keys {sorted(unknown)} or no 'params' (params, lr_scale, weight_decay)")
                scale, wd = float(g.get("lr_scale", 1.0)), float(g.get("weight_decay", weight_decay))
                if not (np.isfinite(scale) and scale >= 0.0 and np.isfinite(wd) and wd >= 0.0):
                    raise ValueError(f"FusedAdam: group {k}: lr_scale {scale!r} and weight_decay {wd!r} must be finite and >= 0")
                for p in g["params"]:
                    if id(p) in self._hyper:
                        raise ValueError(f"FusedAdam: a parameter of shape {tuple(p.shape)} appears in more than one group (group {k})")
                    self._hyper[id(p)] = (scale, wd)
                    flat.append(p)
            params = flat
        self.params = [p for p in params if p.requires_grad]
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.norm_launches = 0                    # sum-of-squares and finaliser launches issued so far (tests)
        self._guard = self._partials = None
        self.step_count = 0
        self.multi_tensor = multi_tensor          # False: one launch per tensor (tests compare the two)
        self.state = {}
        for p in self.params:
            st = dict(m=torch.zeros(p.shape, dtype=torch.float32, device=p.device),
                      v=torch.zeros(p.shape, dtype=torch.float32, device=p.device))
            if p.dtype != torch.float32:
                st["master"] = p.detach().float().clone()
            self.state[id(p)] = st
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_start_update, self.ema_update_freq = int(ema_start_update), int(ema_update_freq)
        self.ema_arena = None
        self._tab, self._outside = None, self.params        # the step's tables by dtype, and the parameters they leave out
        self._swap_tab, self._in_ema = None, False
        if self.ema_decay is not None:
            if not 0.0 <= self.ema_decay <= 1.0 or self.ema_update_freq < 1:
                raise ValueError(f"FusedAdam: ema_decay {ema_decay!r} must lie in [0, 1] and ema_update_freq {ema_update_freq!r} be >= 1")
            # one flat fp32 arena, a slot per parameter on a 16-byte boundary, seeded from the master (or the fp32 parameter)
            offs, n = [], 0
            for p in self.params:
                offs.append(n)
                n += (p.numel() + 3) // 4 * 4
            self.ema_arena = torch.zeros(max(n, 1), dtype=torch.float32, device=self.params[0].device if self.params else "cpu")
            for p, off in zip(self.params, offs):
                self.state[id(p)]["ema"] = self.ema_arena[off:off + p.numel()].view(p.shape)
            self.seed_ema_from_weights()

    def _fp32_source(self, p):
        """The fp32 weights of ``p``: its master, or the parameter itself where there is none."""
        st = self.state[id(p)]
        return st["master"] if "master" in st else p.detach().float()

    def hyper_of(self, p):
        """(lr_scale, weight_decay) of parameter ``p``: its group's, or (1, the optimiser's weight decay)."""
        return self._hyper.get(id(p), (1.0, float(self.weight_decay)))

    def _grouped(self, p):
        """True where ``p`` needs the group entry points: the fp32 numbers the kernel would get differ from (1, global)."""
        scale, wd = self.hyper_of(p)
        return np.float32(scale) != np.float32(1.0) or np.float32(wd) != np.float32(self.weight_decay)

    @property
    def has_groups(self):
        """True where any parameter differs from (1, the optimiser's weight decay): the step then issues the group entry points."""
        key = float(self.weight_decay)
        if self._has_groups[0] != key:
            self._has_groups = (key, any(self._grouped(p) for p in self.params))
        return self._has_groups[1]

    @property
    def param_groups(self):
        """torch-style view: one dict per distinct (lr_scale, weight_decay) in order of first appearance, ``lr`` = base x scale."""
        out = {}
        for p in self.params:
            key = self.hyper_of(p)
            if key not in out:
                out[key] = {"params": [], "lr": self.lr * key[0], "lr_scale": key[0], "weight_decay": key[1],
                            "betas": tuple(self.betas), "eps": self.eps}
            out[key]["params"].append(p)
        return list(out.values())

    def _build_tables(self, params, with_grads):
        """{dtype: Table} over ``params`` in their order; ``with_grads``: the records point at ``p.main_grad``."""
        groups = {}
        for p in params:
            groups.setdefault(p.dtype, []).append(p)
        tab = {}
        for dtype, ps in groups.items():
            gptrs = [p.main_grad.data_ptr() if with_grads else 0 for p in ps]
            rec = np.zeros((len(ps), 6), dtype=np.int64)
            first = np.zeros(len(ps) + 1, dtype=np.int64)
            for i, p in enumerate(ps):
                st = self.state[id(p)]
                rec[i] = (p.data.data_ptr(), st["master"].data_ptr() if "master" in st else 0, gptrs[i], st["m"].data_ptr(),
                          st["v"].data_ptr(), p.numel())
                first[i + 1] = first[i] + (p.numel() + 4095) // 4096
            dev = ps[0].device
            ema = None
            if self.ema_decay is not None:
                ema = torch.from_numpy(np.asarray([self.state[id(p)]["ema"].data_ptr() for p in ps], dtype=np.int64)).to(dev)
            grp = None
            if with_grads and any(self._grouped(p) for p in ps):
                grp = torch.from_numpy(np.asarray([self.hyper_of(p) for p in ps], dtype=np.float32).reshape(len(ps), 2)).to(dev)
            tab[dtype] = Table(torch.from_numpy(rec).to(dev), torch.from_numpy(first).to(dev), len(ps), int(first[-1]), ps, gptrs, ema, grp)
        return tab

    def _tables(self):
        """Device tables for the one-launch update: parameters of one dtype whose gradients live in the fp32 ``main_grad``
        arena.  Others (``_outside``) take one launch per tensor.  Built once, and again when a ``main_grad`` moved: the views
        move when the DDP arena is re-laid-out after the first step."""
        if not self.multi_tensor:
            return {}
        if self._tab is None or any([p.main_grad.data_ptr() for p in t.params] != t.grad_ptrs for t in self._tab.values()):
            inside = [p for p in self.params if getattr(p, "main_grad", None) is not None and p.main_grad.is_contiguous()
                      and p.data.is_contiguous()]
            self._tab = self._build_tables(inside, True)
            ids = {id(p) for p in inside}
            self._outside = [p for p in self.params if id(p) not in ids]
        return self._tab

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
        for t in tables.values():
            check(lib.mdt_grad_sumsq_multi(stream(), t.n, ptr(t.rec), ptr(t.first), t.total, ptr(partials[n:])), "mdt_grad_sumsq_multi")
            n += t.total
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

    def step(self, lr=None, grad_scale: torch.Tensor = None, num_updates: int = None):
        """Gradients are read from ``p.main_grad`` (fp32 arena) or ``p.grad``; ``grad_scale`` is an optional
        fp32 device scalar multiplied into every gradient.  Never synchronises with the host.  ``num_updates``: the
        trainer's count including this update, which the EMA schedule follows (default: the count of ``step`` calls)."""
        if self._in_ema:
            raise RuntimeError("FusedAdam.step() inside ema_weights(): the parameters hold the averaged weights")
        self.step_count += 1
        lr = self.lr if lr is None else lr
        ema = None                                # None: the plain launches; a number: the decay of this update's _ema launches
        if self.ema_decay is not None:
            k = self.step_count if num_updates is None else int(num_updates)
            if k % self.ema_update_freq == 0:
                ema = 0.0 if k < self.ema_start_update else self.ema_decay
        tables = self._tables()
        rest = list(self._rest())
        guard = self._norm_pass(lr, grad_scale, tables, rest) if self.clip_norm is not None else None
        hyper = (float(lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay), self.step_count)
        for t in tables.values():
            self._adam(True, (stream(), dt(t.params[0]), t.n, ptr(t.rec), ptr(t.first), t.total, *hyper), grad_scale, guard,
                       () if ema is None else (ptr(t.ema_ptrs), ema), None if t.groups is None else (ptr(t.groups),))
        grouped = self.has_groups               # then every per-tensor launch is the group form, trivial records included
        for p, g in rest:
            st = self.state[id(p)]
            self._adam(False, (stream(), dt(p), p.numel(), ptr(p.data), ptr(st.get("master")), ptr(g), ptr(st["m"]), ptr(st["v"]), *hyper),
                       grad_scale, guard, () if ema is None else (ptr(st["ema"]), ema), self.hyper_of(p) if grouped else None)
        from . import engine
        engine.weights_changed()                 # copies derived from the weights (engine._k_padded, fp8.Fp8State.weight) are stale now

    @staticmethod
    def _adam(multi, head, grad_scale, guard, ema_tail, group=None):
        """One Adam launch.  ``head``: the arguments up to ``step``; then the guard state where there is one, else the optional
        gradient scale; then ``ema_tail`` (averages, decay) or nothing.  ``group``: None, or what the group form takes after
        ``step`` — (records,) of a table, (lr_scale, weight_decay) of one tensor; that form has the global weight decay taken
        out of ``head`` and both of gradient scale and guard, averages and decay as nullable arguments.  The entry point is
        looked up in ``lib`` by its name, at the call."""
        if group is not None:
            name = "mdt_adam_step_multi_groups" if multi else "mdt_adam_step_group"
            check(getattr(lib, name)(*head[:-2], head[-1], *group, ptr(grad_scale) if guard is None else None, ptr(guard),
                                     *(ema_tail or (None, 0.0))), name)
            return
        name = "mdt_adam_step" + ("_multi" if multi else "") + ("_ema" if ema_tail else "") + ("" if guard is None else "_guarded")
        check(getattr(lib, name)(*head, ptr(grad_scale if guard is None else guard), *ema_tail), name)

    def _rest(self):
        """(parameter, contiguous fp32 gradient) of every parameter the tables do not cover and that has a gradient."""
        for p in self._outside:
            g = getattr(p, "main_grad", None)
            if g is None:
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32:
                    g = g.float()
            yield p, g.contiguous()

    # -- the weight average (FairSeq --store-ema)
    def _need_ema(self):
        if self.ema_decay is None:
            raise RuntimeError("FusedAdam(ema_decay=None) keeps no weight average: construct it with ema_decay=<decay>")

    def _ema_entries(self, model):
        """(state-dict key, fp32 view into the EMA arena) of every state-dict entry of ``model`` that is a trainable
        parameter of this optimiser or a row slice of one (the fused q/k/v parameter is saved as its three parts, as
        checkpoint.py saves the weights)."""
        spans = []
        for p in self.params:
            beg = p.data.data_ptr()
            spans.append((beg, beg + p.numel() * p.element_size(), p))
        for k, v in model.state_dict().items():
            for beg, end, p in spans:
                if beg <= v.data_ptr() < end and v.dtype == p.dtype:
                    off = (v.data_ptr() - beg) // p.element_size()
                    e = self.state[id(p)]["ema"]      # the entry's own view (a transposed adapter slice is strided) of the average
                    yield k, e.as_strided(tuple(v.shape), tuple(v.stride()), e.storage_offset() + off)
                    break

    def ema_state_dict(self, model):
        """The averaged weights as fp32 CPU tensors under ``model``'s state-dict keys (trainable entries only)."""
        self._need_ema()
        from collections import OrderedDict
        return OrderedDict((k, e.detach().cpu().clone()) for k, e in self._ema_entries(model))

    def load_ema_state_dict(self, model, sd):
        """Inverse of ``ema_state_dict``: every trainable entry must be there with its shape (a missing key raises, as a
        strict model load does); entries of ``sd`` that are no trainable entry of the model raise as unexpected."""
        self._need_ema()
        if self._in_ema:
            raise RuntimeError("FusedAdam.load_ema_state_dict() inside ema_weights()")
        want = dict(self._ema_entries(model))
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if missing or unexpected:
            raise RuntimeError(f"EMA state dict: missing keys {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                               f"unexpected keys {unexpected[:8]}")
        for k, e in want.items():
            if tuple(sd[k].shape) != tuple(e.shape):
                raise ValueError(f"EMA state dict: shape of {k} is {tuple(sd[k].shape)}, the model expects {tuple(e.shape)}")
            e.copy_(sd[k])

    def seed_ema_from_weights(self):
        """The average restarts as a copy of the current weights (the masters where there are any)."""
        self._need_ema()
        for p in self.params:
            self.state[id(p)]["ema"].copy_(self._fp32_source(p))

    def _all_tables(self):
        """Tables of the swap launch: EVERY parameter of the optimiser by dtype, no gradients (the step's tables leave out what
        has no ``main_grad``), rebuilt when a parameter's storage moved."""
        now = [p.data.data_ptr() for p in self.params]
        if self._swap_tab is None or self._swap_tab[0] != now:
            if not all(p.data.is_contiguous() for p in self.params):
                raise RuntimeError("FusedAdam.ema_weights(): a parameter is not contiguous")
            self._swap_tab = (now, self._build_tables(self.params, False))
        return self._swap_tab[1]

    def _swap(self, restore):
        for t in self._all_tables().values():
            check(lib.mdt_ema_swap_multi(stream(), dt(t.params[0]), t.n, ptr(t.rec), ptr(t.ema_ptrs), ptr(t.first), t.total, int(restore)),
                  "mdt_ema_swap_multi")
        from . import engine
        engine.weights_changed()                 # both ends: the cached weight copies (fp8, zero-padded) are stale

    @contextlib.contextmanager
    def ema_weights(self):
        """The working parameters hold the averaged weights inside the context (one swap launch per dtype at each end) and
        their own bits after it.  No ``step()`` and no nesting inside."""
        self._need_ema()
        if self._in_ema:
            raise RuntimeError("FusedAdam.ema_weights() does not nest")
        self._swap(0)
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap(1)


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
