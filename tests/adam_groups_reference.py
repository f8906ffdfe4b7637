"""Reference of the parameter-group forms of the Adam step (csrc/optim.hip, include/mdt_hip.h: mdt_adam_group,
mdt_adam_step_multi_groups, mdt_adam_step_group) and the inputs of tests/test_adam_groups_gpu.py.  Pure torch: no device, no native
library.

There is NO second error model here.  The header pins what the group form hands the one Adam update per tensor:

    lr_t        = lr * lr_scale                 one fp32 product
    step_size_t = step_size * lr_scale          one fp32 product; step_size is the host's adam_step_size(), or the guard state's
                                                once an update has been skipped
    wd_t        = weight_decay of the record

so the reference of tensor t is tests/loss_optim_reference.py's reference_adam() called with (lr_t, wd_t) and, through its ``guard``
argument — the one way it takes a step size as given — with step_size_t and the effective gradient scale.  Those three numbers are
fp32 numbers the kernel holds in registers: they carry no δ, and reference_adam's per-element bound is used unchanged.  (Its
``wd lr`` product is then f32(wd_t) * f32(lr_t), the kernel's ``wd * lr * p`` evaluated left to right.)

Consequences the reference shows by itself: lr_scale == 1 gives lr_t == lr and step_size_t == step_size, the plain call;
lr_scale == 0 gives p' = p with δ = 0 (both subtrahends are exact zeros) while m and v advance.
"""
from __future__ import annotations

import numpy as np
import torch

import tests.loss_optim_reference as R
from tests.loss_optim_reference import f32v

HYP = R.RECIPE
GLOBAL_WD = HYP["wd"]
STEP, GS = 3, 0.37
CHUNK = R.CHUNK
SEED = 5231

# one table: a chunk tail of every kind; 4097 and 2 * 4096 + 3 own several chunks (a record indexed by chunk goes wrong there)
NUMELS = (1, 255, 256, 4095, 4096, 4097, 2 * 4096 + 3)
# (lr_scale, weight_decay) per tensor, all distinct: the trivial record, torch's lr = 0 group, a power of two without decay, scales
# that round (0.37, 0.81, 0.043) and one above 1, decays below, at and above the global value.  The last record has a decay and a
# scale far from those of records 0 .. 2, which a chunk-indexed lookup would hand its three chunks.
RECORDS = ((1.0, GLOBAL_WD), (0.0, 0.0), (0.5, 0.0), (0.37, 0.05), (0.81, 0.0), (1.7, 0.02), (0.043, 0.3))
ZERO_TENSOR = 1                                 # the tensor with lr_scale == 0
BIG_TENSORS = 65540                             # one-element tensors: more chunks than the launch's grid of 65 536
BIG_RECORDS = ((0.5, 0.0), (1.7, 0.3))          # alternating

GUARDS = {"unguarded": None, "clipped": dict(R.ADAM_GUARDS)["clipped"], "after_skips": dict(R.ADAM_GUARDS)["after_skips"],
          "skip": dict(R.ADAM_GUARDS)["skip"]}


def segments(numels):
    return np.concatenate([[0], np.cumsum(numels)]).astype(np.int64)


def table_inputs(numels=NUMELS, seed=SEED):
    """(p0, grad, m0, v0) fp32 [sum(numels)]: adam_inputs of tests/loss_optim_reference.py over the whole table, with the
    parameters of the first half of every tensor of 255 elements or more raised to 1e1 .. 1e2: there the decay term wd lr p is
    large against the bound of the Adam term, so a wrong decay is seen whatever m / sqrt(v) happens to be."""
    total = int(sum(numels))
    p0, grad, m0, v0 = R.adam_inputs(total, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    seg = segments(numels)
    for a, b in zip(seg[:-1], seg[1:]):
        n = int(b - a)
        if n >= 255:
            h = n // 2
            p0[a:a + h] = R._spread(h, gen, 1, 2) * R._signs(h, gen)
            m0[a:a + h] = R._spread(h, gen, -9, -6) * R._signs(h, gen)       # a small Adam term: |m| <= 1e-6 ...
            v0[a:a + h] = R._spread(h, gen, -8, -2)                          # ... over sqrt(v) >= 1e-4
            grad[a:a + h] = R._spread(h, gen, -8, -5) * R._signs(h, gen)
    return p0, grad, m0, v0


def group_hyper(hyp, step, scale, guard=None):
    """(lr_t, step_size_t) as fp32 numbers: the two products the header pins."""
    base = R.adam_step_size(hyp["lr"], hyp["beta1"], hyp["beta2"], step)
    if guard is not None and guard["skipped"]:
        base = f32v(guard["step_size"])
    return float(np.float32(hyp["lr"]) * np.float32(scale)), float(np.float32(base) * np.float32(scale))


def reference_tensor(p0, grad, m0, v0, hyp, step, record, gs=None, guard=None):
    """reference_adam for one tensor under its record (lr_scale, weight_decay)."""
    scale, wd = record
    lr_t, ss_t = group_hyper(hyp, step, scale, guard)
    eff = dict(scale=1.0 if gs is None else gs, skip=0, skipped=1, step_size=ss_t)
    if guard is not None:
        eff.update(scale=guard["scale"], skip=guard["skip"])
    return R.reference_adam(p0, grad, m0, v0, lr_t, hyp["beta1"], hyp["beta2"], hyp["eps"], wd, step, None, eff)


def reference_table(inputs, numels, records, hyp, step, gs=None, guard=None):
    """{"m", "v", "p"}: (value, δ) over the flat table, tensor t under records[t]."""
    # the update is elementwise: the elements of all tensors that share a record go through reference_adam in one call
    distinct = list(dict.fromkeys(tuple(r) for r in records))
    number = {r: k for k, r in enumerate(distinct)}
    of_tensor = np.asarray([number[tuple(r)] for r in records], dtype=np.int64)
    of_element = torch.from_numpy(np.repeat(of_tensor, np.asarray(numels, dtype=np.int64)))
    total = int(of_element.numel())
    out = {k: (torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)) for k in "mvp"}
    for r, record in enumerate(distinct):
        idx = torch.nonzero(of_element == r).view(-1)
        if idx.numel() == 0:
            continue
        ref = reference_tensor(*(x[idx] for x in inputs), hyp, step, record, gs, guard)
        for k in "mvp":
            out[k][0][idx], out[k][1][idx] = ref[k][0], ref[k][1]
    return out


def guard_words(gname, hyp=HYP, step=STEP):
    return None if GUARDS[gname] is None else R.adam_guard(GUARDS[gname], hyp, step)


def records_array(records):
    return np.asarray(records, dtype=np.float32).reshape(len(records), 2)
