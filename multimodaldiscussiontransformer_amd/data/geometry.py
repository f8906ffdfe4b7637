"""Row geometry of a batch: which row of the text, image and graph buffers holds what, as int32 index vectors.

Every row mover and sparse adjoint of engine.py is addressed through these vectors, so each rule is written once, here, in
torch arithmetic, which runs on host tensors as on device tensors: ``pack_batch`` and the encoder feed it the packer's host
arrays (in the prefetch thread: no kernel, no synchronisation) and upload the results with ``place``; a collated dict that
is already on the device feeds it device tensors and the results stay there.

Text: nb bottleneck tokens in front of every comment; comment m starts at m (nb + L) in the padded layout (every comment
owns nb + L rows) and at offsets[m] + m nb in the ragged one (only valid tokens own rows, data/packer.py RaggedText);
bottleneck token k sits at first + k, [CLS] at first + nb, token t at first + nb + t.  Image i owns Sv = nb + P rows from
i Sv, bottleneck tokens first.  Tree b owns T = N + 1 graph rows from b T: the graph token, then node n at b T + 1 + n.
"""
from __future__ import annotations

import torch

I32 = torch.int32


def _arange(n, device):
    return torch.arange(n, dtype=I32, device=device)


def bottleneck_rows(first: torch.Tensor, nb: int) -> torch.Tensor:
    """i32[n * nb]: the rows of the nb bottleneck tokens of the sequences whose first rows are ``first`` i32[n]."""
    return (first[:, None] + _arange(nb, first.device)[None]).reshape(-1).contiguous()


def graph_rows(B: int, N: int, device) -> torch.Tensor:
    """i32[B * N]: the graph row b T + 1 + n of node (b, n)."""
    return (_arange(B, device)[:, None] * (N + 1) + 1 + _arange(N, device)[None]).reshape(-1)


def degree_scatter(deg: torch.Tensor) -> torch.Tensor:
    """deg [B, N] → i32[B, T]: the degree-embedding row that graph row (b, t) feeds in backward; -1 for the graph token
    and for degree 0 (padding_idx: no gradient)."""
    d = deg.to(I32)
    return torch.cat([torch.full_like(d[:, :1], -1), torch.where(d > 0, d, torch.full_like(d, -1))], dim=1)


def csr_view(token_mask: torch.Tensor, in_degree: torch.Tensor) -> dict:
    """token_mask bool[B, N] (a real comment), in_degree [B, N] → the comment ↔ graph-row fields of a PackedBatch: node_row,
    graph_row, key_pad, deg_scatter.  One ``nonzero``: free on host tensors, the single synchronisation on device tensors."""
    B, N = token_mask.shape
    dev = token_mask.device
    real = torch.nonzero(token_mask.reshape(-1)).flatten()
    node_row = torch.full((B * N,), -1, dtype=I32, device=dev)
    node_row[real] = _arange(int(real.numel()), dev)
    key_pad = torch.cat([torch.zeros_like(token_mask[:, :1]), ~token_mask], dim=1).to(torch.uint8)    # the graph token is never padding
    return dict(node_row=node_row, graph_row=graph_rows(B, N, dev)[real], key_pad=key_pad,
                deg_scatter=degree_scatter(in_degree.reshape(B, N)).view(-1))


def first_rows(nb: int, M: int, L: int, offsets=None, device=None) -> torch.Tensor:
    """i32[M + 1]: the first row (bottleneck token 0) of every comment in the fused text buffer, then its row count.
    Ragged layout when ``offsets`` i32[M + 1] (RaggedText.offsets) is given, padded layout (on ``device``) otherwise."""
    return _arange(M + 1, device) * (nb + L) if offsets is None else offsets + _arange(M + 1, offsets.device) * nb


def text_rows(nb: int, M: int, L: int, I: int, Sv: int, *, ragged: bool, max_len: int = 0, offsets=None, comment=None,
              node_row, img_comment, text_mask) -> dict:
    """The encoder's index vectors (MultiGraphormerGraphEncoder._indices), on the device of the inputs.  ``offsets``, ``comment``
    and ``max_len`` (RaggedText) are read in the ragged layout only; ``node_row``, ``img_comment``, ``text_mask`` as in PackedBatch.
    ``spec_pre`` / ``spec_fus``: AttnSpec keywords of the text sequences before / after the bottleneck rows are inserted."""
    dev = node_row.device
    St = nb + L
    rows_pre = int(comment.numel()) if ragged else M * L
    rows_fus = rows_pre + M * nb
    assert rows_fus < 2 ** 31 and I * Sv < 2 ** 31, "row numbers are int32"
    first = first_rows(nb, M, L, offsets if ragged else None, dev)
    bn0 = first[:M]
    if ragged:
        pre2fus = torch.add(torch.arange(nb, nb + rows_pre, dtype=I32, device=dev), comment, alpha=nb)    # r + (comment + 1) nb
        spec_pre = dict(S=max_len, seq_offsets=offsets)
        spec_fus = dict(S=max_len + nb, seq_offsets=first)
    else:
        r = _arange(rows_pre, dev)
        pre2fus = torch.div(r, L, rounding_mode="floor") * St + nb + r % L
        spec_pre = dict(S=L, key_mask=text_mask)
        spec_fus = dict(S=St, key_mask=torch.cat([torch.ones(M, nb, dtype=torch.uint8, device=dev), text_mask], dim=1))
    return dict(
        ragged=ragged, Sv=Sv, P=Sv - nb, rows_pre=rows_pre, rows_fus=rows_fus, spec_pre=spec_pre, spec_fus=spec_fus,
        pre2fus=pre2fus, bn0_rows=bn0, cls_rows=bn0 + nb, bn_rows_all=bottleneck_rows(bn0, nb),
        text_row_of_node=torch.where(node_row >= 0, bn0[node_row.clamp(min=0).long()], node_row),
        img_text_bn_rows=bottleneck_rows(bn0[img_comment.long()], nb), vit_bn_rows=bottleneck_rows(_arange(I, dev) * Sv, nb))


def prune_rows(nb: int, M: int, I: int, Sv: int, bn0_rows: torch.Tensor, img_comment: torch.Tensor):
    """The rows the pruned last fusion layer keeps (bottleneck token 0 and [CLS] of every comment, bottleneck token 0 of
    every image) and where they land in its compact [2M, D] / [I, D] outputs: comment m at 2m and 2m + 1, image i at i."""
    m2 = _arange(M, bn0_rows.device) * 2
    prune = dict(text_keep=torch.stack([bn0_rows, bn0_rows + nb], dim=1).reshape(-1),
                 vit_keep=_arange(I, bn0_rows.device) * Sv, img_bn0_compact=img_comment * 2)
    return prune, dict(bn0_rows=m2, cls_rows=m2 + 1)


def place(x, device, pin: bool = False, non_blocking: bool = False):
    """The only host-specific step: every tensor of ``x`` (nested dicts / tuples) made contiguous and, when it is not on
    ``device`` yet, uploaded — from pinned memory when the packer pinned, on whatever stream is current (the prefetch
    thread's copy stream).  For results that were computed on the device it is the identity."""
    if isinstance(x, dict):
        return {k: place(v, device, pin, non_blocking) for k, v in x.items()}
    if isinstance(x, tuple):
        return tuple(place(v, device, pin, non_blocking) for v in x)
    if not torch.is_tensor(x):
        return x
    x = x.contiguous()
    if x.device.type == torch.device(device).type:
        return x
    return (x.pin_memory() if pin else x).to(device, non_blocking=non_blocking)
