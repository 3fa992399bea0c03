"""Top-k gradient sparsification ops (``topk_oracle`` is the definition, matched bit for bit).

GPU tensors run the hand-written CDNA4 kernels of ``csrc/topk/topk_kernels.hip`` (a missing extension is a hard error
on GPU); CPU tensors run the NumPy oracle. Every op checks its arguments and raises ``ValueError``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _ext
from . import topk_oracle as O

MAX_WORLD = O.MAX_WORLD
count, k_pad = O.count, O.k_pad


def layout(n_pad: int, k: int) -> tuple[int, int, int]:
    """(tiles, int32 words of the select scratch, bytes of one wire). The scratch is zeroed once by the caller
    (``torch.zeros``); every select leaves it ready for the next."""
    return O.layout(n_pad, k)


def _plane(t, dtype, n: int, ref, what: str):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"topk: {what} must be a contiguous {dtype} tensor")
    if ref is not None and t.device != ref.device:
        raise ValueError(f"topk: {what} lives on {t.device}, the gradient on {ref.device}")
    if t.numel() != n:
        raise ValueError(f"topk: {what} has {t.numel()} elements, the shape needs {n}")
    return t


def _grid(max_blocks) -> int:
    if max_blocks is None:
        return 0
    if isinstance(max_blocks, bool) or not isinstance(max_blocks, int) or max_blocks < 1:
        raise ValueError(f"topk: max_blocks must be a positive int or None, got {max_blocks!r}")
    return max_blocks


def _wire_views(wire, kp: int):
    """(idx as int32[k_pad], val as f32[k_pad]) over one wire's bytes."""
    return wire[: 4 * kp].view(torch.int32), wire[4 * kp:].view(torch.float32)


def select(g, e, wire, scratch, n: int, k: int, max_blocks=None):
    """``e[:n] = g[:n] + e[:n]``; ``wire`` = ``[u32 idx[k_pad]][f32 val[k_pad]]`` of the k largest ``|e|`` (ties to
    the lowest index), ascending by index; ``e`` = +0 where sent. ``g`` and ``e`` are f32 planes of ``n_pad`` elements,
    ``wire`` uint8 and ``scratch`` int32 of the lengths :func:`layout` gives."""
    if not isinstance(g, torch.Tensor):
        raise ValueError("topk: g must be a tensor")
    n_pad = g.numel()
    O.check_shape(n_pad, n, k)
    _, words, nbytes = layout(n_pad, k)
    _plane(g, torch.float32, n_pad, None, "g")
    _plane(e, torch.float32, n_pad, g, "e")
    _plane(wire, torch.uint8, nbytes, g, "wire")
    _plane(scratch, torch.int32, words, g, "scratch")
    if e.data_ptr() == g.data_ptr():
        raise ValueError("topk: e must not be g")
    grid = _grid(max_blocks)
    if g.is_cuda:
        _ext.require().topk.select(g, e, wire, scratch, n, k, grid)
        return wire
    idx, val, en = O.select(g.numpy(), e.numpy(), n, k)
    wi, wv = _wire_views(wire, k_pad(k))
    wi.copy_(torch.from_numpy(idx.view(np.int32)))
    wv.copy_(torch.from_numpy(val))
    e.copy_(torch.from_numpy(en))
    return wire


def accumulate(wires, world: int, g, n: int, k: int, inv: float, max_blocks=None):
    """``g[i] = (+0 + val_0[i] + val_1[i] + ...) * inv`` over the ranks that sent i, in rank order, for ``i < n``.
    ``wires``: the ``world`` wires back to back (what ``transport.all_gather`` leaves); ``inv`` = f32(1 / world)."""
    if not isinstance(g, torch.Tensor):
        raise ValueError("topk: g must be a tensor")
    if isinstance(world, bool) or not isinstance(world, int) or not 1 <= world <= MAX_WORLD:
        raise ValueError(f"topk: 1..{MAX_WORLD} ranks, got {world!r}")
    n_pad = g.numel()
    O.check_shape(n_pad, n, k)
    nbytes = layout(n_pad, k)[2]
    _plane(g, torch.float32, n_pad, None, "g")
    _plane(wires, torch.uint8, world * nbytes, g, "wires")
    grid = _grid(max_blocks)
    inv = float(np.float32(inv))
    if g.is_cuda:
        _ext.require().topk.accumulate(wires, world, g, n, k, inv, grid)
        return g
    kp = k_pad(k)
    parts = [_wire_views(wires[r * nbytes:(r + 1) * nbytes], kp) for r in range(world)]
    g.copy_(torch.from_numpy(O.accumulate([(i.numpy().view(np.uint32), v.numpy()) for i, v in parts], g.numpy(), n,
                                          np.float32(inv))))
    return g
