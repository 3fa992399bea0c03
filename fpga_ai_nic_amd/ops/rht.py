"""Rotated one-bit gradient compression ops (``rht_oracle`` is the definition).

GPU tensors run the hand-written CDNA4 kernels of ``csrc/rht/rht_kernels.hip`` (a missing extension is a hard error on
GPU); CPU tensors run the NumPy oracle. The GPU transform sums in f32 on the matrix cores, the oracle in float64: they
agree bit for bit wherever every partial sum is exact and within a few ulp of the block's ``sum|x| / 64`` otherwise.
Every op checks its arguments and raises ``ValueError``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _ext
from . import rht_oracle as O

B, MAX_WORLD = O.B, O.MAX_WORLD


def layout(n_pad: int, n: int) -> tuple[int, int, int]:
    """(blocks of 4096, f32 elements of the residual plane, bytes of one rank's wire). The residual is zeroed once by
    the caller; the wire needs no initial value."""
    return O.layout(n_pad, n)


def _plane(t, dtype, n: int, ref, what: str):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"rht: {what} must be a contiguous {dtype} tensor")
    if ref is not None and t.device != ref.device:
        raise ValueError(f"rht: {what} lives on {t.device}, the gradient on {ref.device}")
    if t.numel() != n:
        raise ValueError(f"rht: {what} has {t.numel()} elements, the shape needs {n}")
    return t


def _grid(max_blocks) -> int:
    if max_blocks is None:
        return 0
    if isinstance(max_blocks, bool) or not isinstance(max_blocks, int) or max_blocks < 1:
        raise ValueError(f"rht: max_blocks must be a positive int or None, got {max_blocks!r}")
    return max_blocks


def _own(*ts):
    if len({t.data_ptr() for t in ts}) != len(ts):
        raise ValueError("rht: the planes must be buffers of their own")


def transform(x, seed: int, inverse: bool = False, n: int | None = None, max_blocks=None):
    """Forward: ``(1/64) H D x`` per block of 4096 of the plane ``x`` (``n`` valid elements, default all; +0 behind
    them), a new tensor of ``blocks * 4096`` f32. Inverse: ``x`` holds whole rotated blocks; returns the first ``n``
    (default all) elements of ``D (1/64) H x``."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("rht: x must be a tensor")
    _plane(x, torch.float32, x.numel(), None, "x")
    O.check_seed(seed)
    n = x.numel() if n is None else n
    n_pad = -(-n // 4) * 4 if inverse else x.numel()
    _, rot, _ = O.layout(n_pad, n)
    if inverse and x.numel() != rot:
        raise ValueError(f"rht: x has {x.numel()} elements, the inverse of n = {n} needs {rot}")
    grid = _grid(max_blocks)
    if x.is_cuda:
        out = torch.zeros(n_pad if inverse else rot, dtype=torch.float32, device=x.device)
        _ext.require().rht.transform(x, out, n_pad, n, seed, inverse, grid)
        return out[:n] if inverse else out
    return torch.from_numpy(O.transform(x.numpy(), seed, inverse, n))


def _views(wire, nb: int):
    return wire[: O.SIGN_BYTES * nb], wire[O.SIGN_BYTES * nb:].view(torch.float32)


def encode(g, e, wire, n: int, seed: int, max_blocks=None):
    """``y = rht(g[:n]) + e``; ``wire`` = ``[u8 sign[512 * nb]][f32 scale[nb4]]`` of y; ``e = y -`` its one-bit value.
    g is only read."""
    if not isinstance(g, torch.Tensor):
        raise ValueError("rht: g must be a tensor")
    nb, rot, nbytes = O.layout(g.numel(), n)
    O.check_seed(seed)
    _plane(g, torch.float32, g.numel(), None, "g")
    _plane(e, torch.float32, rot, g, "e")
    _plane(wire, torch.uint8, nbytes, g, "wire")
    _own(g, e, wire)
    grid = _grid(max_blocks)
    if g.is_cuda:
        _ext.require().rht.encode(g, e, wire, n, seed, grid)
        return wire
    sign, scale, left = O.encode(g.numpy(), e.numpy(), n, seed)
    ws, wc = _views(wire, nb)
    ws.copy_(torch.from_numpy(sign))
    wc.copy_(torch.from_numpy(scale))
    e.copy_(torch.from_numpy(left))
    return wire


def decode(wires, world: int, g, n: int, seed: int, max_blocks=None):
    """``g[:n]`` = the inverse rotation of the ``world`` ranks' one-bit values, added in rank order, times
    ``f32(1 / world)``; ``wires``: the ranks' wires back to back."""
    if not isinstance(g, torch.Tensor):
        raise ValueError("rht: g must be a tensor")
    nb, _, nbytes = O.layout(g.numel(), n)
    O.check_seed(seed)
    if isinstance(world, bool) or not isinstance(world, int) or not 1 <= world <= MAX_WORLD:
        raise ValueError(f"rht: world must be an int in 1 .. {MAX_WORLD}, got {world!r}")
    _plane(g, torch.float32, g.numel(), None, "g")
    _plane(wires, torch.uint8, world * nbytes, g, "wires")
    _own(g, wires)
    grid = _grid(max_blocks)
    if g.is_cuda:
        _ext.require().rht.decode(wires, world, g, n, seed, float(np.float32(1.0) / np.float32(world)), grid)
        return g
    per = [_views(wires[r * nbytes:(r + 1) * nbytes], nb) for r in range(world)]
    g.copy_(torch.from_numpy(O.decode([(s.numpy(), c.numpy()) for s, c in per], g.numpy(), n, seed)))
    return g
