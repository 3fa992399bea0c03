"""Count-sketch gradient compression ops (``sketch_oracle`` is the definition, matched bit for bit).

GPU tensors run the hand-written CDNA4 kernels of ``csrc/sketch/sketch_kernels.hip`` and the keys-only radix select of
``csrc/topk/topk_kernels.hip`` (a missing extension is a hard error on GPU); CPU tensors run the NumPy oracle. Every op
checks its arguments and raises ``ValueError``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _ext
from . import sketch_oracle as O
from . import topk as TK

count, k_pad = TK.count, TK.k_pad


def layout(n_pad: int, k: int, rows: int, cols: int) -> tuple[int, int, int, int]:
    """(f32 elements of the sketch, f32 elements of the partial buffer, int32 words of the select scratch, bytes of the
    wire). The scratch is zeroed once by the caller (``torch.zeros``); the others need no initial value."""
    _, _, part, sk = O.layout(n_pad, k, rows, cols)
    _, words, nbytes = TK.layout(n_pad, k)
    return sk, part, words, nbytes


def _plane(t, dtype, n: int, ref, what: str):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"sketch: {what} must be a contiguous {dtype} tensor")
    if ref is not None and t.device != ref.device:
        raise ValueError(f"sketch: {what} lives on {t.device}, the gradient on {ref.device}")
    if t.numel() != n:
        raise ValueError(f"sketch: {what} has {t.numel()} elements, the shape needs {n}")
    return t


def _grid(max_blocks) -> int:
    if max_blocks is None:
        return 0
    if isinstance(max_blocks, bool) or not isinstance(max_blocks, int) or max_blocks < 1:
        raise ValueError(f"sketch: max_blocks must be a positive int or None, got {max_blocks!r}")
    return max_blocks


def _planes(g, e, S, n, k, rows, cols, seed):
    """Checks the two planes and the sketch; returns n_pad."""
    if not isinstance(g, torch.Tensor):
        raise ValueError("sketch: g must be a tensor")
    n_pad = g.numel()
    O.check_params(rows, cols, seed)
    try:
        TK.O.check_shape(n_pad, n, k)
    except ValueError as err:
        raise ValueError(str(err).replace("topk:", "sketch:")) from None
    _plane(g, torch.float32, n_pad, None, "g")
    _plane(e, torch.float32, n_pad, g, "e")
    _plane(S, torch.float32, rows * cols, g, "S")
    if len({g.data_ptr(), e.data_ptr(), S.data_ptr()}) != 3:
        raise ValueError("sketch: g, e and S must be buffers of their own")
    return n_pad


def sketch(g, e, S, part, n: int, rows: int, cols: int, seed: int, max_blocks=None):
    """``S[rows][cols]`` = the count sketch of ``(g + e)[:n]`` (step 1 of the oracle); g and e are only read. ``S`` and
    ``part`` are f32 of the lengths :func:`layout` gives."""
    n_pad = _planes(g, e, S, n, 1, rows, cols, seed)
    _plane(part, torch.float32, O.layout(n_pad, 1, rows, cols)[2], g, "part")
    grid = _grid(max_blocks)
    if g.is_cuda:
        _ext.require().sketch.sketch(g, e, part, S, n, rows, cols, seed, grid)
        return S
    S.copy_(torch.from_numpy(O.sketch(g.numpy(), e.numpy(), n, rows, cols, seed)).reshape(-1))
    return S


def estimate_select(g, e, S, wire, scratch, n: int, k: int, rows: int, cols: int, seed: int, max_blocks=None):
    """``e[:n] = g[:n] + e[:n]``, ``g[:n]`` = the median estimates from the (summed) sketch ``S``, and ``wire`` =
    ``[u32 idx[k_pad]][f32 val[k_pad]]`` of the k largest ``|g|`` (ties to the lowest index), ascending by index, val
    holding the estimates (steps 3 and 4)."""
    n_pad = _planes(g, e, S, n, k, rows, cols, seed)
    _, words, nbytes = TK.layout(n_pad, k)
    _plane(wire, torch.uint8, nbytes, g, "wire")
    _plane(scratch, torch.int32, words, g, "scratch")
    grid = _grid(max_blocks)
    if g.is_cuda:
        C = _ext.require()
        C.sketch.estimate(g, e, S, n, rows, cols, seed, grid)
        C.topk.select_keys(g, wire, scratch, n, k, grid)
        return wire
    est, x = O.estimate(g.numpy(), e.numpy(), S.numpy().reshape(rows, cols), n, seed)
    idx, val = O.select_keys(est, n, k)
    wi, wv = TK._wire_views(wire, k_pad(k))
    wi.copy_(torch.from_numpy(idx.view(np.int32)))
    wv.copy_(torch.from_numpy(val))
    g.copy_(torch.from_numpy(est))
    e.copy_(torch.from_numpy(x))
    return wire


def fetch(e, wire, n: int, k: int, max_blocks=None):
    """``val[j] = e[idx[j]]`` and ``e[idx[j]] = +0.0`` for ``j < k`` on the wire (step 5); returns the val view
    (``k_pad`` f32), which the second exchange all-reduces."""
    if not isinstance(e, torch.Tensor):
        raise ValueError("sketch: e must be a tensor")
    n_pad = e.numel()
    try:
        TK.O.check_shape(n_pad, n, k)
    except ValueError as err:
        raise ValueError(str(err).replace("topk:", "sketch:")) from None
    _plane(e, torch.float32, n_pad, None, "e")
    _plane(wire, torch.uint8, TK.layout(n_pad, k)[2], e, "wire")
    grid = _grid(max_blocks)
    wi, wv = TK._wire_views(wire, k_pad(k))
    if e.is_cuda:
        _ext.require().sketch.fetch(e, wire, n, k, grid)
        return wv
    val, left = O.fetch(e.numpy(), wi.numpy().view(np.uint32), k)
    wv.copy_(torch.from_numpy(val))
    e.copy_(torch.from_numpy(left))
    return wv
