"""PowerSGD low-rank compression ops (``lowrank_oracle`` is the definition).

GPU tensors run the hand-written CDNA4 kernels of ``csrc/lowrank/lowrank_kernels.hip`` (a missing extension is a hard
error on GPU); CPU tensors run the NumPy oracle, so a CPU run exercises the same numerics up to the summation order
inside a strip. Every op checks its arguments and raises ``ValueError``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _ext
from . import lowrank_oracle as O

RANK_PAD = O.RANK_PAD


def layout(rows: int, cols: int) -> tuple[int, int, int]:
    """(project strips, backproject strips, f32 elements of a partial buffer that serves both products)."""
    return O.layout(rows, cols)


def _plane(t, n: int, ref, what: str, exact: bool = True):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"lowrank: {what} must be a contiguous float32 tensor")
    if ref is not None and t.device != ref.device:
        raise ValueError(f"lowrank: {what} lives on {t.device}, the gradient on {ref.device}")
    if t.numel() != n if exact else t.numel() < n:
        raise ValueError(f"lowrank: {what} has {t.numel()} elements, the shape needs {n}")
    return t


def _shape(g, e, rows: int, cols: int):
    if rows <= 0 or cols <= 0 or rows % 16 or cols % 16:
        raise ValueError(f"lowrank: rows and cols must be positive multiples of 16, got {rows} x {cols}")
    _plane(g, rows * cols, None, "g", exact=False)
    _plane(e, rows * cols, g, "e")


def _np2(t, rows, cols):
    return t.view(-1)[: rows * cols].view(rows, cols).numpy()


def project(g, e, q, part, out, rows: int, cols: int):
    """out[rows][16] = (g + e) q over the two planes of the rows x cols matrix (``g`` may be the head of a longer
    bucket); ``part`` is the strip partials' scratch (:func:`layout`)."""
    _shape(g, e, rows, cols)
    sp = layout(rows, cols)[0]
    _plane(q, cols * RANK_PAD, g, "q")
    _plane(out, rows * RANK_PAD, g, "out")
    if g.is_cuda:
        _plane(part, sp * rows * RANK_PAD, g, "part", exact=False)
        C = _ext.require().lowrank
        C.project(g, e, q, part, rows, cols)
        C.combine(part, sp, out)
        return out
    out.view(rows, RANK_PAD).copy_(torch.from_numpy(
        O.project(_np2(g, rows, cols), _np2(e, rows, cols), _np2(q, cols, RANK_PAD))))
    return out


def backproject(g, e, ph, part, out, rows: int, cols: int):
    """out[cols][16] = (g + e)^T ph."""
    _shape(g, e, rows, cols)
    sb = layout(rows, cols)[1]
    _plane(ph, rows * RANK_PAD, g, "ph")
    _plane(out, cols * RANK_PAD, g, "out")
    if g.is_cuda:
        _plane(part, sb * cols * RANK_PAD, g, "part", exact=False)
        C = _ext.require().lowrank
        C.backproject(g, e, ph, part, rows, cols)
        C.combine(part, sb, out)
        return out
    out.view(cols, RANK_PAD).copy_(torch.from_numpy(
        O.backproject(_np2(g, rows, cols), _np2(e, rows, cols), _np2(ph, rows, RANK_PAD))))
    return out


def orth(p, rank: int, method: str = "mgs", part=None):
    """p[rows][16] -> its orthonormalised columns 0..rank-1 in place (columns >= rank zeroed). ``method``: ``"mgs"``
    (modified Gram-Schmidt, one workgroup) or ``"cholqr2"`` (CholeskyQR2 over strips of ``ORTH_STRIP`` rows, three
    launches), which on the GPU needs ``part``: a partial buffer of at least ``4 * ceil(rows / ORTH_STRIP) * 256``
    elements (two 16 x 16 fp64 Gram matrices per strip)."""
    if method not in ("mgs", "cholqr2"):
        raise ValueError(f"lowrank: unknown orth method {method!r}; mgs or cholqr2")
    if not (isinstance(p, torch.Tensor) and p.dim() == 2 and p.shape[1] == RANK_PAD):
        raise ValueError("lowrank: p must be a [rows][16] tensor")
    rows = p.shape[0]
    O.check_shape(rows, max(rows, RANK_PAD), rank)  # (the rank in 1..16 and <= rows; rows a multiple of 16)
    _plane(p, rows * RANK_PAD, None, "p")
    if not p.is_cuda:
        p.copy_(torch.from_numpy((O.orth if method == "mgs" else O.orth_cholqr2)(p.numpy(), rank)))
    elif method == "mgs":
        _ext.require().lowrank.orth(p, rank)
    else:
        _plane(part, 4 * -(-rows // O.ORTH_STRIP) * 256, p, "part", exact=False)
        _ext.require().lowrank.orth_cholqr2(p, rank, part)
    return p


def reconstruct(g, e, ph, qn, q_out, inv: float, rows: int, cols: int):
    """q_out = qn * inv; g <- ph q_out^T (fma chain over k = 0..15); e <- (g + e) - that. ``inv`` = f32(1 / world)."""
    _shape(g, e, rows, cols)
    _plane(ph, rows * RANK_PAD, g, "ph")
    _plane(qn, cols * RANK_PAD, g, "qn")
    _plane(q_out, cols * RANK_PAD, g, "q_out")
    if q_out.data_ptr() == qn.data_ptr():
        raise ValueError("lowrank: q_out must not be qn")
    inv = float(np.float32(inv))
    if g.is_cuda:
        _ext.require().lowrank.reconstruct(g, e, ph, qn, q_out, inv, rows, cols)
        return
    gh, en, qm = O.reconstruct(_np2(g, rows, cols), _np2(e, rows, cols), _np2(ph, rows, RANK_PAD),
                               _np2(qn, cols, RANK_PAD), np.float32(inv))
    g.view(-1)[: rows * cols].copy_(torch.from_numpy(gh).view(-1))
    e.view(-1).copy_(torch.from_numpy(en).view(-1))
    q_out.view(-1).copy_(torch.from_numpy(qm).view(-1))
