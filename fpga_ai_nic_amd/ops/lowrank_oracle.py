"""NumPy oracle of the PowerSGD low-rank gradient compression (Vogels, Karimireddy, Jaggi, NeurIPS 2019) — the
definition the kernels of ``csrc/lowrank/lowrank_kernels.hip`` follow.

A layer bucket holds the matrix ``G[rows][cols]`` (row-major f32) and a tail (the bias). Per-rank state: a residual
plane ``E`` (rows * cols f32, zeroed) and ``Q[cols][16]`` f32 whose columns ``>= r`` are zero and whose columns ``< r``
are standard normal from a seeded CPU generator (:func:`init_q`: every rank starts with the same Q). The rank is
``1 <= r <= 16``, always padded to :data:`RANK_PAD` columns. One reduction over ``world`` ranks, ``inv = f32(1 /
world)``:

1. ``X = G + E``: one f32 add per element, never stored (every stage recomputes it, with the same bits);
2. ``P = X Q`` (rows x 16): f32 accumulation inside a strip of :data:`PROJ_STRIP` columns, the strip partials added in
   strip order (:func:`project`); the ranks' P are summed (a plain all-reduce: the wire is linear);
3. ``P^ = orth(P)`` (:func:`orth`): modified Gram-Schmidt over columns 0..r-1 in ``torch.distributed``'s
   ``powerSGD_hook`` order — column j is scaled by ``1 / (||col_j|| + 1e-8)``, then its projection is subtracted from
   every later column; dot products and norms in fp64, every stored value rounded to f32 once per statement;
4. ``Qn = X^T P^`` (cols x 16), split over strips of :data:`BACK_STRIP` rows and combined in strip order
   (:func:`backproject`); the ranks' Qn are summed;
5. ``Qm = Qn * inv``; ``G^[i][j]`` = the fma chain over k = 0..15 of ``P^[i][k] * Qm[j][k]`` from 0 in that order;
   ``E' = X - G^``; ``G <- G^``, ``E <- E'``, ``Q <- Qm`` (the warm start) (:func:`reconstruct`);
6. the tail is summed over the ranks and multiplied by ``inv`` (uncompressed).

Afterwards G holds the rank-averaged rank-r approximation, the same bits on every rank. :func:`step` runs all of it
for a list of ranks; ``dtype=np.float64`` runs the same algorithm in double precision (the reference of the f32 run).

The order of the f32 sums INSIDE a strip is not part of the definition (the kernels' matrix instruction has its own):
the two products are checked against an fp64 product within the f32 summation bound, everything else bit for bit. The
fma of step 5 is emulated as f32(fp64(p * q) + acc): the product is exact in fp64, so this differs from a fused
multiply-add only where the fp64 sum itself lands on an f32 rounding tie.
"""
from __future__ import annotations

import numpy as np

RANK_PAD = 16      # columns of P and Q, whatever the rank
PROJ_PANEL = 64    # rows of a project workgroup
PROJ_STRIP = 512   # columns of a project strip
BACK_TILE = 256    # columns of a backproject workgroup
BACK_STRIP = 512   # rows of a backproject strip
ORTH_EPS = 1e-8


def check_shape(rows: int, cols: int, rank: int) -> None:
    if isinstance(rank, bool) or not (isinstance(rank, int) and 1 <= rank <= RANK_PAD):
        raise ValueError(f"lowrank: the rank must be an int in 1..{RANK_PAD}, got {rank!r}")
    if rows <= 0 or cols <= 0 or rows % 16 or cols % 16:
        raise ValueError(f"lowrank: rows and cols must be positive multiples of 16, got {rows} x {cols}")
    if rank > min(rows, cols):
        raise ValueError(f"lowrank: rank {rank} above min(rows, cols) = {min(rows, cols)}")


def layout(rows: int, cols: int) -> tuple[int, int, int]:
    """(project strips, backproject strips, f32 elements of a partial buffer that serves both products)."""
    sp = -(-cols // PROJ_STRIP)
    sb = -(-rows // BACK_STRIP)
    return sp, sb, max(sp * rows, sb * cols) * RANK_PAD


def init_q(cols: int, rank: int, seed: int = 0, dtype=np.float32) -> np.ndarray:
    """Q[cols][16]: columns < rank standard normal from ``np.random.default_rng(seed)``, the others zero."""
    q = np.zeros((cols, RANK_PAD), dtype=dtype)
    q[:, :rank] = np.random.default_rng(seed).standard_normal((cols, rank)).astype(np.float32)
    return q


def _strips(x, b, strip):
    """sum over strips of x[:, strip] @ b[strip], each in x's dtype, the partials added in strip order."""
    out = None
    for k0 in range(0, x.shape[1], strip):
        part = x[:, k0:k0 + strip] @ b[k0:k0 + strip]
        out = part if out is None else out + part
    return out


def project(g, e, q):
    """P = (G + E) Q."""
    return _strips(g + e, q, PROJ_STRIP)


def backproject(g, e, ph):
    """Qn = (G + E)^T P^."""
    return _strips(np.ascontiguousarray((g + e).T), ph, BACK_STRIP)


def orth(p, rank: int):
    """Modified Gram-Schmidt over columns 0..rank-1 (fp64 dots and norms, one rounding to p's dtype per statement)."""
    out = np.zeros_like(p)
    out[:, :rank] = p[:, :rank]
    dt = p.dtype
    for j in range(rank):
        cj = out[:, j].astype(np.float64)
        out[:, j] = (cj * (1.0 / (np.sqrt(np.sum(cj * cj)) + ORTH_EPS))).astype(dt)
        cj = out[:, j].astype(np.float64)
        for k in range(j + 1, rank):
            ck = out[:, k].astype(np.float64)
            out[:, k] = (ck - np.sum(cj * ck) * cj).astype(dt)
    return out


def reconstruct(g, e, ph, qn, inv):
    """(G^, E', Qm) of step 5; ``inv`` is already rounded to the working dtype."""
    dt = g.dtype
    qm = qn * dt.type(inv)
    acc = np.zeros(g.shape, dtype=dt)
    for k in range(RANK_PAD):
        prod = ph[:, k].astype(np.float64)[:, None] * qm[:, k].astype(np.float64)[None, :]
        acc = (prod + acc).astype(dt)
    return acc, (g + e) - acc, qm


def step(gs, es, q, rank: int, tails=None, dtype=np.float32):
    """One reduction over ``len(gs)`` ranks (per-rank G and E, one shared Q): returns (G^, [E' per rank], Qm, tail).
    The ranks' P, Qn and tails are summed in rank order."""
    world = len(gs)
    gs = [np.asarray(g, dtype=dtype) for g in gs]
    es = [np.asarray(e, dtype=dtype) for e in es]
    q = np.asarray(q, dtype=dtype)
    inv = dtype(1.0) / dtype(world)
    p = sum(project(g, e, q) for g, e in zip(gs, es))
    ph = orth(p, rank)
    qn = sum(backproject(g, e, ph) for g, e in zip(gs, es))
    outs = [reconstruct(g, e, ph, qn, inv) for g, e in zip(gs, es)]
    tail = None if tails is None else sum(np.asarray(t, dtype=dtype) for t in tails) * inv
    return outs[0][0], [o[1] for o in outs], outs[0][2], tail
