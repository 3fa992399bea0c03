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

``orth="cholqr2"`` replaces step 3 by CholeskyQR2 (:func:`orth_cholqr2`), which spreads over workgroups because its only
cross-row dependency is one 16 x 16 Gram matrix per pass. One pass over ``A[rows][16]``:

a. Gram: ``W = A^T A`` in fp64 (every f32 x f32 product is exact there), rows cut into strips of :data:`ORTH_STRIP`, the
   order inside a strip free, the strip partials added in strip order;
b. Factor, fp64 and sequential, its order part of the definition (:func:`cholqr_factor`): ``d_j = W_jj``; a column
   ``>= r`` or with ``d_j`` zero or non-finite is dead; ``s_j = 1 / sqrt(d_j)`` and ``C_jk = (W_jk * s_j) * s_k``
   (Jacobi scaling: a unit diagonal, so the column scales of a warm-started P do not enter the conditioning); Cholesky
   ``C = L L^T`` column by column, ``piv_j = C_jj - L_j0^2 - L_j1^2 - ...``; a pivot ``<= 2^-40`` (or NaN) marks column j
   dead — it depends on the earlier ones to beyond f32 resolution — and the row and column of a dead j are zero in L;
   ``T = (L^T)^-1`` by back substitution over the live indices; ``Rinv = diag(s) T`` rounded to f32 once;
c. Apply: ``out[i][j] = sum_{k <= j} A[i][k] * Rinv[k][j]`` over the live k, in f32, the order inside the 16-term sum free.

``orth_cholqr2`` is the pass applied twice. A dead column comes out as zeros and the others stay orthonormal; a dead
direction stays dead through the warm start (Q's column is then zero as well), as an exactly zero column does under
modified Gram-Schmidt.

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
ORTH_STRIP = 256   # rows of a CholeskyQR2 Gram strip
CHOL_PIVOT_MIN = 2.0 ** -40


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


def cholqr_factor(w, rank: int):
    """(Rinv, live) of the fp64 Gram matrix ``w``: step b of the module docstring, in exactly this order."""
    n = RANK_PAD
    d = np.diagonal(w).copy()
    live = np.isfinite(d) & (d != 0.0) & (np.arange(n) < rank)
    s = np.zeros(n)
    s[live] = 1.0 / np.sqrt(d[live])
    with np.errstate(invalid="ignore"):  # (a non-finite entry of a dead row: masked right here)
        low = np.where(live[:, None] & live[None, :], (w * s[:, None]) * s[None, :], 0.0)  # C, overwritten by L
    for j in range(n):
        acc = low[:, j].copy()
        for k in range(j):
            acc = acc - low[:, k] * low[j, k]
        if not (live[j] and acc[j] > CHOL_PIVOT_MIN):
            live[j] = False
            low[j, :] = 0.0
            low[:, j] = 0.0
            continue
        ljj = np.sqrt(acc[j])
        low[:, j] = np.where(np.arange(n) > j, acc / ljj, 0.0)
        low[j, j] = ljj
    t = np.zeros((n, n))
    for k in range(n - 1, -1, -1):
        if not live[k]:
            continue
        acc = np.zeros(n)
        for m in range(k + 1, n):
            acc = acc + low[m, k] * t[m, :]
        t[k, :] = np.where(np.arange(n) > k, -acc / low[k, k], 0.0)
        t[k, k] = 1.0 / low[k, k]
    t[:, ~live] = 0.0
    return s[:, None] * t, live


def cholqr_pass(a, rank: int):
    """One CholeskyQR pass: (out, Rinv in a's dtype, the masked A the apply used)."""
    w = None
    for r0 in range(0, a.shape[0], ORTH_STRIP):
        s64 = a[r0:r0 + ORTH_STRIP].astype(np.float64)
        part = s64.T @ s64
        w = part if w is None else w + part
    rinv, live = cholqr_factor(w, rank)
    rinv = rinv.astype(a.dtype)
    am = np.where(live[None, :], a, a.dtype.type(0))
    return am @ rinv, rinv, am


def orth_cholqr2(p, rank: int):
    """CholeskyQR2 over columns 0..rank-1: two passes of Gram, scaled Cholesky and triangular apply."""
    return cholqr_pass(cholqr_pass(p, rank)[0], rank)[0]


def reconstruct(g, e, ph, qn, inv):
    """(G^, E', Qm) of step 5; ``inv`` is already rounded to the working dtype."""
    dt = g.dtype
    qm = qn * dt.type(inv)
    acc = np.zeros(g.shape, dtype=dt)
    for k in range(RANK_PAD):
        prod = ph[:, k].astype(np.float64)[:, None] * qm[:, k].astype(np.float64)[None, :]
        acc = (prod + acc).astype(dt)
    return acc, (g + e) - acc, qm


def step(gs, es, q, rank: int, tails=None, dtype=np.float32, orth_fn=None):
    """One reduction over ``len(gs)`` ranks (per-rank G and E, one shared Q): returns (G^, [E' per rank], Qm, tail).
    The ranks' P, Qn and tails are summed in rank order. ``orth_fn``: :func:`orth` (the default) or
    :func:`orth_cholqr2`."""
    world = len(gs)
    gs = [np.asarray(g, dtype=dtype) for g in gs]
    es = [np.asarray(e, dtype=dtype) for e in es]
    q = np.asarray(q, dtype=dtype)
    inv = dtype(1.0) / dtype(world)
    p = sum(project(g, e, q) for g, e in zip(gs, es))
    ph = (orth_fn or orth)(p, rank)
    qn = sum(backproject(g, e, ph) for g, e in zip(gs, es))
    outs = [reconstruct(g, e, ph, qn, inv) for g, e in zip(gs, es)]
    tail = None if tails is None else sum(np.asarray(t, dtype=dtype) for t in tails) * inv
    return outs[0][0], [o[1] for o in outs], outs[0][2], tail
