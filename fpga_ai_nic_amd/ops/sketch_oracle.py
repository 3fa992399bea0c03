"""NumPy oracle of count-sketch gradient compression (Ivkin et al., "Communication-efficient distributed SGD with
sketching", NeurIPS 2019, two rounds; Rothchild et al., FetchSGD, ICML 2020, the same sketch) — the definition the
kernels of ``csrc/sketch/sketch_kernels.hip`` follow bit for bit.

A bucket is an f32 plane ``g`` of ``n_pad`` elements, ``n`` of them valid (``n_pad % 4 == 0``, ``n_pad < 2^31``), with
a per-rank residual plane ``e`` (zeroed by the caller). The sketch has ``R`` rows (1, 3 or 5) of ``C`` columns (a
multiple of 1024 in 1024 .. 2^22) under a 64-bit ``seed``. Element ``i`` lies in chunk ``q = i // C`` at ``t = i % C``;
``Q = ceil(n_pad / C)`` chunks come in strips of 16. With ``sr_hash`` / ``sr_key`` of ``bfp_oracle``, for row j:

* ``koff_j = sr_key(seed, j, 0)``, ``ksgn_j = sr_key(seed, j, 1)``;
* ``off(j, q) = 4 * (sr_hash(koff_j, q) mod (C / 4))``: the chunk is rotated as a whole, by whole 16-B vectors;
* ``neg(j, i)`` = bit ``i & 31`` of ``sr_hash(ksgn_j, i >> 5)``; sgn(v) flips v's f32 sign bit where neg is set (exact
  for zeros, infinities and NaN);
* the column of element i in row j is ``(t + off(j, q)) mod C``.

One reduction over ``world`` ranks:

1. ``x[i] = g[i] + e[i]`` (one f32 add) for ``i < n``. For row j, column b, strip s: ``p_s = +0.0``; for the strip's
   chunks q ascending, ``i = q * C + ((b - off(j, q)) mod C)``, and if ``i < n``: ``p_s = p_s + sgn(x[i])``.
   ``S[j][b] = p_0 + p_1 + ...`` in strip order (:func:`sketch`). No sum is ever -0.0, so an absent element adds
   like +0.0;
2. the ranks' S are all-reduced (R * C f32);
3. for ``i < n``: ``v_j = sgn(S[j][col_j(i)])``; ``est[i]`` = the median of the R values by the compare-exchange
   network of :func:`median` (a pair is swapped where the second is less than the first; -0.0 is not less than
   +0.0); if any ``v_j`` is NaN, ``est[i]`` is the canonical NaN 0x7fc00000, whose key is the largest: a non-finite
   gradient is sent, never hidden. ``e[i] = x[i]``, ``g[i] = est[i]`` (:func:`estimate`);
4. the k largest ``|g|`` by the top-k keys and tie rule (ties to the lowest index, idx ascending) go into the top-k
   wire ``[u32 idx[k_pad]][f32 val[k_pad]]`` with the top-k pads (:func:`select_keys`; val holds the estimates);
5. ``val[j] = e[idx[j]]``, ``e[idx[j]] = +0.0`` (:func:`fetch`);
6. the ranks' val are all-reduced (k_pad f32);
7. ``topk_oracle.accumulate`` of that one wire with ``inv = f32(1) / f32(world)``: g is the rank mean at the agreed
   indices and +0.0 elsewhere.

Elements at or past n are never touched.
"""
from __future__ import annotations

from functools import reduce

import numpy as np

from . import topk_oracle as T
from .bfp_oracle import sr_hash, sr_key, sr_seed_check

ROWS = (1, 3, 5)
COL_STEP, MAX_COLS = 1024, 1 << 22
STRIP = 16  # chunks of one strip
CANONICAL_NAN = 0x7FC00000


def check_params(rows, cols, seed) -> None:
    if isinstance(rows, bool) or rows not in ROWS:
        raise ValueError(f"sketch: rows must be one of {ROWS}, got {rows!r}")
    if isinstance(cols, bool) or not isinstance(cols, int) or cols % COL_STEP or not COL_STEP <= cols <= MAX_COLS:
        raise ValueError(f"sketch: cols must be a multiple of {COL_STEP} in {COL_STEP}..2^22, got {cols!r}")
    try:
        sr_seed_check(seed)
    except ValueError:
        raise ValueError(f"sketch: the seed is an int in [0, 2^64), got {seed!r}") from None


def layout(n_pad: int, k: int, rows: int, cols: int) -> tuple[int, int, int, int]:
    """(chunks, strips, f32 elements of the per-strip partial sketches, f32 elements of the sketch)."""
    check_params(rows, cols, 0)
    chunks = -(-n_pad // cols)
    strips = -(-chunks // STRIP)
    return chunks, strips, strips * rows * cols, rows * cols


def offsets(rows: int, cols: int, seed: int, chunks: int) -> np.ndarray:
    """off(j, q) as int64 [rows][chunks]."""
    q = np.arange(chunks, dtype=np.uint32)
    return np.stack([4 * (sr_hash(*sr_key(seed, j, 0), q).astype(np.int64) % (cols // 4)) for j in range(rows)])


def negs(row: int, seed: int, n: int) -> np.ndarray:
    """neg(row, i) for i < n as uint32 sign masks (0 or 0x80000000)."""
    i = np.arange(n, dtype=np.uint32)
    return ((sr_hash(*sr_key(seed, row, 1), i >> np.uint32(5)) >> (i & np.uint32(31))) & np.uint32(1)) << np.uint32(31)


def _flip(v, mask):
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) ^ mask).view(np.float32)


def sketch(g, e, n: int, rows: int, cols: int, seed: int) -> np.ndarray:
    """Step 1: S as f32 [rows][cols]."""
    check_params(rows, cols, seed)
    g, e = np.asarray(g, dtype=np.float32), np.asarray(e, dtype=np.float32)
    chunks, strips = layout(g.size, 1, rows, cols)[:2]
    off = offsets(rows, cols, seed, chunks)
    x = np.zeros(chunks * cols, dtype=np.float32)
    S = np.zeros((rows, cols), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x[:n] = g[:n] + e[:n]
        for j in range(rows):
            y = np.zeros(chunks * cols, dtype=np.float32)  # (an absent element adds like +0.0)
            y[:n] = _flip(x[:n], negs(j, seed, n))
            y = y.reshape(chunks, cols)
            for s in range(strips):
                p = np.zeros(cols, dtype=np.float32)
                for q in range(s * STRIP, min((s + 1) * STRIP, chunks)):
                    p = p + np.roll(y[q], off[j, q])  # column b takes t = (b - off) mod C
                S[j] = p if s == 0 else S[j] + p
    return S


def _cx(a, b):
    """Compare-exchange: (a, b) with the pair swapped where b < a."""
    sw = b < a
    return np.where(sw, b, a), np.where(sw, a, b)


def median(v):
    """The median of 1, 3 or 5 f32 arrays by a fixed compare-exchange network; canonical NaN where any is NaN."""
    nan = np.zeros(v[0].shape, dtype=bool)
    for a in v:
        nan |= np.isnan(a)
    if len(v) == 5:  # drop the least of the first four and the greatest of them: the median of the other three
        a, b = _cx(v[0], v[1])
        c, d = _cx(v[2], v[3])
        a, c = _cx(a, c)
        b, d = _cx(b, d)
        v = [b, c, v[4]]
    if len(v) == 3:
        a, b = _cx(v[0], v[1])
        b, c = _cx(b, v[2])
        a, b = _cx(a, b)
        v = [b]
    return np.where(nan, np.array([CANONICAL_NAN], dtype=np.uint32).view(np.float32), v[0]).astype(np.float32)


def estimate(g, e, S, n: int, seed: int):
    """Step 3 on copies: returns (g' = est, e' = x)."""
    g, e = np.array(g, dtype=np.float32), np.array(e, dtype=np.float32)
    S = np.asarray(S, dtype=np.float32)
    rows, cols = S.shape
    check_params(rows, cols, seed)
    off = offsets(rows, cols, seed, -(-g.size // cols))
    i = np.arange(n, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = [_flip(S[j][(i % cols + off[j][i // cols]) % cols], negs(j, seed, n)) for j in range(rows)]
        e[:n] = g[:n] + e[:n]
        g[:n] = median(v)
    return g, e


def select_keys(plane, n: int, k: int):
    """Step 4: (idx u32[k_pad], val f32[k_pad]) of the k largest keys of plane[:n]; the plane is left alone."""
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    T.check_shape(plane.size, n, k)
    key = plane[:n].view(np.uint32) & np.uint32(0x7FFFFFFF)
    t = np.partition(key, n - k)[n - k]  # the k-th largest key
    pick = key > t
    pick[np.flatnonzero(key == t)[: k - int(np.count_nonzero(pick))]] = True
    chosen = np.flatnonzero(pick)
    idx = np.full(T.k_pad(k), T.PAD_IDX, dtype=np.uint32)
    val = np.zeros(T.k_pad(k), dtype=np.float32)
    idx[:k], val[:k] = chosen, plane[chosen]
    return idx, val


def fetch(e, idx, k: int):
    """Step 5 on a copy: returns (val f32[k_pad], e')."""
    e = np.array(e, dtype=np.float32)
    val = np.zeros(idx.size, dtype=np.float32)
    val[:k] = e[idx[:k]]
    e[idx[:k]] = 0.0
    return val, e


def step(gs, es, n: int, k: int, rows: int, cols: int, seed: int):
    """One reduction over ``len(gs)`` ranks (the all-reduces add in rank order): returns (g' — the same on every rank
    —, [e' per rank], (idx, val) of the second exchange, S of the first)."""
    T.check_shape(np.asarray(gs[0]).size, n, k)
    with np.errstate(invalid="ignore", over="ignore"):
        S = reduce(np.add, [sketch(g, e, n, rows, cols, seed) for g, e in zip(gs, es)])
        est = [estimate(g, e, S, n, seed) for g, e in zip(gs, es)]
        idx, _ = select_keys(est[0][0], n, k)  # (the estimates are the same on every rank)
        got = [fetch(x, idx, k) for _, x in est]
        val = reduce(np.add, [v for v, _ in got])
    inv = np.float32(1.0) / np.float32(len(gs))
    return T.accumulate([(idx, val)], est[0][0], n, inv), [x for _, x in got], (idx, val), S
