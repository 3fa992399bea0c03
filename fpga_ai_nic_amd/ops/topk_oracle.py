"""NumPy oracle of top-k gradient sparsification with memory (Stich, Cordonnier, Jaggi, NeurIPS 2018; Lin et al.,
Deep Gradient Compression, ICLR 2018) — the definition the kernels of ``csrc/topk/topk_kernels.hip`` follow bit for
bit.

A bucket is an f32 plane ``g`` of ``n_pad`` elements, ``n`` of them valid (``1 <= n <= n_pad < 2^31``, ``n_pad % 4 ==
0``), with a per-rank residual plane ``e`` (``n_pad`` f32, zeroed by the caller). ``k = count(n, density)`` components
cross the transport per rank; ``k_pad`` is k rounded up to a multiple of 4. One reduction over ``world`` ranks:

1. ``e[i] = g[i] + e[i]`` for ``i < n``: one f32 add, stored into the residual plane;
2. ``key[i] = bits(e[i]) & 0x7fffffff`` compared as unsigned; the selected set S is the k indices of largest key,
   ties to the lowest index. So NaN > Inf > finite (a non-finite gradient is sent, never hidden) and -0.0 ties +0.0;
3. the wire is ``[u32 idx[k_pad]][f32 val[k_pad]]`` (``8 * k_pad`` bytes): idx ascending, ``val[j]`` the bits of
   ``e[idx[j]]``; pad entries are idx = 0xffffffff, val = +0.0;
4. ``e[i] = +0.0`` for i in S; every other element keeps its accumulated value (:func:`select` is steps 1 to 4);
5. the ranks' wires are all-gathered (every rank sends the same byte count);
6. for ``i < n``: ``acc = +0.0``; for ``r = 0 .. world - 1`` in rank order, if i in S_r then ``acc = acc + val_r[i]``
   (f32); ``g[i] = acc * inv`` with ``inv = f32(1) / f32(world)`` (:func:`accumulate`).

Elements at or past n are never touched. Every rank computes the same bits from the same gathered wires.
:func:`select` finds the set the way the kernels do — the threshold key T = the k-th largest, everything above it,
and the first ``k - #(key > T)`` of the ties — so a test can hold it against a plain stable sort.
"""
from __future__ import annotations

import numpy as np

TILE = 4096          # elements of a count / compact / accumulate tile
HIST_BINS = 2048     # bins of the first radix digit (key bits 30..20); the other two digits take 1024
MAX_WORLD = 16       # wires one accumulate launch takes
PAD_IDX = 0xFFFFFFFF


def count(n: int, density: float) -> int:
    """k = max(1, min(n, int(n * density))), 0 < density <= 1."""
    if isinstance(density, bool) or not isinstance(density, (int, float)) or not 0.0 < density <= 1.0:
        raise ValueError(f"topk: the density must lie in (0, 1], got {density!r}")
    return max(1, min(n, int(n * density)))


def k_pad(k: int) -> int:
    return (k + 3) // 4 * 4


def check_shape(n_pad: int, n: int, k: int) -> None:
    if n_pad <= 0 or n_pad % 4 or n_pad >= 2 ** 31:
        raise ValueError(f"topk: n_pad must be a positive multiple of 4 below 2^31, got {n_pad}")
    if not 1 <= n <= n_pad:
        raise ValueError(f"topk: n must lie in 1..n_pad = {n_pad}, got {n}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= n:
        raise ValueError(f"topk: k must be an int in 1..n = {n}, got {k!r}")


def layout(n_pad: int, k: int) -> tuple[int, int, int]:
    """(tiles, u32 words of the select scratch, bytes of one wire). The scratch holds the histogram, four state
    words and four words per tile; the caller zeroes it once and every select leaves the histogram zeroed."""
    tiles = -(-n_pad // TILE)
    return tiles, HIST_BINS + 4 + 4 * tiles, 8 * k_pad(k)


def select(g, e, n: int, k: int):
    """Steps 1 to 4 on copies: returns (idx u32[k_pad], val f32[k_pad], e')."""
    g, e = np.asarray(g, dtype=np.float32), np.array(e, dtype=np.float32)
    check_shape(e.size, n, k)
    e[:n] = g[:n] + e[:n]
    key = e[:n].view(np.uint32) & np.uint32(0x7FFFFFFF)
    t = np.partition(key, n - k)[n - k]  # the k-th largest key
    ties = k - int(np.count_nonzero(key > t))
    pick = key > t
    pick[np.flatnonzero(key == t)[:ties]] = True
    chosen = np.flatnonzero(pick)
    kp = k_pad(k)
    idx = np.full(kp, PAD_IDX, dtype=np.uint32)
    val = np.zeros(kp, dtype=np.float32)
    idx[:k], val[:k] = chosen, e[chosen]
    e[chosen] = 0.0
    return idx, val, e


def accumulate(wires, g, n: int, inv):
    """Step 6 on a copy of g: ``wires`` is the ranks' (idx, val) in rank order."""
    if not 1 <= len(wires) <= MAX_WORLD:
        raise ValueError(f"topk: 1..{MAX_WORLD} ranks, got {len(wires)}")
    g = np.array(g, dtype=np.float32)
    acc = np.zeros(n, dtype=np.float32)
    for idx, val in wires:
        live = idx != PAD_IDX
        acc[idx[live]] = acc[idx[live]] + val[live]
    g[:n] = acc * np.float32(inv)
    return g


def step(gs, es, n: int, k: int):
    """One reduction over ``len(gs)`` ranks: returns (g' — the same on every rank —, [e' per rank], [(idx, val)])."""
    sel = [select(g, e, n, k) for g, e in zip(gs, es)]
    wires = [(i, v) for i, v, _ in sel]
    inv = np.float32(1.0) / np.float32(len(gs))
    return accumulate(wires, gs[0], n, inv), [s[2] for s in sel], wires
