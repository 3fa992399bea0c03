"""NumPy oracle of rotated one-bit gradient compression (DRIVE: Vargaftik et al., NeurIPS 2021; the rotation also in
EDEN, ICML 2022, and THC, NSDI 2024) — the definition the kernels of ``csrc/rht/rht_kernels.hip`` follow.

A bucket is an f32 plane ``g`` of ``n_pad`` elements, ``n`` of them valid (``n_pad % 4 == 0``, ``n_pad < 2^31``,
``1 <= n <= n_pad``), cut into ``nb = ceil(n / 4096)`` blocks of ``B = 4096``; elements at or past ``n`` read as +0.0 and
are never written. Each rank keeps one residual plane ``e`` of ``nb * B`` f32 (zeroed by the caller) **in rotated
coordinates**: the rotation is orthonormal and fixed for the bucket's lifetime, so the residual in rotated space is the
rotated residual and the encoder needs one transform. A 64-bit ``seed`` is the same on every rank.

* ``neg(i)`` = bit ``i & 31`` of ``sr_hash(*sr_key(seed, 0, 2), i >> 5)``, i the element index in the bucket; ``D x``
  flips the f32 sign bit where ``neg(i)``;
* ``rht(x) = (H (D x)) / 64`` per block, ``H[i][j] = (-1)^popcount(i & j)``; the inverse is ``D (H y) / 64``. Both are
  computed in float64 and rounded to f32 once; a zero result of ``H`` is +0.0.

Encode, per block: ``y = f32(rht(g)) + e`` (one f32 add); ``s = f32(sum|y| / 4096)`` (the sum in float64); bit ``i & 7`` of
byte ``i >> 3`` of the sign plane is ``y_i < 0`` (so +-0.0 and NaN give 0); ``e' = y - (bit ? -s : s)`` (one f32
subtract). A NaN anywhere in the block makes ``s`` NaN: a non-finite gradient is sent, never hidden.

One rank's wire is ``[u8 sign[512 * nb]][f32 scale[nb4]]``, ``nb4 = nb`` rounded up to 4, pads +0.0.

Decode, per block: ``acc_i = +0.0``, then ``+ (bit_r,i ? -s_r : s_r)`` for r = 0 .. world - 1 as f32 adds in rank order;
``g_i = f32(inverse(acc))_i * f32(1 / world)`` for ``i < n``.
"""
from __future__ import annotations

import numpy as np

from .bfp_oracle import sr_hash, sr_key, sr_seed_check

B = 4096
SIGN_BYTES = B // 8
MAX_WORLD = 16


def check_seed(seed) -> int:
    try:
        return sr_seed_check(seed)
    except ValueError:
        raise ValueError(f"rht: the seed is an int in [0, 2^64), got {seed!r}") from None


def check_shape(n_pad, n) -> None:
    for name, v in (("n_pad", n_pad), ("n", n)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"rht: {name} must be an int, got {v!r}")
    if n_pad <= 0 or n_pad % 4 or n_pad >= 1 << 31:
        raise ValueError(f"rht: n_pad must be a positive multiple of 4 below 2^31, got {n_pad}")
    if not 1 <= n <= n_pad:
        raise ValueError(f"rht: 1 <= n <= n_pad = {n_pad}, got n = {n}")


def layout(n_pad: int, n: int) -> tuple[int, int, int]:
    """(blocks, f32 elements of the residual plane, bytes of one rank's wire)."""
    check_shape(n_pad, n)
    nb = -(-n // B)
    return nb, nb * B, nb * SIGN_BYTES + 4 * (-(-nb // 4) * 4)


def negs(seed: int, count: int) -> np.ndarray:
    """neg(i) for i < count as uint32 sign masks (0 or 0x80000000)."""
    i = np.arange(count, dtype=np.uint32)
    return ((sr_hash(*sr_key(seed, 0, 2), i >> np.uint32(5)) >> (i & np.uint32(31))) & np.uint32(1)) << np.uint32(31)


def _flip(v, mask):
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) ^ mask).view(np.float32)


def fwht(x) -> np.ndarray:
    """H x along the last axis (a power of two long) in float64; a zero result is +0.0."""
    x = np.array(x, dtype=np.float64)
    shape, h = x.shape, 1
    with np.errstate(invalid="ignore", over="ignore"):
        while h < shape[-1]:
            x = x.reshape(-1, shape[-1] // (2 * h), 2, h)
            x = np.stack([x[:, :, 0] + x[:, :, 1], x[:, :, 0] - x[:, :, 1]], axis=2)
            h *= 2
        return x.reshape(shape) + 0.0


def rht64(x, n: int, seed: int) -> np.ndarray:
    """rht(x[:n]) in float64, [nb][B], before the rounding to f32."""
    nb = -(-n // B)
    p = np.zeros(nb * B, dtype=np.float32)
    p[:n] = np.asarray(x, dtype=np.float32).reshape(-1)[:n]
    return fwht(_flip(p, negs(seed, nb * B)).reshape(nb, B)) / 64


def irht64(y, seed: int) -> np.ndarray:
    """inverse(y) in float64 for the flat f32 array y of whole blocks."""
    y = np.asarray(y, dtype=np.float32).reshape(-1, B)
    sgn = 1.0 - 2.0 * (negs(seed, y.size) >> np.uint32(31)).astype(np.float64)
    return (fwht(y) / 64).reshape(-1) * sgn


def transform(x, seed: int, inverse: bool = False, n: int | None = None) -> np.ndarray:
    """Forward: f32 ``rht`` of ``x[:n]`` (n defaults to all), ``nb * B`` long. Inverse: f32 ``inverse(x)[:n]``."""
    check_seed(seed)
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.size if n is None else n
    with np.errstate(invalid="ignore", over="ignore"):
        if inverse:
            return irht64(x, seed)[:n].astype(np.float32)
        return rht64(x, n, seed).reshape(-1).astype(np.float32)


def encode(g, e, n: int, seed: int):
    """One rank's encode on copies: (sign u8[512 * nb], scale f32[nb4], e')."""
    g, e = np.asarray(g, dtype=np.float32), np.asarray(e, dtype=np.float32)
    nb, rot, _ = layout(g.size, n)
    if e.size != rot:
        raise ValueError(f"rht: e has {e.size} elements, the shape needs {rot}")
    with np.errstate(invalid="ignore", over="ignore"):
        y = transform(g, seed, n=n) + e
        s = (np.abs(y.astype(np.float64)).reshape(nb, B).sum(axis=1) / B).astype(np.float32)
        bit = y < 0
        left = y - np.where(bit, -np.repeat(s, B), np.repeat(s, B))
    scale = np.zeros(-(-nb // 4) * 4, dtype=np.float32)
    scale[:nb] = s
    return np.packbits(bit, bitorder="little"), scale, left.astype(np.float32)


def decode(wires, g, n: int, seed: int) -> np.ndarray:
    """g' from the ranks' (sign, scale) in rank order; elements at or past n keep g's."""
    g = np.array(g, dtype=np.float32)
    nb = layout(g.size, n)[0]
    if not 1 <= len(wires) <= MAX_WORLD:
        raise ValueError(f"rht: 1 .. {MAX_WORLD} ranks, got {len(wires)}")
    acc = np.zeros(nb * B, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for sign, scale in wires:
            s = np.repeat(np.asarray(scale, dtype=np.float32)[:nb], B)
            acc = acc + np.where(np.unpackbits(np.asarray(sign, dtype=np.uint8), bitorder="little") != 0, -s, s)
        g[:n] = transform(acc, seed, inverse=True, n=n) * (np.float32(1.0) / np.float32(len(wires)))
    return g


def step(gs, es, n: int, seed: int):
    """One reduction over ``len(gs)`` ranks: (g' — the same on every rank —, [e' per rank], [(sign, scale) per rank])."""
    enc = [encode(g, e, n, seed) for g, e in zip(gs, es)]
    wires = [(sign, scale) for sign, scale, _ in enc]
    return decode(wires, gs[0], n, seed), [left for _, _, left in enc], wires
