"""Spec-level simulators of the all-reduce algorithms (pure NumPy, independent of the planner/engine).

They compute, from the algorithm definitions alone, the exact decoded result every rank must end up with —
the role the reference's 3-NIC RTL testbench golden model played (readme.pdf p.3-5 §3.2-3.3), but
tolerance-free: with the bit-exact codec oracle the engine must match these results bit for bit.

* ring  (SURVEY.md Appendix B): the chain for slice j of a block starts at ring position j (SEND_LOCAL) and
  moves to position j-1, j-2, ... each hop computing enc(dec(partial) + local); the position j+1 (= j-N+1)
  finishes the sum and owns slice j; the encoded full slice is then forwarded unchanged.
* mesh: owner s of shard s sums slot r = dec(enc(g_r[s])) for r != s and its own un-quantised g_s[s]
  (in rank order), re-encodes, and everyone decodes the gathered result.
"""
from __future__ import annotations

import numpy as np

from ..ops import bfp_oracle as O


def _enc_dec(x, codec):
    return O.quantize(x, codec)


def mesh_allreduce(grads: list[np.ndarray], shard: int, codec="bfp_rne") -> np.ndarray:
    N = len(grads)
    n_pad = shard * N
    out = np.zeros(n_pad, np.float32)
    for s in range(N):
        acc = np.zeros(shard, np.float32)
        for r in range(N):
            v = grads[r][s * shard:(s + 1) * shard].astype(np.float32)
            if r != s:
                v = _enc_dec(v, codec)
            acc = (acc + v).astype(np.float32)
        out[s * shard:(s + 1) * shard] = _enc_dec(acc, codec)
    return out


def ring_allreduce(grads: list[np.ndarray], orders: list[list[int]], slice_elems: int, blocks: int,
                   codec="bfp_rne", owner_fp32: bool = False) -> list[np.ndarray]:
    """Returns per-rank decoded results (identical unless owner_fp32 reproduces the reference quirk)."""
    N = len(grads)
    S = slice_elems
    part = blocks * N * S
    outs = [np.zeros(part * len(orders), np.float32) for _ in range(N)]
    for i, order in enumerate(orders):
        off = i * part
        for b in range(blocks):
            for j in range(N):
                lo = off + (b * N + j) * S
                chain = [order[(j - k) % N] for k in range(N)]  # ring positions j, j-1, ..., j-N+1
                val = _enc_dec(grads[chain[0]][lo:lo + S], codec)
                full_f32 = grads[chain[0]][lo:lo + S].astype(np.float32)
                for k in range(1, N):
                    s = (np.zeros(S, np.float32) + val).astype(np.float32)
                    s = (s + grads[chain[k]][lo:lo + S].astype(np.float32)).astype(np.float32)
                    full_f32 = s
                    val = _enc_dec(s, codec)
                owner = chain[-1]
                for r in range(N):
                    outs[r][lo:lo + S] = full_f32 if (owner_fp32 and r == owner and N > 1) else val
    return outs


def mesh_allreduce_ef(grads: list[np.ndarray], residuals: list[np.ndarray], shard: int, codec="bfp_rne"):
    """The mesh all-reduce with error feedback: rank r keeps one f32 residual plane ``residuals[r]`` of
    ``shard * N`` elements. Sender r ships ``enc(g_r[q] + e_r[q])`` for every shard q != r and keeps what the codec
    dropped in ``e_r[q]``; owner s sums the decoded slots in rank order (its own g_s[s] un-quantised), adds
    ``e_s[s]`` after the sum, re-encodes, and keeps what that encode dropped in ``e_s[s]``. Returns
    (decoded result every rank ends up with, the N new planes); with zero planes the result is
    :func:`mesh_allreduce`'s."""
    N = len(grads)
    f32 = np.float32
    new = [np.array(e, dtype=f32).reshape(-1)[: shard * N].copy() for e in residuals]
    out = np.zeros(shard * N, f32)
    for s in range(N):
        sl = slice(s * shard, (s + 1) * shard)
        acc = np.zeros(shard, f32)
        for r in range(N):
            v = grads[r][sl].astype(f32)
            if r != s:
                x = (v + new[r][sl]).astype(f32)
                v = _enc_dec(x, codec)
                new[r][sl] = (x - v).astype(f32)
            acc = (acc + v).astype(f32)
        y = (acc + new[s][sl]).astype(f32)
        out[sl] = _enc_dec(y, codec)
        new[s][sl] = (y - out[sl]).astype(f32)
    return out, new


def mesh_allreduce_sr(grads: list[np.ndarray], shard: int, codec="bfp_rne", seed: int = 0) -> np.ndarray:
    """The mesh all-reduce with stochastic rounding under the request seed ``seed``: sender r encodes shard q != r of
    its gradient with key (seed, r, 0), owner s sums the decoded slots in rank order (its own g_s[s] un-quantised) and
    re-encodes the sum with key (seed, s, 1); element i of the padded bucket draws byte i & 3 of hash word i >> 2.
    Returns the decoded result every rank ends up with. One rank: the owner stage alone."""
    N = len(grads)
    f32 = np.float32
    out = np.zeros(shard * N, f32)
    for s in range(N):
        sl = slice(s * shard, (s + 1) * shard)
        acc = np.zeros(shard, f32)
        for r in range(N):
            v = grads[r][sl].astype(f32)
            if r != s:
                v = O.sr_quantize(v, codec, O.sr_key(seed, r, 0), s * shard)
            acc = (acc + v).astype(f32)
        out[sl] = O.sr_quantize(acc, codec, O.sr_key(seed, s, 1), s * shard)
    return out
