"""The 1-bit sign wire codec ``sign1`` in the NumPy oracle and the mesh simulator: layout, special values, the
re-encode fixed point, contractivity (what makes error feedback valid) and error feedback itself."""
import argparse

import numpy as np
import pytest

from fpga_ai_nic_amd.config import add_named_flags, config_from_args, wire_codec
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.parallel import sim

S1 = "sign1"


def _values(n, seed):
    """Normal values under a log-normal scale per group of 16."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.repeat(np.exp(rng.standard_normal(n // 16)), 16)).astype(np.float32)


def test_layout_special_values_and_fixed_point():
    x = _values(512, 1)
    x[0:16] = 0.0
    x[16:32] = np.float32(1e-42) * np.arange(-8, 8)   # a denormal mean
    x[32:48] = [3, -1, 0, -0.0] * 4                    # mean 1: -0.0 is negative, +0.0 decodes to +s
    x[48], x[64], x[80] = np.inf, -np.inf, np.nan
    w = O.pack(x, 256, S1)
    assert wire_codec("sign") == S1 and O.CODECS[S1] == 5 and w.size == 2 * O.shard_bytes(S1, 256) == 2 * 48
    assert np.array_equal(w[:32], np.packbits(np.signbit(x[:256]), bitorder="little")), "bit i & 7 of byte i >> 3"
    assert list(w[32:38]) == [0, 0, 127, 255, 255, 255]
    d = O.unpack(w, 512, 256, S1)
    assert not d[:32].view(np.uint32).any(), "zero and denormal-mean groups decode to +0.0"
    assert np.array_equal(d[32:48], np.array([1, -1, 1, -1] * 4, np.float32)) and np.isnan(d[48:96]).all()
    mean = np.abs(x[96:].astype(np.float64)).reshape(-1, 16).mean(1)
    assert np.array_equal(np.abs(d[96:]).reshape(-1, 16)[:, 0], np.exp2(np.floor(np.log2(mean))))
    # re-encoding what was decoded: the exponent plane at once, every byte from the second trip on (a group of E 0 or
    # 255 decodes to +0.0 / NaN, which carry no sign)
    w2 = O.pack(d, 256, S1)
    assert np.array_equal(w2[32:48], w[32:48]) and np.array_equal(w2[48:], w[48:]), "finite non-zero groups: all bytes"
    assert np.array_equal(O.pack(O.unpack(w2, 512, 256, S1), 256, S1), w2)


def test_refused():
    cli = lambda *a: config_from_args(add_named_flags(argparse.ArgumentParser()).parse_args(a))  # noqa: E731
    assert cli("--compress", "sign", "--error-feedback").compress == "sign"
    with pytest.raises(ValueError, match="sign1 needs error feedback"):
        cli("--compress", "sign")
    with pytest.raises(ValueError, match="sign"):
        cli("--compress", "sign", "--error-feedback", "--rounding", "trunc")
    with pytest.raises(ValueError, match="stochastic rounding"):
        O.sr_codec(S1)


def test_contractive():
    """||x - dec(enc(x))||^2 <= (1 - 1/33) ||x||^2 per group, in float64 (1/32 exactly, 1/33 with S's f32 rounding)."""
    x = _values(4096, 2)
    E = O.pack(x, 4096, S1)[4096 // 8:]
    assert E.min() > 0 and E.max() < 255
    x64 = x.astype(np.float64).reshape(-1, 16)
    err = ((x64 - O.quantize(x, S1).astype(np.float64).reshape(-1, 16)) ** 2).sum(1)
    assert (err <= (1 - 1 / 33) * (x64 ** 2).sum(1)).all()


def test_error_feedback_constant_gradient():
    """The mean of T decoded steps is g - e_{T+1} / T, and ||e_{t+1}|| <= rho ||g + e_t|| per group."""
    g = _values(4096, 3)
    g64 = g.astype(np.float64).reshape(-1, 16)
    norm, gmax = np.sqrt((g64 ** 2).sum(1, keepdims=True)), np.abs(g64).max(1, keepdims=True)
    rho = np.sqrt(32 / 33)
    e, acc, fig = np.zeros(4096, np.float32), np.zeros(4096, np.float64), {}
    for t in range(1, 257):
        w, e = O.ef_pack(g, e, 4096, S1)
        acc += O.unpack(w, 4096, 4096, S1)
        if t in (1, 16, 64, 256):
            dev = np.abs(acc.reshape(-1, 16) / t - g64)
            fig[t] = (dev / gmax).max()
            print(f"T={t}: max |mean of decoded - g| / group max = {fig[t]:.4g}")
            assert (dev <= rho / (1 - rho) * norm / t + 2.0 ** -20 * norm / (1 - rho)).all(), t
    assert fig[256] < fig[16]


@pytest.mark.parametrize("N", [2, 4])
def test_mesh_allreduce_ef(N):
    """The simulator against the mesh built from ef_pack / ef_reduce: every rank decodes one gathered wire."""
    shard, sb = 256, O.shard_bytes(S1, 256)
    planes = mine = [np.zeros(shard * N, np.float32) for _ in range(N)]
    for step in range(2):
        grads = [_values(shard * N, 10 * step + r) for r in range(N)]
        ref, planes = sim.mesh_allreduce_ef(grads, planes, shard, S1)
        sent, mine = zip(*(O.ef_pack(grads[r], mine[r], shard, S1, self_shard=r) for r in range(N)))
        owner = [O.ef_reduce([x[s * sb:(s + 1) * sb] for x in sent], grads[s][s * shard:(s + 1) * shard], s,
                             mine[s][s * shard:(s + 1) * shard], S1, shard) for s in range(N)]
        for s, (_, e) in enumerate(owner):
            mine[s][s * shard:(s + 1) * shard] = e
        assert np.array_equal(O.unpack(np.concatenate([w for w, _ in owner]), shard * N, shard, S1), ref)
        assert all(np.array_equal(a, b) and a.any() for a, b in zip(mine, planes))
