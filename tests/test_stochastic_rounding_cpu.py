"""Stochastic rounding for the compressed mesh all-reduce, CPU side: the NumPy oracle (``bfp_oracle.sr_*``), the
simulator (``sim.mesh_allreduce_sr``), the Python engine over ThreadFabric, the trainer, the CLI, the checkpointed
counter and the refusals."""
import io
import json
import math

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.cli import mlp_mpi
from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import sim
from fpga_ai_nic_amd.parallel.allreduce import BucketLayout, CompressedAllReduce, sr_request
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, RcclAllReduce
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

CODECS = ["bfp_rne", "bfp4_rne"]
TOP = {"bfp_rne": (133, 127), "bfp4_rne": (129, 7)}
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


# --------------------------------------------------------------------------- the definition, in plain Python
def _mix(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def _h(k0, k1, w):
    return _mix((_mix(w ^ k0) + k1) & M32)


def _key(seed, r, stage):
    return seed & M32, (seed >> 32) ^ (((2 * r + stage + 1) * 0x9E3779B9) & M32)


def _step_seed(base, step, bucket):
    return base ^ ((step * 0x9E3779B97F4A7C15 + bucket * 0xD1B54A32D192ED03) & M64)


def test_pinned_vectors():
    assert [f"{_h(1, 2, w):08x}" for w in range(4)] == ["caffe390", "d1132181", "d4b2dc82", "f1cdb2b7"]
    assert tuple(f"{k:08x}" for k in _key(0x0123456789ABCDEF, 5, 1)) == ("89abcdef", "6bbaf1cb")
    assert f"{_step_seed(7, 3, 2):016x}" == "7e11019221054e42"
    # the shipped oracle is that definition
    assert [int(v) for v in O.sr_hash(1, 2, np.arange(4))] == [_h(1, 2, w) for w in range(4)]
    assert O.sr_key(0x0123456789ABCDEF, 5, 1) == _key(0x0123456789ABCDEF, 5, 1)
    assert O.sr_step_seed(7, 3, 2) == _step_seed(7, 3, 2)
    rng = np.random.default_rng(0)
    for _ in range(50):
        k0, k1, w = (int(v) for v in rng.integers(0, 1 << 32, 3))
        seed, r, st = int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 16)), int(rng.integers(0, 2))
        assert int(O.sr_hash(k0, k1, w)) == _h(k0, k1, w)
        assert O.sr_key(seed, r, st) == _key(seed, r, st)
        assert O.sr_step_seed(seed, w, r) == _step_seed(seed, w, r)
    # one word serves 4 consecutive elements, a byte each, whatever the base
    key = _key(99, 3, 0)
    b = O.sr_bytes(key, 64, 32)
    assert [int(v) for v in b] == [(_h(*key, i >> 2) >> (8 * (i & 3))) & 0xFF for i in range(64, 96)]


def _mixed_input(n=4096, seed=3):
    """Normal values under a log-normal scale, with groups of zeros and of denormals mixed in."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 2)).astype(np.float32)
    x[16:32] = 0
    x[48:64] = (rng.standard_normal(16) * 1e-41).astype(np.float32)
    x[80:96] *= np.float32(1e-30)
    return x


@pytest.mark.parametrize("codec", CODECS)
def test_q_is_floor_or_floor_plus_one(codec):
    top, qmax = TOP[codec]
    x = _mixed_input()
    E = (np.abs(x).reshape(-1, 16).view(np.uint32).max(axis=1) >> 23).astype(np.int64)
    t = np.ldexp(x.astype(np.float64).reshape(-1, 16), (top - E)[:, None]).reshape(-1)  # exact
    lo, hi = np.clip(np.floor(t), -qmax, qmax), np.clip(np.floor(t) + 1, -qmax, qmax)
    ups = 0
    for seed in (0, 1, 0xDEADBEEF12345678):
        q, E2 = O.sr_encode_groups(x, codec, O.sr_key(seed, 2, 0), 4096)
        assert np.array_equal(E2, E.astype(np.uint8))
        assert np.all((q == lo) | (q == hi))
        ups += int(np.sum((q == hi) & (lo != hi)))
        # the plain-Python definition, element by element, on a slice
        key = _key(seed, 2, 0)
        for i in range(0, 200):
            f = math.floor(t[i])
            d = np.float32(np.float32(t[i]) - np.float32(f))
            u = ((_h(*key, (4096 + i) >> 2) >> (8 * (i & 3)) & 0xFF) + 0.5) / 256
            assert int(q[i]) == max(-qmax, min(qmax, f + (1 if d > u else 0))), (seed, i)
    assert ups > 1000, "both outcomes occur"


@pytest.mark.parametrize("codec", CODECS)
def test_exactly_representable_values_are_unchanged(codec):
    top, qmax = TOP[codec]
    rng = np.random.default_rng(4)
    q = rng.integers(-qmax, qmax + 1, 2048).astype(np.float32)
    q.reshape(-1, 16)[:, 0] = qmax  # every group's exponent is that of its first value
    scale = np.repeat(rng.integers(-30, 30, 128), 16)
    x = np.ldexp(q, scale).astype(np.float32)
    for seed in (0, 1, 2, 0xFFFFFFFFFFFFFFFF, 123456789123456789):
        for r, st in ((0, 0), (5, 1)):
            assert np.array_equal(O.sr_quantize(x, codec, O.sr_key(seed, r, st), 256), x)
        assert np.array_equal(sim.mesh_allreduce_sr([x], x.size, codec, seed), x)
    assert np.array_equal(O.quantize(x, codec), x)


@pytest.mark.parametrize("codec", CODECS)
def test_nonfinite_group_takes_the_rne_bytes(codec):
    x = _mixed_input(1024)
    x[0:16] = np.float32(3e38) * np.linspace(-1, 1, 16, dtype=np.float32)
    x[5] = np.nan
    x[32:48] = np.linspace(-1e38, 1e38, 16, dtype=np.float32)
    x[40] = np.inf
    x[41] = -np.inf
    w_rne = O.pack(x, 512, codec)
    sb = O.shard_bytes(codec, 512)
    per = 16 if codec == "bfp_rne" else 8
    for seed in (0, 7):
        w = O.sr_pack(x, 512, codec, seed, 1)
        assert w.shape == w_rne.shape
        for g in (0, 2):
            assert np.array_equal(w[g * per:(g + 1) * per], w_rne[g * per:(g + 1) * per])
        assert w[sb - 32] == 255 and w[sb - 30] == 255
        assert not np.array_equal(w[:sb], w_rne[:sb]), "the finite groups are rounded stochastically"
        assert np.array_equal(w[sb - 32:sb], w_rne[sb - 32:sb]), "the exponent plane is the rne encoder's"


def test_own_shard_is_plain_rne_and_keys_differ():
    rng = np.random.default_rng(5)
    s, N = 256, 3
    g = rng.standard_normal(s * N).astype(np.float32)
    for codec in CODECS:
        sb = O.shard_bytes(codec, s)
        plain = O.pack(g, s, codec)
        for r in range(N):
            w = O.sr_pack(g, s, codec, 11, r, self_shard=r)
            assert np.array_equal(w[r * sb:(r + 1) * sb], plain[r * sb:(r + 1) * sb])
            for q in range(N):
                if q != r:
                    assert not np.array_equal(w[q * sb:(q + 1) * sb], plain[q * sb:(q + 1) * sb])
                    # the shard alone, at its place in the bucket: the same bytes
                    assert np.array_equal(w[q * sb:(q + 1) * sb],
                                          O.sr_pack(g[q * s:(q + 1) * s], s, codec, 11, r, base=q * s))
        a, b, c = O.sr_pack(g, s, codec, 11, 0), O.sr_pack(g, s, codec, 11, 1), O.sr_pack(g, s, codec, 12, 0)
        assert not np.array_equal(a, b) and not np.array_equal(a, c)
        slots = [a[q * sb:(q + 1) * sb] for q in range(N)]
        assert not np.array_equal(O.sr_reduce(slots, g[:s], 0, codec, s, 11, 0), O.sr_pack(
            O.reduce_slots(slots, g[:s], 0, codec, s), s, codec, 11, 0)), "the stages draw from different keys"


# --------------------------------------------------------------------------- unbiasedness
def _unbiased_input():
    """n = 4096, per-group scale s = 2^k with k in [-20, 5), values uniform in [-s, s], one element of each group set
    to +-s: every |t| is at most 64 (8-bit) or 4 (4-bit), nothing saturates and no element is left out."""
    rng = np.random.default_rng(2026)
    n = 4096
    s = np.ldexp(1.0, rng.integers(-20, 5, n // 16)).astype(np.float32)
    x = (rng.uniform(-1, 1, (n // 16, 16)) * s[:, None]).astype(np.float32)
    x[np.arange(n // 16), rng.integers(0, 16, n // 16)] = s * rng.choice([-1.0, 1.0], n // 16).astype(np.float32)
    return x.reshape(-1), np.repeat(s, 16).astype(np.float64)


def _hoeffding(n, T):
    return math.sqrt(math.log(2 * n / 1e-9) / (2 * T)) + 2.0 ** -9


def _mean_decoded(x, codec, T, stage):
    acc = np.zeros(x.size, np.float64)
    for t in range(T):
        acc += O.sr_quantize(x, codec, O.sr_key(O.sr_step_seed(1234, t, 0), 0, stage), 0)
    return acc / T


@pytest.mark.parametrize("codec", CODECS)
def test_unbiased(codec):
    """max over elements of |mean of T decoded values - x| / step <= sqrt(ln(2n / 1e-9) / (2T)) + 2^-9: Hoeffding for a
    mean of T values in an interval of one step, a union bound over the n elements at total probability 1e-9, plus the
    resolution of the 8-bit threshold (u sits on a grid of 1/256, so the expectation is off by at most 1/512 step)."""
    x, s = _unbiased_input()
    n = x.size
    step = s / (64 if codec == "bfp_rne" else 4)
    assert abs(_hoeffding(n, 256) - 0.243) < 5e-4
    for T in (16, 64, 256, 1024):
        err = float(np.max(np.abs(_mean_decoded(x, codec, T, 0) - x) / step))
        print(f"unbiased {codec} T={T}: max |mean - x| / step = {err:.3f} (bound {_hoeffding(n, T):.3f})")
        if T == 256:
            got = err
        assert err <= _hoeffding(n, T)
    assert got <= 0.243
    # the owner stage's key, through the simulator at one rank
    acc = np.zeros(n, np.float64)
    for t in range(256):
        acc += sim.mesh_allreduce_sr([x], n, codec, O.sr_step_seed(1234, t, 0))
    err = float(np.max(np.abs(acc / 256 - x) / step))
    print(f"unbiased {codec} simulator, one rank, T=256: {err:.3f}")
    assert err <= _hoeffding(n, 256)


def test_readme_metric_printed():
    """The README's constant-gradient figure (normal values under a log-normal scale, constant over T steps; max over
    elements of |mean of the decoded values - g| / group max), stochastic rounding beside round-to-nearest. Printed,
    not asserted: on this input a group's largest value can sit above qmax steps, where the clamp is a bias that no
    number of steps removes (the unbiasedness test's input has no such element)."""
    rng = np.random.default_rng(0)
    n = 4096
    g = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 2)).astype(np.float32)
    gmax = np.repeat(np.abs(g).reshape(-1, 16).max(axis=1), 16).astype(np.float64)
    for codec in CODECS:
        top, qmax = TOP[codec]
        E = np.repeat(np.abs(g).reshape(-1, 16).view(np.uint32).max(axis=1) >> 23, 16).astype(np.int64)
        inside = np.abs(np.ldexp(g.astype(np.float64), top - E)) <= qmax  # the elements the clamp leaves alone
        rne = np.abs(O.quantize(g, codec).astype(np.float64) - g) / gmax
        row, row_in = [], []
        for T in (16, 64, 256):
            err = np.abs(_mean_decoded(g, codec, T, 0) - g) / gmax
            row.append(float(err.max()))
            row_in.append(float(err[inside].max()))
        print(f"README metric {codec}: rne {rne.max():.3g}; stochastic T=16 {row[0]:.3g}, T=64 {row[1]:.3g}, "
              f"T=256 {row[2]:.3g}; over the {int(inside.sum())} of {n} elements at or below qmax steps: rne "
              f"{rne[inside].max():.3g}; stochastic {row_in[0]:.3g}, {row_in[1]:.3g}, {row_in[2]:.3g}")
        assert all(math.isfinite(v) for v in row + row_in)


# --------------------------------------------------------------------------- wire ops (CPU path)
@pytest.mark.parametrize("codec", CODECS)
def test_wire_ops_cpu_follow_the_oracle(codec):
    rng = np.random.default_rng(6)
    s, N = 256, 3
    g = rng.standard_normal(s * N).astype(np.float32)
    sb = O.shard_bytes(codec, s)
    for dt in (torch.float32, torch.bfloat16):
        x = torch.from_numpy(g).to(dt)
        gv = x.float().numpy()
        out = torch.full((sb * N + 8,), 0xAB, dtype=torch.uint8)
        wire.pack_sr(x, out[: sb * N], s, codec, 77, 1, self_shard=1, base=s * N)
        assert np.array_equal(out[: sb * N].numpy(), O.sr_pack(gv, s, codec, 77, 1, 1, s * N))
        assert torch.all(out[sb * N:] == 0xAB)
        d = [torch.zeros(sb, dtype=torch.uint8), None, torch.zeros(sb, dtype=torch.uint8)]
        wire.pack_sr(x, d, s, codec, 77, 0)
        ref = O.sr_pack(gv, s, codec, 77, 0)
        assert np.array_equal(d[0].numpy(), ref[:sb]) and np.array_equal(d[2].numpy(), ref[2 * sb:])
        slots = torch.from_numpy(O.pack(g, s, codec))
        o1, o2 = torch.zeros(sb, dtype=torch.uint8), torch.zeros(sb, dtype=torch.uint8)
        wire.reduce_sr(slots, N, 2, x[:s], [o1, None, o2], s, codec, 5, 2, base=2 * s)
        refr = O.sr_reduce([slots.numpy()[r * sb:(r + 1) * sb] for r in range(N)], gv[:s], 2, codec, s, 5, 2, 2 * s)
        assert np.array_equal(o1.numpy(), refr) and np.array_equal(o2.numpy(), refr)
    with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
        wire.pack_sr(torch.zeros(256), torch.zeros(512, dtype=torch.uint8), 256, "bfp_trunc", 0, 0)
    with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
        wire.reduce_sr(torch.zeros(1024, dtype=torch.uint8), 1, 0, torch.zeros(256), torch.zeros(1024, dtype=torch.uint8),
                       256, "raw_f32", 0, 0)
    for bad in (-1, 1 << 64, 1.5, "3", None, True):
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            wire.pack_sr(torch.zeros(256), torch.zeros(512, dtype=torch.uint8), 256, codec, bad, 0)
    with pytest.raises(ValueError, match="2\\^32 or more"):
        wire.pack_sr(torch.zeros(256), torch.zeros(512, dtype=torch.uint8), 256, codec, 0, 0, base=(1 << 32) - 240)
    wire.pack_sr(torch.zeros(256), torch.zeros(512, dtype=torch.uint8), 256, codec, M64, 15, base=(1 << 32) - 256)
    with pytest.raises(ValueError, match="local operand"):
        wire.reduce_sr(torch.zeros(512, dtype=torch.uint8), 1, 0, None, torch.zeros(512, dtype=torch.uint8), 256, codec,
                       0, 0)


# --------------------------------------------------------------------------- Python engine against the simulator
def _grads(N, n, seed, dt):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32) * (1 + r)).to(dt)
            for r in range(N)]


def _engine_run(t, grads, n, codec, seeds, **kw):
    eng = CompressedAllReduce(t, codec=codec, device="cpu", **kw)
    L = eng.layout(n)
    outs = []
    for seed in seeds:
        g = torch.zeros(L.n_pad, dtype=grads[t.rank].dtype)
        g[:n] = grads[t.rank]
        out = torch.zeros(L.n_pad)
        eng.allreduce(g, out, n_valid=n, **({} if seed is None else dict(sr_seed=seed))).synchronize()
        outs.append(out.numpy().copy())
    return outs, L.shard


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_python_engine_matches_the_simulator(N, codec, dt):
    n = 1000
    grads = _grads(N, n, 40 + N, dt)
    seeds = [O.sr_step_seed(9, 1, 0), O.sr_step_seed(9, 1, 0), O.sr_step_seed(9, 2, 0), None]
    if N == 1:
        res = [_engine_run(ThreadFabric(1).transport(0), grads, n, codec, seeds)]
    else:
        res = ThreadFabric(N, timeout_s=60).run(lambda t: _engine_run(t, grads, n, codec, seeds))
    shard = res[0][1]
    gin = [np.pad(g.float().numpy(), (0, shard * N - n)) for g in grads]
    ref = [sim.mesh_allreduce_sr(gin, shard, codec, s) for s in seeds[:3]] + [sim.mesh_allreduce(gin, shard, codec)]
    for r in range(N):
        outs = res[r][0]
        for k in range(4):
            assert np.array_equal(outs[k], ref[k]), (r, k)  # (hence replicas identical, and today's bits unflagged)
        assert np.array_equal(outs[0], outs[1]), "the same seed gives the same bits"
        # another seed, or none, gives other decoded values, hence other wire bytes
        assert not np.array_equal(outs[0], outs[2]) and not np.array_equal(outs[0], outs[3])


def test_python_engine_one_rank_forced_and_update_request():
    """World 1 through the multi-rank path is the owner stage alone, as inline; allreduce_sgd takes the seed too."""
    n, codec = 700, "bfp_rne"
    grads = _grads(1, n, 50, torch.float32)
    a, shard = _engine_run(ThreadFabric(1).transport(0), grads, n, codec, [3])
    b, _ = _engine_run(ThreadFabric(1).transport(0), grads, n, codec, [3], force_comm=True)
    ref = O.sr_quantize(np.pad(grads[0].numpy(), (0, shard - n)), codec, O.sr_key(3, 0, 1), 0)
    assert np.array_equal(a[0], ref) and np.array_equal(b[0], ref)
    eng = CompressedAllReduce(ThreadFabric(1).transport(0), codec=codec, device="cpu")
    g, w = torch.zeros(shard), torch.zeros(shard)
    g[:n] = grads[0]
    eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, sr_seed=3).synchronize()
    assert np.array_equal(w.numpy()[:n], -ref[:n])


# --------------------------------------------------------------------------- refusals
def _eng(**kw):
    return CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu", **kw)


def test_sr_request_and_engine_refusals():
    n = 100
    eng = _eng()
    L = eng.layout(n)
    g, w, out = torch.ones(L.n_pad), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
    kw = dict(codec_id=1, algo="mesh", world=2)
    assert sr_request(None, L, **kw) is None
    assert sr_request(5, L, **kw) == 5 and sr_request(np.int64(5), L, **{**kw, "codec_id": 4}) == 5
    assert sr_request(M64, L, **kw) == M64
    for cid, name in ((0, "bfp_trunc"), (2, "raw_f32"), (3, "raw_bf16")):
        with pytest.raises(ValueError, match=f"bfp_rne and bfp4_rne only, got '{name}'"):
            sr_request(5, L, **{**kw, "codec_id": cid})
    with pytest.raises(ValueError, match="prepacked"):
        sr_request(5, L, **kw, prepacked=True)
    with pytest.raises(ValueError, match="ring schedule"):
        sr_request(5, L, **{**kw, "algo": "ring"})
    with pytest.raises(ValueError, match="chunked"):
        sr_request(5, BucketLayout(n=n, n_pad=L.n_pad, algo="mesh", world=1, shard=128, chunks=2), **kw)
    with pytest.raises(ValueError, match="sharded"):
        sr_request(5, L, **kw, sharded=True)
    with pytest.raises(ValueError, match="pick one"):
        sr_request(5, L, **kw, residual=torch.zeros(L.n_pad))
    for bad in (-1, 1 << 64, 0.5, "1", True):
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            sr_request(bad, L, **kw)
    with pytest.raises(ValueError, match="at most 16 ranks"):
        sr_request(5, L, **{**kw, "world": 17})
    big = 1 << 32
    for n_pad in (big, big + 512):
        with pytest.raises(ValueError, match="2\\^32 or more"):
            sr_request(5, BucketLayout(n=n_pad - 3, n_pad=n_pad, algo="mesh", world=2, shard=n_pad // 2, chunks=1), **kw)
    assert sr_request(5, BucketLayout(n=big - 515, n_pad=big - 512, algo="mesh", world=2, shard=big // 2 - 256,
                                      chunks=1), **kw) == 5
    # through the engine's two entry points
    for codec in ("bfp_trunc", "raw_f32", "raw_bf16"):
        with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
            _eng(codec=codec).allreduce_sgd(g, w, n_valid=n, lr=1.0, sr_seed=1)
        with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
            _eng(codec=codec).allreduce(g, out, n_valid=n, sr_seed=1)
    ring = _eng(algo="ring")
    with pytest.raises(ValueError, match="ring schedule"):
        ring.allreduce_sgd(torch.ones(ring.layout(n).n_pad), w, n_valid=n, lr=1.0, sr_seed=1)
    with pytest.raises(ValueError, match="pick one"):
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, sr_seed=1, residual=torch.zeros(L.n_pad))
    with pytest.raises(ValueError, match="pick one"):
        eng.allreduce(g, out, n_valid=n, sr_seed=1, residual=torch.zeros(L.n_pad))
    with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, sr_seed=-3)
    assert not w.any() and not out.any(), "refused: nothing ran"
    eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, sr_seed=0).synchronize()  # an ordinary request still completes
    assert torch.all(w[:n] == -1.0), "1.0 is representable: unchanged whatever the seed"


def test_trainer_refusals():
    model = MLP([32, 32], dtype=torch.float32)

    class Fake:  # what the trainer reads of an engine
        world, codec, algo, shard_update = 2, "bfp_rne", "mesh", False

        def layout(self, n):
            return type("L", (), {"chunks": 1, "n_pad": (n + 511) // 512 * 512})()

    sr = dict(stochastic_rounding=True)
    with pytest.raises(ValueError, match="ring"):
        DataParallelTrainer(model, type("Ring", (Fake,), {"algo": "ring"})(), **sr)
    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, type("Sh", (Fake,), {"shard_update": True})(), **sr)
    for codec in ("raw_f32", "raw_bf16", "bfp_trunc"):
        with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
            DataParallelTrainer(model, type("C", (Fake,), {"codec": codec})(), **sr)
    with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
        DataParallelTrainer(model, RcclAllReduce(ThreadFabric(1).transport(0), device="cpu"), **sr)
    with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
        DataParallelTrainer(model, None, error_feedback_codec="bfp_trunc", **sr)
    with pytest.raises(ValueError, match="at most 16 ranks"):
        DataParallelTrainer(model, type("W", (Fake,), {"world": 17})(), **sr)

    class Chunked(Fake):
        def layout(self, n):
            return type("L", (), {"chunks": 2, "n_pad": n})()

    with pytest.raises(ValueError, match="chunked"):
        DataParallelTrainer(model, Chunked(), **sr)
    with pytest.raises(ValueError, match="pick one"):
        DataParallelTrainer(model, Fake(), error_feedback=True, **sr)
    for bad in (-1, 1 << 64, 2.0):
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            DataParallelTrainer(model, Fake(), sr_seed=bad, **sr)
    tr = DataParallelTrainer(model, None)
    assert not tr.stochastic_rounding and tr.sr_step == 0
    assert DataParallelTrainer(model, Fake(), sr_seed=M64, **sr).sr_seed == M64


# --------------------------------------------------------------------------- trainer
def _data(sizes, mb=16):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(mb, sizes[0], generator=g) * 2 - 1,
            torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32))


def _train(engine_kind, steps=3, codec="bfp_rne", **kw):
    sizes = [32, 64, 32]
    eng = None if engine_kind == "none" else _eng(codec=codec)
    pad = (lambda n: eng.layout(n).n_pad) if eng is not None else None
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True, momentum=True, adam=kw.get("optimizer") == "adamw",
                pad_fn=pad)
    tr = DataParallelTrainer(model, eng, lr=0.05, error_feedback_codec=codec, **kw)
    x, y = _data(sizes)
    hist = []
    for _ in range(steps):
        tr.step(x, y)
        tr.finish()
        hist.append([l.master.numpy().copy() for l in model.layers])
    return model, tr, hist


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw", trust_ratio=True, max_grad_norm=0.05)],
                         ids=["sgd", "lamb_clip"])
@pytest.mark.parametrize("codec", CODECS)
def test_trainer_local_and_python_engine_agree(codec, kw):
    """One rank: the engine-less trainer's one-slot round trip is the inline engine's owner stage."""
    sr = dict(stochastic_rounding=True, sr_seed=77, codec=codec)
    _, tl, hl = _train("none", **sr, **kw)
    _, te, he = _train("python", **sr, **kw)
    assert tl.sr_step == te.sr_step == 3 and not te.prepack
    assert _same(hl, he)
    assert _same(he, _train("python", **sr, **kw)[2]), "deterministic under a repeat"
    assert not _same(he[:1], _train("python", codec=codec, **kw)[2][:1]), "differs from the unflagged run at step 1"
    assert not _same(he[:1], _train("python", **{**sr, "sr_seed": 78}, **kw)[2][:1]), "the seed matters"


def test_trainer_flag_off_is_the_trainer_without_it():
    assert _same(_train("python", stochastic_rounding=False, sr_seed=5)[2], _train("python")[2])
    assert _same(_train("none", stochastic_rounding=False)[2], _train("none")[2])


def test_trainer_local_step_matches_oracle():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True)
    tr = DataParallelTrainer(model, None, lr=0.05, stochastic_rounding=True, sr_seed=1 << 40)
    x, y = _data(sizes)
    for step in (1, 2):
        prev = [l.master.numpy().copy() for l in model.layers]
        tr.step(x, y)
        tr.finish()
        assert tr.sr_step == step
        for i, l in enumerate(model.layers):
            seed = _step_seed(1 << 40, step, i)
            q = O.sr_quantize(l.grad.numpy(), "bfp_rne", _key(seed, 0, 1), 0)
            w, _ = O.sgd(prev[i][: l.n], q[: l.n], 0.05)
            assert np.array_equal(l.master.numpy()[: l.n], w)


# --------------------------------------------------------------------------- CLI and checkpoint
ARGS = ["32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0"]


def _cli(iters, *flags):
    out = io.StringIO()
    r = mlp_mpi.run([str(iters)] + ARGS + list(flags), out=out)
    assert out.getvalue()
    return r["trainer"], [l.master.numpy().copy() for l in r["model"].layers]


def test_cli_flag_and_refusals():
    parse = lambda *f: mlp_mpi.config_from_args(mlp_mpi.build_parser().parse_args(["1"] + ARGS + list(f)))  # noqa: E731
    c = parse("--stochastic-rounding", "--sr-seed", "12")
    assert c.stochastic_rounding and c.sr_seed == 12 and not parse().stochastic_rounding and parse().sr_seed == 0
    t_sr, w_sr = _cli(1, "--stochastic-rounding", "--sr-seed", "12")
    t_no, w_no = _cli(1)
    assert t_sr.stochastic_rounding and t_sr.sr_seed == 12 and t_sr.sr_step == 1 and not t_no.stochastic_rounding
    assert not all(np.array_equal(a, b) for a, b in zip(w_sr, w_no))
    assert all(np.array_equal(a, b) for a, b in zip(w_sr, _cli(1, "--stochastic-rounding", "--sr-seed", "12")[1]))
    assert not all(np.array_equal(a, b) for a, b in zip(w_sr, _cli(1, "--stochastic-rounding", "--sr-seed", "13")[1]))
    t4, _ = _cli(1, "--stochastic-rounding", "--compress", "bfp4")
    assert t4.engine.codec == "bfp4_rne" and t4.stochastic_rounding
    t_loc, _ = _cli(1, "--stochastic-rounding", "--compress", "local")
    assert t_loc.engine is None and t_loc.ef_codec == "bfp_rne"
    for flags, match in ((["--rounding", "trunc"], "bfp_rne and bfp4_rne only"),
                         (["--compress", "raw"], "bfp_rne and bfp4_rne only"),
                         (["--compress", "raw_bf16"], "bfp_rne and bfp4_rne only"),
                         (["--compress", "local", "--rounding", "trunc"], "bfp_rne and bfp4_rne only"),
                         (["--algo", "ring"], "ring"),
                         (["--error-feedback"], "pick one"),
                         (["--sr-seed", "-1"], r"\[0, 2\^64\)"),
                         (["--sr-seed", str(1 << 64)], r"\[0, 2\^64\)")):
        with pytest.raises(ValueError, match=match):
            _cli(1, "--stochastic-rounding", *flags)
    help_text = mlp_mpi.build_parser().format_help().replace("\n", " ")
    assert "--stochastic-rounding" in help_text and "--sr-seed" in help_text


def test_checkpoint_carries_the_counter(tmp_path):
    """The counter round-trips through --checkpoint / --resume, and a resumed run's next step is bit-identical to the
    uninterrupted run's; a checkpoint of a run without the flag is unchanged (no counter in its index)."""
    ck = str(tmp_path / "ck")
    sr = ["--stochastic-rounding", "--sr-seed", "21", "--momentum", "0.9"]
    t2, _ = _cli(2, *sr, "--checkpoint", ck)
    assert t2.sr_step == 2
    with open(ck + ".json") as f:
        assert json.load(f)["sr_step"] == 2
    t_res, w_res = _cli(1, *sr, "--resume", ck)
    t3, w3 = _cli(3, *sr)
    assert t_res.sr_step == t3.sr_step == 3
    assert all(np.array_equal(a, b) for a, b in zip(w_res, w3))
    # a resumed run that lost the counter draws step 1's seeds again: other bits
    with open(ck + ".json") as f:
        info = json.load(f)
    del info["sr_step"]
    with open(ck + ".json", "w") as f:
        json.dump(info, f)
    t_lost, w_lost = _cli(1, *sr, "--resume", ck)
    assert t_lost.sr_step == 1 and not all(np.array_equal(a, b) for a, b in zip(w_lost, w3))
    plain = str(tmp_path / "plain")
    _cli(1, "--checkpoint", plain)
    with open(plain + ".json") as f:
        assert "sr_step" not in json.load(f)
