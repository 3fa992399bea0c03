"""AdamW's moments in 8-bit block floating point (moment_codec="bfp8") on the CPU: the plane format, the statistics of
the stochastic store, the toy-problem trajectory, the Python engine, trainer, CLI and checkpoint (no GPU)."""
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
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce, moment_request
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

M64 = (1 << 64) - 1
KEY_M = lambda seed: O.sr_key(seed, 16, 0)  # noqa: E731
KEY_R = lambda seed: O.sr_key(seed, 16, 1)  # noqa: E731


def _scalars(step, wd=0.01):
    return O.adamw_scalars(1e-2, wd, 0.9, 0.999, 1e-8, step)


def _group_step(plane):
    """One mantissa step 2^(E-133) of every element's group of a plane."""
    plane = np.asarray(plane, np.uint8)
    n = plane.size // 17 * 16
    return np.repeat(np.ldexp(1.0, plane[n:].astype(np.int64) - 133), 16)


# --------------------------------------------------------------------------- format
def test_plane_is_one_packed_shard_and_zero_is_the_zero_state():
    n_pad = 768
    assert O.moment_plane_bytes(n_pad) == n_pad * 17 // 16 == O.shard_bytes("bfp_rne", n_pad)
    z = wire.moment_plane(n_pad, "cpu")
    assert z.dtype == torch.uint8 and z.numel() == 816 and not z.any()
    assert not O.moment_decode(z.numpy()).any() and not wire.moment_decode(z).any()
    # values the codec holds exactly: the stochastic encoder stores them as pack() does, whatever the random bytes
    rng = np.random.default_rng(0)
    q = rng.integers(-127, 128, n_pad)
    q[::16] = 64 * rng.choice([-1, 1], n_pad // 16)  # (pins each group's exponent)
    q = np.clip(q.reshape(-1, 16), -127, 127).reshape(-1)
    x = (q * np.repeat(np.ldexp(1.0, rng.integers(-30, 10, n_pad // 16)), 16)).astype(np.float32)
    x.reshape(-1, 16)[:, 0] = np.sign(x.reshape(-1, 16)[:, 0]) * np.abs(x.reshape(-1, 16)).max(axis=1)
    x = O.quantize(x, "bfp_rne")
    qm, E = O.moment_encode(x, KEY_M(5), 0, False)
    plane = np.concatenate([qm.view(np.uint8), E])
    assert np.array_equal(plane, O.pack(x, n_pad, "bfp_rne"))
    assert np.array_equal(O.moment_decode(plane), x)
    assert np.array_equal(wire.moment_decode(torch.from_numpy(plane)).numpy(), x)
    for bad in (100, 255):
        with pytest.raises(ValueError, match="multiple of 256"):
            O.moment_plane_bytes(bad)
    with pytest.raises(ValueError, match=r"2\^32 or more"):
        O.moment_plane_bytes(1 << 32)
    assert O.moment_plane_bytes((1 << 32) - 256) == ((1 << 32) - 256) * 17 // 16


def test_stored_values_are_within_one_step_and_r_is_never_zero():
    rng = np.random.default_rng(3)
    n_pad, n = 1024, 1024 - 16 - 5
    g = (rng.standard_normal(n_pad) * np.exp(2 * rng.standard_normal(n_pad))).astype(np.float32)
    g[40:56] = 0  # a group whose r' is 0: stored as 0, no floor
    w0 = rng.standard_normal(n_pad).astype(np.float32)
    mq, vq = (np.zeros(O.moment_plane_bytes(n_pad), np.uint8) for _ in range(2))
    saw_floor = False
    for step in (1, 2, 3):
        s = _scalars(step)
        m_old, r_old = O.moment_decode(mq), O.moment_decode(vq)
        w1, m1, v1 = O.adamw(w0, g, m_old, (r_old * r_old).astype(np.float32), s)
        r1 = np.sqrt(v1.astype(np.float64)).astype(np.float32)
        w2, mq, vq = O.adamw_q(w0, g, mq, vq, s, 1.0, 11 * step, n_valid=n)
        assert np.array_equal(w2[:n], w1[:n]) and np.array_equal(w2[n:], w0[n:])
        dm, dr = O.moment_decode(mq), O.moment_decode(vq)
        assert np.all(np.abs(dm[:n] - m1[:n]) < _group_step(mq)[:n])
        assert np.all(dr[:n][r1[:n] > 0] > 0), "a positive r' is never stored as 0"
        lifted = (r1[:n] > 0) & (r1[:n] < _group_step(vq)[:n])
        saw_floor |= bool(np.any(lifted & (dr[:n] == _group_step(vq)[:n])))
        ok = np.abs(dr[:n] - r1[:n]) < _group_step(vq)[:n]
        assert np.all(ok), "within one step (the floor lifts a value below one step to exactly one step)"
        assert not dm[40:56].any() and not dr[40:56].any()
        assert not dm[n:].any() and not dr[n:].any(), "values at or past n_valid enter the encode as 0"
        w0 = w2
    assert saw_floor, "the input exercises the floor"
    # the planes' bytes: the two encoders under rank slot 16
    q, E = O.moment_encode(np.where(np.arange(n_pad) < n, m1, 0).astype(np.float32), KEY_M(33), 0, False)
    assert np.array_equal(mq, np.concatenate([q.view(np.uint8), E]))
    q, E = O.moment_encode(np.where(np.arange(n_pad) < n, r1, 0).astype(np.float32), KEY_R(33), 0, True)
    assert np.array_equal(vq, np.concatenate([q.view(np.uint8), E]))
    qs, _ = O.sr_encode_groups(np.where(np.arange(n_pad) < n, r1, 0).astype(np.float32), "bfp_rne", KEY_R(33), 0)
    assert np.array_equal(q, np.where((qs == 0) & (r1 > 0) & (np.arange(n_pad) < n), 1, qs))


def test_nonfinite_group_stores_exponent_255_and_propagates():
    n_pad = 256
    g = np.ones(n_pad, np.float32)
    g[35] = np.inf
    g[70] = np.nan
    mq, vq = (np.zeros(O.moment_plane_bytes(n_pad), np.uint8) for _ in range(2))
    w, mq, vq = O.adamw_q(np.zeros(n_pad, np.float32), g, mq, vq, _scalars(1), 1.0, 1)
    for plane in (mq, vq):
        E = plane[n_pad:]
        assert E[2] == 255 and E[4] == 255 and np.all(np.delete(E, [2, 4]) != 255)
        d = O.moment_decode(plane)
        assert np.isnan(d[32:48]).all() and np.isnan(d[64:80]).all() and np.isfinite(np.delete(d, np.r_[32:48, 64:80])).all()
    # E == 255 takes the rne encoder's bytes unchanged
    z = np.zeros(n_pad, np.float32)
    _, m1, v1 = O.adamw(z, g, z, z, _scalars(1))
    assert np.array_equal(mq[32:48].view(np.int8), O.encode_groups(m1)[0][32:48])
    assert np.array_equal(vq[32:48].view(np.int8), O.encode_groups(np.sqrt(v1))[0][32:48])
    # the state stays non-finite, as an f32 state would
    w, mq, vq = O.adamw_q(w, np.ones(n_pad, np.float32), mq, vq, _scalars(2), 1.0, 2)
    assert np.isnan(O.moment_decode(mq)[32:48]).all() and np.isnan(w[32:48]).all() and np.isfinite(w[:32]).all()


def test_bits_do_not_depend_on_the_region_split():
    rng = np.random.default_rng(8)
    n_pad, n = 1024, 1000
    g = rng.standard_normal(n_pad).astype(np.float32)
    w0 = rng.standard_normal(n_pad).astype(np.float32)
    z = np.zeros(O.moment_plane_bytes(n_pad), np.uint8)
    s = _scalars(1)
    w1, m1, v1 = O.adamw_q(w0, g, z, z, s, 0.5, 9, n_valid=n)
    wa, ma, va = O.adamw_q(w0[:512], g[:512], z, z, s, 0.5, 9, base=0)
    wb, mb, vb = O.adamw_q(w0[512:], g[512:], ma, va, s, 0.5, 9, n_valid=n - 512, base=512)
    assert np.array_equal(np.concatenate([wa, wb]), w1) and np.array_equal(mb, m1) and np.array_equal(vb, v1)
    # the wire op's CPU path: shards, a skipped shard, elem_base into larger planes
    for codec in ("bfp_rne", "bfp4_rne", "raw_f32", "raw_bf16", "bfp_trunc"):
        buf = torch.from_numpy(O.pack(g[:768], 256, codec))
        dec = O.unpack(buf.numpy(), 768, 256, codec)
        master = torch.from_numpy(w0[:768].copy())
        lp = torch.zeros(768, dtype=torch.bfloat16)
        pm, pv = wire.moment_plane(n_pad, "cpu"), wire.moment_plane(n_pad, "cpu")
        wire.adamw_q(buf, 256, 3, master, codec=codec, mom_q=pm, var_q=pv, scalars=s, seed=9, lp=lp, grad_scale=0.5,
                     n_valid=700, skip_shard=1, skip_period=2, elem_base=256)
        wr, mr, vr = O.adamw_q(w0[:256], dec[:256], z, z, s, 0.5, 9, base=256)
        wr2, mr, vr = O.adamw_q(w0[512:768], dec[512:768], mr, vr, s, 0.5, 9, n_valid=700 - 512, base=768)
        ref = np.concatenate([wr, w0[256:512], wr2])
        assert np.array_equal(master.numpy(), ref), codec
        assert np.array_equal(pm.numpy(), mr) and np.array_equal(pv.numpy(), vr), codec
        assert np.array_equal(lp[:256].float().numpy(), O.bf16_bits_to_f32(O.f32_to_bf16_bits(wr)))
        assert not lp[256:512].any() and not lp[700:].any()


# --------------------------------------------------------------------------- statistics of the store
def _unbiased_input():
    """The stochastic-rounding test's construction: n = 4096, per-group scale s = 2^k with k in [-20, 5), values uniform
    in [-s, s], one element of each group set to +-s: every |t| is at most 64, nothing saturates."""
    rng = np.random.default_rng(2026)
    n = 4096
    s = np.ldexp(1.0, rng.integers(-20, 5, n // 16)).astype(np.float32)
    x = (rng.uniform(-1, 1, (n // 16, 16)) * s[:, None]).astype(np.float32)
    x[np.arange(n // 16), rng.integers(0, 16, n // 16)] = s * rng.choice([-1.0, 1.0], n // 16).astype(np.float32)
    return x.reshape(-1), np.repeat(s, 16).astype(np.float64)


def _hoeffding(n, T):
    return math.sqrt(math.log(2 * n / 1e-9) / (2 * T)) + 2.0 ** -9


def test_m_store_is_unbiased():
    """max over elements of |mean of T decoded stores - x| / step <= sqrt(ln(2n / 1e-9) / (2T)) + 2^-9 at n = 4096,
    T = 256 seeds sr_step_seed(1234, t, 0) (Hoeffding for a mean of T values in an interval of one step, a union bound
    over the elements at total probability 1e-9, plus the 8-bit threshold's resolution)."""
    x, s = _unbiased_input()
    n, T = x.size, 256
    acc = np.zeros(n, np.float64)
    for t in range(T):
        q, E = O.moment_encode(x, KEY_M(O.sr_step_seed(1234, t, 0)), 0, False)
        acc += O.decode_groups(q, E, "rne")
    err = float(np.max(np.abs(acc / T - x) / (s / 64)))
    print(f"m store, T={T}: max |mean - x| / step = {err:.3f} (bound {_hoeffding(n, T):.3f})")
    assert abs(_hoeffding(n, T) - 0.243) < 5e-4
    assert err <= _hoeffding(n, T)
    # the state's random bytes are not the wire's: rank slot 16 is outside the wire's 0..15
    k = O.sr_step_seed(1234, 0, 0)
    assert all(not np.array_equal(O.sr_bytes(KEY_M(k), 0, 64), O.sr_bytes(O.sr_key(k, r, st), 0, 64))
               for r in range(16) for st in (0, 1))
    assert not np.array_equal(O.sr_bytes(KEY_M(k), 0, 64), O.sr_bytes(KEY_R(k), 0, 64))


def test_stagnation_control():
    """A constant gradient g = c * r0 (c = 3.96) from a state r0 whose mantissas lie in [48, 64] (each group's largest
    at 64), over K = 3 steps: per step r' = r * sqrt(0.999 + 0.001 c^2 (r0 / r)^2) moves r by at most 0.00734 r, i.e.
    0.35 (q = 48) to 0.47 (q = 64) of a mantissa step — below half a step, so the round-to-nearest store returns to r0
    every step and never moves, while the f32 recursion climbs about one step or more over the K steps.

    The mean over T = 256 seeds of the stochastically stored r follows the f32 recursion inside the unbiasedness test's
    bound, sqrt(ln(2n / 1e-9) / (2T)) + 2^-9 = 0.243 steps. That bound is Hoeffding's for ONE store; over K steps a
    seed's deviation is a sum of K rounding errors (each of conditional mean 0 and variance p (1 - p) <= 1/4 with p the
    fraction to be rounded, carried forward by factors dr'/dr in (0, 1]), so its guarantee at 1e-9 would be sqrt(K)
    wider. The recursion is therefore kept to 3 steps: the accumulated variance is at most 3/4 step^2, the seed-mean's
    standard deviation at most sqrt(0.75 / 256) = 0.054 steps, and the largest of 4096 such deviations is expected
    near 3.6 of them, 0.19 steps, with 3 * 2^-9 of threshold bias: inside 0.243, though not at Hoeffding's
    confidence. The seeds are fixed, so the outcome is deterministic."""
    rng = np.random.default_rng(77)
    n, K, T, c = 4096, 3, 256, np.float32(3.96)
    q0 = rng.integers(48, 65, (n // 16, 16))
    q0[np.arange(n // 16), rng.integers(0, 16, n // 16)] = 64
    quantum = np.ldexp(1.0, rng.integers(-24, 0, n // 16))
    r0 = (q0 * quantum[:, None]).astype(np.float32).reshape(-1)
    step = np.repeat(quantum, 16)
    g = (c * r0).astype(np.float32)
    plane0 = O.pack(r0, n, "bfp_rne")
    assert np.array_equal(O.moment_decode(plane0), r0)
    # f32 recursion, and the round-to-nearest store
    v = (r0 * r0).astype(np.float32)
    r_rne = r0.copy()
    for k in range(1, K + 1):
        s = _scalars(k, wd=0.0)
        v = O.adamw(0 * g, g, 0 * g, v, s)[2]
        v_rne = O.adamw(0 * g, g, 0 * g, (r_rne * r_rne).astype(np.float32), s)[2]
        r_rne = O.quantize(np.sqrt(v_rne.astype(np.float64)).astype(np.float32), "bfp_rne")
    rho = np.sqrt(v.astype(np.float64))
    moved = (rho - r0) / step
    assert np.array_equal(r_rne, r0), "the round-to-nearest store does not move"
    bound = _hoeffding(n, T)
    assert abs(bound - 0.243) < 5e-4
    assert moved.min() >= 3 * bound, (moved.min(), bound)
    acc = np.zeros(n, np.float64)
    for seed in range(T):
        mq, vq = np.zeros_like(plane0), plane0.copy()
        w = np.zeros(n, np.float32)
        for k in range(1, K + 1):
            w, mq, vq = O.adamw_q(w, g, mq, vq, _scalars(k, wd=0.0), 1.0, O.sr_step_seed(seed, k, 0))
        acc += O.moment_decode(vq)
    err = float(np.max(np.abs(acc / T - rho) / step))
    print(f"stagnation: f32 recursion moved {moved.min():.2f} .. {moved.max():.2f} steps in {K} updates; mean over {T} "
          f"seeds of the stochastic store off by {err:.3f} steps at most (bound {bound:.3f}); round-to-nearest store: "
          f"did not move")
    assert err <= bound


# --------------------------------------------------------------------------- trajectory
TOY_N, TOY_T = 4096, 400
TOY_SEEDS = (0, 7, 99, 5, 1, 2, 3, 4)
TOY_R = 1.333  # the largest loss_q(400) / loss_f32(400) over TOY_SEEDS, measured on the shipped oracle


def _toy(store):
    """n = 4096, rng = default_rng(1); h = exp(2 * normal), wstar = normal, w0 = 0; per step g = h * (w - wstar) + 0.3 *
    sqrt(h) * normal; AdamW lr 1e-2, betas (0.9, 0.999), eps 1e-8, wd 0, T = 400; loss 0.5 * sum(h * (w - wstar)^2).
    ``store(w, g, state, scalars, t)`` -> (w', state'). Returns ({100, 200, 400: loss}, largest |step|)."""
    rng = np.random.default_rng(1)
    h = np.exp(2 * rng.standard_normal(TOY_N))
    wstar = rng.standard_normal(TOY_N)
    w = np.zeros(TOY_N, np.float32)
    state, out, big = None, {}, 0.0
    for t in range(1, TOY_T + 1):
        g = (h * (w - wstar) + 0.3 * np.sqrt(h) * rng.standard_normal(TOY_N)).astype(np.float32)
        w2, state = store(w, g, state, O.adamw_scalars(1e-2, 0.0, 0.9, 0.999, 1e-8, t), t)
        with np.errstate(invalid="ignore", over="ignore"):
            big = max(big, float(np.nanmax(np.abs(w2 - w))))
        w = w2
        if t in (100, 200, 400):
            with np.errstate(invalid="ignore", over="ignore"):
                out[t] = float(0.5 * np.sum(h * (w - wstar) ** 2))
    return out, big


def _store_f32(w, g, st, s, t):
    m, v = st if st is not None else (np.zeros(TOY_N, np.float32),) * 2
    w2, m2, v2 = O.adamw(w, g, m, v, s)
    return w2, (m2, v2)


def _store_bfp8(base):
    def f(w, g, st, s, t):
        mq, vq = st if st is not None else (np.zeros(O.moment_plane_bytes(TOY_N), np.uint8),) * 2
        w2, mq, vq = O.adamw_q(w, g, mq, vq, s, 1.0, O.sr_step_seed(base, t, 0))
        return w2, (mq, vq)
    return f


def _store_rne(w, g, st, s, t):
    """Negative control: both moments through quantize(bfp_rne)."""
    m, v = st if st is not None else (np.zeros(TOY_N, np.float32),) * 2
    w2, m2, v2 = O.adamw(w, g, m, v, s)
    return w2, (O.quantize(m2, "bfp_rne"), O.quantize(v2, "bfp_rne"))


def _store_no_floor(w, g, st, s, t):
    """Negative control: the chosen form (stochastic rounding, r = sqrt(v)) without the floor: a 0 may be stored."""
    m, r = st if st is not None else (np.zeros(TOY_N, np.float32),) * 2
    with np.errstate(invalid="ignore", over="ignore"):
        w2, m2, v2 = O.adamw(w, g, m, (r * r).astype(np.float32), s)
        r2 = np.sqrt(v2.astype(np.float64)).astype(np.float32)
    seed = O.sr_step_seed(0, t, 0)
    return w2, tuple(O.decode_groups(*O.moment_encode(x, O.sr_key(seed, 16, st_), 0, False), "rne")
                     for x, st_ in ((m2, 0), (r2, 1)))


def test_trajectory_on_the_toy_problem():
    """Loss at T = 400 with the 8-bit state against the f32 state, 8 base seeds: on the shipped oracle f32 reads 23.76
    (largest step 0.011) and the 8 seeds 25.20 / 30.33 / 31.67 / 25.78 / 28.23 / 26.99 / 27.82 / 26.87, ratios 1.060 ..
    R = 1.333 (largest step 0.045). Asserted: loss_q(400) <= loss_f32(400) * (1 + 2 * (R - 1)) for every seed, and both
    negative controls — round to nearest (2.6e8, diverges) and the stochastic sqrt(v) store without the floor (5895) —
    are worse than every seed of the chosen form."""
    ref, big = _toy(_store_f32)
    print(f"f32 state: loss {ref[100]:.4g} / {ref[200]:.4g} / {ref[400]:.4g} at T = 100 / 200 / 400, largest step {big:.3g}")
    assert abs(ref[400] - 23.76) < 0.01
    worst = 0.0
    for base in TOY_SEEDS:
        out, big = _toy(_store_bfp8(base))
        print(f"bfp8 state, base seed {base}: loss {out[100]:.4g} / {out[200]:.4g} / {out[400]:.4g}, largest step "
              f"{big:.3g}, ratio {out[400] / ref[400]:.3f}")
        assert out[400] <= ref[400] * (1 + 2 * (TOY_R - 1))
        assert big <= 0.1
        worst = max(worst, out[400])
    for name, store in (("round to nearest", _store_rne), ("no floor", _store_no_floor)):
        out, big = _toy(store)
        print(f"negative control, {name}: loss {out[100]:.4g} / {out[200]:.4g} / {out[400]:.4g}, largest step {big:.3g}")
        assert not out[400] <= worst, name


# --------------------------------------------------------------------------- Python engine
def _grads(N, n, steps, seed):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32) * (1 + r) for r in range(N)]
            for _ in range(steps)]


def _w0(n_pad, n):
    w = np.zeros(n_pad, np.float32)
    w[:n] = np.random.default_rng(4).standard_normal(n)
    return w


def _rank_run(t, grads, n, codec, base, **kw):
    eng = CompressedAllReduce(t, codec=codec, device="cpu", **kw)
    L = eng.layout(n)
    w = torch.from_numpy(_w0(L.n_pad, n))
    pm, pv = wire.moment_plane(L.n_pad, "cpu"), wire.moment_plane(L.n_pad, "cpu")
    for k, gs in enumerate(grads, 1):
        g = torch.zeros(L.n_pad)
        g[:n] = torch.from_numpy(gs[t.rank])
        eng.allreduce_sgd(g, w, None, pm, n_valid=n, lr=1e-2, weight_decay=0.01, grad_scale=1.0 / t.world, opt="adamw",
                          var=pv, step=k, moment_codec="bfp8", moment_seed=O.sr_step_seed(base, k, 0)).synchronize()
    return w.numpy().copy(), pm.numpy().copy(), pv.numpy().copy(), L.shard, L.n_pad


def _reference(grads, n, N, shard, n_pad, codec, base, scale=None):
    w = _w0(n_pad, n)
    mq, vq = (np.zeros(O.moment_plane_bytes(n_pad), np.uint8) for _ in range(2))
    for k, gs in enumerate(grads, 1):
        total = sim.mesh_allreduce([np.pad(g, (0, n_pad - n)) for g in gs], shard, codec)
        w, mq, vq = O.adamw_q(w, total, mq, vq, _scalars(k), (1.0 / N) if scale is None else scale,
                              O.sr_step_seed(base, k, 0), n_valid=n)
    return w, mq, vq


@pytest.mark.parametrize("codec", ["bfp_rne", "bfp4_rne"])
@pytest.mark.parametrize("N", [2, 3])
def test_python_engine_matches_sim_plus_oracle(N, codec):
    n, steps, base = 1000, 3, 21
    grads = _grads(N, n, steps, 60 + N)
    res = ThreadFabric(N, timeout_s=60).run(lambda t: _rank_run(t, grads, n, codec, base))
    shard, n_pad = res[0][3], res[0][4]
    w, mq, vq = _reference(grads, n, N, shard, n_pad, codec, base)
    for r in range(N):
        assert np.array_equal(res[r][0], w) and np.array_equal(res[r][1], mq) and np.array_equal(res[r][2], vq), r
    assert mq[:n].any() and vq[:n].any()


@pytest.mark.parametrize("kw", [dict(), dict(force_comm=True), dict(algo="ring")], ids=["inline", "forced", "ring"])
def test_python_engine_one_rank_schedules(kw):
    n, base = 1000, 5
    grads = _grads(1, n, 2, 9)
    w, pm, pv, shard, n_pad = _rank_run(ThreadFabric(1).transport(0), grads, n, "bfp_rne", base, **kw)
    ref = _reference(grads, n, 1, n_pad, n_pad, "bfp_rne", base)
    assert np.array_equal(w, ref[0]) and np.array_equal(pm, ref[1]) and np.array_equal(pv, ref[2])


def test_python_engine_clip_group_is_the_premultiplied_update():
    n, N, base = 1000, 2, 3
    grads = _grads(N, n, 1, 31)[0]

    def run(t, clip):
        eng = CompressedAllReduce(t, codec="bfp_rne", device="cpu")
        L = eng.layout(n)
        words = torch.full((4,), math.nan)
        planes, hs = [], []
        for b in range(2):
            w = torch.from_numpy(_w0(L.n_pad, n) * (b + 1))
            pm, pv = wire.moment_plane(L.n_pad, "cpu"), wire.moment_plane(L.n_pad, "cpu")
            g = torch.zeros(L.n_pad)
            g[:n] = torch.from_numpy(grads[t.rank]) * (b + 1)
            kw = dict(clip=words, defer=True) if clip is True else {}
            gs = 0.5 if clip is True else clip
            h = eng.allreduce_sgd(g, w, None, pm, n_valid=n, lr=1e-2, grad_scale=gs, opt="adamw", var=pv, step=1,
                                  moment_codec="bfp8", moment_seed=O.sr_step_seed(base, 1, b), **kw)
            planes.append((w, pm, pv))
            hs.append(h)
        if clip is True:
            eng.commit_group(hs, max_norm=0.5, grad_scale=0.5)
        for h in hs:
            h.synchronize()
        return [tuple(x.numpy().copy() for x in p) for p in planes], words.numpy().copy()

    clipped = ThreadFabric(N, timeout_s=60).run(lambda t: run(t, True))
    words = clipped[0][1]
    assert 0 < words[0] < 1 and all(np.array_equal(c[1], words) for c in clipped)
    plain = ThreadFabric(N, timeout_s=60).run(lambda t: run(t, O.clip_scale(0.5, words)))
    for r in range(N):
        for b in range(2):
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], plain[r][0][b])), (r, b)
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], clipped[0][0][b]))


# --------------------------------------------------------------------------- refusals
def _eng(**kw):
    return CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu", **kw)


def test_refusals():
    eng = _eng(codec="bfp_rne")
    n = 1000
    L = eng.layout(n)
    nb = O.moment_plane_bytes(L.n_pad)
    g, w = torch.zeros(L.n_pad), torch.zeros(L.n_pad)
    pm, pv = wire.moment_plane(L.n_pad, "cpu"), wire.moment_plane(L.n_pad, "cpu")
    ok = dict(n_valid=n, lr=1e-2, opt="adamw", var=pv, step=1, moment_codec="bfp8", moment_seed=0)

    def call(mom=pm, **kw):
        return eng.allreduce_sgd(g, w, None, mom, **{**ok, **kw})

    call().synchronize()
    with pytest.raises(ValueError, match="AdamW only"):
        eng.allreduce_sgd(g, w, None, pm, n_valid=n, lr=1e-2, moment_codec="bfp8", moment_seed=0)
    with pytest.raises(ValueError, match="not with trust_ratio"):
        call(trust_ratio=True)
    with pytest.raises(ValueError, match="one of"):
        call(moment_codec="bfp4")
    with pytest.raises(ValueError, match="needs moment_seed"):
        call(moment_seed=None)
    with pytest.raises(ValueError, match="belongs to moment_codec='bfp8'"):
        eng.allreduce_sgd(g, w, None, torch.zeros(L.n_pad), n_valid=n, lr=1e-2, opt="adamw", var=torch.zeros(L.n_pad),
                          step=1, moment_seed=3)
    for bad in (-1, 1 << 64, 1.5, "3", True):
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            call(moment_seed=bad)
    call(moment_seed=M64).synchronize()
    with pytest.raises(ValueError, match="uint8"):
        call(mom=torch.zeros(L.n_pad))
    with pytest.raises(ValueError, match="uint8"):
        call(var=torch.zeros(nb, dtype=torch.int8))
    with pytest.raises(ValueError, match="contiguous"):
        call(mom=torch.zeros(2 * nb, dtype=torch.uint8)[::2])
    for size in (nb - 17 * 16, nb + 17 * 16, nb + 1, L.n_pad):
        with pytest.raises(ValueError, match="bytes, not exactly"):
            call(var=torch.zeros(size, dtype=torch.uint8))
    if torch.cuda.is_available():  # (another device needs one)
        with pytest.raises(ValueError, match="lives on"):
            call(mom=pm.cuda())
    with pytest.raises(ValueError, match="lives on"):
        wire.moment_check(torch.zeros(nb, dtype=torch.uint8, device="meta"), w, L.n_pad)

    class Big:
        n_pad = 1 << 32

    with pytest.raises(ValueError, match=r"2\^32 or more"):
        moment_request("bfp8", 0, pm, pv, Big(), w, opt="adamw")
    with pytest.raises(ValueError, match="sharded-update"):
        moment_request("bfp8", 0, pm, pv, L, w, opt="adamw", sharded=True)
    assert moment_request("f32", None, None, None, L, w, opt="sgd") is None
    assert moment_request("bfp8", 7, pm, pv, L, w, opt="adamw") == 7
    # the op itself
    buf = torch.zeros(O.shard_bytes("bfp_rne", L.n_pad), dtype=torch.uint8)
    s = _scalars(1)
    with pytest.raises(ValueError, match="elem_base"):
        wire.adamw_q(buf, L.n_pad, 1, w, codec="bfp_rne", mom_q=pm, var_q=pv, scalars=s, seed=0, elem_base=128)
    with pytest.raises(ValueError, match="elem_base"):
        wire.adamw_q(buf, L.n_pad, 1, w, codec="bfp_rne", mom_q=pm, var_q=pv, scalars=s, seed=0, elem_base=256)
    with pytest.raises(TypeError, match="adamw_scalars"):
        wire.adamw_q(buf, L.n_pad, 1, w, codec="bfp_rne", mom_q=pm, var_q=pv, seed=0,
                     scalars=O.lamb_scalars(1e-2, 0, 0.9, 0.999, 1e-8, 1))
    with pytest.raises((ValueError, KeyError)):
        wire.adamw_q(buf, L.n_pad, 1, w, codec="bfp9", mom_q=pm, var_q=pv, scalars=s, seed=0)


def test_trainer_refusals():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, adam=True)
    with pytest.raises(ValueError, match="optimizer='adamw' only"):
        DataParallelTrainer(MLP(sizes, dtype=torch.float32), None, moment_codec="bfp8")
    with pytest.raises(ValueError, match="not with trust_ratio"):
        DataParallelTrainer(model, None, optimizer="adamw", trust_ratio=True, moment_codec="bfp8")
    with pytest.raises(ValueError, match="one of"):
        DataParallelTrainer(model, None, optimizer="adamw", moment_codec="int8")

    class Fake:
        world, shard_update = 2, True

        def layout(self, n):
            return type("L", (), {"n_pad": (n + 255) // 256 * 256, "chunks": 1})()

    with pytest.raises(ValueError, match="sharded-update"):
        DataParallelTrainer(model, Fake(), optimizer="adamw", moment_codec="bfp8")
    with pytest.raises(ValueError, match="adam=True"):
        MLP(sizes, dtype=torch.float32, moment_codec="bfp8")
    q = MLP(sizes, dtype=torch.float32, adam=True, moment_codec="bfp8")
    assert all(l.mom.dtype == torch.uint8 and l.var.numel() == l.n_pad * 17 // 16 for l in q.layers)
    with pytest.raises(ValueError, match="moment_codec='bfp8'"):
        DataParallelTrainer(q, None, optimizer="adamw")


# --------------------------------------------------------------------------- trainer
def _data(sizes, mb=16):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(mb, sizes[0], generator=g) * 2 - 1,
            torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32))


def _train(engine_kind, steps=3, **kw):
    sizes = [32, 64, 32]
    eng = None if engine_kind == "none" else _eng(codec="bfp_rne")
    pad = (lambda n: eng.layout(n).n_pad) if eng is not None else None
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True, adam=True, pad_fn=pad)
    tr = DataParallelTrainer(model, eng, lr=0.01, weight_decay=0.01, optimizer="adamw", **kw)
    x, y = _data(sizes)
    hist = []
    for _ in range(steps):
        tr.step(x, y)
        tr.finish()
        hist.append([l.master.numpy().copy() for l in model.layers])
    return model, tr, hist


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


def test_trainer_local_step_matches_oracle_and_allocates_planes():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True, adam=True)
    tr = DataParallelTrainer(model, None, lr=0.01, optimizer="adamw", moment_codec="bfp8", sr_seed=1 << 40)
    assert all(l.mom.dtype == l.var.dtype == torch.uint8 and l.mom.numel() == O.moment_plane_bytes(l.n_pad)
               for l in model.layers)
    x, y = _data(sizes)
    for step in (1, 2):
        prev = [(l.master.numpy().copy(), l.mom.numpy().copy(), l.var.numpy().copy()) for l in model.layers]
        tr.step(x, y)
        tr.finish()
        for i, l in enumerate(model.layers):
            s = O.adamw_scalars(0.01, 0.0, 0.9, 0.999, 1e-8, step)
            w, mq, vq = O.adamw_q(prev[i][0], l.grad.numpy(), prev[i][1], prev[i][2], s, 1.0,
                                  O.sr_step_seed(1 << 40, step, i), n_valid=l.n)
            assert np.array_equal(l.master.numpy(), w) and np.array_equal(l.mom.numpy(), mq)
            assert np.array_equal(l.var.numpy(), vq)


@pytest.mark.parametrize("kw", [dict(), dict(max_grad_norm=0.05), dict(stochastic_rounding=True),
                                dict(error_feedback=True)], ids=["plain", "clip", "sr", "ef"])
def test_trainer_local_and_python_engine_agree(kw):
    """One rank. With wire-side stochastic rounding or error feedback the engine-less trainer takes the gradient through
    the inline engine's one-slot round trip, so the two agree bit for bit, planes included (without them the
    engine-less update reads the f32 gradient itself, another input)."""
    q = dict(moment_codec="bfp8", sr_seed=77, **kw)
    me, _, he = _train("python", **q)
    if "stochastic_rounding" in kw or "error_feedback" in kw:
        ml, _, hl = _train("none", **q)
        assert _same(hl, he)
        assert all(np.array_equal(a.mom.numpy(), b.mom.numpy()) and np.array_equal(a.var.numpy(), b.var.numpy())
                   for a, b in zip(ml.layers, me.layers))
    assert _same(he, _train("python", **q)[2]), "deterministic under a repeat"
    assert not _same(he[1:2], _train("python", **{**q, "sr_seed": 78})[2][1:2]), "the seed matters"
    assert not _same(he[1:2], _train("python", **kw)[2][1:2]), "differs from the f32 state"


def test_f32_codec_is_the_run_without_the_keyword():
    assert _same(_train("python", moment_codec="f32")[2], _train("python")[2])
    assert _same(_train("none", moment_codec="f32")[2], _train("none")[2])
    # the engine's keyword too
    eng = _eng(codec="bfp_rne")
    n = 1000
    L = eng.layout(n)
    g = torch.from_numpy(np.pad(_grads(1, n, 1, 2)[0][0], (0, L.n_pad - n)))
    outs = []
    for kw in (dict(), dict(moment_codec="f32")):
        w, m, v = torch.from_numpy(_w0(L.n_pad, n)), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=1e-2, opt="adamw", var=v, step=1, **kw).synchronize()
        outs.append((w.numpy().copy(), m.numpy().copy(), v.numpy().copy()))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


# --------------------------------------------------------------------------- CLI and checkpoint
ARGS = ["32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0"]
Q = ["--optimizer", "adamw", "--lr", "0.01", "--moment-codec", "bfp8", "--sr-seed", "21"]


def _cli(iters, *flags):
    out = io.StringIO()
    r = mlp_mpi.run([str(iters)] + ARGS + list(flags), out=out)
    assert out.getvalue()
    m = r["model"]
    return r["trainer"], [l.master.numpy().copy() for l in m.layers], [(l.mom, l.var) for l in m.layers]


def test_cli_flag_and_refusals():
    parse = lambda *f: mlp_mpi.config_from_args(mlp_mpi.build_parser().parse_args(["1"] + ARGS + list(f)))  # noqa: E731
    assert parse(*Q).moment_codec == "bfp8" and parse().moment_codec == "f32"
    t, w, planes = _cli(2, *Q)
    assert t.moment_codec == "bfp8" and t.opt_step == 2
    assert all(p.dtype == torch.uint8 and p.any() for pair in planes for p in pair)
    assert all(np.array_equal(a, b) for a, b in zip(w, _cli(2, *Q)[1]))
    assert not all(np.array_equal(a, b) for a, b in zip(w, _cli(2, *Q[:-1], "22")[1]))
    assert not all(np.array_equal(a, b) for a, b in zip(w, _cli(2, *Q[:4])[1]))
    t_loc, _, _ = _cli(1, *Q, "--compress", "local")
    assert t_loc.engine is None and t_loc.moment_codec == "bfp8"
    _cli(1, *Q, "--stochastic-rounding")
    _cli(1, *Q, "--error-feedback")
    _cli(1, *Q, "--algo", "ring")
    with pytest.raises(ValueError, match="optimizer='adamw' only"):
        _cli(1, "--moment-codec", "bfp8")
    with pytest.raises(ValueError, match="not with trust_ratio"):
        _cli(1, *Q, "--trust-ratio")
    with pytest.raises(SystemExit):
        _cli(1, *Q[:4], "--moment-codec", "bfp4")
    assert "--moment-codec" in mlp_mpi.build_parser().format_help()


def test_checkpoint_round_trip(tmp_path):
    """The planes' bytes go into the checkpoint under the AdamW names with the codec's name in the index; a resumed run's
    next step is bit-identical to the uninterrupted run's; another codec or another n_pad is a clear error."""
    ck = str(tmp_path / "ck")
    t2, _, planes2 = _cli(2, *Q, "--checkpoint", ck)
    with open(ck + ".json") as f:
        info = json.load(f)
    assert info["moment_codec"] == "bfp8" and info["opt_step"] == 2 and info["optimizer"] == "adamw"
    assert info["moment_n_pad"] == [p[0].numel() // 17 * 16 for p in planes2]
    from safetensors.torch import load_file
    sd = load_file(ck + ".safetensors")
    for i, (pm, pv) in enumerate(planes2):
        assert sd[f"fc{i}.exp_avg"].dtype == torch.uint8 and torch.equal(sd[f"fc{i}.exp_avg"], pm)
        assert torch.equal(sd[f"fc{i}.exp_avg_sq"], pv)
    t_res, w_res, p_res = _cli(1, *Q, "--resume", ck)
    t3, w3, p3 = _cli(3, *Q)
    assert t_res.opt_step == t3.opt_step == 3
    assert all(np.array_equal(a, b) for a, b in zip(w_res, w3))
    assert all(torch.equal(a, b) for x, y in zip(p_res, p3) for a, b in zip(x, y))
    with pytest.raises(ValueError, match="saved under moment_codec='bfp8'"):
        _cli(1, *Q[:4], "--resume", ck)
    f32 = str(tmp_path / "f32")
    _cli(1, *Q[:4], "--checkpoint", f32)
    with open(f32 + ".json") as f:
        assert "moment_codec" not in json.load(f)
    with pytest.raises(ValueError, match="saved under moment_codec='f32'"):
        _cli(1, *Q, "--resume", f32)
    # another padding of the same model (an engine layout that pads the buckets further): the plane layout differs
    from fpga_ai_nic_amd.utils import checkpoint
    wide = MLP([64, 64, 32], dtype=torch.float32, adam=True, moment_codec="bfp8", bias=False, relu="none",
               pad_fn=lambda n: (n + 1023) // 1024 * 1024 + 1024)
    with pytest.raises(ValueError, match="n_pad"):
        checkpoint.load(ck, wide)
