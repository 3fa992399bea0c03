"""Error feedback for the compressed mesh all-reduce, CPU side: the NumPy oracle (``bfp_oracle.ef_pack`` /
``ef_reduce``), the simulator (``sim.mesh_allreduce_ef``), the Python engine over ThreadFabric and gloo, the trainer
and the refusals."""
import io
import math
import os
import socket

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.cli import mlp_mpi
from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import sim
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, RcclAllReduce
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

BFP = ["bfp_rne", "bfp_trunc"]
T = 64


def _issue_input():
    """The input the feature was specified on: normal values under a log-normal scale, constant over the steps."""
    rng = np.random.default_rng(0)
    n = 4096
    return (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 2)).astype(np.float32)


def _group_max(g):
    return np.repeat(np.abs(g).reshape(-1, 16).max(axis=1), 16).astype(np.float64)


# --------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("codec", BFP)
def test_oracle_zero_residual_is_todays_wire(codec):
    rng = np.random.default_rng(1)
    s, N = 512, 3
    g = rng.standard_normal(s * N).astype(np.float32)
    zero = np.zeros(s * N, np.float32)
    for self_shard in (-1, 0, 1, 2):
        w, e = O.ef_pack(g, zero, s, codec, self_shard)
        assert np.array_equal(w, O.pack(g, s, codec))
        assert not zero.any(), "the incoming plane is not modified"
        q = O.quantize(g, codec)
        exp = (g - q).astype(np.float32)
        if self_shard >= 0:
            exp[self_shard * s:(self_shard + 1) * s] = 0
        assert np.array_equal(e, exp)
    sb = O.shard_bytes(codec, s)
    packed = O.pack(g, s, codec)
    slots = [packed[r * sb:(r + 1) * sb] for r in range(N)]
    local = rng.standard_normal(s).astype(np.float32)
    for self_pos in range(N):
        w, e = O.ef_reduce(slots, local, self_pos, zero[:s], codec, s)
        acc = O.reduce_slots(slots, local, self_pos, codec, s)
        assert np.array_equal(w, O.pack(acc, s, codec))
        assert np.array_equal(e, (acc - O.quantize(acc, codec)).astype(np.float32))


@pytest.mark.parametrize("codec", BFP)
def test_oracle_own_shard_untouched_and_stages_disjoint(codec):
    rng = np.random.default_rng(2)
    s, N = 256, 4
    g = rng.standard_normal(s * N).astype(np.float32)
    e0 = (rng.standard_normal(s * N) * 1e-2).astype(np.float32)
    sb = O.shard_bytes(codec, s)
    for r in range(N):
        own = slice(r * s, (r + 1) * s)
        w, e1 = O.ef_pack(g, e0, s, codec, self_shard=r)
        assert np.array_equal(e1[own].view(np.uint32), e0[own].view(np.uint32)), "own slice: the incoming bits"
        assert np.array_equal(w[r * sb:(r + 1) * sb], O.pack(g[own], s, codec)), "own shard: enc(g), no residual"
        changed = e1.view(np.uint32) != e0.view(np.uint32)
        assert not changed[own].any() and changed.reshape(N, s).any(axis=1).sum() == N - 1
        # the composed plane of one step: the sender stage wrote every shard but r, the owner stage writes r alone
        # (ef_reduce takes and returns that slice only), so no element is written twice and none is left out
        slots = [w[q * sb:(q + 1) * sb] for q in range(N)]
        _, e_own = O.ef_reduce(slots, g[own], r, e1[own], codec, s)
        assert e_own.shape == (s,) and e_own.dtype == np.float32
        e2 = e1.copy()
        e2[own] = e_own
        by_pack, by_owner = changed, e2.view(np.uint32) != e1.view(np.uint32)
        assert not (by_pack & by_owner).any() and not by_owner.reshape(N, s)[np.arange(N) != r].any()
        assert by_owner[own].any() and (by_pack | by_owner).reshape(N, s).any(axis=1).all()
        # x = g + e on the others, e' = x - dec(enc(x))
        for q in range(N):
            if q == r:
                continue
            sl = slice(q * s, (q + 1) * s)
            x = (g[sl] + e0[sl]).astype(np.float32)
            assert np.array_equal(w[q * sb:(q + 1) * sb], O.pack(x, s, codec))
            assert np.array_equal(e1[sl], (x - O.quantize(x, codec)).astype(np.float32))


def test_oracle_refuses_raw_codecs():
    g = np.zeros(256, np.float32)
    for codec in ("raw_f32", "raw_bf16"):
        with pytest.raises(ValueError, match="BFP codecs only"):
            O.ef_pack(g, g, 256, codec)
        with pytest.raises(ValueError, match="BFP codecs only"):
            O.ef_reduce([g.view(np.uint8)], g, 0, g, codec, 256)


VIAS = ["pack", "reduce", "sim"]


def _iterate(g, codec, steps, via):
    """`steps` steps of the shipped error-feedback code on the constant input g (one shard of g.size elements), from
    a zero plane. via "pack": the sender stage, ``O.ef_pack`` (no own shard) decoded with ``O.unpack``; "reduce": the
    owner stage at one slot, ``O.ef_reduce``; "sim": ``sim.mesh_allreduce_ef`` with one rank. Every decoded value q_t
    and every residual comes from that code; the test itself only forms x_t = fl(g + e_t), the definition's one f32
    add, from the plane the code returned. Returns the per-step (x, q, e_before) and the final residual."""
    n = g.size
    e = np.zeros(n, np.float32)
    hist = []
    for _ in range(steps):
        x = (g + e).astype(np.float32)
        if via == "pack":
            w, e2 = O.ef_pack(g, e, n, codec, -1)
            q = O.unpack(w, n, n, codec)
        elif via == "reduce":
            w, e2 = O.ef_reduce([np.zeros(0, np.uint8)], g, 0, e, codec, n)
            q = O.unpack(w, n, n, codec)
        else:
            q, planes = sim.mesh_allreduce_ef([g], [e], n, codec)
            e2 = planes[0]
        assert e2.dtype == np.float32 and e2.shape == (n,) and q.shape == (n,)
        hist.append((x, q, e))
        e = e2
    return hist, e


@pytest.mark.parametrize("via", VIAS)
def test_telescoping_rne(via):
    """Sum_t q_t = T g - e_T + Sum_t (fl(g + e_t) - (g + e_t)) when every x - q is exact, so elementwise
    |Sum_t q_t - (T g - e_T)| <= Sum_t |fl(g + e_t) - (g + e_t)|. Both sides are exactly rounded float64 sums
    (math.fsum) of the f32 terms; the 1e-12 relative slack covers that one rounding per side."""
    g = _issue_input()
    hist, e_T = _iterate(g, "bfp_rne", T, via)
    g64 = g.astype(np.float64)
    nxt = [h[2] for h in hist[1:]] + [e_T]
    for (x, q, _), e2 in zip(hist, nxt):
        # every x - q is exact: the residual the code stored equals the float64 difference (itself exact: the two
        # operands share a group, so their bits span far fewer than 53 positions)
        assert np.array_equal(e2.astype(np.float64), x.astype(np.float64) - q.astype(np.float64))
    assert e_T.any()
    qs = np.stack([q.astype(np.float64) for _, q, _ in hist])
    xs = np.stack([x.astype(np.float64) for x, _, _ in hist])
    es = np.stack([e.astype(np.float64) for _, _, e in hist])
    e64 = e_T.astype(np.float64)
    for i in range(g.size):
        lhs = abs(math.fsum(list(qs[:, i]) + [-T * g64[i], e64[i]]))  # (T * g: exact, T is a power of two)
        rhs = math.fsum(abs(math.fsum((xs[t, i], -g64[i], -es[t, i]))) for t in range(T))
        assert lhs <= rhs * (1 + 1e-12), (i, lhs, rhs)


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("codec", BFP)
def test_convergence(codec, via):
    """max over ALL elements of |mean_t q_t - g| / group max |g| at T = 64 is at most 1/16 of the same quantity
    without feedback (the oracle gives about 1/64 for both codecs)."""
    g = _issue_input()
    gm = _group_max(g)
    assert (gm > 0).all()
    base = (np.abs(O.quantize(g, codec).astype(np.float64) - g) / gm).max()
    hist, _ = _iterate(g, codec, T, via)
    assert np.array_equal(hist[0][1], O.quantize(g, codec)), "step 1 (zero plane) is the codec without feedback"
    mean = np.mean(np.stack([q.astype(np.float64) for _, q, _ in hist]), axis=0)
    fed = (np.abs(mean - g) / gm).max()
    print(f"{codec} via {via}: no feedback {base:.3e}, T={T} {fed:.3e}, ratio {fed / base:.4f}")
    assert fed <= base / 16, (fed, base)


def test_simulator_zero_planes_is_plain_mesh():
    rng = np.random.default_rng(3)
    for codec in BFP:
        for N in (1, 2, 3):
            s = 256
            grads = [rng.standard_normal(s * N).astype(np.float32) for _ in range(N)]
            zero = [np.zeros(s * N, np.float32) for _ in range(N)]
            out, new = sim.mesh_allreduce_ef(grads, zero, s, codec)
            assert np.array_equal(out, sim.mesh_allreduce(grads, s, codec))
            assert all(not z.any() for z in zero) and any(e.any() for e in new)


def test_simulator_matches_the_oracle_stages():
    """The spec-level simulator against the two oracle stages chained the way the engines chain them."""
    rng = np.random.default_rng(4)
    codec, N, s = "bfp_trunc", 3, 256
    sb = O.shard_bytes(codec, s)
    grads = [rng.standard_normal(s * N).astype(np.float32) for _ in range(N)]
    planes = [(rng.standard_normal(s * N) * 1e-2).astype(np.float32) for _ in range(N)]
    out, new = sim.mesh_allreduce_ef(grads, planes, s, codec)
    packed = [O.ef_pack(grads[r], planes[r], s, codec, self_shard=r) for r in range(N)]
    for r in range(N):
        own = slice(r * s, (r + 1) * s)
        slots = [packed[q][0][r * sb:(r + 1) * sb] for q in range(N)]
        w, e_own = O.ef_reduce(slots, grads[r][own], r, packed[r][1][own], codec, s)
        exp = packed[r][1].copy()
        exp[own] = e_own
        assert np.array_equal(new[r], exp)
        assert np.array_equal(out[own], O.unpack(w, s, s, codec))


# --------------------------------------------------------------------------- wire ops on CPU tensors
@pytest.mark.parametrize("codec", BFP)
def test_wire_ops_cpu_follow_the_oracle(codec):
    rng = np.random.default_rng(5)
    s, N = 256, 3
    sb = wire.shard_bytes(codec, s)
    g = rng.standard_normal(s * N).astype(np.float32)
    e0 = (rng.standard_normal(s * N) * 1e-2).astype(np.float32)
    w_ref, e_ref = O.ef_pack(g, e0, s, codec, self_shard=1)
    e = torch.from_numpy(e0.copy())
    out = torch.zeros(sb * N, dtype=torch.uint8)
    wire.pack_ef(torch.from_numpy(g), e, out, s, codec, self_shard=1)
    assert np.array_equal(out.numpy(), w_ref) and np.array_equal(e.numpy(), e_ref)
    # a null destination skips its shard: neither encoded nor fed back
    e = torch.from_numpy(e0.copy())
    dsts = [torch.full((sb,), 0xA5, dtype=torch.uint8) for _ in range(N)]
    wire.pack_ef(torch.from_numpy(g), e, [dsts[0], None, dsts[2]], s, codec, self_shard=-1)
    w_all, e_all = O.ef_pack(g, e0, s, codec, -1)
    assert np.array_equal(dsts[0].numpy(), w_all[:sb]) and np.array_equal(dsts[2].numpy(), w_all[2 * sb:])
    assert (dsts[1] == 0xA5).all() and np.array_equal(e.numpy()[s:2 * s], e0[s:2 * s])
    assert np.array_equal(e.numpy()[:s], e_all[:s]) and np.array_equal(e.numpy()[2 * s:], e_all[2 * s:])
    # reduce_ef
    slots = torch.from_numpy(w_all.copy())
    local = torch.from_numpy(g[:s].copy())
    er = torch.from_numpy(e0[:s].copy())
    o1, o2 = torch.zeros(sb, dtype=torch.uint8), torch.zeros(sb, dtype=torch.uint8)
    wire.reduce_ef(slots, N, 2, local, er, [o1, None, o2], s, codec)
    w_ref, e_ref = O.ef_reduce([w_all[r * sb:(r + 1) * sb] for r in range(N)], g[:s], 2, e0[:s], codec, s)
    assert np.array_equal(o1.numpy(), w_ref) and np.array_equal(o2.numpy(), w_ref) and np.array_equal(er.numpy(), e_ref)
    with pytest.raises(ValueError, match="BFP codecs only"):
        wire.pack_ef(torch.from_numpy(g), e, out, s, "raw_f32")
    with pytest.raises(ValueError, match="float32"):
        wire.pack_ef(torch.from_numpy(g), e.double(), out, s, codec)
    with pytest.raises(ValueError, match="needs"):
        wire.reduce_ef(slots, N, 2, local, er[: s - 1].clone(), o1, s, codec)


# --------------------------------------------------------------------------- the Python engine
STEPS = 4


def _step_grads(N, n, seed):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(n) * (1 + r)).astype(np.float32) for r in range(N)] for _ in range(STEPS)]


def _sim_steps(grads, n, shard, codec):
    """[(decoded result, planes after the step)] of STEPS simulated steps from zero planes."""
    N = len(grads[0])
    planes = [np.zeros(shard * N, np.float32) for _ in range(N)]
    res = []
    for t in range(STEPS):
        gin = [np.pad(g, (0, shard * N - n)) for g in grads[t]]
        out, planes = sim.mesh_allreduce_ef(gin, planes, shard, codec)
        res.append((out, [p.copy() for p in planes]))
    return res


def _engine_steps(t, grads, n, codec, **kw):
    eng = CompressedAllReduce(t, codec=codec, device="cpu", **kw)
    L = eng.layout(n)
    e = torch.zeros(L.n_pad)
    res = []
    for step in range(STEPS):
        g, out = torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        g[:n] = torch.from_numpy(grads[step][t.rank])
        eng.allreduce(g, out, n_valid=n, residual=e).synchronize()
        res.append((out.numpy().copy(), e.numpy().copy()))
    return res, L.shard


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("codec", BFP)
def test_python_engine_threadfabric(N, codec):
    n = 1000
    grads = _step_grads(N, n, 10 + N)
    res = ThreadFabric(N, timeout_s=60).run(lambda t: _engine_steps(t, grads, n, codec))
    ref = _sim_steps(grads, n, res[0][1], codec)
    for r in range(N):
        for step in range(STEPS):
            out, plane = res[r][0][step]
            assert np.array_equal(out, ref[step][0]), (r, step)
            assert np.array_equal(plane, ref[step][1][r]), (r, step)
    assert any(np.any(ref[-1][1][r]) for r in range(N))
    plain = sim.mesh_allreduce([np.pad(g, (0, res[0][1] * N - n)) for g in grads[1]], res[0][1], codec)
    assert not np.array_equal(ref[1][0], plain), "the second step already differs from the engine without feedback"


@pytest.mark.parametrize("force", [False, True])
def test_python_engine_one_rank(force):
    """One rank, inline or through the forced multi-rank path: the owner stage alone, y = g + e."""
    n, codec = 700, "bfp_rne"
    grads = _step_grads(1, n, 21)
    res, shard = _engine_steps(ThreadFabric(1).transport(0), grads, n, codec, force_comm=force)
    ref = _sim_steps(grads, n, shard, codec)
    e = np.zeros(shard, np.float32)
    for step in range(STEPS):
        y = (np.pad(grads[step][0], (0, shard - n)) + e).astype(np.float32)
        q = O.quantize(y, codec)
        e = (y - q).astype(np.float32)
        assert np.array_equal(res[step][0], q) and np.array_equal(res[step][1], e)
        assert np.array_equal(ref[step][0], q) and np.array_equal(ref[step][1][0], e)


def test_python_engine_update_request_and_zero_plane_first_step():
    """allreduce_sgd takes the plane too; with a zero plane the first step's update is the engine's without one."""
    N, n, codec = 2, 600, "bfp_rne"
    grads = _step_grads(N, n, 31)

    def fn(t):
        eng = CompressedAllReduce(t, codec=codec, device="cpu")
        L = eng.layout(n)
        e = torch.zeros(L.n_pad)
        w_ef, w_plain = torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        hist = []
        for step in range(2):
            g = torch.zeros(L.n_pad)
            g[:n] = torch.from_numpy(grads[step][t.rank])
            eng.allreduce_sgd(g, w_ef, n_valid=n, lr=1.0, residual=e).synchronize()
            eng.allreduce_sgd(g, w_plain, n_valid=n, lr=1.0).synchronize()
            hist.append((w_ef.numpy().copy(), w_plain.numpy().copy()))
        return hist, L.shard

    res = ThreadFabric(N, timeout_s=60).run(fn)
    ref = _sim_steps(grads, n, res[0][1], codec)
    for r in range(N):
        (a1, p1), (a2, p2) = res[r][0]
        assert np.array_equal(a1, p1), "zero plane: today's bytes, today's update"
        assert np.array_equal(a1[:n], -ref[0][0][:n])
        assert np.array_equal(a2[:n], (a1[:n] - ref[1][0][:n]).astype(np.float32))
        assert not np.array_equal(a2, p2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, grads, n, codec, q):
    import torch.distributed as dist

    from fpga_ai_nic_amd.parallel.transport import TorchDistTransport

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    try:
        res, shard = _engine_steps(TorchDistTransport(), grads, n, codec)
        q.put((rank, res, shard))
    except Exception as e:  # noqa: BLE001 (reported to the parent, which never waits for a worker that failed)
        q.put((rank, repr(e), -1))
    finally:
        dist.destroy_process_group()


@pytest.mark.slow
def test_python_engine_gloo_world2():
    import queue as _queue

    import torch.multiprocessing as mp

    world, n, codec = 2, 1000, "bfp_rne"
    grads = _step_grads(world, n, 41)
    q = mp.get_context("spawn").Queue()
    pc = mp.start_processes(_gloo_worker, args=(world, _free_port(), grads, n, codec, q), nprocs=world, join=False,
                            start_method="spawn")
    got = {}
    try:
        for _ in range(world):
            r, res, shard = q.get(timeout=120)
            got[r] = (res, shard)
    except _queue.Empty:
        for p in pc.processes:
            p.kill()
        pytest.fail("gloo workers did not report within 120 s")
    while not pc.join(60):
        pass
    for r in range(world):
        assert got[r][1] != -1, f"rank {r}: {got[r][0]}"
    ref = _sim_steps(grads, n, got[0][1], codec)
    for r in range(world):
        for step in range(STEPS):
            assert np.array_equal(got[r][0][step][0], ref[step][0])
            assert np.array_equal(got[r][0][step][1], ref[step][1][r])


# --------------------------------------------------------------------------- refusals
def _eng(**kw):
    return CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu", **kw)


def test_engine_refusals():
    n = 100
    eng = _eng()
    L = eng.layout(n)
    g, w, out = torch.ones(L.n_pad), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
    good = torch.zeros(L.n_pad)
    cases = [
        (torch.zeros(L.n_pad, dtype=torch.float64), "float32"),
        (torch.zeros(L.n_pad, dtype=torch.bfloat16), "float32"),
        (torch.zeros(2 * L.n_pad)[::2], "contiguous"),
        (torch.zeros(L.n_pad - 1), "layout needs"),
        (torch.zeros(L.n_pad, device="meta"), "lives on"),
    ]
    for bad, match in cases:
        with pytest.raises(ValueError, match=match):
            eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, residual=bad)
        with pytest.raises(ValueError, match=match):
            eng.allreduce(g, out, n_valid=n, residual=bad)
    with pytest.raises(ValueError, match="nothing to feed back"):
        _eng(codec="raw_f32").allreduce_sgd(g, w, n_valid=n, lr=1.0, residual=good)
    with pytest.raises(ValueError, match="raw_bf16 is not supported yet"):
        _eng(codec="raw_bf16").allreduce_sgd(g, w, n_valid=n, lr=1.0, residual=good)
    ring = _eng(algo="ring")
    with pytest.raises(ValueError, match="ring schedule"):
        ring.allreduce_sgd(torch.ones(ring.layout(n).n_pad), w, n_valid=n, lr=1.0,
                           residual=torch.zeros(ring.layout(n).n_pad))
    assert not good.any() and not w.any(), "refused: nothing ran"
    # the shared check's other arms (the native engine's configurations)
    from fpga_ai_nic_amd.parallel.allreduce import BucketLayout, residual_request

    kw = dict(codec_id=1, algo="mesh", world=2, device="cpu")
    with pytest.raises(ValueError, match="prepacked"):
        residual_request(good, L, **kw, prepacked=True)
    with pytest.raises(ValueError, match="sharded"):
        residual_request(good, L, **kw, sharded=True)
    with pytest.raises(ValueError, match="chunked"):
        residual_request(good, BucketLayout(n=n, n_pad=L.n_pad, algo="mesh", world=1, shard=128, chunks=2), **kw)
    with pytest.raises(ValueError, match="at most 16 ranks"):
        residual_request(good, L, **{**kw, "world": 17})
    assert residual_request(None, L, **kw) is None
    # an ordinary request still completes
    eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, residual=good).synchronize()
    assert torch.all(w[:n] == -1.0)


def test_trainer_refusals():
    model = MLP([32, 32], dtype=torch.float32)

    class Fake:  # what the trainer reads of an engine
        world, codec, algo, shard_update = 2, "bfp_rne", "mesh", False

        def layout(self, n):
            return type("L", (), {"chunks": 1, "n_pad": (n + 511) // 512 * 512})()

    with pytest.raises(ValueError, match="ring"):
        DataParallelTrainer(model, type("Ring", (Fake,), {"algo": "ring"})(), error_feedback=True)
    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, type("Sh", (Fake,), {"shard_update": True})(), error_feedback=True)
    with pytest.raises(ValueError, match="raw codec"):
        DataParallelTrainer(model, type("Raw", (Fake,), {"codec": "raw_f32"})(), error_feedback=True)
    with pytest.raises(ValueError, match="raw codec"):
        DataParallelTrainer(model, RcclAllReduce(ThreadFabric(1).transport(0), device="cpu"), error_feedback=True)

    class Chunked(Fake):
        def layout(self, n):
            return type("L", (), {"chunks": 2, "n_pad": n})()

    with pytest.raises(ValueError, match="chunked"):
        DataParallelTrainer(model, Chunked(), error_feedback=True)
    tr = DataParallelTrainer(model, None)
    assert tr.residuals is None and not tr.error_feedback


# --------------------------------------------------------------------------- trainer
def _data(sizes, mb=16):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(mb, sizes[0], generator=g) * 2 - 1,
            torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32))


def _train(engine_kind, steps=3, **kw):
    sizes = [32, 64, 32]
    eng = None if engine_kind == "none" else _eng()
    pad = (lambda n: eng.layout(n).n_pad) if eng is not None else None
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True, momentum=True, adam=kw.get("optimizer") == "adamw",
                pad_fn=pad)
    tr = DataParallelTrainer(model, eng, lr=0.05, **kw)
    x, y = _data(sizes)
    hist = []
    for _ in range(steps):
        tr.step(x, y)
        tr.finish()
        hist.append([l.master.numpy().copy() for l in model.layers])
    return model, tr, hist


@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw", trust_ratio=True, max_grad_norm=0.05)],
                         ids=["sgd", "lamb_clip"])
def test_trainer_local_and_python_engine_agree(kw):
    """One rank: the engine-less trainer's one-slot round trip is the inline engine's owner stage."""
    _, tl, hl = _train("none", error_feedback=True, **kw)
    _, te, he = _train("python", error_feedback=True, **kw)
    assert tl.residuals is not None and len(tl.residuals) == 2
    for a, b in zip(hl, he):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for a, b in zip(tl.residuals, te.residuals):
        assert torch.equal(a, b) and a.any() and a.dtype == torch.float32
    # live: differs from the trainer without feedback after step 2 (step 1 starts from zero planes)
    _, _, hp = _train("python", **kw)
    assert all(np.array_equal(x, y) for x, y in zip(he[0], hp[0]))
    assert not all(np.array_equal(x, y) for x, y in zip(he[1], hp[1]))


def test_trainer_flag_off_is_the_trainer_without_it():
    _, _, a = _train("python", error_feedback=False)
    _, _, b = _train("python")
    assert all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


def test_trainer_local_step_matches_oracle():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True)
    tr = DataParallelTrainer(model, None, lr=0.05, error_feedback=True)
    x, y = _data(sizes)
    planes = [np.zeros(l.n_pad, np.float32) for l in model.layers]
    for _ in range(2):
        prev = [l.master.numpy().copy() for l in model.layers]
        tr.step(x, y)
        tr.finish()
        for i, l in enumerate(model.layers):
            yv = (l.grad.numpy() + planes[i]).astype(np.float32)
            q = O.quantize(yv, "bfp_rne")
            planes[i] = (yv - q).astype(np.float32)
            w, _ = O.sgd(prev[i][: l.n], q[: l.n], 0.05)
            assert np.array_equal(l.master.numpy()[: l.n], w)
            assert np.array_equal(tr.residuals[i].numpy(), planes[i])


def test_cli_flag():
    """--error-feedback reaches the trainer: its planes exist and are live, the run differs from the run without the
    flag after step 2 (and not after step 1, whose planes are still zero), and the engine-less run takes --rounding."""
    args = ["32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0"]

    def run(iters, *flags):
        out = io.StringIO()
        r = mlp_mpi.run([str(iters)] + args + list(flags), out=out)
        assert out.getvalue()
        return r["trainer"], [l.master.numpy().copy() for l in r["model"].layers]

    parse = lambda *f: mlp_mpi.config_from_args(mlp_mpi.build_parser().parse_args(["1"] + args + list(f)))  # noqa: E731
    assert parse("--error-feedback").error_feedback and not parse().error_feedback
    for iters, same in ((1, True), (2, False)):
        t_ef, w_ef = run(iters, "--error-feedback")
        t_no, w_no = run(iters)
        assert t_ef.error_feedback and len(t_ef.residuals) == 2 and all(bool(e.any()) for e in t_ef.residuals)
        assert not t_no.error_feedback and t_no.residuals is None
        assert all(np.array_equal(a, b) for a, b in zip(w_ef, w_no)) == same
    t_tr, w_tr = run(2, "--error-feedback", "--compress", "local", "--rounding", "trunc")
    t_rn, w_rn = run(2, "--error-feedback", "--compress", "local")
    assert t_tr.engine is None and (t_tr.ef_codec, t_rn.ef_codec) == ("bfp_trunc", "bfp_rne")
    assert not all(np.array_equal(a, b) for a, b in zip(w_tr, w_rn))
    assert "restarts" in mlp_mpi.build_parser().format_help().replace("\n", " ")
