"""Error feedback on the GPU: wire_pack_ef / wire_reduce_ef against the NumPy oracle bit for bit (wire bytes and
residual plane), the native engine over virtual ranks (LoopbackFabric) and over the direct P2P transport (two processes
on one GPU) against the simulator and the Python engine, the trainer at world 1 inline and through the forced
multi-rank path, and the refusals. Every comparison is exact: the kernels perform the oracle's operations (one f32 add,
the codec, one f32 subtract) per value."""
import math
import os
import queue as _queue
import socket
import threading

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd import _ext
from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import sim
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
from fpga_ai_nic_amd.parallel.transport import NativeTransport, ThreadFabric

pytestmark = pytest.mark.gpu

DEV = "cuda"
BFP = ["bfp_rne", "bfp_trunc"]
SENTINEL = 0x4ABCD123  # a finite f32 pattern no arithmetic here produces
# (shard elements, shards): 16 active lanes; a second block that is almost empty; 40 blocks' worth over 3 shards
SHAPES = [(256, 2), (4096 + 256, 2), (256 * 40, 3)]


def _inputs(n, dtype, seed):
    """A gradient (as the GPU tensor and as the f32 values the kernels read) and a non-zero incoming residual."""
    rng = np.random.default_rng(seed)
    g = torch.from_numpy((rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32)).to(dtype)
    e = (rng.standard_normal(n) * 2e-2).astype(np.float32)
    return g.to(DEV), g.to(torch.float32).numpy(), e


# --------------------------------------------------------------------------- wire_pack_ef
@pytest.mark.parametrize("codec", BFP)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_pack_ef_matches_oracle(n_s, n_sh, dtype, codec):
    n = n_s * n_sh
    sb = wire.shard_bytes(codec, n_s)
    g_dev, g, e0 = _inputs(n, dtype, n_s + n_sh)
    for self_shard in sorted({-1, 0, n_sh // 2, n_sh - 1}):
        e_in = e0.copy()
        if self_shard >= 0:
            e_in.view(np.uint32)[self_shard * n_s:(self_shard + 1) * n_s] = SENTINEL
        e = torch.from_numpy(e_in.copy()).to(DEV)
        out = torch.full((sb * n_sh + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        wire.pack_ef(g_dev, e, out, n_s, codec, self_shard=self_shard)
        torch.cuda.synchronize()
        w_ref, e_ref = O.ef_pack(g, e_in, n_s, codec, self_shard)
        assert np.array_equal(out.cpu().numpy()[: sb * n_sh], w_ref), (self_shard, "wire")
        assert (out[sb * n_sh:] == 0xA5).all(), "bytes past the last shard untouched"
        got = e.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), e_ref.view(np.uint32)), (self_shard, "residual")
        if self_shard >= 0:
            assert (got.view(np.uint32)[self_shard * n_s:(self_shard + 1) * n_s] == SENTINEL).all()
            assert np.array_equal(w_ref[self_shard * sb:(self_shard + 1) * sb],
                                  O.pack(g[self_shard * n_s:(self_shard + 1) * n_s], n_s, codec))


@pytest.mark.parametrize("codec", BFP)
def test_pack_ef_null_destination_skips_the_shard(codec):
    n_s, n_sh = 4096 + 256, 3
    sb = wire.shard_bytes(codec, n_s)
    g_dev, g, e0 = _inputs(n_s * n_sh, torch.float32, 5)
    e = torch.from_numpy(e0.copy()).to(DEV)
    bufs = [torch.full((sb,), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(n_sh)]
    wire.pack_ef(g_dev, e, [bufs[0], None, bufs[2]], n_s, codec, self_shard=2)
    torch.cuda.synchronize()
    w_ref, e_ref = O.ef_pack(g, e0, n_s, codec, 2)
    assert np.array_equal(bufs[0].cpu().numpy(), w_ref[:sb]) and np.array_equal(bufs[2].cpu().numpy(), w_ref[2 * sb:])
    assert (bufs[1] == 0xA5).all(), "the buffer behind the null destination is untouched"
    got = e.cpu().numpy()
    assert np.array_equal(got[:n_s], e_ref[:n_s])
    assert np.array_equal(got[n_s:].view(np.uint32), e0[n_s:].view(np.uint32)), "skipped and own shards: not fed back"


def test_pack_ef_second_trip():
    """One shard above the grid cap's 2048 blocks x 4096 elements: the first 16 lanes take a second trip."""
    n_s, codec = 2048 * 4096 + 256, "bfp_rne"
    sb = wire.shard_bytes(codec, n_s)
    g_dev, g, e0 = _inputs(n_s, torch.float32, 6)
    e = torch.from_numpy(e0.copy()).to(DEV)
    out = torch.zeros(sb, dtype=torch.uint8, device=DEV)
    wire.pack_ef(g_dev, e, out, n_s, codec)
    torch.cuda.synchronize()
    w_ref, e_ref = O.ef_pack(g, e0, n_s, codec, -1)
    assert np.array_equal(out.cpu().numpy(), w_ref)
    assert np.array_equal(e.cpu().numpy().view(np.uint32), e_ref.view(np.uint32))
    assert not np.array_equal(e_ref[-256:], e0[-256:]), "the second trip's elements were fed back"


# --------------------------------------------------------------------------- wire_reduce_ef
def _slots(n_slots, n_s, codec, seed):
    rng = np.random.default_rng(seed)
    vals = (rng.standard_normal(n_slots * n_s) * np.exp(rng.standard_normal(n_slots * n_s))).astype(np.float32)
    return O.pack(vals, n_s, codec)


@pytest.mark.parametrize("codec", BFP)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_slots", [1, 2, 3, 8])
def test_reduce_ef_matches_oracle(C, n_slots, dtype, codec):
    saved = C.wire_reduce4()
    try:
        for n_s in (256, 4096 + 256):
            sb = wire.shard_bytes(codec, n_s)
            packed = _slots(n_slots, n_s, codec, n_slots * 7 + n_s)
            slots = torch.from_numpy(packed).to(DEV)
            l_dev, l_np, e0 = _inputs(n_s, dtype, n_slots + n_s)
            for self_pos in sorted({0, n_slots // 2, n_slots - 1}):
                w_ref, e_ref = O.ef_reduce([packed[r * sb:(r + 1) * sb] for r in range(n_slots)], l_np, self_pos, e0,
                                           codec, n_s)
                got = []
                for lanes4 in ((0, 1) if n_slots <= 2 else (saved,)):
                    C.set_wire_reduce4(lanes4)
                    e = torch.from_numpy(e0.copy()).to(DEV)
                    o1 = torch.full((sb + 64,), 0xA5, dtype=torch.uint8, device=DEV)
                    o2 = torch.zeros(sb, dtype=torch.uint8, device=DEV)
                    wire.reduce_ef(slots, n_slots, self_pos, l_dev, e, [o1[:sb], None, o2], n_s, codec)
                    torch.cuda.synchronize()
                    assert torch.equal(o1[:sb], o2) and (o1[sb:] == 0xA5).all()
                    got.append((o2.cpu().numpy(), e.cpu().numpy()))
                for w, e in got:
                    assert np.array_equal(w, w_ref), (n_s, self_pos, "wire")
                    assert np.array_equal(e.view(np.uint32), e_ref.view(np.uint32)), (n_s, self_pos, "residual")
    finally:
        C.set_wire_reduce4(saved)


@pytest.mark.parametrize("codec", BFP)
def test_zero_residual_gives_todays_bytes(codec):
    n_s, n_sh = 4096 + 256, 3
    sb = wire.shard_bytes(codec, n_s)
    g_dev, _, _ = _inputs(n_s * n_sh, torch.bfloat16, 8)
    a = torch.zeros(sb * n_sh, dtype=torch.uint8, device=DEV)
    b = torch.zeros_like(a)
    wire.pack(g_dev, a, n_s, codec)
    wire.pack_ef(g_dev, torch.zeros(n_s * n_sh, device=DEV), b, n_s, codec, self_shard=1)
    assert torch.equal(a, b)
    for n_slots in (1, 2, 3):
        local = g_dev[:n_s].to(torch.float32)
        s1 = torch.zeros(sb, dtype=torch.uint8, device=DEV)
        s2 = torch.zeros_like(s1)
        wire.reduce(a, n_slots, n_slots - 1, local, s1, None, n_s, codec)
        wire.reduce_ef(a, n_slots, n_slots - 1, local, torch.zeros(n_s, device=DEV), s2, n_s, codec)
        assert torch.equal(s1, s2)


def test_wire_op_refusals():
    n_s = 256
    g = torch.zeros(n_s, device=DEV)
    out = torch.zeros(wire.shard_bytes("bfp_rne", n_s), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="BFP codecs only"):
        wire.pack_ef(g, torch.zeros(n_s, device=DEV), torch.zeros(4 * n_s, dtype=torch.uint8, device=DEV), n_s, "raw_f32")
    with pytest.raises(ValueError, match="float32"):
        wire.pack_ef(g, torch.zeros(n_s, device=DEV, dtype=torch.bfloat16), out, n_s, "bfp_rne")
    with pytest.raises(ValueError, match="needs"):
        wire.pack_ef(g, torch.zeros(n_s - 16, device=DEV), out, n_s, "bfp_rne")
    with pytest.raises(ValueError, match="lives on"):
        wire.reduce_ef(out, 1, 0, g, torch.zeros(n_s), out, n_s, "bfp_rne")
    with pytest.raises(RuntimeError, match="residual"):  # the binding's own check
        _ext.require().wire_reduce_ef(out, 1, 0, g, torch.zeros(n_s - 16, device=DEV), [out], n_s, 1)


# --------------------------------------------------------------------------- engines over virtual ranks
def _threads(N, fn):
    out, errs = [None] * N, [None] * N

    def run(r):
        try:
            out[r] = fn(r)
        except Exception as e:  # noqa: BLE001
            errs[r] = e

    ts = [threading.Thread(target=run, args=(r,)) for r in range(N)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts), "virtual rank thread hung"
    for e in errs:
        if e is not None:
            raise e
    return out


STEPS, N_ELEMS, LR = 4, 12000 - 48, 0.5


def _step_grads(N, seed):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(N_ELEMS) * (1 + r)).astype(np.float32) for r in range(N)] for _ in range(STEPS)]


def _sim_steps(grads, shard, codec):
    N = len(grads[0])
    planes = [np.zeros(shard * N, np.float32) for _ in range(N)]
    res = []
    for t in range(STEPS):
        gin = [np.pad(g, (0, shard * N - N_ELEMS)) for g in grads[t]]
        out, planes = sim.mesh_allreduce_ef(gin, planes, shard, codec)
        res.append((out, [p.copy() for p in planes]))
    return res


def _engine_steps(eng, r, grads, w0):
    """STEPS steps on rank r: a sum-only request on one plane and an SGD request on a second one (same gradients, so
    the planes stay equal). Returns per step (decoded sum, weights, plane a, plane b)."""
    torch.cuda.set_device(0)
    L = eng.layout(N_ELEMS)
    ea, eb = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    w = torch.zeros(L.n_pad, device=DEV)
    w[:N_ELEMS] = torch.from_numpy(w0)
    res = []
    for t in range(STEPS):
        g, out = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
        g[:N_ELEMS] = torch.from_numpy(grads[t][r])
        torch.cuda.synchronize()
        eng.allreduce(g, out, n_valid=N_ELEMS, residual=ea).synchronize(60)
        h = eng.allreduce_sgd(g, w, n_valid=N_ELEMS, lr=LR, defer=True, residual=eb)
        h.commit_after_current()
        h.synchronize(60)
        torch.cuda.synchronize()
        res.append(tuple(x.cpu().numpy().copy() for x in (out, w, ea, eb)))
    return res, L.shard


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("codec", BFP)
def test_native_engine_loopback(nranks, codec):
    C = _ext.require()
    grads = _step_grads(nranks, 100 + nranks)
    w0 = np.random.default_rng(9).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(nranks, 60.0)
    engs = [NativeAllReduce(None, codec=codec, comm=fabric.comm(r)) for r in range(nranks)]
    res = _threads(nranks, lambda r: _engine_steps(engs[r], r, grads, w0))
    shard = res[0][1]
    ref = _sim_steps(grads, shard, codec)
    w = w0
    for t in range(STEPS):
        w, _ = O.sgd(w, ref[t][0][:N_ELEMS], LR)
        for r in range(nranks):
            out, wg, ea, eb = res[r][0][t]
            assert np.array_equal(out, ref[t][0]), (r, t, "decoded result")
            assert np.array_equal(ea, ref[t][1][r]) and np.array_equal(eb, ref[t][1][r]), (r, t, "plane")
            assert np.array_equal(wg[:N_ELEMS], w) and not wg[N_ELEMS:].any(), (r, t, "weights")
    # the Python engine issues the same launches on the same GPU tensors: the same bits
    pys = [None] * nranks

    def py_rank(t):
        eng = CompressedAllReduce(t, codec=codec, device=DEV)
        assert eng.layout(N_ELEMS).shard == shard
        pys[t.rank] = _engine_steps(eng, t.rank, grads, w0)

    ThreadFabric(nranks, timeout_s=60).run(py_rank)
    for r in range(nranks):
        for a, b in zip(pys[r][0], res[r][0]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), "native engine differs from the Python engine"


def _clip_adamw_steps(eng, r, grads, w0, steps=2):
    """Two buckets (the same gradients, halves of a clip group) per step with AdamW and error feedback."""
    torch.cuda.set_device(0)
    L = eng.layout(N_ELEMS)
    words = torch.full((4,), math.nan, device=DEV)
    planes = []
    for _ in range(2):
        w = torch.zeros(L.n_pad, device=DEV)
        w[:N_ELEMS] = torch.from_numpy(w0)
        planes.append([w] + [torch.zeros(L.n_pad, device=DEV) for _ in range(3)])  # w, m, v, residual
    hist = []
    for t in range(steps):
        g = torch.zeros(L.n_pad, device=DEV)
        g[:N_ELEMS] = torch.from_numpy(grads[t][r])
        torch.cuda.synchronize()
        hs = [eng.allreduce_sgd(g, w, None, m, n_valid=N_ELEMS, lr=0.01, weight_decay=0.01, grad_scale=0.5, defer=True,
                                opt="adamw", var=v, step=t + 1, clip=words, residual=e, name=f"b{b}")
              for b, (w, m, v, e) in enumerate(planes)]
        eng.commit_group(hs, max_norm=1.0, grad_scale=0.5)
        for h in hs:
            h.synchronize(60)
        torch.cuda.synchronize()
        hist.append(([[x.cpu().numpy().copy() for x in p] for p in planes], words.cpu().numpy().copy()))
    return hist, L.shard


def test_native_engine_loopback_adamw_clip_group():
    C = _ext.require()
    N, codec = 2, "bfp_rne"
    grads = _step_grads(N, 77)
    w0 = np.random.default_rng(10).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engs = [NativeAllReduce(None, codec=codec, comm=fabric.comm(r)) for r in range(N)]
    res = _threads(N, lambda r: _clip_adamw_steps(engs[r], r, grads, w0))
    ref = _sim_steps(grads, res[0][1], codec)
    pys = [None] * N

    def py_rank(t):
        pys[t.rank] = _clip_adamw_steps(CompressedAllReduce(t, codec=codec, device=DEV), t.rank, grads, w0)

    ThreadFabric(N, timeout_s=60).run(py_rank)
    for r in range(N):
        for t, (planes, words) in enumerate(res[r][0]):
            assert 0 < words[0] < 1 and words[3] == 0, "the group was clipped"
            assert np.array_equal(words, res[0][0][t][1]) and np.array_equal(words, pys[r][0][t][1])
            for b in range(2):
                assert np.array_equal(planes[b][3], ref[t][1][r]), "plane differs from the simulator"
                for x, y, z in zip(planes[b], res[0][0][t][0][b][:3] + [planes[b][3]], pys[r][0][t][0][b]):
                    assert np.array_equal(x, y), "replicas must be bit-identical"
                    assert np.array_equal(x, z), "native engine differs from the Python engine"
            assert not np.array_equal(planes[0][0][:N_ELEMS], w0)


# --------------------------------------------------------------------------- trainer
_NT = {}


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


def _native_transport():
    if "t" not in _NT:  # one 1-rank communicator for the whole module
        _NT["t"] = NativeTransport(rank=0, world=1, device=0, store=_Store(), force_collectives=True)
    return _NT["t"]


def _train(engine, steps=3, **kw):
    sizes, mb = [64, 128, 64], 256
    eng = {"native": lambda: NativeAllReduce(None, codec="bfp_rne"),
           "python": lambda: CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", device=DEV),
           "forced": lambda: NativeAllReduce(_native_transport(), codec="bfp_rne", force_comm=True)}[engine]()
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, momentum=True, adam=kw.get("optimizer") == "adamw",
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=0.05, weight_decay=1e-2, **kw)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=g) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32).to(DEV)
    hist = []
    for _ in range(steps):
        tr.step(x, y)
        tr.finish()
        hist.append([(l.master.cpu(), l.mom.cpu(), l.lp.cpu()) for l in model.layers])
    return hist, tr


def _same(a, b):
    return all(torch.equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))


@pytest.mark.parametrize("kw", [dict(momentum=0.9), dict(optimizer="adamw", trust_ratio=True, max_grad_norm=0.05)],
                         ids=["sgd", "lamb_clip"])
def test_trainer_world1_inline_and_forced(kw):
    inl, ti = _train("native", error_feedback=True, **kw)
    frc, tf = _train("forced", error_feedback=True, **kw)
    assert ti.error_feedback and not ti.prepack and not ti.fused_update and ti.fused_updates == 0
    assert not tf.engine.inline and len(ti.residuals) == 2
    for t in range(3):
        assert _same(inl[t], frc[t]), f"step {t + 1}: inline and forced multi-rank paths differ"
    for a, b in zip(ti.residuals, tf.residuals):
        assert torch.equal(a, b) and a.dtype == torch.float32 and bool(a.any())
    py, tp = _train("python", error_feedback=True, **kw)
    assert all(_same(a, b) for a, b in zip(inl, py)) and all(torch.equal(a, b) for a, b in zip(ti.residuals,
                                                                                               tp.residuals))
    # live: with zero planes step 1 is the engine-packed trainer's without feedback, step 2 is not
    off, _ = _train("native", error_feedback=False, prepack=False, **kw)
    assert _same(inl[0], off[0]) and not _same(inl[1], off[1])


def test_trainer_flag_off_is_the_trainer_without_it():
    a, ta = _train("native", error_feedback=False, momentum=0.9)
    b, tb = _train("native", momentum=0.9)
    assert ta.residuals is None and ta.prepack == tb.prepack and ta.fused_update == tb.fused_update
    assert all(_same(x, y) for x, y in zip(a, b))


# --------------------------------------------------------------------------- direct P2P mesh, two processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _p2p_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from fpga_ai_nic_amd.parallel.transport import make_p2p_comm

        torch.cuda.set_device(0)
        comm = make_p2p_comm(rank, world, 0, slot_bytes=4 << 20)
        codec, m, steps = "bfp_rne", 30000, 3
        rng = np.random.default_rng(11)
        grads = [[rng.standard_normal(m).astype(np.float32) for _ in range(world)] for _ in range(steps)]
        eng = NativeAllReduce(None, codec=codec, algo="mesh", comm=comm)
        L = eng.layout(m)
        e = torch.zeros(L.n_pad, device="cuda")
        planes = [np.zeros(L.n_pad, np.float32) for _ in range(world)]
        ok = {}
        for t in range(steps):
            g = torch.zeros(L.n_pad, device="cuda")
            g[:m] = torch.from_numpy(grads[t][rank]).cuda()
            out = torch.zeros(L.n_pad, device="cuda")
            eng.allreduce(g, out, n_valid=m, residual=e).synchronize(30)
            torch.cuda.synchronize()
            ref, planes = sim.mesh_allreduce_ef([np.pad(x, (0, L.n_pad - m)) for x in grads[t]], planes, L.shard, codec)
            ok[f"step{t}_result"] = bool(np.array_equal(out.cpu().numpy(), ref))
            ok[f"step{t}_plane"] = bool(np.array_equal(e.cpu().numpy(), planes[rank]))
        ok["direct_rounds"] = eng.counters()["direct_rounds"] >= 2 * steps
        ok["live"] = bool(np.any(planes[rank]))
        q.put((rank, ok, comm.sequence))
    except Exception as ex:  # noqa: BLE001
        q.put((rank, {"error": repr(ex)}, -1))
    finally:
        dist.destroy_process_group()


def test_p2p_two_processes_one_gpu():
    import torch.multiprocessing as mp

    world = 2
    q = mp.get_context("spawn").Queue()
    pc = mp.start_processes(_p2p_worker, args=(world, _free_port(), q), nprocs=world, join=False, start_method="spawn")
    res = {}
    try:
        for _ in range(world):
            rank, ok, seq = q.get(timeout=180)
            res[rank] = (ok, seq)
    except _queue.Empty:
        for p in pc.processes:
            p.kill()
        pytest.fail("p2p workers did not report within 180 s")
    while not pc.join(60):
        pass
    for rank, (ok, _) in res.items():
        assert "error" not in ok, ok
        assert all(ok.values()), f"rank {rank}: {ok}"
    assert res[0][1] == res[1][1], "ranks issued different numbers of rounds"


# --------------------------------------------------------------------------- refusals
def test_native_engine_refusals():
    C = _ext.require()
    n = 50000 - 48

    def bufs(eng, **lay):
        L = eng.layout(n, **lay)
        return [torch.zeros(L.n_pad, device=DEV) for _ in range(3)]

    eng = NativeAllReduce(None, codec="bfp_rne")
    g, w, e = bufs(eng)
    kw = dict(n_valid=n, lr=1.0)
    for bad, match in [(e.double(), "float32"), (e.to(torch.bfloat16), "float32"), (e[:-16].clone(), "layout needs"),
                       (torch.zeros(2 * e.numel(), device=DEV)[::2], "contiguous"), (e.cpu(), "lives on")]:
        with pytest.raises(ValueError, match=match):
            eng.allreduce_sgd(g, w, residual=bad, **kw)
        with pytest.raises(ValueError, match=match):
            eng.allreduce(g, w, n_valid=n, residual=bad)
    with pytest.raises(RuntimeError, match="residual"):  # the binding's own check of what the wrapper lets through
        eng.C.submit(g, w, None, None, n, 1.0, residual=e[:-16].clone())
    with pytest.raises(RuntimeError, match="residual"):
        eng.C.submit(g, w, None, None, n, 1.0, residual=e.double())
    # prepacked input
    tgt = eng.prepack_target(g, n)
    with pytest.raises(ValueError, match="prepacked"):
        eng.allreduce_sgd(g, w, residual=e, prepacked=(tgt[0], 0), **kw)
    with pytest.raises(RuntimeError, match="prepacked"):
        eng.C.submit(g, w, None, None, n, 1.0, prepacked=tgt[0], prepacked_elems=0, residual=e)
    # raw codecs
    for codec, match in (("raw_f32", "nothing to feed back"), ("raw_bf16", "raw_bf16 is not supported yet")):
        raw = NativeAllReduce(None, codec=codec)
        with pytest.raises(ValueError, match=match):
            raw.allreduce_sgd(g, w, residual=e, **kw)
        with pytest.raises(RuntimeError, match=match):
            raw.C.submit(g, w, None, None, n, 1.0, residual=e)
    # the ring schedule
    ring = NativeAllReduce(None, codec="bfp_rne", algo="ring", comm=C.LoopbackFabric(2, 60.0).comm(0))
    gr, wr, er = bufs(ring)
    with pytest.raises(ValueError, match="ring schedule"):
        ring.allreduce_sgd(gr, wr, residual=er, **kw)
    with pytest.raises(RuntimeError, match="ring schedule"):
        ring.C.submit(gr, wr, None, None, n, 1.0, residual=er)
    # chunked layouts: a bucket above chunk_elems, and an explicit layout=(shard, chunks)
    ch = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), chunk_elems=8192)
    assert ch.layout(n).chunks > 1
    gc, wc, ec = bufs(ch)
    with pytest.raises(ValueError, match="chunked"):
        ch.allreduce_sgd(gc, wc, residual=ec, **kw)
    with pytest.raises(RuntimeError, match="chunked"):
        ch.C.submit(gc, wc, None, None, n, 1.0, residual=ec)
    ex = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0))
    gx, wx, exr = bufs(ex, shard=8192, chunks=4)
    with pytest.raises(ValueError, match="chunked"):
        ex.allreduce_sgd(gx, wx, residual=exr, layout=(8192, 4), **kw)
    # the sharded update (request and trainer)
    sh = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), shard_update=True)
    assert sh.shard_update
    gs, ws, es = bufs(sh)
    with pytest.raises(ValueError, match="sharded"):
        sh.allreduce_sgd(gs, ws, ws.to(torch.bfloat16), residual=es, **kw)
    with pytest.raises(RuntimeError, match="sharded"):
        sh.C.submit(gs, ws, ws.to(torch.bfloat16), None, n, 1.0, residual=es)
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, pad_fn=lambda k, x=sh: x.layout(k).n_pad)
    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, sh, error_feedback=True)
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, pad_fn=lambda k, x=ring: x.layout(k).n_pad)
    with pytest.raises(ValueError, match="ring"):
        DataParallelTrainer(model, ring, error_feedback=True)
    # more ranks than the kernels' destination table holds
    wide = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(17, 60.0).comm(0))
    gw, ww, ew = bufs(wide)
    with pytest.raises(ValueError, match="at most 16 ranks"):
        wide.allreduce_sgd(gw, ww, residual=ew, **kw)
    with pytest.raises(RuntimeError, match="at most 16 ranks"):
        wide.C.submit(gw, ww, None, None, n, 1.0, residual=ew)
    # nothing ran, and an ordinary request with a plane still completes on the first engine
    assert not e.any() and not w.any()
    g.fill_(1.0)
    eng.allreduce_sgd(g, w, residual=e, **kw).synchronize(30)
    torch.cuda.synchronize()
    assert torch.all(w[:n] == -1.0) and not e.any(), "1.0 is exactly representable: nothing dropped"
