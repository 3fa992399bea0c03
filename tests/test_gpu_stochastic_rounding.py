"""Stochastic rounding on the GPU: ``wire_pack_sr_kernel`` / ``wire_reduce_sr_kernel`` against the NumPy oracle, the
native engine against the simulator (LoopbackFabric ranks and two processes over the direct P2P mesh), the trainer and
the refusals. Everything is compared bit for bit."""
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
CODECS = ["bfp_rne", "bfp4_rne"]
QMAX = {"bfp_rne": 127, "bfp4_rne": 7}
# (shard elements, shards): 16 active lanes; a second block that is almost empty; 40 blocks' worth over 3 shards
SHAPES = [(256, 2), (4096 + 256, 2), (256 * 40, 3)]
SEED = 0x9E3779B97F4A7C15


def _values(n, dtype, seed, codec):
    """Normal values under a log-normal scale, plus groups of zeros, of denormals, a NaN group, an Inf group and values
    at +-qmax steps of their group. Returns the GPU tensor and the f32 values the kernels read."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 2)).astype(np.float32)
    x[16:32] = 0
    x[48:64] = (rng.standard_normal(16) * 1e-41).astype(np.float32)  # (bf16 input flushes these to zero or its denormals)
    x[80] = np.nan
    x[112:128] = rng.standard_normal(16).astype(np.float32)
    x[115], x[116] = np.inf, -np.inf
    q = QMAX[codec]
    x[144:160] = np.ldexp(rng.integers(-q, q + 1, 16).astype(np.float32), -3)
    x[144], x[145] = np.ldexp(np.float32(q), -3), np.ldexp(np.float32(-q), -3)
    x[160:176] = np.ldexp(rng.uniform(-q, q, 16).astype(np.float32), 5)
    x[160], x[161] = np.ldexp(np.float32(q + 0.75), 5), np.ldexp(np.float32(-q - 0.75), 5)  # clamped at +-qmax
    t = torch.from_numpy(x).to(dtype)
    return t.to(DEV), t.to(torch.float32).numpy()


# --------------------------------------------------------------------------- wire_pack_sr
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_pack_sr_matches_oracle(n_s, n_sh, dtype, codec):
    n = n_s * n_sh
    sb = wire.shard_bytes(codec, n_s)
    g_dev, g = _values(n, dtype, n_s + n_sh, codec)
    plain = O.pack(g, n_s, codec)
    for self_shard in (-1, 0, n_sh - 1):
        out = torch.full((sb * n_sh + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        wire.pack_sr(g_dev, out[: sb * n_sh], n_s, codec, SEED, 3, self_shard=self_shard, base=n_s)
        torch.cuda.synchronize()
        ref = O.sr_pack(g, n_s, codec, SEED, 3, self_shard, n_s)
        got = out.cpu().numpy()
        assert np.array_equal(got[: sb * n_sh], ref), (self_shard, "wire")
        assert (got[sb * n_sh:] == 0xA5).all(), "bytes past the last shard untouched"
        for q in range(n_sh):
            same = np.array_equal(ref[q * sb:(q + 1) * sb], plain[q * sb:(q + 1) * sb])
            assert same == (q == self_shard), "the own shard alone is the plain rne encoding"
    # decoding is today's: the NaN and Inf groups decode to NaN, the representable values to themselves
    dec = O.unpack(ref[:sb], n_s, n_s, codec)
    assert np.isnan(dec[80:96]).all() and np.isnan(dec[112:128]).all()
    if dtype == torch.float32:
        assert np.array_equal(dec[144:160], g[144:160])


@pytest.mark.parametrize("codec", CODECS)
def test_pack_sr_null_destination_and_grid(C, codec):
    n_s, n_sh = 256 * 40, 3
    sb = wire.shard_bytes(codec, n_s)
    g_dev, g = _values(n_s * n_sh, torch.float32, 5, codec)
    ref = O.sr_pack(g, n_s, codec, 7, 0, 2)
    bufs = [torch.full((sb,), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(n_sh)]
    wire.pack_sr(g_dev, [bufs[0], None, bufs[2]], n_s, codec, 7, 0, self_shard=2)
    torch.cuda.synchronize()
    assert np.array_equal(bufs[0].cpu().numpy(), ref[:sb]) and np.array_equal(bufs[2].cpu().numpy(), ref[2 * sb:])
    assert (bufs[1] == 0xA5).all(), "the buffer behind the null destination is untouched"
    # the bits do not depend on the grid: one block (every lane takes three trips per shard) against the default
    saved = C.p2p_grid_cap()
    try:
        C.set_p2p_grid_cap(1)
        one = torch.zeros(sb * n_sh, dtype=torch.uint8, device=DEV)
        wire.pack_sr(g_dev, one, n_s, codec, 7, 0, self_shard=2, peers=True)
        torch.cuda.synchronize()
    finally:
        C.set_p2p_grid_cap(0)
    assert C.p2p_grid_cap() == saved
    assert np.array_equal(one.cpu().numpy(), ref)


def test_pack_sr_last_elements_below_2_32():
    """The last 256 elements a bucket may hold: indices up to 2^32 - 1 (the word index does not wrap)."""
    n_s, codec = 256, "bfp_rne"
    g_dev, g = _values(n_s, torch.float32, 6, codec)
    out = torch.zeros(wire.shard_bytes(codec, n_s), dtype=torch.uint8, device=DEV)
    wire.pack_sr(g_dev, out, n_s, codec, 1, 15, base=(1 << 32) - 256)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), O.sr_pack(g, n_s, codec, 1, 15, -1, (1 << 32) - 256))


# --------------------------------------------------------------------------- wire_reduce_sr
def _slots(n_slots, n_s, codec, seed):
    rng = np.random.default_rng(seed)
    vals = (rng.standard_normal(n_slots * n_s) * np.exp(rng.standard_normal(n_slots * n_s))).astype(np.float32)
    return O.pack(vals, n_s, codec)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_slots", [1, 2, 3, 8])
def test_reduce_sr_matches_oracle(C, n_slots, dtype, codec):
    saved, saved_cap = C.wire_reduce4(), C.p2p_grid_cap()
    try:
        for n_s in (256, 4096 + 256):
            sb = wire.shard_bytes(codec, n_s)
            packed = _slots(n_slots, n_s, codec, n_slots * 7 + n_s)
            slots = torch.from_numpy(packed).to(DEV)
            l_dev, l_np = _values(n_s, dtype, n_slots + n_s, codec)
            for self_pos in sorted({0, n_slots // 2, n_slots - 1}):
                ref = O.sr_reduce([packed[r * sb:(r + 1) * sb] for r in range(n_slots)], l_np, self_pos, codec, n_s,
                                  SEED, 2, 2 * n_s)
                for lanes4 in (0, 1):  # both lane layouts (the 4-value one runs for the 8-bit codec at <= 2 slots)
                    for cap in (0, 1):  # the default grid, and one block through the P2P launch form
                        C.set_wire_reduce4(lanes4)
                        C.set_p2p_grid_cap(cap)
                        o1 = torch.full((sb + 64,), 0xA5, dtype=torch.uint8, device=DEV)
                        o2 = torch.zeros(sb, dtype=torch.uint8, device=DEV)
                        wire.reduce_sr(slots, n_slots, self_pos, l_dev, [o1[:sb], None, o2], n_s, codec, SEED, 2,
                                       base=2 * n_s, peers=cap == 1)
                        torch.cuda.synchronize()
                        assert torch.equal(o1[:sb], o2) and (o1[sb:] == 0xA5).all()
                        assert np.array_equal(o2.cpu().numpy(), ref), (n_s, self_pos, lanes4, cap)
                plain = torch.zeros(sb, dtype=torch.uint8, device=DEV)
                wire.reduce(slots, n_slots, self_pos, l_dev, plain, None, n_s, codec)
                assert not torch.equal(plain, o2)
    finally:
        C.set_wire_reduce4(saved)
        C.set_p2p_grid_cap(0)
    assert C.p2p_grid_cap() == saved_cap


def test_wire_op_refusals():
    C = _ext.require()
    n_s = 256
    g = torch.zeros(n_s, device=DEV)
    out = torch.zeros(wire.shard_bytes("bfp_rne", n_s), dtype=torch.uint8, device=DEV)
    big = torch.zeros(4 * n_s, dtype=torch.uint8, device=DEV)
    for codec in ("bfp_trunc", "raw_f32", "raw_bf16"):
        with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
            wire.pack_sr(g, big, n_s, codec, 0, 0)
        with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
            wire.reduce_sr(big, 1, 0, g, big, n_s, codec, 0, 0)
    with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
        wire.pack_sr(g, out, n_s, "bfp_rne", 1 << 64, 0)
    with pytest.raises(ValueError, match="2\\^32 or more"):
        wire.reduce_sr(out, 1, 0, g, out, n_s, "bfp_rne", 0, 0, base=1 << 32)
    # the bindings' own checks
    with pytest.raises(RuntimeError, match="bfp_rne and bfp4_rne only"):
        C.wire_pack_sr(g, [big], n_s, 0, 0, 0)
    with pytest.raises(RuntimeError, match="bfp_rne and bfp4_rne only"):
        C.wire_reduce_sr(big, 1, 0, g, [big], n_s, 3, 0, 0)
    with pytest.raises(RuntimeError, match=r"\[0, 2\^64\)"):
        C.wire_pack_sr(g, [out], n_s, 1, -1, 0)
    with pytest.raises(RuntimeError, match=r"\[0, 2\^64\)"):
        C.wire_reduce_sr(out, 1, 0, g, [out], n_s, 1, 1 << 64, 0)
    with pytest.raises(RuntimeError, match="2\\^32 or more"):
        C.wire_pack_sr(g, [out], n_s, 1, 0, 0, -1, (1 << 32) - 16)
    with pytest.raises(RuntimeError, match="2\\^32 or more"):
        C.wire_reduce_sr(out, 1, 0, g, [out], n_s, 1, 0, 0, 1 << 32)
    with pytest.raises(RuntimeError, match="rank"):
        C.wire_pack_sr(g, [out], n_s, 1, 0, 16)
    assert not out.any(), "refused: nothing ran"


# --------------------------------------------------------------------------- native engine over virtual ranks
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


STEPS, N_ELEMS, LR, MOM = 2, 12000 - 48, 0.5, 0.9


def _step_grads(N, seed):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(N_ELEMS) * (1 + r)).astype(np.float32) for r in range(N)] for _ in range(STEPS)]


def _seed_of(t, bucket):
    return O.sr_step_seed(SEED, t + 1, bucket)


def _sgd_steps(eng, r, grads, w0):
    """STEPS steps on rank r: a sum-only request, an SGD-with-momentum request under the same seed, and the same
    sum-only request without a seed. Returns per step (stochastic sum, weights, momentum, plain sum)."""
    torch.cuda.set_device(0)
    L = eng.layout(N_ELEMS)
    w, m = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    w[:N_ELEMS] = torch.from_numpy(w0)
    res = []
    for t in range(STEPS):
        g = torch.zeros(L.n_pad, device=DEV)
        out, plain = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
        g[:N_ELEMS] = torch.from_numpy(grads[t][r])
        torch.cuda.synchronize()
        eng.allreduce(g, out, n_valid=N_ELEMS, sr_seed=_seed_of(t, 0)).synchronize(60)
        h = eng.allreduce_sgd(g, w, None, m, n_valid=N_ELEMS, lr=LR, momentum=MOM, defer=True, sr_seed=_seed_of(t, 0))
        h.commit_after_current()
        h.synchronize(60)
        eng.allreduce(g, plain, n_valid=N_ELEMS).synchronize(60)
        torch.cuda.synchronize()
        res.append(tuple(x.cpu().numpy().copy() for x in (out, w, m, plain)))
    return res, L.shard


@pytest.mark.parametrize("nranks", [2, 3, 4, 8])
@pytest.mark.parametrize("codec", CODECS)
def test_native_engine_loopback_sgd(nranks, codec):
    C = _ext.require()
    grads = _step_grads(nranks, 100 + nranks)
    w0 = np.random.default_rng(9).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(nranks, 60.0)
    engs = [NativeAllReduce(None, codec=codec, comm=fabric.comm(r)) for r in range(nranks)]
    res = _threads(nranks, lambda r: _sgd_steps(engs[r], r, grads, w0))
    shard = res[0][1]
    w, m = w0, np.zeros(N_ELEMS, np.float32)
    for t in range(STEPS):
        gin = [np.pad(g, (0, shard * nranks - N_ELEMS)) for g in grads[t]]
        ref = sim.mesh_allreduce_sr(gin, shard, codec, _seed_of(t, 0))
        plain = sim.mesh_allreduce(gin, shard, codec)
        assert not np.array_equal(ref, plain)
        w, m = O.sgd(w, ref[:N_ELEMS], LR, momentum=MOM, mom=m)
        for r in range(nranks):  # (every rank against one reference: replicas identical)
            out, wg, mg, pl = res[r][0][t]
            assert np.array_equal(out, ref), (r, t, "decoded result")
            assert np.array_equal(wg[:N_ELEMS], w) and not wg[N_ELEMS:].any(), (r, t, "weights")
            assert np.array_equal(mg[:N_ELEMS], m), (r, t, "momentum")
            assert np.array_equal(pl, plain), (r, t, "without a seed: today's bits")


def _clip_adamw_steps(eng, r, grads, w0):
    """Two buckets (the same gradients, seeds of their own, halves of a clip group) per step with AdamW."""
    torch.cuda.set_device(0)
    L = eng.layout(N_ELEMS)
    words = torch.full((4,), math.nan, device=DEV)
    planes = []
    for _ in range(2):
        w = torch.zeros(L.n_pad, device=DEV)
        w[:N_ELEMS] = torch.from_numpy(w0)
        planes.append([w] + [torch.zeros(L.n_pad, device=DEV) for _ in range(2)])  # w, m, v
    hist = []
    for t in range(STEPS):
        g = torch.zeros(L.n_pad, device=DEV)
        g[:N_ELEMS] = torch.from_numpy(grads[t][r])
        torch.cuda.synchronize()
        hs = [eng.allreduce_sgd(g, w, None, m, n_valid=N_ELEMS, lr=0.01, weight_decay=0.01, grad_scale=0.5, defer=True,
                                opt="adamw", var=v, step=t + 1, clip=words, sr_seed=_seed_of(t, b), name=f"b{b}")
              for b, (w, m, v) in enumerate(planes)]
        eng.commit_group(hs, max_norm=1.0, grad_scale=0.5)
        for h in hs:
            h.synchronize(60)
        torch.cuda.synchronize()
        hist.append(([[x.cpu().numpy().copy() for x in p] for p in planes], words.cpu().numpy().copy()))
    return hist, L.shard


@pytest.mark.parametrize("nranks", [2, 3, 4, 8])
@pytest.mark.parametrize("codec", CODECS)
def test_native_engine_loopback_adamw_clip_group(nranks, codec):
    """AdamW with a clip group on top of the stochastic wire: the simulator's decoded gradients through the oracle's
    clip coefficient and AdamW step, bit for bit on every rank."""
    C = _ext.require()
    grads = _step_grads(nranks, 200 + nranks)
    w0 = np.random.default_rng(10).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(nranks, 60.0)
    engs = [NativeAllReduce(None, codec=codec, comm=fabric.comm(r)) for r in range(nranks)]
    res = _threads(nranks, lambda r: _clip_adamw_steps(engs[r], r, grads, w0))
    shard = res[0][1]
    # the Python engine issues the same update launches over the same wire: the reference of the epilogue
    pys = [None] * nranks

    def py_rank(t):
        pys[t.rank] = _clip_adamw_steps(CompressedAllReduce(t, codec=codec, device=DEV), t.rank, grads, w0)

    ThreadFabric(nranks, timeout_s=60).run(py_rank)
    state = [[w0.copy(), np.zeros(N_ELEMS, np.float32), np.zeros(N_ELEMS, np.float32)] for _ in range(2)]
    for t in range(STEPS):
        gin = [np.pad(g, (0, shard * nranks - N_ELEMS)) for g in grads[t]]
        dec = [sim.mesh_allreduce_sr(gin, shard, codec, _seed_of(t, b))[:N_ELEMS] for b in range(2)]
        assert not np.array_equal(dec[0], dec[1]), "the buckets draw from seeds of their own"
        # the group's coefficient: the kernels' fp64 block sums against the oracle's exactly rounded sum (the last
        # bits of an fp64 sum in another order), then the device's own f32 word into the oracle's update
        want = O.clip_words(O.clip_sumsq(dec[0]) + O.clip_sumsq(dec[1]), 0.5, 1.0)
        coef = res[0][0][t][1][0]
        assert abs(float(coef) - float(want[0])) <= 2.0 ** -22 * float(want[0])
        sc = O.adamw_scalars(0.01, 0.01, 0.9, 0.999, 1e-8, t + 1)
        for b in range(2):
            state[b] = list(O.adamw(state[b][0], dec[b], state[b][1], state[b][2], sc,
                                    grad_scale=O.clip_scale(0.5, [coef])))
        for r in range(nranks):
            planes, words = res[r][0][t]
            assert 0 < words[0] < 1 and words[3] == 0, "the group was clipped"
            assert words[0] == coef and np.array_equal(words, pys[r][0][t][1])
            for b in range(2):
                for k in range(3):
                    assert np.array_equal(planes[b][k], pys[r][0][t][0][b][k]), "native differs from the Python engine"
                    assert np.array_equal(planes[b][k][:N_ELEMS], state[b][k]), (r, t, b, k, "oracle update")


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


def _train(engine, steps=2, **kw):
    sizes, mb = [256, 256, 256], 256
    eng = {"native": lambda: NativeAllReduce(None, codec="bfp_rne"),
           "python": lambda: CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", device=DEV),
           "forced": lambda: NativeAllReduce(_native_transport(), codec="bfp_rne", force_comm=True)}[engine]()
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, momentum=True,
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=0.05, weight_decay=1e-2, momentum=0.9, **kw)
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
    return all(torch.equal(x, y) for sa, sb in zip(a, b) for pa, pb in zip(sa, sb) for x, y in zip(pa, pb))


def test_trainer_world1_inline_and_forced():
    sr = dict(stochastic_rounding=True, sr_seed=5)
    inl, ti = _train("native", **sr)
    frc, tf = _train("forced", **sr)
    assert ti.stochastic_rounding and not ti.prepack and not ti.fused_update and ti.fused_updates == 0
    assert not tf.engine.inline and ti.sr_step == tf.sr_step == 2
    assert _same(inl, frc), "inline and forced multi-rank paths differ"
    assert _same(inl, _train("native", **sr)[0]) and _same(frc, _train("forced", **sr)[0]), "deterministic"
    assert _same(inl, _train("python", **sr)[0]), "native engine differs from the Python engine"
    off, _ = _train("native", prepack=False)
    assert not _same(inl[:1], off[:1]), "differs from the unflagged run from step 1 on"
    assert not _same(inl[:1], _train("native", stochastic_rounding=True, sr_seed=6)[0][:1])


def test_trainer_flag_off_is_the_trainer_without_it():
    a, ta = _train("native", stochastic_rounding=False, sr_seed=5)
    b, tb = _train("native")
    assert not ta.stochastic_rounding and ta.prepack == tb.prepack and ta.fused_update == tb.fused_update
    assert _same(a, b)


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
        m, steps = 30000, 2
        rng = np.random.default_rng(11)
        grads = [[rng.standard_normal(m).astype(np.float32) for _ in range(world)] for _ in range(steps)]
        ok = {}
        for codec in CODECS:
            eng = NativeAllReduce(None, codec=codec, algo="mesh", comm=comm)
            L = eng.layout(m)
            for t in range(steps):
                g = torch.zeros(L.n_pad, device="cuda")
                g[:m] = torch.from_numpy(grads[t][rank]).cuda()
                out, plain = torch.zeros(L.n_pad, device="cuda"), torch.zeros(L.n_pad, device="cuda")
                seed = O.sr_step_seed(SEED, t + 1, 0)
                eng.allreduce(g, out, n_valid=m, sr_seed=seed).synchronize(30)
                eng.allreduce(g, plain, n_valid=m).synchronize(30)
                torch.cuda.synchronize()
                gin = [np.pad(x, (0, L.n_pad - m)) for x in grads[t]]
                ok[f"{codec}_step{t}_result"] = bool(np.array_equal(out.cpu().numpy(),
                                                                    sim.mesh_allreduce_sr(gin, L.shard, codec, seed)))
                ok[f"{codec}_step{t}_unflagged"] = bool(np.array_equal(plain.cpu().numpy(),
                                                                       sim.mesh_allreduce(gin, L.shard, codec)))
                ok[f"{codec}_step{t}_live"] = not torch.equal(out, plain)
            ok[f"{codec}_direct_rounds"] = eng.counters()["direct_rounds"] >= 4 * steps
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
    sub = dict(sr=True, sr_seed=1)
    # the seed
    for bad in (-1, 1 << 64, 1.5, "1"):
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            eng.allreduce_sgd(g, w, sr_seed=bad, **kw)
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            eng.allreduce(g, w, n_valid=n, sr_seed=bad)
    with pytest.raises(TypeError):  # the binding takes a uint64
        eng.C.submit(g, w, None, None, n, 1.0, sr=True, sr_seed=-1)
    # together with error feedback
    with pytest.raises(ValueError, match="pick one"):
        eng.allreduce_sgd(g, w, sr_seed=1, residual=e, **kw)
    with pytest.raises(RuntimeError, match="pick one"):
        eng.C.submit(g, w, None, None, n, 1.0, residual=e, **sub)
    # prepacked input
    tgt = eng.prepack_target(g, n)
    with pytest.raises(ValueError, match="prepacked"):
        eng.allreduce_sgd(g, w, sr_seed=1, prepacked=(tgt[0], 0), **kw)
    with pytest.raises(RuntimeError, match="prepacked"):
        eng.C.submit(g, w, None, None, n, 1.0, prepacked=tgt[0], prepacked_elems=0, **sub)
    # raw codecs and bfp_trunc
    for codec in ("raw_f32", "raw_bf16", "bfp_trunc"):
        other = NativeAllReduce(None, codec=codec)
        with pytest.raises(ValueError, match="bfp_rne and bfp4_rne only"):
            other.allreduce_sgd(g, w, sr_seed=1, **kw)
        with pytest.raises(RuntimeError, match="bfp_rne and bfp4_rne only"):
            other.C.submit(g, w, None, None, n, 1.0, **sub)
    # the ring schedule
    ring = NativeAllReduce(None, codec="bfp_rne", algo="ring", comm=C.LoopbackFabric(2, 60.0).comm(0))
    gr, wr, _ = bufs(ring)
    with pytest.raises(ValueError, match="ring schedule"):
        ring.allreduce_sgd(gr, wr, sr_seed=1, **kw)
    with pytest.raises(RuntimeError, match="ring schedule"):
        ring.C.submit(gr, wr, None, None, n, 1.0, **sub)
    # chunked layouts: a bucket above chunk_elems, and an explicit layout=(shard, chunks)
    ch = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), chunk_elems=8192)
    assert ch.layout(n).chunks > 1
    gc, wc, _ = bufs(ch)
    with pytest.raises(ValueError, match="chunked"):
        ch.allreduce_sgd(gc, wc, sr_seed=1, **kw)
    with pytest.raises(RuntimeError, match="chunked"):
        ch.C.submit(gc, wc, None, None, n, 1.0, **sub)
    ex = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0))
    gx, wx, _ = bufs(ex, shard=8192, chunks=4)
    with pytest.raises(ValueError, match="chunked"):
        ex.allreduce_sgd(gx, wx, sr_seed=1, layout=(8192, 4), **kw)
    # the sharded update (request and trainer)
    sh = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), shard_update=True)
    gs, ws, _ = bufs(sh)
    with pytest.raises(ValueError, match="sharded"):
        sh.allreduce_sgd(gs, ws, ws.to(torch.bfloat16), sr_seed=1, **kw)
    with pytest.raises(RuntimeError, match="sharded"):
        sh.C.submit(gs, ws, ws.to(torch.bfloat16), None, n, 1.0, **sub)
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, pad_fn=lambda k, x=sh: x.layout(k).n_pad)
    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, sh, stochastic_rounding=True)
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, pad_fn=lambda k, x=ring: x.layout(k).n_pad)
    with pytest.raises(ValueError, match="ring"):
        DataParallelTrainer(model, ring, stochastic_rounding=True)
    # more ranks than the kernels' destination table holds
    wide = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(17, 60.0).comm(0))
    gw, ww, _ = bufs(wide)
    with pytest.raises(ValueError, match="at most 16 ranks"):
        wide.allreduce_sgd(gw, ww, sr_seed=1, **kw)
    with pytest.raises(RuntimeError, match="at most 16 ranks"):
        wide.C.submit(gw, ww, None, None, n, 1.0, **sub)
    # nothing ran, and an ordinary request with a seed still completes on the first engine
    assert not w.any()
    g.fill_(1.0)
    eng.allreduce_sgd(g, w, sr_seed=(1 << 64) - 1, **kw).synchronize(30)
    torch.cuda.synchronize()
    assert torch.all(w[:n] == -1.0), "1.0 is exactly representable: unchanged whatever the seed"
