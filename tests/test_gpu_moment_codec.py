"""AdamW's moments in 8-bit block floating point on the GPU (csrc/bfp/bfp_kernels.hip wire_adamw_q_kernel): the op
against the NumPy oracle bit for bit, the C++ engine's schedules against the reduced gradient + ``bfp_oracle.adamw_q``,
the refusals, and the trainer. The direct-P2P case runs in a child process (see test_gpu_shard_update.py).

The engine cases' reference starts from the reduced gradient of the schedule under test, taken from the same engine's
sum-only request on the same input (existing code with tests of its own), and every rank is compared with that one
reference, hence with every other rank. For the plain mesh schedules (inline, forced, loopback mesh, direct P2P) that
reduced gradient is also checked against ``sim.mesh_allreduce``; for the ring, the chunked mesh and the stochastically
rounded bfp4 wire it is the engine's output alone."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fpga_ai_nic_amd import _ext  # noqa: E402
from fpga_ai_nic_amd.models.mlp import MLP  # noqa: E402
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402
from fpga_ai_nic_amd.parallel import sim  # noqa: E402
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer  # noqa: E402
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce  # noqa: E402
from fpga_ai_nic_amd.utils import checkpoint  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 2048 * 4096 + 256  # tests/test_gpu_bfp4.py: above 2048 blocks * 256 lanes * 16 values, a lane takes a second trip
WIRE_CODECS = ["bfp_rne", "bfp_trunc", "bfp4_rne", "raw_f32", "raw_bf16"]
SENT = 0xA5


@pytest.fixture(scope="module")
def C():
    return _ext.require()


def _scalars(step, wd=0.01):
    return O.adamw_scalars(1e-2, wd, 0.9, 0.999, 1e-8, step)


def _guarded(data: np.ndarray, tail=64):
    """A device uint8 buffer holding ``data`` with sentinel bytes behind it; returns (whole buffer, view of data)."""
    buf = torch.full((data.size + tail,), SENT, dtype=torch.uint8, device=DEV)
    buf[: data.size] = torch.from_numpy(np.ascontiguousarray(data).view(np.uint8)).to(DEV)
    return buf, buf[: data.size]


def _reference(dec, w0, mq, vq, n_s, n_shards, s, seed, gs, n_valid, skip, elem_base):
    """The oracle over the op's traversal: every shard but the skipped ones, cut at n_valid."""
    w = w0.copy()
    period = skip[1] if skip[1] >= 1 else 1 << 30
    for sh in range(n_shards):
        if skip[0] >= 0 and sh % period == skip[0]:
            continue
        lo, hi = sh * n_s, min((sh + 1) * n_s, n_valid)
        if hi <= lo:
            continue
        top = lo + -(-(hi - lo) // 16) * 16
        w2, mq, vq = O.adamw_q(w[lo:top], dec[lo:top], mq, vq, s, gs, seed, hi - lo, elem_base + lo)
        w[lo:hi] = w2[: hi - lo]
    return w, mq, vq


def _run_case(n_s, n_shards, codec, *, n_valid=None, skip=(-1, 0), stride_pad=0, elem_base=0, extra=0, clip=None,
              lp=True, steps=1, seed0=5):
    n = n_s * n_shards
    n_valid = n if n_valid is None else n_valid
    n_pad = elem_base + n + extra
    rng = np.random.default_rng(n_s + 7 * n_shards)
    w0 = rng.standard_normal(n).astype(np.float32)
    nb = O.moment_plane_bytes(n_pad)
    # planes that already hold state outside the region (everything outside must stay untouched)
    mq = O.pack((rng.standard_normal(n_pad) * 0.1).astype(np.float32), n_pad, "bfp_rne")
    vq = O.pack(np.abs(rng.standard_normal(n_pad) * 0.1).astype(np.float32), n_pad, "bfp_rne")
    assert mq.size == nb
    sb = O.shard_bytes(codec, n_s)
    stride = sb + stride_pad if stride_pad else 0
    pm_all, pm = _guarded(mq)
    pv_all, pv = _guarded(vq)
    master = torch.from_numpy(w0).to(DEV)
    lp_t = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if lp else None
    words = None if clip is None else torch.tensor([clip, 5.0, 1.0, 0.0], device=DEV)
    w_ref = w0
    for k in range(1, steps + 1):
        g = (rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32)
        packed = O.pack(g, n_s, codec)
        dec = O.unpack(packed, n, n_s, codec)
        if stride:
            laid = np.full(stride * (n_shards - 1) + sb, SENT, np.uint8)
            for sh in range(n_shards):
                laid[sh * stride: sh * stride + sb] = packed[sh * sb:(sh + 1) * sb]
        else:
            laid = packed
        w_all, w_t = _guarded(laid)
        s, seed = _scalars(k), O.sr_step_seed(seed0, k, 0)
        gs = 0.5
        kw = dict(codec=codec, mom_q=pm, var_q=pv, scalars=s, seed=seed, lp=lp_t, grad_scale=gs, n_valid=n_valid,
                  skip_shard=skip[0], skip_period=skip[1], shard_stride=stride, clip=words, elem_base=elem_base)
        wire.adamw_q(w_t, n_s, n_shards, master, **kw)
        torch.cuda.synchronize()
        gs_ref = gs if clip is None else O.clip_scale(gs, np.array([clip, 5.0, 1.0, 0.0], np.float32))
        w_ref, mq, vq = _reference(dec, w_ref, mq, vq, n_s, n_shards, s, seed, gs_ref, n_valid, skip, elem_base)
        tag = (n_s, n_shards, codec, k)
        assert np.array_equal(master.cpu().numpy(), w_ref), tag
        assert np.array_equal(pm.cpu().numpy(), mq), tag
        assert np.array_equal(pv.cpu().numpy(), vq), tag
        assert (pm_all[nb:] == SENT).all() and (pv_all[nb:] == SENT).all() and (w_all[laid.size:] == SENT).all(), tag
        assert np.array_equal(w_all[: laid.size].cpu().numpy(), laid), "the wire is read-only"
    if lp:
        period = skip[1] if skip[1] >= 1 else 1 << 30
        e = np.arange(n)
        touched = (e < n_valid) & ~((skip[0] >= 0) & ((e // n_s) % period == skip[0]))
        want = np.where(touched, O.bf16_bits_to_f32(O.f32_to_bf16_bits(w_ref)), 0).astype(np.float32)
        assert np.array_equal(lp_t.float().cpu().numpy(), want)
    return master.cpu().numpy(), pm.cpu().numpy(), pv.cpu().numpy()


@pytest.mark.parametrize("codec", WIRE_CODECS)
@pytest.mark.parametrize("shape", [(256, 1), (4352, 1), (1024, 3)], ids=["16lanes", "2blocks", "3shards"])
def test_op_matches_oracle(shape, codec):
    """w, lp and both planes bit for bit over three consecutive steps (stored state is read back), sentinels behind the
    planes and the wire."""
    _run_case(*shape, codec, steps=3)


@pytest.mark.parametrize("codec", WIRE_CODECS)
def test_op_n_valid_tails(codec):
    n_s = 1024
    for nv in (3 * n_s, n_s + 512, n_s + 512 - 5, 700, 0):  # whole; a group boundary in shard 1; 5 short; shard 0; 0
        _run_case(n_s, 3, codec, n_valid=nv, steps=2)


@pytest.mark.parametrize("codec", WIRE_CODECS)
def test_op_skip_stride_base_clip(codec):
    _run_case(1024, 3, codec, skip=(1, 2), steps=2)
    _run_case(1024, 3, codec, stride_pad=4096, n_valid=3 * 1024 - 21)
    _run_case(1024, 2, codec, elem_base=512, extra=768, n_valid=2048 - 37, steps=2)
    for coef in (1.0, 0.37):
        _run_case(256, 2, codec, clip=coef, lp=coef == 1.0)
    _run_case(1024, 3, codec, skip=(0, 2), stride_pad=256, elem_base=512, extra=256, clip=0.37, n_valid=3000, lp=False)


def test_op_clip_of_one_is_the_unclipped_update():
    a = _run_case(1024, 2, "bfp_rne", clip=1.0)
    b = _run_case(1024, 2, "bfp_rne")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_op_big_lanes_take_a_second_trip():
    """One step at BIG elements: the last 256 elements belong to the lanes' second trip."""
    n = BIG
    rng = np.random.default_rng(6)
    g = rng.standard_normal(n).astype(np.float32)
    w0 = rng.standard_normal(n).astype(np.float32)
    nv = n - 16 - 5
    packed = O.pack(g, n, "bfp_rne")
    dec = O.unpack(packed, n, n, "bfp_rne")
    z = np.zeros(O.moment_plane_bytes(n), np.uint8)
    pm_all, pm = _guarded(z)
    pv_all, pv = _guarded(z)
    w_all, w_t = _guarded(packed)
    master = torch.from_numpy(w0).to(DEV)
    lp = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    s = _scalars(1)
    wire.adamw_q(w_t, n, 1, master, codec="bfp_rne", mom_q=pm, var_q=pv, scalars=s, seed=77, lp=lp, n_valid=nv)
    torch.cuda.synchronize()
    w, mq, vq = O.adamw_q(w0, dec, z, z, s, 1.0, 77, nv)
    got = master.cpu().numpy()
    assert np.array_equal(got, w) and not np.array_equal(got[-256:nv - n], w0[-256:nv - n])
    assert np.array_equal(pm.cpu().numpy(), mq) and np.array_equal(pv.cpu().numpy(), vq)
    assert (pm_all[z.size:] == SENT).all() and (pv_all[z.size:] == SENT).all() and (w_all[packed.size:] == SENT).all()
    assert np.array_equal(w_all[: packed.size].cpu().numpy(), packed), "the wire is read-only"
    want = O.bf16_bits_to_f32(O.f32_to_bf16_bits(w))
    want[nv:] = 0
    assert np.array_equal(lp.float().cpu().numpy(), want)


def test_op_bits_do_not_depend_on_the_grid(C):
    """One block (every lane takes several trips per shard) against the default grid."""
    saved = C.moment_grid_cap()
    try:
        C.set_moment_grid_cap(1)
        assert C.moment_grid_cap() == 1
        a = _run_case(4352, 3, "bfp_rne", n_valid=3 * 4352 - 21, steps=2)
    finally:
        C.set_moment_grid_cap(0)
    assert C.moment_grid_cap() == saved == 0
    b = _run_case(4352, 3, "bfp_rne", n_valid=3 * 4352 - 21, steps=2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_moment_plane_and_decode_on_the_gpu():
    x = (np.random.default_rng(1).standard_normal(768) * 3).astype(np.float32)
    plane = torch.from_numpy(O.pack(x, 768, "bfp_rne")).to(DEV)
    assert np.array_equal(wire.moment_decode(plane).cpu().numpy(), O.moment_decode(plane.cpu().numpy()))
    z = wire.moment_plane(768, DEV)
    assert z.is_cuda and z.dtype == torch.uint8 and z.numel() == 816 and not z.any()


# --------------------------------------------------------------------------- C++ engine
N_ELEMS, STEPS, BASE = 50000 - 48, 3, 41


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


def _grads(N, seed):
    rng = np.random.default_rng(seed)
    return [[(rng.standard_normal(N_ELEMS) * np.exp(rng.standard_normal(N_ELEMS)) * (1 + r)).astype(np.float32)
             for r in range(N)] for _ in range(STEPS)]


def _w0():
    return np.random.default_rng(9).standard_normal(N_ELEMS).astype(np.float32)


def _engine_steps(eng, r, N, grads, *, immediate=False, sr=False, bucket=0):
    """STEPS AdamW steps with the 8-bit state on rank r; per step also the sum-only request of the same input (the
    schedule's reduced gradient). Returns per step (reduced gradient, weights, lp, planes) and the layout."""
    torch.cuda.set_device(0)
    L = eng.layout(N_ELEMS)
    w = torch.zeros(L.n_pad, device=DEV)
    w[:N_ELEMS] = torch.from_numpy(_w0())
    lp = w.to(torch.bfloat16)
    pm, pv = wire.moment_plane(L.n_pad, DEV), wire.moment_plane(L.n_pad, DEV)
    res = []
    for k in range(1, STEPS + 1):
        g = torch.zeros(L.n_pad, device=DEV)
        g[:N_ELEMS] = torch.from_numpy(grads[k - 1][r])
        out = torch.zeros(L.n_pad, device=DEV)
        # (this rank's stream only: a device-wide wait would also wait for a peer's stream, which on the direct-P2P
        # transport may itself be waiting for this rank's next request)
        torch.cuda.current_stream().synchronize()
        srk = dict(sr_seed=O.sr_step_seed(BASE + 1, k, bucket)) if sr else {}
        eng.allreduce(g, out, n_valid=N_ELEMS, **srk).synchronize(60)
        h = eng.allreduce_sgd(g, w, lp, pm, n_valid=N_ELEMS, lr=1e-2, weight_decay=0.01, grad_scale=1.0 / N,
                              opt="adamw", var=pv, step=k, moment_codec="bfp8",
                              moment_seed=O.sr_step_seed(BASE, k, bucket), defer=not immediate, **srk)
        if not immediate:
            h.commit_after_current()
        h.synchronize(60)
        torch.cuda.current_stream().synchronize()
        res.append(tuple(x.cpu().numpy().copy() for x in (out, w, lp.float(), pm, pv)))
    return res, (L.shard, L.n_pad)


def _check_engine(res, N, bucket=0, sim_grads=None, codec="bfp_rne"):
    """Every rank's weights and planes equal adamw_q applied to the reduced gradient; replicas identical."""
    why = []
    shard, n_pad = res[0][1]
    w = np.zeros(n_pad, np.float32)
    w[:N_ELEMS] = _w0()
    mq, vq = (np.zeros(O.moment_plane_bytes(n_pad), np.uint8) for _ in range(2))
    for k in range(1, STEPS + 1):
        total = res[0][0][k - 1][0]
        if sim_grads is not None:
            ref = sim.mesh_allreduce([np.pad(g, (0, n_pad - N_ELEMS)) for g in sim_grads[k - 1]], shard, codec)
            if not np.array_equal(total, ref):
                why.append(f"step {k}: the reduced gradient differs from the simulator's")
        w, mq, vq = O.adamw_q(w, total, mq, vq, _scalars(k), 1.0 / N, O.sr_step_seed(BASE, k, bucket), n_valid=N_ELEMS)
        for r in range(N):
            out, wg, lpg, pmg, pvg = res[r][0][k - 1]
            for name, a, b in (("reduced gradient", out, total), ("weights", wg, w), ("first-moment plane", pmg, mq),
                               ("second-moment plane", pvg, vq),
                               ("bf16 copy", lpg[:N_ELEMS], O.bf16_bits_to_f32(O.f32_to_bf16_bits(w[:N_ELEMS])))):
                if not np.array_equal(a, b):
                    why.append(f"step {k} rank {r}: {name} differs")
    return why


def _fabric_case(C, N, **kw):
    grads = _grads(N, 200 + N)
    fabric = C.LoopbackFabric(N, 60.0)
    codec = kw.pop("codec", "bfp_rne")
    sr = kw.pop("sr", False)
    engs = [NativeAllReduce(None, codec=codec, comm=fabric.comm(r), **kw) for r in range(N)]
    res = _threads(N, lambda r: _engine_steps(engs[r], r, N, grads, sr=sr))
    plain_mesh = kw.get("algo", "mesh") == "mesh" and "chunk_elems" not in kw and not sr
    assert not _check_engine(res, N, sim_grads=grads if plain_mesh else None, codec=codec)


def test_engine_inline_world_1():
    grads = _grads(1, 11)
    res = [_engine_steps(NativeAllReduce(None, codec="bfp_rne"), 0, 1, grads)]
    assert not _check_engine(res, 1, sim_grads=grads)


def test_engine_forced_one_rank(C):
    _fabric_case(C, 1, force_comm=True)


@pytest.mark.parametrize("N", [2, 3])
def test_engine_loopback_mesh(C, N):
    _fabric_case(C, N)


def test_engine_loopback_ring(C):
    _fabric_case(C, 3, algo="ring")


def test_engine_chunked_mesh(C):
    _fabric_case(C, 2, chunk_elems=8192)


def test_engine_bfp4_wire_with_sr_seed(C):
    _fabric_case(C, 2, codec="bfp4_rne", sr=True)


def test_engine_clip_group_of_two(C):
    """Two deferred requests of one clip group equal the same updates with the premultiplied grad_scale."""
    N = 2
    grads = _grads(N, 77)

    def run(eng, r, clip):
        torch.cuda.set_device(0)
        L = eng.layout(N_ELEMS)
        words = torch.full((4,), float("nan"), device=DEV)
        planes, hs = [], []
        for b in range(2):
            w = torch.zeros(L.n_pad, device=DEV)
            w[:N_ELEMS] = torch.from_numpy(_w0() * (b + 1))
            pm, pv = wire.moment_plane(L.n_pad, DEV), wire.moment_plane(L.n_pad, DEV)
            g = torch.zeros(L.n_pad, device=DEV)
            g[:N_ELEMS] = torch.from_numpy(grads[b][r])
            torch.cuda.synchronize()
            kw = dict(clip=words) if clip is True else {}
            h = eng.allreduce_sgd(g, w, None, pm, n_valid=N_ELEMS, lr=1e-2, grad_scale=0.5 if clip is True else clip,
                                  opt="adamw", var=pv, step=1, moment_codec="bfp8",
                                  moment_seed=O.sr_step_seed(BASE, 1, b), defer=True, **kw)
            planes.append((w, pm, pv))
            hs.append(h)
        if clip is True:
            eng.commit_group(hs, max_norm=0.5, grad_scale=0.5)
        else:
            for h in hs:
                h.commit_after_current()
        for h in hs:
            h.synchronize(60)
        torch.cuda.synchronize()
        return [tuple(x.cpu().numpy().copy() for x in p) for p in planes], words.cpu().numpy()

    def arm(clip):
        fabric = C.LoopbackFabric(N, 60.0)
        engs = [NativeAllReduce(None, codec="bfp_rne", comm=fabric.comm(r)) for r in range(N)]
        return _threads(N, lambda r: run(engs[r], r, clip))

    clipped = arm(True)
    words = clipped[0][1]
    assert 0 < words[0] < 1
    plain = arm(O.clip_scale(0.5, words))
    for r in range(N):
        for b in range(2):
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], plain[r][0][b])), (r, b)
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], clipped[0][0][b])), (r, b)
            assert clipped[r][0][b][1].any()


def _p2p_case(world=2):
    """Direct-P2P mesh, immediate requests (the update reads the receive arena strided), virtual ranks on one GPU."""
    C = _ext.require()
    grads = _grads(world, 300)
    cs = [C.P2PComm(r, world, 0, 2 << 20, 2) for r in range(world)]
    C.P2PComm.connect_local(cs)
    engs = [NativeAllReduce(None, codec="bfp_rne", algo="mesh", comm=cs[r]) for r in range(world)]
    out, errs = [None] * world, []

    def run(r):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                out[r] = _engine_steps(engs[r], r, world, grads, immediate=True)
        except Exception as e:  # noqa: BLE001
            errs.append(f"rank {r}: {e!r}")

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    why = list(errs)
    if any(t.is_alive() for t in ts):
        why.append("virtual rank thread hung")
    if not why:
        why = _check_engine(out, world, sim_grads=grads)
    return {"ok": not why, "why": why}


def test_engine_direct_p2p_immediate():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="32")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "2"], env=env, capture_output=True, text=True,
                           timeout=150)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"direct P2P child timed out\n{(e.stderr or '')[-3000:]}")
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(recs) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert recs[0]["ok"], recs[0]["why"]


# --------------------------------------------------------------------------- refusals
def test_refusals_wrapper_and_submit(C):
    eng = NativeAllReduce(None, codec="bfp_rne")
    n = 1000
    L = eng.layout(n)
    nb = O.moment_plane_bytes(L.n_pad)
    g, w = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    pm, pv = wire.moment_plane(L.n_pad, DEV), wire.moment_plane(L.n_pad, DEV)
    f32 = torch.zeros(L.n_pad, device=DEV)
    ok = dict(n_valid=n, lr=1e-2, opt="adamw", var=pv, step=1, moment_codec="bfp8", moment_seed=0)

    def call(mom=pm, **kw):
        return eng.allreduce_sgd(g, w, None, mom, **{**ok, **kw})

    call().synchronize(60)
    for kw, match in ((dict(opt="sgd", var=None, step=None), "AdamW only"), (dict(trust_ratio=True), "trust_ratio"),
                      (dict(moment_codec="bfp4"), "one of"), (dict(moment_seed=None), "needs moment_seed"),
                      (dict(moment_seed=-1), r"\[0, 2\^64\)"), (dict(moment_seed=1 << 64), r"\[0, 2\^64\)"),
                      (dict(var=f32), "uint8"), (dict(var=pv.cpu()), "lives on"),
                      (dict(var=torch.zeros(2 * nb, dtype=torch.uint8, device=DEV)[::2]), "contiguous"),
                      (dict(var=torch.zeros(nb + 272, dtype=torch.uint8, device=DEV)), "not exactly"),
                      (dict(var=torch.zeros(nb - 272, dtype=torch.uint8, device=DEV)), "not exactly")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(ValueError, match="uint8"):
        call(mom=f32)
    off8 = torch.zeros(nb + 16, dtype=torch.uint8, device=DEV)[8: nb + 8]  # contiguous, but not 16-byte aligned
    with pytest.raises(ValueError, match="16-byte aligned"):
        call(var=off8)
    fab = C.LoopbackFabric(2, 60.0)
    sh = NativeAllReduce(None, codec="bfp_rne", comm=fab.comm(0), shard_update=True)
    with pytest.raises(ValueError, match="sharded-update"):
        sh.allreduce_sgd(g, w, w.to(torch.bfloat16), pm, **ok)
    # C.submit itself
    a = _scalars(1).kernel_args()
    base = (g, w, None, None, n, 1e-2, 1.0, 0.0, 0.0, False, True, True, None, None, 0, 0, 0, False)

    def submit(e=eng, **kw):
        return e.C.submit(*base, **{**dict(opt=1, adamw=a, mom_q=pm, var_q=pv, moment_seed=3), **kw})

    slot = submit()
    eng.C.commit(slot)
    eng.C.synchronize(slot, 60.0)
    for kw, match in ((dict(opt=0), "AdamW only"), (dict(lamb=O.lamb_scalars(1e-2, 0, 0.9, 0.999, 1e-8, 1).kernel_args()),
                                                    "trust ratio"),
                      (dict(var_q=None), "both moment planes"), (dict(var=f32), "not in f32 planes"),
                      (dict(var_q=torch.zeros(nb + 272, dtype=torch.uint8, device=DEV)), "exactly n_pad"),
                      (dict(var_q=torch.zeros(nb, dtype=torch.int8, device=DEV)), "uint8"),
                      (dict(mom_q=pm.cpu()), "uint8 tensor"), (dict(var_q=off8), "16-byte aligned"),
                      (dict(mom_q=torch.zeros(2 * nb, dtype=torch.uint8, device=DEV)[::2]), "contiguous")):
        with pytest.raises(RuntimeError, match=match):
            submit(**kw)
    with pytest.raises((RuntimeError, TypeError, OverflowError)):
        submit(moment_seed=-1)
    with pytest.raises((RuntimeError, TypeError, OverflowError)):
        submit(moment_seed=1 << 64)
    with pytest.raises(RuntimeError, match="sharded update"):
        sh.C.submit(g, w, w.to(torch.bfloat16), None, n, 1e-2, 1.0, 0.0, 0.0, False, True, True, None, None, 0, 0, 0,
                    False, opt=1, adamw=a, mom_q=pm, var_q=pv, moment_seed=3)
    # the op's binding
    buf = torch.zeros(O.shard_bytes("bfp_rne", L.n_pad), dtype=torch.uint8, device=DEV)
    args = lambda **kw: {**dict(codec="bfp_rne", mom_q=pm, var_q=pv, scalars=_scalars(1), seed=0), **kw}  # noqa: E731
    with pytest.raises(ValueError, match="elem_base"):
        wire.adamw_q(buf, L.n_pad, 1, w, **args(elem_base=128))
    with pytest.raises(ValueError, match="uint8"):
        wire.adamw_q(buf, L.n_pad, 1, w, **args(var_q=f32))
    with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
        wire.adamw_q(buf, L.n_pad, 1, w, **args(seed=1 << 64))
    with pytest.raises(RuntimeError, match="elem_base"):
        C.wire_adamw_q(buf, L.n_pad, 1, -1, 0, w, None, pm, pv, a, 1.0, 0.0, 0, n, 1, 0, None, 128)
    with pytest.raises(RuntimeError, match="moment planes"):
        C.wire_adamw_q(buf, L.n_pad, 1, -1, 0, w, None, f32, pv, a, 1.0, 0.0, 0, n, 1, 0, None, 0)


# --------------------------------------------------------------------------- trainer
def _data(sizes, mb=32):
    g = torch.Generator().manual_seed(5)
    return ((torch.rand(mb, sizes[0], generator=g) * 2 - 1).to(DEV, torch.bfloat16),
            torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32).to(DEV))


def _trainer(engine, model=None, opt_step=0):
    sizes = [64, 128, 64]
    eng = NativeAllReduce(None, codec="raw_f32") if engine else None
    pad = (lambda n: eng.layout(n).n_pad) if eng is not None else None
    model = model or MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, adam=True, moment_codec="bfp8", pad_fn=pad)
    tr = DataParallelTrainer(model, eng, lr=0.01, weight_decay=0.01, optimizer="adamw", moment_codec="bfp8", sr_seed=9)
    tr.opt_step = opt_step
    return model, tr


def _state(model):
    torch.cuda.synchronize()
    return [tuple(t.cpu().numpy().copy() for t in (l.master, l.lp.float(), l.mom, l.var)) for l in model.layers]


def test_trainer_engine_equals_engine_less_and_resume(tmp_path):
    """3 steps through the native engine (raw_f32 wire: the engine-less update reads the f32 gradient itself) equal the
    engine-less trainer's; a step resumed from a checkpoint is bit-identical to the uninterrupted run's."""
    x, y = _data([64, 128, 64])
    me, te = _trainer(True)
    ml, tl = _trainer(False)
    ck = str(tmp_path / "ck")
    for k in range(3):
        for tr in (te, tl):
            tr.step(x, y)
            tr.finish()
        a, b = _state(me), _state(ml)
        assert all(np.array_equal(p, q) for s, t in zip(a, b) for p, q in zip(s, t)), k
        if k == 1:
            checkpoint.save(ck, ml, optimizer="adamw", opt_step=tl.opt_step)
    assert all(l.mom.dtype == torch.uint8 and l.mom.any() and l.var.any() for l in me.layers)
    fresh = MLP([64, 128, 64], dtype=torch.bfloat16, device=DEV, seed=4, adam=True, moment_codec="bfp8")
    info = checkpoint.load(ck, fresh)
    assert info["moment_codec"] == "bfp8" and info["opt_step"] == 2
    _, tr = _trainer(False, model=fresh, opt_step=info["opt_step"])
    tr.step(x, y)
    tr.finish()
    assert all(np.array_equal(p, q) for s, t in zip(_state(fresh), _state(ml)) for p, q in zip(s, t))


if __name__ == "__main__":
    print(json.dumps(_p2p_case(int(sys.argv[1]))), flush=True)
