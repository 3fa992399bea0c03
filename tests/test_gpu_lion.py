"""Lion in the all-reduce epilogues on the GPU: the decode + Lion kernel against the oracle, the native engine over
virtual ranks (LoopbackFabric) against the Python engine, and the trainer at world 1.

Bounds against the oracle (bfp_oracle.lion, each fma emulated in float64 and rounded):
  * m' within 1 ulp — the emulated fma's rare double rounding, as test_gpu_adamw.py allows;
  * w' within 1 ulp for the same reason. A wrong sign decision would put w' 2 * lr away, about 10^4 ulp at lr = 1e-3 on
    weights of order 1, so this bound pins every sign as well.
Everything that compares two runs of the kernels (grids, clip words, engines, trainers) compares bits.
"""
import hashlib
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
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce  # noqa: E402
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer  # noqa: E402
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce  # noqa: E402
from fpga_ai_nic_amd.parallel.transport import ThreadFabric  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, WD, B1, B2 = 1e-3, 1e-2, 0.9, 0.99
CODECS = ["bfp_trunc", "bfp_rne", "bfp4_rne", "raw_f32", "raw_bf16"]
# 32 elements with m = g = 0 in a shard that is not skipped: two whole groups, as the reference's truncating decoder
# (bfp_trunc) returns 2^-23 of the group's scale, not 0, for a zero beside non-zero values
ZEROS = slice(2048 + 32, 2048 + 64)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _inputs(n_s, N):
    n = n_s * N
    rng = np.random.default_rng(2)
    g = rng.standard_normal(n).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    g[ZEROS] = 0
    m[ZEROS] = 0
    return g, w, m


def _launch(codec, has_lp, strided, n_s=1024, N=4, grad_scale=0.25, clip=None, skip=True):
    """One wire.lion launch on the kernel test's inputs; (w', m', lp') as numpy (lp' as f32), and the inputs."""
    n, n_valid = n_s * N, n_s * N - 77
    g, w, m = _inputs(n_s, N)
    buf = O.pack(g, n_s, codec)
    sb = O.shard_bytes(codec, n_s)
    stride = sb + 256 if strided else 0
    if stride:
        spread = np.zeros(stride * N, np.uint8)
        for q in range(N):
            spread[q * stride: q * stride + sb] = buf[q * sb:(q + 1) * sb]
        wbuf = torch.from_numpy(spread).to(DEV)
    else:
        wbuf = torch.from_numpy(buf).to(DEV)
    wt, mt = (torch.from_numpy(x.copy()).to(DEV) for x in (w, m))
    lp = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV) if has_lp else None
    words = None if clip is None else torch.tensor([clip, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    wire.lion(wbuf, n_s, N, wt, codec=codec, mom=mt, scalars=O.lion_scalars(LR, WD, B1, B2), lp=lp,
              grad_scale=grad_scale, n_valid=n_valid, skip_shard=1 if skip else -1, skip_period=N if skip else 0,
              shard_stride=stride, clip=words)
    torch.cuda.synchronize()
    got = (wt.cpu().numpy(), mt.cpu().numpy(), None if lp is None else lp.float().cpu().numpy())
    return got, (g, w, m, buf, n, n_valid)


# the strided wire in half the cases: every codec takes it with or without lp
CASES = [(c, lp, (i + int(lp)) % 2 == 1) for i, c in enumerate(CODECS) for lp in (True, False)]


@pytest.mark.parametrize("codec,has_lp,strided", CASES)
@pytest.mark.parametrize("n_s", [1024, 8192])  # one block; four blocks, each lane one trip per shard
def test_lion_epilogue(codec, has_lp, strided, n_s):
    N = 4
    (gw, gm, glp), (g, w, m, buf, n, n_valid) = _launch(codec, has_lp, strided, n_s=n_s)
    s = O.lion_scalars(LR, WD, B1, B2)
    gd = O.unpack(buf, n, n_s, codec)
    assert np.all(gd[ZEROS] == 0)
    rw, rm = O.lion(w, gd, m, s, 0.25)
    keep = np.zeros(n, bool)
    keep[n_valid:] = True
    keep[n_s:2 * n_s] = True
    for a, old, name in ((gw, w, "w"), (gm, m, "m")):
        assert np.array_equal(a[n_valid:], old[n_valid:]), f"{name}: padding must not be touched"
        assert np.array_equal(a[n_s:2 * n_s], old[n_s:2 * n_s]), f"{name}: skipped shard must not be touched"
    uw, um = _ulps(gw[~keep], rw[~keep]), _ulps(gm[~keep], rm[~keep])
    print(f"{codec} lp={has_lp} strided={strided} n_s={n_s}: w' max {uw.max()} ulp ({(uw > 0).sum()} off), "
          f"m' max {um.max()} ulp ({(um > 0).sum()} off)")
    assert um.max() <= 1
    assert uw.max() <= 1
    assert not np.array_equal(gw[~keep], w[~keep])
    # c == 0: the weight stays on w * decay exactly, the moment on 0
    assert np.array_equal(gw[ZEROS], (w[ZEROS] * s.decay).astype(np.float32)) and np.all(gm[ZEROS] == 0)
    if has_lp:
        assert np.all(glp[keep] == 3.0), "lp: padding / skipped shard must not be touched"
        assert np.array_equal(glp[~keep], O.bf16_bits_to_f32(O.f32_to_bf16_bits(gw))[~keep])


def _digests():
    """sha256 of (w', m', lp') of every kernel case at both shard sizes, in a fixed order."""
    out = {}
    for n_s in (1024, 8192):
        for codec, has_lp, strided in CASES:
            got, _ = _launch(codec, has_lp, strided, n_s=n_s)
            h = hashlib.sha256()
            for a in got:
                if a is not None:
                    h.update(np.ascontiguousarray(a).tobytes())
            out[f"{codec}-{int(has_lp)}-{int(strided)}-{n_s}"] = h.hexdigest()
    return out


def test_bits_do_not_depend_on_the_grid():
    """The same launches under FAN_WIRE_MAX_BLOCKS=1 (read once per process: a child): at n_s = 8192 the default grid
    has four blocks, the capped one a single block whose lanes take four trips per shard."""
    env = dict(os.environ, FAN_WIRE_MAX_BLOCKS="1")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "digests"], env=env, capture_output=True,
                           text=True, timeout=150)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"one-block child timed out\n{(e.stderr or '')[-3000:]}")
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(recs) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert recs[0] == _digests()


@pytest.mark.parametrize("codec", ["bfp_rne", "bfp4_rne", "raw_f32"])
@pytest.mark.parametrize("has_lp", [True, False])
def test_clip_words_are_one_product(codec, has_lp):
    s = 0.25
    words = np.array([0.37, 0, 0, 0], np.float32)
    a, _ = _launch(codec, has_lp, False, clip=0.37, grad_scale=s)
    b, _ = _launch(codec, has_lp, False, grad_scale=O.clip_scale(s, words))
    plain, _ = _launch(codec, has_lp, False, grad_scale=s)
    one, _ = _launch(codec, has_lp, False, clip=1.0, grad_scale=s)
    for x, y, p, o in zip(a, b, plain, one):
        if x is not None:
            assert np.array_equal(x, y), "clip words differ from the premultiplied grad_scale"
            assert np.array_equal(o, p), "a coefficient of 1 must leave the unclipped update"
    assert not np.array_equal(a[1], plain[1])


# --------------------------------------------------------------------------- engines
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


def _two_steps(eng, L, n, N, w0, grads, r, extra=None, layout=None):
    """Two Lion requests on rank r's engine; the planes (numpy) and the bf16 copy after each. ``extra(step)``: further
    request arguments (residual=, sr_seed=)."""
    w = torch.zeros(L.n_pad, device=DEV)
    w[:n] = torch.from_numpy(w0)
    lp = torch.zeros(L.n_pad, device=DEV, dtype=torch.bfloat16)
    m = torch.zeros(L.n_pad, device=DEV)
    state = {}
    snaps = []
    for step in (1, 2):
        g = torch.zeros(L.n_pad, device=DEV)
        g[:n] = torch.from_numpy(grads[step - 1][r])
        torch.cuda.synchronize()
        kw = {} if extra is None else extra(step, L, state)
        h = eng.allreduce_sgd(g, w, lp, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N, opt="lion",
                              betas=(B1, B2), defer=True, **kw)
        h.commit_after_current()
        h.synchronize(60)
        torch.cuda.synchronize()
        snaps.append((w.cpu().numpy(), m.cpu().numpy(), lp.cpu()))
    return snaps


def _same(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa[:2], sb[:2])) and \
        all(torch.equal(sa[2], sb[2]) for sa, sb in zip(a, b))


def _check_against_oracle(snaps, L, n, N, w0, grads, algo, orders, what):
    prev = (w0, np.zeros(n, np.float32))
    s = O.lion_scalars(LR, WD, B1, B2)
    for step in (1, 2):
        gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step - 1]]
        red = sim.mesh_allreduce(gin, L.shard, "bfp_rne") if algo == "mesh" else \
            sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, "bfp_rne")[0]
        rw, rm = O.lion(prev[0], red[:n], prev[1], s, 1.0 / N)
        gw, gm = (a[:n] for a in snaps[step - 1][:2])
        print(f"{what} step {step}: w' max {_ulps(gw, rw).max()} ulp, m' max {_ulps(gm, rm).max()} ulp")
        assert _ulps(gw, rw).max() <= 1 and _ulps(gm, rm).max() <= 1
        for a in snaps[step - 1][:2]:
            assert np.all(a[n:] == 0), "padding untouched"
        assert torch.equal(snaps[step - 1][2][:n], torch.from_numpy(gw).to(torch.bfloat16))
        prev = (gw, gm)


def _py_arm(N, n, w0, grads, L, extra=None, **ekw):
    pys = [None] * N

    def py_rank(t):
        torch.cuda.set_device(0)
        eng = CompressedAllReduce(t, device=DEV, **ekw)
        Lp = eng.layout(n)
        assert (Lp.n_pad, Lp.shard, Lp.slice_elems, Lp.blocks) == (L.n_pad, L.shard, L.slice_elems, L.blocks)
        pys[t.rank] = _two_steps(eng, Lp, n, N, w0, grads, t.rank, extra)

    ThreadFabric(N, timeout_s=60).run(py_rank)
    return pys


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
def test_native_engine_loopback_lion(N, algo):
    C = _ext.require()
    n = 50000 - 48
    rng = np.random.default_rng(N * 100 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    ekw = dict(codec="bfp_rne", algo=algo, max_slice_elems=8192)
    engines = [NativeAllReduce(None, comm=fabric.comm(r), **ekw) for r in range(N)]
    L = engines[0].layout(n)
    res = _threads(N, lambda r: _two_steps(engines[r], L, n, N, w0, grads, r))
    for r in range(1, N):
        assert _same(res[r], res[0]), "replicas must be bit-identical"
    pys = _py_arm(N, n, w0, grads, L, **ekw)
    for r in range(N):
        assert _same(pys[r], res[r]), "native engine differs from the Python engine"
    assert np.any(res[0][1][1][:n] != 0)
    _check_against_oracle(res[0], L, n, N, w0, grads, algo, engines[0].orders, f"N={N} {algo}")


def test_inline_world1_engine_lion():
    n = 50000 - 48
    rng = np.random.default_rng(23)
    grads = [[rng.standard_normal(n).astype(np.float32)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    eng = NativeAllReduce(None, codec="bfp_rne")
    assert eng.inline
    L = eng.layout(n)
    got = _two_steps(eng, L, n, 1, w0, grads, 0)
    py = CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", device=DEV)
    assert py.layout(n).n_pad == L.n_pad
    assert _same(_two_steps(py, L, n, 1, w0, grads, 0), got)
    _check_against_oracle(got, L, n, 1, w0, grads, "mesh", None, "inline world 1")


def test_chunked_mesh_lion():
    """A bucket above chunk_elems: every chunk's epilogue offsets both planes (immediate: per-chunk epilogues in the
    pipeline; deferred: one epilogue over the whole gathered wire)."""
    C = _ext.require()
    N, n, chunk = 2, 50000 - 48, 8192
    rng = np.random.default_rng(41)
    grads = [rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)]
    w0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    s = O.lion_scalars(LR, WD, B1, B2)
    fabric = C.LoopbackFabric(N, 60.0)
    engines = [NativeAllReduce(None, codec="bfp_rne", comm=fabric.comm(r), chunk_elems=chunk) for r in range(N)]
    L = engines[0].layout(n)
    assert L.chunks > 1

    def fn(r):
        out = []
        g = torch.zeros(L.n_pad, device=DEV)
        g[:n] = torch.from_numpy(grads[r])
        for defer in (False, True):
            planes = []
            for x in (w0, m0):
                t = torch.zeros(L.n_pad, device=DEV)
                t[:n] = torch.from_numpy(x)
                planes.append(t)
            w, m = planes
            torch.cuda.synchronize()
            h = engines[r].allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N,
                                         opt="lion", betas=(B1, B2), defer=defer)
            if defer:
                h.commit_after_current()
            h.synchronize(60)
            torch.cuda.synchronize()
            out.append([t.cpu().numpy() for t in planes])
        return out

    res = _threads(N, fn)
    cw = L.shard * N
    gin = [np.pad(x, (0, L.n_pad - n)) for x in grads]
    red = np.concatenate([sim.mesh_allreduce([x[c * cw:(c + 1) * cw] for x in gin], L.shard, "bfp_rne")
                          for c in range(L.chunks)])
    rw, rm = O.lion(w0, red[:n], m0, s, 1.0 / N)
    for which in (0, 1):
        gw, gm = (a[:n] for a in res[0][which])
        assert _ulps(gw, rw).max() <= 1 and _ulps(gm, rm).max() <= 1
        for a in res[0][which]:
            assert np.all(a[n:] == 0), "padding untouched"
        for a, b in zip(res[1][which], res[0][which]):
            assert np.array_equal(a, b), "replicas must be bit-identical"
    for a, b in zip(res[0][0], res[0][1]):
        assert np.array_equal(a, b), "immediate and deferred epilogues must agree"


def test_ring_compat_owner_fp32_lion():
    """The ring's compat_owner_fp32 schedule: the owner's slices take the update from the raw f32 sum (at their own
    plane offsets), the others from the decoded wire — per rank the same bits as the Python engine."""
    C = _ext.require()
    N, n = 3, 6000
    rng = np.random.default_rng(43)
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    ekw = dict(codec="bfp_rne", algo="ring", max_slice_elems=1024, compat_owner_fp32=True)
    engines = [NativeAllReduce(None, comm=fabric.comm(r), **ekw) for r in range(N)]
    L = engines[0].layout(n)
    assert L.blocks > 1
    res = _threads(N, lambda r: _two_steps(engines[r], L, n, N, w0, grads, r))
    pys = _py_arm(N, n, w0, grads, L, **ekw)
    for r in range(N):
        assert _same(pys[r], res[r]), f"rank {r}: native engine differs from the Python engine"
    assert np.any(res[0][1][1][:n] != 0)


def _residual(step, L, state):
    if "res" not in state:
        state["res"] = torch.zeros(L.n_pad, device=DEV)
    return dict(residual=state["res"])


def _sr(step, L, state):
    return dict(sr_seed=O.sr_step_seed(77, step, 0))


@pytest.mark.parametrize("extra", [_residual, _sr], ids=["residual", "sr_seed"])
def test_mesh_with_the_encoders_options(extra):
    """Error feedback and stochastic rounding act before the update: Lion takes their wire unchanged."""
    C = _ext.require()
    N, n = 2, 50000 - 48
    rng = np.random.default_rng(51)
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engines = [NativeAllReduce(None, codec="bfp_rne", comm=fabric.comm(r)) for r in range(N)]
    L = engines[0].layout(n)
    res = _threads(N, lambda r: _two_steps(engines[r], L, n, N, w0, grads, r, extra))
    pys = _py_arm(N, n, w0, grads, L, extra, codec="bfp_rne")
    plain = _threads(N, lambda r: _two_steps(engines[r], L, n, N, w0, grads, r))
    for r in range(N):
        assert _same(pys[r], res[r]), "native engine differs from the Python engine"
        assert _same(res[r], res[0]), "replicas must be bit-identical"
    assert not _same(plain[0], res[0]), "the option did not reach the encoders"


def test_clip_group_of_two_lion_requests():
    """Two deferred Lion requests of one clip group equal the same updates with the premultiplied grad_scale."""
    C = _ext.require()
    N, n = 2, 50000 - 48
    rng = np.random.default_rng(77)
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)

    def run(eng, r, clip):
        torch.cuda.set_device(0)
        L = eng.layout(n)
        words = torch.full((4,), float("nan"), device=DEV)
        planes, hs = [], []
        for b in range(2):
            w = torch.zeros(L.n_pad, device=DEV)
            w[:n] = torch.from_numpy(w0 * (b + 1))
            m = torch.zeros(L.n_pad, device=DEV)
            g = torch.zeros(L.n_pad, device=DEV)
            g[:n] = torch.from_numpy(grads[b][r])
            torch.cuda.synchronize()
            kw = dict(clip=words) if clip is True else {}
            hs.append(eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, weight_decay=WD,
                                        grad_scale=0.5 if clip is True else clip, opt="lion", defer=True, **kw))
            planes.append((w, m))
        if clip is True:
            eng.commit_group(hs, max_norm=0.5, grad_scale=0.5)
        else:
            for h in hs:
                h.commit_after_current()
        for h in hs:
            h.synchronize(60)
        torch.cuda.synchronize()
        return [tuple(x.cpu().numpy().copy() for x in p) for p in planes], words.cpu().numpy()

    def arm(clip, native=True):
        if native:
            fabric = C.LoopbackFabric(N, 60.0)
            engs = [NativeAllReduce(None, codec="bfp_rne", comm=fabric.comm(r)) for r in range(N)]
            return _threads(N, lambda r: run(engs[r], r, clip))
        out = [None] * N

        def py_rank(t):
            out[t.rank] = run(CompressedAllReduce(t, codec="bfp_rne", device=DEV), t.rank, clip)

        ThreadFabric(N, timeout_s=60).run(py_rank)
        return out

    clipped = arm(True)
    words = clipped[0][1]
    assert 0 < words[0] < 1
    plain = arm(O.clip_scale(0.5, words))
    py = arm(True, native=False)
    for r in range(N):
        assert np.array_equal(py[r][1], words)
        for b in range(2):
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], plain[r][0][b])), (r, b)
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], clipped[0][0][b])), (r, b)
            assert all(np.array_equal(x, y) for x, y in zip(clipped[r][0][b], py[r][0][b])), (r, b)
            assert clipped[r][0][b][1].any()


# --------------------------------------------------------------------------- trainer
def _train(kind, codec, steps=3):
    sizes, mb = [256, 512, 256], 256
    if kind == "native":
        eng = NativeAllReduce(None, codec=codec)
    elif kind == "python":
        eng = CompressedAllReduce(ThreadFabric(1).transport(0), codec=codec, device=DEV)
    else:
        eng = None
    pad = (lambda n, e=eng: e.layout(n).n_pad) if eng is not None else None
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, momentum=True, pad_fn=pad)
    tr = DataParallelTrainer(model, eng, lr=LR, weight_decay=WD, optimizer="lion")
    assert tr.fused_update is False and tr.betas == (0.9, 0.99)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=g) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32).to(DEV)
    hist = []
    for _ in range(steps):
        tr.step(x, y)
        tr.finish()
        torch.cuda.synchronize()
        hist.append([(l.master[: l.n].cpu().numpy().copy(), l.mom[: l.n].cpu().numpy().copy(),
                      l.lp[: l.n].float().cpu().numpy().copy()) for l in model.layers])
    assert tr.fused_updates == 0
    return hist


def _hist_equal(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for la, lb in zip(sa, sb) for x, y in zip(la, lb))


def test_trainer_lion_world1():
    """raw_f32 on the wire (the engine-less update reads the f32 gradient itself): the native inline engine, the Python
    engine and the engine-less trainer agree bit for bit; with bfp_rne the two engines do."""
    nat = _train("native", "raw_f32")
    assert _hist_equal(nat, _train("python", "raw_f32")), "native and Python engine differ"
    assert _hist_equal(nat, _train("none", "raw_f32")), "engine and engine-less trainer differ"
    assert all(np.any(l[1] != 0) for l in nat[-1]) and not np.array_equal(nat[0][0][0], nat[-1][0][0])
    assert _hist_equal(_train("native", "bfp_rne"), _train("python", "bfp_rne"))


# --------------------------------------------------------------------------- refusals
def test_refusals_on_the_gpu_entry_points():
    C = _ext.require()
    eng = NativeAllReduce(None, codec="bfp_rne")
    n = 1000
    L = eng.layout(n)
    g, w, m, v = (torch.zeros(L.n_pad, device=DEV) for _ in range(4))
    ok = dict(n_valid=n, lr=LR, opt="lion")
    eng.allreduce_sgd(g, w, None, m, **ok).synchronize(60)
    pm = wire.moment_plane(L.n_pad, DEV)
    for mom, kw, match in ((None, {}, "needs its moment plane"), (m.double(), {}, "contiguous float32"),
                           (torch.zeros(2 * L.n_pad, device=DEV)[::2], {}, "contiguous float32"),
                           (m.cpu(), {}, "engine's device"), (m, dict(var=v), "var must be None"),
                           (m, dict(momentum=0.9), "belong to SGD"), (m, dict(nesterov=True), "belong to SGD"),
                           (m, dict(trust_ratio=True), "flag of opt='adamw'"),
                           (m, dict(moment_codec="bfp8", moment_seed=1), "AdamW only")):
        with pytest.raises(ValueError, match=match):
            eng.allreduce_sgd(g, w, None, mom, **{**ok, **kw})
    py = CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", device=DEV)
    with pytest.raises(ValueError, match="engine's device"):
        py.allreduce_sgd(g, w, None, m.cpu(), **ok)
    # C.submit itself, past the wrapper's validation
    a = O.lion_scalars(LR, WD, B1, B2).kernel_args()
    base = (g, w, None, m, n, LR, 1.0, 0.0, 0.0, False, True, True, None, None, 0, 0, 0, False)

    def submit(args=base, **kw):
        return eng.C.submit(*args, **{**dict(opt=2, lion=a), **kw})

    slot = submit()
    eng.C.commit(slot)
    eng.C.synchronize(slot, 60.0)
    no_mom = base[:3] + (None,) + base[4:]
    short = base[:3] + (torch.zeros(n, device=DEV),) + base[4:]
    lamb = O.lamb_scalars(LR, 0, 0.9, 0.999, 1e-8, 1).kernel_args()
    for args, kw, match in ((no_mom, {}, "Lion needs its moment plane"), (short, {}, "padded to the layout"),
                            (base, dict(var=v), "no second-moment plane"), (base, dict(lamb=lamb, var=v), "trust ratio"),
                            (base, dict(lamb=lamb), "trust ratio"), (base, dict(mom_q=pm, var_q=pm), "AdamW only"),
                            (base, dict(lion=None), "needs its scalars"), (base, dict(lion=a[:6]), "7 scalars"),
                            (base, dict(opt=3), "opt: 0")):
        with pytest.raises(RuntimeError, match=match):
            submit(args, **kw)
    # the op's binding
    buf = torch.zeros(O.shard_bytes("bfp_rne", L.n_pad), dtype=torch.uint8, device=DEV)
    for args, match in (((buf, L.n_pad, 1, -1, 0, w, None, m[: n - 4], a, 1.0, n, 1, 0, None), "rounded up to 8"),
                        ((buf, L.n_pad, 1, -1, 0, w, None, m.double(), a, 1.0, n, 1, 0, None), "float32"),
                        ((buf, L.n_pad, 1, -1, 0, w, None, m, a, 1.0, L.n_pad + 1, 1, 0, None), "n_valid beyond"),
                        ((buf[:-16], L.n_pad, 1, -1, 0, w, None, m, a, 1.0, n, 1, 0, None), "wire buffer too small"),
                        ((buf, L.n_pad, 1, -1, 0, w, None, m, a[:6], 1.0, n, 1, 0, None), "7 scalars"),
                        ((buf, L.n_pad, 1, -1, 0, w, None, m, a, 1.0, n, 1, 8, None), "shard_stride")):
        with pytest.raises(RuntimeError, match=match):
            C.wire_lion(*args)


if __name__ == "__main__":
    if sys.argv[1] == "digests":
        print(json.dumps(_digests()), flush=True)
