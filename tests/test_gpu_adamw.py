"""AdamW in the all-reduce epilogues on the GPU: the decode + AdamW kernel against the oracle, the native engine over
virtual ranks (LoopbackFabric) against the Python engine and the spec simulator, and the trainer at world 1.

Bounds against the oracle (bfp_oracle.adamw, fma emulated in float64):
  * m' and v' within 1 ulp — the emulated fma's rare double rounding, as test_gpu_kernels.test_sgd_epilogue allows;
  * |w_gpu - w_ref| <= ulp(w_ref) + 4 * 2^-24 * |w_ref - w * decay| — a one-ulp move of m' and of v' moves the
    quotient by at most 1.5 * 2^-24 relative, the two further roundings (d, the quotient) can each flip once, and the
    final fma can flip once.
"""
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
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_bounds(got, ref, w_prev, scalars, what=""):
    """got / ref: (w, m, v) float32 arrays; w_prev: the weights before the step."""
    (gw, gm, gv), (rw, rm, rv) = got, ref
    um, uv = _ulps(gm, rm).max(), _ulps(gv, rv).max()
    base = w_prev.astype(np.float64) * float(scalars.decay) if scalars.wd != 0 else w_prev.astype(np.float64)
    bound = np.spacing(np.abs(rw)).astype(np.float64) + 4 * 2.0 ** -24 * np.abs(rw.astype(np.float64) - base)
    err = np.abs(gw.astype(np.float64) - rw.astype(np.float64))
    print(f"{what}: m' max {um} ulp, v' max {uv} ulp, w max err/bound {float((err / bound).max()):.3f}, "
          f"w max {_ulps(gw, rw).max()} ulp")
    assert um <= 1 and uv <= 1
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("codec", ["bfp_trunc", "bfp_rne", "raw_f32"])
@pytest.mark.parametrize("has_lp", [True, False])
@pytest.mark.parametrize("step", [1, 7])
def test_adamw_epilogue(codec, has_lp, step):
    n_s, N = 1024, 4
    n, n_valid = n_s * N, n_s * N - 77
    rng = np.random.default_rng(2)
    g = rng.standard_normal(n).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    s = O.adamw_scalars(LR, WD, B1, B2, EPS, step)
    buf = O.pack(g, n_s, codec)
    sb = O.shard_bytes(codec, n_s)
    # a strided wire (the shards 256 B further apart than packed) for the step-7 cases
    stride = sb + 256 if step == 7 else 0
    if stride:
        spread = np.zeros(stride * N, np.uint8)
        for q in range(N):
            spread[q * stride: q * stride + sb] = buf[q * sb:(q + 1) * sb]
        wbuf = torch.from_numpy(spread).to(DEV)
    else:
        wbuf = torch.from_numpy(buf).to(DEV)
    wt, mt, vt = (torch.from_numpy(x.copy()).to(DEV) for x in (w, m, v))
    lp0 = torch.full((n,), 3.0, dtype=torch.bfloat16, device=DEV)
    lp = lp0.clone() if has_lp else None
    wire.adamw(wbuf, n_s, N, wt, codec=codec, mom=mt, var=vt, scalars=s, lp=lp, grad_scale=0.25, n_valid=n_valid,
               skip_shard=1, skip_period=N, shard_stride=stride)
    torch.cuda.synchronize()
    gd = O.unpack(buf, n, n_s, codec)
    rw, rm, rv = O.adamw(w, gd, m, v, s, 0.25)
    keep = np.zeros(n, bool)
    keep[n_valid:] = True
    keep[n_s:2 * n_s] = True
    got = [t.cpu().numpy() for t in (wt, mt, vt)]
    for a, old, name in zip(got, (w, m, v), "wmv"):
        assert np.array_equal(a[n_valid:], old[n_valid:]), f"{name}: padding must not be touched"
        assert np.array_equal(a[n_s:2 * n_s], old[n_s:2 * n_s]), f"{name}: skipped shard must not be touched"
    assert not np.array_equal(got[0][~keep], w[~keep])
    check_bounds([a[~keep] for a in got], [a[~keep] for a in (rw, rm, rv)], w[~keep], s,
                 f"{codec} lp={has_lp} step={step}")
    if has_lp:
        k = torch.from_numpy(keep).to(DEV)
        assert torch.equal(lp[k], lp0[k]), "lp: padding / skipped shard must not be touched"
        assert torch.equal(lp[~k], wt.to(torch.bfloat16)[~k])


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


def _two_steps(eng, L, n, N, w0, grads, r):
    """Two AdamW requests on rank r's engine; the planes (numpy) and the bf16 copy after each."""
    w = torch.zeros(L.n_pad, device=DEV)
    w[:n] = torch.from_numpy(w0)
    lp = torch.zeros(L.n_pad, device=DEV, dtype=torch.bfloat16)
    m, v = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    snaps = []
    for step in (1, 2):
        g = torch.zeros(L.n_pad, device=DEV)
        g[:n] = torch.from_numpy(grads[step - 1][r])
        torch.cuda.synchronize()
        h = eng.allreduce_sgd(g, w, lp, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N, opt="adamw", var=v,
                              betas=(B1, B2), eps=EPS, step=step, defer=True)
        h.commit_after_current()
        h.synchronize(60)
        torch.cuda.synchronize()
        snaps.append((w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), lp.cpu()))
    return snaps


def _check_against_oracle(snaps, L, n, N, w0, grads, algo, orders, what):
    """Each step within the kernel test's bounds of the oracle applied, from the planes the step started with, to
    the spec simulator's reduced gradient."""
    prev = (w0, np.zeros(n, np.float32), np.zeros(n, np.float32))
    for step in (1, 2):
        gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step - 1]]
        red = sim.mesh_allreduce(gin, L.shard, "bfp_rne") if algo == "mesh" else \
            sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, "bfp_rne")[0]
        s = O.adamw_scalars(LR, WD, B1, B2, EPS, step)
        got = [a[:n] for a in snaps[step - 1][:3]]
        check_bounds(got, O.adamw(prev[0], red[:n], prev[1], prev[2], s, 1.0 / N), prev[0], s, f"{what} step {step}")
        for a in snaps[step - 1][:3]:
            assert np.all(a[n:] == 0), "padding untouched"
        assert torch.equal(snaps[step - 1][3][:n], torch.from_numpy(got[0]).to(torch.bfloat16))
        prev = got


def _same(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa[:3], sb[:3])) and \
        all(torch.equal(sa[3], sb[3]) for sa, sb in zip(a, b))


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
def test_native_engine_loopback_adamw(N, algo):
    C = _ext.require()
    n = 50000 - 48
    rng = np.random.default_rng(N * 100 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engines = [NativeAllReduce(None, codec="bfp_rne", algo=algo, max_slice_elems=8192, comm=fabric.comm(r))
               for r in range(N)]
    L = engines[0].layout(n)
    res = _threads(N, lambda r: _two_steps(engines[r], L, n, N, w0, grads, r))
    for r in range(1, N):
        assert _same(res[r], res[0]), "replicas must be bit-identical"
    # the Python engine issues the same kernels on the same GPU tensors: the same bits
    tf = ThreadFabric(N, timeout_s=60)
    pys = [None] * N

    def py_rank(t):
        torch.cuda.set_device(0)
        eng = CompressedAllReduce(t, codec="bfp_rne", algo=algo, max_slice_elems=8192, device=DEV)
        Lp = eng.layout(n)
        assert (Lp.n_pad, Lp.shard, Lp.slice_elems, Lp.blocks) == (L.n_pad, L.shard, L.slice_elems, L.blocks)
        pys[t.rank] = _two_steps(eng, Lp, n, N, w0, grads, t.rank)

    tf.run(py_rank)
    assert _same(pys[0], res[0]), "native engine differs from the Python engine"
    _check_against_oracle(res[0], L, n, N, w0, grads, algo, engines[0].orders, f"N={N} {algo}")


def test_inline_world1_engine_adamw():
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


def _train(prepack, steps=3):
    sizes, mb = [256, 512, 256], 256
    eng = NativeAllReduce(None, codec="bfp_rne")
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, adam=True,
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=LR, weight_decay=WD, optimizer="adamw", betas=(B1, B2), eps=EPS,
                             prepack=prepack)
    assert tr.fused_update is False and tr.prepack == prepack
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=g) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32).to(DEV)
    hist = []
    for k in range(1, steps + 1):
        torch.cuda.synchronize()
        prev = [(l.master.cpu().numpy().copy(), l.mom.cpu().numpy().copy(), l.var.cpu().numpy().copy())
                for l in model.layers]
        tr.step(x, y)
        tr.finish()
        hist.append((prev, [l.grad.cpu().numpy().copy() for l in model.layers],
                     [(l.master.cpu().numpy().copy(), l.mom.cpu().numpy().copy(), l.var.cpu().numpy().copy(),
                       l.lp.cpu().clone()) for l in model.layers]))
    assert tr.opt_step == steps and tr.fused_updates == 0 and tr.fused_update is False
    return model, hist


def test_trainer_adamw_world1():
    model, hist = _train(prepack=False)
    for k, (prev, grads, after) in enumerate(hist, 1):
        s = O.adamw_scalars(LR, WD, B1, B2, EPS, k)
        for i, l in enumerate(model.layers):
            w0, m0, v0 = (a[: l.n] for a in prev[i])
            gq = O.quantize(grads[i][: l.n_pad], "bfp_rne")[: l.n]
            assert np.abs(gq).max() > 0
            check_bounds([a[: l.n] for a in after[i][:3]], O.adamw(w0, gq, m0, v0, s), w0, s, f"step {k} fc{i}")
            assert torch.equal(after[i][3][: l.n], torch.from_numpy(after[i][0][: l.n]).to(torch.bfloat16))
    # the default GEMM-encoded wire: the same bits
    _, hist_p = _train(prepack=True)
    for (_, _, a), (_, _, b) in zip(hist, hist_p):
        for la, lb in zip(a, b):
            for x, y in zip(la[:3], lb[:3]):
                assert np.array_equal(x, y), "prepacked run differs from the engine-encoded run"
            assert torch.equal(la[3], lb[3])


def test_adamw_step_refuses_graph_capture(monkeypatch):
    """The step's scalars are by-value kernel arguments: a backward enqueued while the stream captures a graph raises
    before it enqueues anything (the capture state is stubbed: nothing is captured here)."""
    eng = NativeAllReduce(None, codec="bfp_rne")
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, seed=3, adam=True,
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=LR, optimizer="adamw")
    y = torch.zeros(256, dtype=torch.int32, device=DEV)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        tr.backward_pass(y)
    assert tr.opt_step == 0


def test_chunked_mesh_adamw():
    """A bucket above chunk_elems: every chunk's epilogue offsets all three planes (immediate: per-chunk epilogues in
    the pipeline; deferred: one epilogue over the whole gathered wire)."""
    C = _ext.require()
    N, n, chunk = 2, 50000 - 48, 8192
    rng = np.random.default_rng(41)
    grads = [rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)]
    w0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v0 = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    s = O.adamw_scalars(LR, WD, B1, B2, EPS, 5)
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
            for x in (w0, m0, v0):
                t = torch.zeros(L.n_pad, device=DEV)
                t[:n] = torch.from_numpy(x)
                planes.append(t)
            w, m, v = planes
            torch.cuda.synchronize()
            h = engines[r].allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N,
                                         opt="adamw", var=v, betas=(B1, B2), eps=EPS, step=5, defer=defer)
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
    ref = O.adamw(w0, red[:n], m0, v0, s, 1.0 / N)
    for which, name in ((0, "immediate"), (1, "deferred")):
        check_bounds([a[:n] for a in res[0][which]], ref, w0, s, f"chunked {name}")
        for a, old in zip(res[0][which], (w0, m0, v0)):
            assert np.all(a[n:] == 0), "padding untouched"
        for a, b in zip(res[1][which], res[0][which]):
            assert np.array_equal(a, b), "replicas must be bit-identical"


def test_ring_compat_owner_fp32_adamw():
    """The ring's compat_owner_fp32 schedule: the owner's slices take the update from the raw f32 sum (at their own
    plane offsets), the others from the decoded wire — per rank the same bits as the Python engine."""
    C = _ext.require()
    N, n = 3, 6000
    rng = np.random.default_rng(43)
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engines = [NativeAllReduce(None, codec="bfp_rne", algo="ring", max_slice_elems=1024, comm=fabric.comm(r),
                               compat_owner_fp32=True) for r in range(N)]
    L = engines[0].layout(n)
    assert L.blocks > 1
    res = _threads(N, lambda r: _two_steps(engines[r], L, n, N, w0, grads, r))
    pys = [None] * N

    def py_rank(t):
        torch.cuda.set_device(0)
        eng = CompressedAllReduce(t, codec="bfp_rne", algo="ring", max_slice_elems=1024, device=DEV,
                                  compat_owner_fp32=True)
        Lp = eng.layout(n)
        assert (Lp.n_pad, Lp.slice_elems, Lp.blocks) == (L.n_pad, L.slice_elems, L.blocks)
        pys[t.rank] = _two_steps(eng, Lp, n, N, w0, grads, t.rank)

    ThreadFabric(N, timeout_s=60).run(py_rank)
    for r in range(N):
        assert _same(pys[r], res[r]), f"rank {r}: native engine differs from the Python engine"
    assert not _same(res[1], res[0]), "compat mode diverges by design"
