"""AdamW with the layer-wise trust ratio (LAMB) on the GPU: the three kernels against the oracle and against the
AdamW kernel, degenerate inputs, determinism, the native engine over virtual ranks (LoopbackFabric) against the Python
engine and the spec simulator, the inline engine, the trainer at world 1, and the refusals.

Bounds against the oracle (bfp_oracle.lamb_*, fma / sqrt / division emulated in float64 and rounded):
  * m' and v' are bit-identical to the wire.adamw kernel's (the same statements) and within 1 ulp of the oracle's —
    the emulated fma's rare double rounding, as test_gpu_adamw allows;
  * the three scale words within 2 f32 ulp of the oracle's: the fp64 sums of exact products leave at most one flip
    in phi and one more in the product lr * phi;
  * w' against the oracle's pass 2 fed the DEVICE's scale words. With eps = 2^-23 (the largest relative size of one
    ulp) and every operation correctly rounded on both sides, two results of one operation differ by the propagated
    input difference plus eps (half an ulp each side; the oracle's double rounding adds 2^-29 of that). m' and v' start
    eps apart, so: sqrt(v') 0.5 eps + eps = 1.5 eps; d = fma(sqrt, rsbc2, eps) — both terms non-negative, so the
    relative difference carries over — 2.5 eps; u = m' / d: 1 + 2.5 + 1 = 4.5 eps; ub = u * rbc1: 5.5 eps;
    r = fma(wd, w, ub) with the same w on both sides: |dr| <= 5.5 eps |ub| + eps |r|, and |ub| <= |r| + wd |w|;
    w' = fma(-scale, r, w) with the same scale and w: |dw'| <= scale |dr| + ulp(w'). Rounding 5.5 up to 6 for the
    second-order terms:
        |w_gpu - w_ref| <= ulp(max(|w_gpu|, |w_ref|)) + scale * 2^-23 * (7 |r_ref| + 6 wd |w|).
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
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_words(got, ref, what=""):
    print(f"{what}: words gpu {got.tolist()} oracle {ref.tolist()} ulp {_ulps(got, ref).tolist()}")
    assert np.isfinite(got).all()
    assert np.all(_ulps(got, ref) <= 2)
    assert got[1] == ref[1], "the plain lr word is the f32 lr itself"


def check_bounds(got, w_prev, g, m_prev, v_prev, scalars, words, n_adapt, grad_scale, what=""):
    """got: (w, m, v) of the updated elements after the step; w_prev / g / m_prev / v_prev: what the step started
    from (g decoded); words: the device's scale words. The module docstring derives the bound."""
    gw, gm, gv = got
    rm, rv, rr = O.lamb_moments(w_prev, g, m_prev, v_prev, scalars, grad_scale)
    rw = O.lamb_apply(w_prev, rm, rv, scalars, words, n_adapt)
    um, uv = _ulps(gm, rm).max(), _ulps(gv, rv).max()
    scale = np.where(np.arange(w_prev.size) < n_adapt, np.float64(words[0]), np.float64(words[1]))
    bound = np.spacing(np.maximum(np.abs(rw), np.abs(gw))).astype(np.float64) + scale * 2.0 ** -23 * (
        7 * np.abs(rr.astype(np.float64)) + 6 * float(scalars.wd) * np.abs(w_prev.astype(np.float64)))
    err = np.abs(gw.astype(np.float64) - rw.astype(np.float64))
    print(f"{what}: m' max {um} ulp, v' max {uv} ulp, w max err/bound {float((err / bound).max()):.3f}, "
          f"w max {_ulps(gw, rw).max()} ulp")
    assert um <= 1 and uv <= 1
    assert np.all(err <= bound), float((err / bound).max())
    return rr


def _inputs(n, seed=2):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(np.float32)
    w = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    return g, w, m, v


N_S, NSH = 1024, 4
N = N_S * NSH
N_VALID = N - 77


def _kernel_case(codec, n_adapt, has_lp, strided=False, two_regions=False, step=3):
    g, w, m, v = _inputs(N)
    s = O.lamb_scalars(LR, WD, B1, B2, EPS, step)
    buf = O.pack(g, N_S, codec)
    sb = O.shard_bytes(codec, N_S)
    stride = sb + 256 if strided else 0
    if stride:
        spread = np.zeros(stride * NSH, np.uint8)
        for q in range(NSH):
            spread[q * stride: q * stride + sb] = buf[q * sb:(q + 1) * sb]
        wbuf = torch.from_numpy(spread).to(DEV)
    else:
        wbuf = torch.from_numpy(buf).to(DEV)
    wt, mt, vt = (torch.from_numpy(x.copy()).to(DEV) for x in (w, m, v))
    lp0 = torch.full((N,), 3.0, dtype=torch.bfloat16, device=DEV)
    lp = lp0.clone() if has_lp else None
    pairs = wire.lamb_partials_for(wt, N_S)
    assert pairs == 1  # 128 tasks of 8 values: one block
    partials = torch.full((2 * 2 * pairs,), float("nan"), dtype=torch.float64, device=DEV)
    words = torch.zeros(3, device=DEV)
    skip = dict(skip_shard=1, skip_period=NSH)
    k = wire.lamb_moments(wbuf, N_S, NSH, wt, codec=codec, mom=mt, var=vt, scalars=s, partials=partials,
                          grad_scale=0.25, n_valid=N_VALID, n_adapt=n_adapt, shard_stride=stride, **skip)
    assert k == pairs
    keep = np.zeros(N, bool)
    keep[N_VALID:] = True
    if two_regions:  # the complementary launch: shard 1 alone, its partials behind the first launch's
        lo, hi = N_S, 2 * N_S
        a2 = max(0, min(n_adapt - lo, N_S))
        k += wire.lamb_moments(wbuf[sb if not stride else stride:], N_S, 1, wt[lo:hi], codec=codec, mom=mt[lo:hi],
                               var=vt[lo:hi], scalars=s, partials=partials, partials_base=k, grad_scale=0.25,
                               n_adapt=a2, shard_stride=stride)
        assert k == 2 * pairs
    else:
        keep[N_S:2 * N_S] = True
    torch.cuda.synchronize()
    # after pass 1 alone: the weights and their bf16 copy untouched
    assert np.array_equal(wt.cpu().numpy(), w), "pass 1 must not write master"
    if has_lp:
        assert torch.equal(lp, lp0), "pass 1 must not write lp"
    # m' and v' bit-identical to the AdamW kernel on copies of the same inputs
    aw, am, av = (torch.from_numpy(x.copy()).to(DEV) for x in (w, m, v))
    wire.adamw(wbuf, N_S, NSH, aw, codec=codec, mom=am, var=av, scalars=O.adamw_scalars(LR, WD, B1, B2, EPS, step),
               grad_scale=0.25, n_valid=N_VALID, shard_stride=stride, **({} if two_regions else skip))
    assert torch.equal(mt, am) and torch.equal(vt, av), "moments differ from the AdamW kernel's"
    wire.lamb_ratio(partials, k, LR, words)
    wire.lamb_apply(wt, N_S, mom=mt, var=vt, scalars=s, words=words, lp=lp, n_valid=N_VALID, n_adapt=n_adapt, **skip)
    if two_regions:
        wire.lamb_apply(wt[lo:hi], N_S, mom=mt[lo:hi], var=vt[lo:hi], scalars=s, words=words,
                        lp=None if lp is None else lp[lo:hi], n_adapt=a2)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (wt, mt, vt)]
    wd = words.cpu().numpy()
    for a, old, name in zip(got, (w, m, v), "wmv"):
        assert np.array_equal(a[keep], old[keep]), f"{name}: padding / skipped shard must not be touched"
    gd = O.unpack(buf, N, N_S, codec)
    what = f"{codec} n_adapt={n_adapt} lp={has_lp} strided={strided} two={two_regions}"
    # the oracle works on the updated elements in flat order; n_adapt counts flat elements, so map it
    upd = ~keep
    na_upd = int(upd[:n_adapt].sum())
    rr = check_bounds([a[upd] for a in got], w[upd], gd[upd], m[upd], v[upd], s, wd, na_upd, 0.25, what)
    check_words(wd, O.lamb_ratio(w[upd], rr, na_upd, LR), what)
    if n_adapt == 0:
        assert wd[2] == 1.0 and wd[0] == wd[1]
    else:
        assert wd[2] != 1.0
    assert not np.array_equal(got[0][upd], w[upd])
    if has_lp:
        kt = torch.from_numpy(keep).to(DEV)
        assert torch.equal(lp[kt], lp0[kt]), "lp: padding / skipped shard must not be touched"
        assert torch.equal(lp[~kt], wt.to(torch.bfloat16)[~kt])


@pytest.mark.parametrize("codec", ["bfp_trunc", "bfp_rne", "raw_f32"])
@pytest.mark.parametrize("n_adapt", [N_VALID, 3001, 0])
@pytest.mark.parametrize("has_lp", [True, False])
def test_lamb_kernels(codec, n_adapt, has_lp):
    _kernel_case(codec, n_adapt, has_lp)


def test_lamb_kernels_strided_wire():
    _kernel_case("bfp_rne", 3001, True, strided=True)


@pytest.mark.parametrize("n_adapt", [N_VALID, 1500])
def test_lamb_two_regions_one_ratio(n_adapt):
    """Launch 1 skips shard 1 (skip_shard=1, skip_period=4), launch 2 covers shard 1 alone; one ratio over both
    launches' partials. 1500 ends the adapted tensor inside shard 1."""
    _kernel_case("bfp_rne", n_adapt, True, two_regions=True)


def _three(wbuf, n_s, n_sh, wt, mt, vt, s, lp=None, n_valid=None, n_adapt=None, codec="bfp_rne"):
    pairs = wire.lamb_partials_for(wt, n_s)
    partials = torch.zeros(2 * pairs, dtype=torch.float64, device=DEV)
    words = torch.zeros(3, device=DEV)
    k = wire.lamb_moments(wbuf, n_s, n_sh, wt, codec=codec, mom=mt, var=vt, scalars=s, partials=partials,
                          n_valid=n_valid, n_adapt=n_adapt)
    wire.lamb_ratio(partials, k, float(s.lr), words)
    wire.lamb_apply(wt, n_s, mom=mt, var=vt, scalars=s, words=words, lp=lp, n_valid=n_valid, n_adapt=n_adapt)
    torch.cuda.synchronize()
    return words.cpu().numpy(), partials.cpu().numpy()


def test_degenerate_inputs():
    g, w, m, v = _inputs(N, seed=9)
    s = O.lamb_scalars(LR, WD, B1, B2, EPS, 2)
    wbuf = torch.from_numpy(O.pack(g, N_S, "bfp_rne")).to(DEV)
    # adapted weights all zero: phi == 1 (S_w = 0), the tail keeps its own weights
    w[:3001] = 0
    wt, mt, vt = (torch.from_numpy(x.copy()).to(DEV) for x in (w, m, v))
    words, partials = _three(wbuf, N_S, NSH, wt, mt, vt, s, n_valid=N_VALID, n_adapt=3001)
    assert partials[0::2].sum() == 0 and partials[1::2].sum() > 0
    assert words.tolist() == [np.float32(LR), np.float32(LR), 1.0]
    assert torch.isfinite(wt).all()
    # zero gradient, zero moments, no decay: w bit-unchanged, nothing non-finite
    s0 = O.lamb_scalars(LR, 0.0, B1, B2, EPS, 1)
    _, w2, _, _ = _inputs(N, seed=10)
    zbuf = torch.from_numpy(O.pack(np.zeros(N, np.float32), N_S, "bfp_rne")).to(DEV)
    wt = torch.from_numpy(w2.copy()).to(DEV)
    mt, vt = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    lp = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    words, partials = _three(zbuf, N_S, NSH, wt, mt, vt, s0, lp=lp)
    assert np.array_equal(wt.cpu().numpy(), w2)
    assert words.tolist() == [np.float32(LR), np.float32(LR), 1.0] and np.isfinite(partials).all()
    assert torch.equal(mt, torch.zeros_like(mt)) and torch.equal(vt, torch.zeros_like(vt))
    assert torch.equal(lp, wt.to(torch.bfloat16))


def test_deterministic_and_capped_grid():
    """One shard big enough that the capped grid makes lanes loop: pass 1 has n_s / 8 tasks for at most
    wire_max_blocks() = 2048 blocks of 256 lanes (stream_grid), so above 2048 * 256 * 8 = 4 Mi elements a lane takes
    more than one task (pass 2, 4 values per lane, above 2 Mi). The same request twice from the same state gives the
    same partials, words and planes; and the small shape does too."""
    for n_s, n_sh in ((4 * 1024 * 1024 + 65536, 1), (N_S, NSH)):
        n = n_s * n_sh
        g, w, m, v = _inputs(n, seed=4)
        s = O.lamb_scalars(LR, WD, B1, B2, EPS, 4)
        wbuf = torch.from_numpy(O.pack(g, n_s, "bfp_rne")).to(DEV)
        pairs = wire.lamb_partials_for(torch.empty(0, device=DEV), n_s)
        assert pairs == (2048 if n_sh == 1 else 1)
        runs = []
        for _ in range(2):
            wt, mt, vt = (torch.from_numpy(x.copy()).to(DEV) for x in (w, m, v))
            words, partials = _three(wbuf, n_s, n_sh, wt, mt, vt, s, n_valid=n - 77, n_adapt=n - 1000)
            runs.append((words, partials, wt.cpu().numpy(), mt.cpu().numpy(), vt.cpu().numpy()))
        for a, b in zip(*runs):
            assert np.array_equal(a, b)
        nv = n - 77
        rr = check_bounds([a[:nv] for a in runs[0][2:]], w[:nv], O.quantize(g, "bfp_rne")[:nv], m[:nv], v[:nv], s,
                          runs[0][0], n - 1000, 1.0, f"n_s={n_s}")
        check_words(runs[0][0], O.lamb_ratio(w[:nv], rr, n - 1000, LR), f"n_s={n_s}")


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


N_ENG, N_ADAPT_ENG = 50000 - 48, 49000


def _two_steps(eng, L, n, nranks, w0, grads, r):
    """Two trust-ratio requests on rank r's engine; the planes, the bf16 copy and the scale words after each."""
    w = torch.zeros(L.n_pad, device=DEV)
    w[:n] = torch.from_numpy(w0)
    lp = torch.zeros(L.n_pad, device=DEV, dtype=torch.bfloat16)
    m, v = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    words = torch.zeros(2, 3, device=DEV)
    snaps = []
    for step in (1, 2):
        g = torch.zeros(L.n_pad, device=DEV)
        g[:n] = torch.from_numpy(grads[step - 1][r])
        torch.cuda.synchronize()
        h = eng.allreduce_sgd(g, w, lp, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / nranks, opt="adamw",
                              var=v, betas=(B1, B2), eps=EPS, step=step, defer=True, trust_ratio=True,
                              n_adapt=N_ADAPT_ENG, trust_out=words[step - 1])
        h.commit_after_current()
        h.synchronize(60)
        torch.cuda.synchronize()
        snaps.append((w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), lp.cpu(), words[step - 1].cpu().numpy()))
    return snaps


def _check_against_oracle(snaps, L, n, nranks, w0, grads, algo, orders, what):
    prev = (w0, np.zeros(n, np.float32), np.zeros(n, np.float32))
    for step in (1, 2):
        gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step - 1]]
        red = sim.mesh_allreduce(gin, L.shard, "bfp_rne") if algo == "mesh" else \
            sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, "bfp_rne")[0]
        s = O.lamb_scalars(LR, WD, B1, B2, EPS, step)
        got = [a[:n] for a in snaps[step - 1][:3]]
        words = snaps[step - 1][4]
        rr = check_bounds(got, prev[0], red[:n], prev[1], prev[2], s, words, N_ADAPT_ENG, 1.0 / nranks,
                          f"{what} step {step}")
        check_words(words, O.lamb_ratio(prev[0], rr, N_ADAPT_ENG, LR), f"{what} step {step}")
        assert words[2] != 1.0
        for a in snaps[step - 1][:3]:
            assert np.all(a[n:] == 0), "padding untouched"
        assert torch.equal(snaps[step - 1][3][:n], torch.from_numpy(got[0]).to(torch.bfloat16))
        prev = got


def _same(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa[:3] + sa[4:], sb[:3] + sb[4:])) and \
        all(torch.equal(sa[3], sb[3]) for sa, sb in zip(a, b))


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
def test_native_engine_loopback_lamb(nranks, algo):
    C = _ext.require()
    n = N_ENG
    rng = np.random.default_rng(nranks * 100 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(nranks)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = C.LoopbackFabric(nranks, 60.0)
    engines = [NativeAllReduce(None, codec="bfp_rne", algo=algo, max_slice_elems=8192, comm=fabric.comm(r))
               for r in range(nranks)]
    L = engines[0].layout(n)
    res = _threads(nranks, lambda r: _two_steps(engines[r], L, n, nranks, w0, grads, r))
    for r in range(1, nranks):
        assert _same(res[r], res[0]), "replicas must be bit-identical, planes and scale words"
    _check_against_oracle(res[0], L, n, nranks, w0, grads, algo, engines[0].orders, f"N={nranks} {algo}")
    if algo != "mesh":
        return
    # the Python engine issues the same launches on the same GPU tensors: the same bits
    pys = [None] * nranks

    def py_rank(t):
        torch.cuda.set_device(0)
        eng = CompressedAllReduce(t, codec="bfp_rne", algo=algo, max_slice_elems=8192, device=DEV)
        Lp = eng.layout(n)
        assert (Lp.n_pad, Lp.shard) == (L.n_pad, L.shard)
        pys[t.rank] = _two_steps(eng, Lp, n, nranks, w0, grads, t.rank)

    ThreadFabric(nranks, timeout_s=60).run(py_rank)
    assert _same(pys[0], res[0]), "native engine differs from the Python engine"


def test_inline_world1_engine_lamb():
    n = N_ENG
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
    # without trust_out the words live in the engine's own scratch: the same planes
    w = torch.zeros(L.n_pad, device=DEV)
    w[:n] = torch.from_numpy(w0)
    m, v = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    g = torch.zeros(L.n_pad, device=DEV)
    g[:n] = torch.from_numpy(grads[0][0])
    eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, weight_decay=WD, opt="adamw", var=v, betas=(B1, B2), eps=EPS,
                      step=1, trust_ratio=True, n_adapt=N_ADAPT_ENG).synchronize(60)
    torch.cuda.synchronize()
    assert np.array_equal(w.cpu().numpy(), got[0][0])


def test_empty_request_still_writes_its_words():
    """n_valid == 0: no region, no pass 1; the ratio launch sums nothing and writes {lr, lr, 1} over stale words."""
    eng = NativeAllReduce(None, codec="bfp_rne")
    n_pad = eng.layout(0).n_pad
    g, w, m, v = _planes(n_pad)
    out = torch.full((3,), float("nan"), device=DEV)
    eng.allreduce_sgd(g, w, None, m, n_valid=0, lr=LR, opt="adamw", var=v, betas=(B1, B2), eps=EPS, step=1,
                      trust_ratio=True, trust_out=out).synchronize(60)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.array([LR, LR, 1.0], np.float32))
    assert all(torch.equal(t, torch.zeros_like(t)) for t in (w, m, v))


def _train(prepack, steps=2):
    sizes, mb = [256, 512, 256], 256
    eng = NativeAllReduce(None, codec="bfp_rne")
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, adam=True,
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=LR, weight_decay=WD, optimizer="adamw", betas=(B1, B2), eps=EPS,
                             trust_ratio=True, prepack=prepack)
    assert tr.fused_update is False and tr.prepack == prepack
    assert tr.trust_ratios.shape == (2, 3) and tr.trust_ratios.is_cuda
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
                       l.lp.cpu().clone()) for l in model.layers], tr.trust_ratios.cpu().numpy().copy()))
    assert tr.opt_step == steps and tr.fused_updates == 0
    return model, hist


def test_trainer_lamb_world1():
    model, hist = _train(prepack=False)
    for k, (prev, grads, after, ratios) in enumerate(hist, 1):
        assert np.isfinite(ratios).all() and np.all(ratios[:, 2] > 0) and np.all(ratios[:, 2] != 1.0)
        s = O.lamb_scalars(LR, WD, B1, B2, EPS, k)
        for i, l in enumerate(model.layers):
            na = l.cin * l.cout
            assert na < l.n, "the bucket ends in a bias segment, which takes ratio 1"
            w0, m0, v0 = (a[: l.n] for a in prev[i])
            gq = O.quantize(grads[i][: l.n_pad], "bfp_rne")[: l.n]
            assert np.abs(gq).max() > 0
            got = [a[: l.n] for a in after[i][:3]]
            rr = check_bounds(got, w0, gq, m0, v0, s, ratios[i], na, 1.0, f"step {k} fc{i}")
            check_words(ratios[i], O.lamb_ratio(w0, rr, na, LR), f"step {k} fc{i}")
            assert torch.equal(after[i][3][: l.n], torch.from_numpy(got[0]).to(torch.bfloat16))
    # the default GEMM-encoded wire: the same bits
    _, hist_p = _train(prepack=True)
    for (_, _, a, ra), (_, _, b, rb) in zip(hist, hist_p):
        assert np.array_equal(ra, rb)
        for la, lb in zip(a, b):
            for x, y in zip(la[:3], lb[:3]):
                assert np.array_equal(x, y), "prepacked run differs from the engine-encoded run"
            assert torch.equal(la[3], lb[3])


def _planes(n_pad):
    return [torch.zeros(n_pad, device=DEV) for _ in range(4)]


def test_refusals():
    C = _ext.require()
    n = 50000 - 48
    kw = dict(n_valid=n, lr=LR, opt="adamw", betas=(B1, B2), eps=EPS, step=1, trust_ratio=True)
    # a sharded-update engine (request and trainer)
    fabric = C.LoopbackFabric(2, 60.0)
    eng = NativeAllReduce(None, codec="bfp_rne", comm=fabric.comm(0), shard_update=True)
    assert eng.shard_update
    g, w, m, v = _planes(eng.layout(n).n_pad)
    with pytest.raises(ValueError, match="sharded"):
        eng.allreduce_sgd(g, w, w.to(torch.bfloat16), m, var=v, **kw)
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, adam=True, pad_fn=lambda k, e=eng: e.layout(k).n_pad)
    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, eng, optimizer="adamw", trust_ratio=True)
    # a chunked layout: a bucket above chunk_elems, and an explicit layout=(shard, chunks)
    eng = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), chunk_elems=8192)
    L = eng.layout(n)
    assert L.chunks > 1
    g, w, m, v = _planes(L.n_pad)
    with pytest.raises(ValueError, match="chunked"):
        eng.allreduce_sgd(g, w, None, m, var=v, **kw)
    eng = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0))
    g, w, m, v = _planes(eng.layout(n, 8192, 4).n_pad)
    with pytest.raises(ValueError, match="chunked"):
        eng.allreduce_sgd(g, w, None, m, var=v, layout=(8192, 4), **kw)
    # the engine itself refuses what the wrapper lets through
    with pytest.raises(RuntimeError, match="chunked"):
        eng.C.submit(g, w, None, m, n, LR, 1.0, WD, 0.0, False, False, True, None, None, 0, 8192, 4, False, opt=1,
                     var=v, adamw=O.adamw_scalars(LR, WD, B1, B2, EPS, 1).kernel_args(),
                     lamb=O.lamb_scalars(LR, WD, B1, B2, EPS, 1).kernel_args())
    # the ring's compat_owner_fp32
    eng = NativeAllReduce(None, codec="bfp_rne", algo="ring", comm=C.LoopbackFabric(2, 60.0).comm(0),
                          compat_owner_fp32=True)
    g, w, m, v = _planes(eng.layout(n).n_pad)
    with pytest.raises(ValueError, match="compat_owner_fp32"):
        eng.allreduce_sgd(g, w, None, m, var=v, **kw)
    # opt="sgd" and a bad n_adapt
    eng = NativeAllReduce(None, codec="bfp_rne")
    g, w, m, v = _planes(eng.layout(n).n_pad)
    with pytest.raises(ValueError):
        eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, trust_ratio=True)
    with pytest.raises(ValueError):
        eng.allreduce_sgd(g, w, None, m, var=v, n_adapt=n + 1, **kw)


def test_lamb_step_refuses_graph_capture(monkeypatch):
    """As AdamW's: a backward enqueued while the stream captures raises before it enqueues anything (the capture
    state is stubbed: nothing is captured here)."""
    eng = NativeAllReduce(None, codec="bfp_rne")
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, seed=3, adam=True,
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=LR, optimizer="adamw", trust_ratio=True)
    y = torch.zeros(256, dtype=torch.int32, device=DEV)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="captured"):
        tr.backward_pass(y)
    assert tr.opt_step == 0
