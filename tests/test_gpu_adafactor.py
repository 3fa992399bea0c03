"""Adafactor in the all-reduce epilogues on the GPU: the op ``wire.adafactor`` against the NumPy oracle at the shapes
where its tiling can go wrong, grid independence, the C++ engine on the schedules one device can run (the direct-P2P
mesh branch needs two and is not exercised), the trainer."""
import math
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from fpga_ai_nic_amd import _ext  # noqa: E402
from fpga_ai_nic_amd.models.mlp import MLP  # noqa: E402
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402
from fpga_ai_nic_amd.parallel import sim  # noqa: E402
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer  # noqa: E402
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce  # noqa: E402
from fpga_ai_nic_amd.parallel.transport import NativeTransport  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, WD, GS, SENT = 1e-2, 1e-2, 0.5, 12288.0  # (the sentinel is exact in bf16)


def _shapes():
    """(rows, cols, shard_elems, n_shards, tail) with the kernel's own panel and strip: one group; a row across the
    shard boundary plus a tail; a second column strip one group wide with n_valid inside a group of the tail; three row
    panels, the last one short."""
    lay = wire.adafactor_layout(1, 16, 16)
    panel, strip = lay["panel"], lay["strip"]
    return {"1x16": (1, 16, 256, 1, 0), "cross": (40, 48, 1024, 2, 48),
            "strip": (16, strip + 16, (16 * (strip + 16) + 512) // 512 * 256, 2, 100),
            "panels": (2 * panel + 3, 32, 256 * math.ceil((2 * panel + 3) * 32 / 256 + 1), 1, 37)}


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _run(shape, codec, steps=2, max_blocks=0, check=True):
    rows, cols, n_s, n_shards, tail = _shapes()[shape]
    n_adapt, n = rows * cols, rows * cols + tail
    state = rows + cols + tail
    rng = np.random.default_rng(7)
    lay = wire.adafactor_layout(rows, cols, n)
    # every buffer is a slice of a larger one filled with a sentinel: what lies behind it must stay
    big = {k: torch.full((sz + 64,), SENT, dtype=dt, device=DEV)
           for k, sz, dt in (("w", n, torch.float32), ("lp", n, torch.bfloat16), ("fac", state, torch.float32),
                             ("ab", state, torch.float32), ("words", 4, torch.float32),
                             ("partials", lay["length"], torch.float64))}
    w, lp, fac, ab, words, partials = (b[: b.numel() - 64] for b in big.values())
    w.copy_(torch.from_numpy(rng.standard_normal(n).astype(np.float32)))
    fac.zero_()
    out = []
    for step in range(1, steps + 1):
        g = (rng.standard_normal(n_s * n_shards) * np.exp(rng.standard_normal(n_s * n_shards))).astype(np.float32)
        raw = O.pack(g, n_s, codec)
        s = O.adafactor_scalars(LR, WD, step)
        w0, fac0 = w.cpu().numpy().copy(), fac.cpu().numpy().copy()
        wire.adafactor(torch.from_numpy(raw).to(DEV), n_s, n_shards, w, fac, codec=codec, rows=rows, cols=cols,
                       scalars=s, lp=lp, grad_scale=GS, n_valid=n, words=words, ab=ab, partials=partials,
                       max_blocks=max_blocks)
        torch.cuda.synchronize()
        got = dict(w=w.cpu().numpy(), fac=fac.cpu().numpy(), ab=ab.cpu().numpy(), words=words.cpu().numpy(),
                   lp=lp.cpu(), partials=partials.cpu().numpy())
        out.append(got)
        for k, b in big.items():
            assert bool((b[-64:] == SENT).all()), f"{k}: bytes behind the buffer were written"
        if not check:
            continue
        gd = O.unpack(raw, n_s * n_shards, n_s, codec)
        g2, rowmean, colmean, s_tail = O.adafactor_stats(gd, rows, cols, n, GS)
        # the sums before rounding, rebuilt from the tiles' partials, against math.fsum
        P = got["partials"]
        col = P[lay["col"]: lay["col"] + lay["panels"] * cols].reshape(lay["panels"], cols)
        row = P[lay["row"]: lay["row"] + lay["strips"] * rows].reshape(lay["strips"], rows)
        csum, rsum = col.sum(0), row.sum(0)
        assert np.all(np.abs(csum - colmean * rows) <= rows * 2.0 ** -52 * colmean * rows)
        assert np.all(np.abs(rsum - rowmean * cols) <= cols * 2.0 ** -52 * rowmean * cols)
        rfac, rab = O.adafactor_factors(fac0, rowmean, colmean, s_tail, s)
        assert _ulps(got["fac"], rfac).max() <= 1, "R', C', V' within 1 ulp"
        assert _ulps(got["ab"], rab).max() <= 2, "a, b, a_tail within 2 ulp"
        # u^2 sums from the kernel's own a | b (so their 2 ulp do not enter), tile partials in order
        u, sm, st = O.adafactor_rms(g2, got["ab"], rows, cols)
        nt = lay["panels"] * lay["strips"]
        tm, tt = sum(P[lay["rms"]: lay["rms"] + nt].tolist()), sum(P[lay["rms"] + nt:][: lay["tail_tiles"]].tolist())
        assert abs(tm - sm) <= n_adapt * 2.0 ** -52 * sm and abs(tt - st) <= max(tail, 1) * 2.0 ** -52 * st
        rwords = O.adafactor_scale(sm, n_adapt, st, tail, s)
        assert _ulps(got["words"], rwords).max() <= 2
        # w' = fma(-scale, u, base): scale, a and b are within 2 ulp each and each of u's two products rounds once, so
        # scale * u is within (2 + 2 + 1 + 2 + 1) = 8 ulp relative of the oracle's (from the kernel's own ab: 4), and
        # the fma rounds once more on either side: 8 * 2^-23 * |scale * u| + 1 ulp(w').
        rw = O.adafactor_apply(w0, u, got["words"], n_adapt, s)
        su = np.abs(np.where(np.arange(n) < n_adapt, got["words"][0], got["words"][2]).astype(np.float64) * u)
        assert np.all(np.abs(got["w"].astype(np.float64) - rw) <= 8 * 2.0 ** -23 * su + np.spacing(np.abs(rw)))
        assert torch.equal(got["lp"], torch.from_numpy(got["w"]).to(torch.bfloat16))
    return out


@pytest.mark.parametrize("shape,codec", [(s, "bfp_rne") for s in ("1x16", "cross", "strip", "panels")] +
                         [("cross", c) for c in ("bfp_trunc", "bfp4_rne", "raw_f32", "raw_bf16")])
def test_op_against_the_oracle(shape, codec):
    _run(shape, codec)


@pytest.mark.parametrize("shape", ["strip", "panels"])
def test_bits_do_not_depend_on_the_grid(shape):
    a, b = _run(shape, "bfp_rne", check=False), _run(shape, "bfp_rne", max_blocks=1, check=False)
    for x, y in zip(a, b):
        assert all(np.array_equal(x[k], y[k]) for k in ("w", "fac", "ab", "words")) and torch.equal(x["lp"], y["lp"])


# --------------------------------------------------------------------------- engines
ROWS, COLS, TAIL, N_EL = 72, 208, 200, 72 * 208 + 200


def _two_steps(eng, L, N, w0, grads, r):
    """Two updates on rank r's engine, or (eng None) by the op on the simulator's gathered wire."""
    w = torch.zeros(L.n_pad, device=DEV)
    w[:N_EL] = torch.from_numpy(w0)
    lp = torch.zeros(L.n_pad, device=DEV, dtype=torch.bfloat16)
    fac, words = torch.zeros(ROWS + COLS + TAIL, device=DEV), torch.zeros(4, device=DEV)
    snaps = []
    for step in (1, 2):
        if eng is None:
            red = sim.mesh_allreduce([np.pad(g, (0, L.n_pad - N_EL)) for g in grads[step - 1]], L.shard, "bfp_rne")
            G = torch.from_numpy(O.pack(red, L.shard, "bfp_rne")).to(DEV)
            wire.adafactor(G, L.shard, L.n_pad // L.shard, w, fac, codec="bfp_rne", rows=ROWS, cols=COLS, lp=lp,
                           scalars=O.adafactor_scalars(LR, WD, step), grad_scale=1.0 / N, n_valid=N_EL, words=words)
        else:
            g = torch.zeros(L.n_pad, device=DEV)
            g[:N_EL] = torch.from_numpy(grads[step - 1][r])
            torch.cuda.synchronize()
            h = eng.allreduce_sgd(g, w, lp, n_valid=N_EL, lr=LR, weight_decay=WD, grad_scale=1.0 / N, opt="adafactor",
                                  fac=fac, rows=ROWS, cols=COLS, step=step, adafactor_out=words, defer=True)
            h.commit_after_current()
            h.synchronize(60)
        torch.cuda.synchronize()
        snaps.append([t.cpu().numpy().copy() for t in (w, fac, words, lp.float())])
    return snaps


def _same(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


def _data(N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N_EL).astype(np.float32), \
        [[rng.standard_normal(N_EL).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]


@pytest.mark.parametrize("N", [2, 3])
def test_native_engine_loopback(N):
    w0, grads = _data(N, 40 + N)
    fabric = _ext.require().LoopbackFabric(N, 60.0)
    engines = [NativeAllReduce(None, comm=fabric.comm(r), codec="bfp_rne", algo="mesh") for r in range(N)]
    L = engines[0].layout(N_EL)
    out, errs = [None] * N, []

    def run(r):
        try:
            out[r] = _two_steps(engines[r], L, N, w0, grads, r)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(r,)) for r in range(N)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts) and not errs, errs
    assert all(_same(out[r], out[0]) for r in range(1, N)), "replicas must be bit-identical"
    assert _same(out[0], _two_steps(None, L, N, w0, grads, 0)), "engine differs from the op on the simulated wire"
    assert np.any(out[0][1][1] != out[0][0][1]) and np.all(out[0][1][0][N_EL:] == 0)


@pytest.mark.parametrize("path", ["inline", "forced"])
def test_one_rank_engine(path):
    w0, grads = _data(1, 50)
    if path == "inline":
        eng = NativeAllReduce(None, codec="bfp_rne")
        assert eng.inline
    else:
        store = type("Store", (dict,), {"set": dict.__setitem__, "get": dict.__getitem__})()
        tp = NativeTransport(rank=0, world=1, device=0, store=store, force_collectives=True)
        eng = NativeAllReduce(tp, codec="bfp_rne", force_comm=True)
    L = eng.layout(N_EL)
    assert _same(_two_steps(eng, L, 1, w0, grads, 0), _two_steps(None, L, 1, w0, grads, 0))


def _train(native):
    sizes, mb = [256, 512, 256], 256
    eng = NativeAllReduce(None, codec="raw_f32") if native else None
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3,
                pad_fn=(lambda n: eng.layout(n).n_pad) if native else None)
    tr = DataParallelTrainer(model, eng, lr=LR, weight_decay=WD, optimizer="adafactor")
    assert tr.fused_update is False
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=gen) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=gen, dtype=torch.int32).to(DEV)
    hist = []
    for _ in range(2):
        tr.step(x, y)
        tr.finish()
        torch.cuda.synchronize()
        hist.append([[l.master[: l.n].cpu().numpy().copy(), l.fac.cpu().numpy().copy(),
                      l.lp[: l.n].float().cpu().numpy().copy()] for l in model.layers] +
                    [[tr.adafactor_words.cpu().numpy().copy()]])
    return hist


def test_trainer_two_steps_against_the_engineless_trainer():
    """raw_f32 on the wire (the engine-less update reads the f32 gradient itself): bit for bit."""
    a, b = _train(True), _train(False)
    assert all(np.array_equal(x, y) for sa, sb in zip(a, b) for la, lb in zip(sa, sb) for x, y in zip(la, lb))
    assert np.all(a[-1][-1][0][:, 0] > 0) and not np.array_equal(a[0][0][0], a[1][0][0])


def test_refusals_from_cpp():
    a = O.adafactor_scalars(LR, WD, 1).kernel_args()
    g, w, m = (torch.zeros(1 << 16, device=DEV) for _ in range(3))  # (above every layout's n_pad)
    fac = torch.zeros(ROWS + COLS + TAIL, device=DEV)

    def submit(eng, mom=None, update=True, layout=(0, 0), **kw):
        return eng.C.submit(g, w, None, mom, N_EL, LR, 1.0, 0.0, 0.0, False, True, update, None, None, 0, *layout, False,
                            **{**dict(opt=3, adafactor=a, fac=fac, rows=ROWS, cols=COLS), **kw})

    mesh = NativeAllReduce(None, codec="bfp_rne")
    slot = submit(mesh)
    mesh.C.commit(slot)
    mesh.C.synchronize(slot, 60.0)
    for kw, match in ((dict(cols=COLS + 8, rows=ROWS - 3), "multiple of 16"), (dict(rows=ROWS + 1), "exceed n_valid"),
                      (dict(fac=fac[:-1]), "exactly rows"), (dict(mom=m), "no moment plane"),
                      (dict(var=m), "no moment plane"), (dict(adafactor=a[:6]), "7 scalars"),
                      (dict(adafactor=None), "needs its scalars"), (dict(fac=None), "needs its state"),
                      (dict(clip=m[:4]), "clip: not with Adafactor"), (dict(fac=fac.double()), "float32"),
                      (dict(lamb=O.lamb_scalars(LR, 0, 0.9, 0.999, 1e-8, 1).kernel_args()), "trust ratio"),
                      (dict(mom_q=wire.moment_plane(256, DEV), var_q=wire.moment_plane(256, DEV)), "AdamW only"),
                      (dict(update=False), "update requests only"), (dict(layout=(8192, 2)), "chunked layout")):
        with pytest.raises(RuntimeError, match=match):
            submit(mesh, **kw)
    fabric = _ext.require().LoopbackFabric(2, 60.0)  # (a refused request takes no slot: rank 0 alone submits)
    for ekw, match in ((dict(algo="ring"), "mesh schedule only"),
                       (dict(comm=fabric.comm(0), shard_update=True), "sharded update"),
                       (dict(compat_owner_fp32=True), "compat_owner_fp32")):
        with pytest.raises(RuntimeError, match=match):
            submit(NativeAllReduce(None, codec="bfp_rne", **ekw))
