"""Adafactor (opt="adafactor") without a GPU: the oracle against a textbook float64 Adafactor, the Python engine over
ThreadFabric against the oracle on the simulator's reduced gradient, the refusals, the checkpoint."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from fpga_ai_nic_amd.models.mlp import MLP  # noqa: E402
from fpga_ai_nic_amd.ops import bfp_oracle as O  # noqa: E402
from fpga_ai_nic_amd.ops import wire  # noqa: E402
from fpga_ai_nic_amd.parallel import sim  # noqa: E402
from fpga_ai_nic_amd.parallel.allreduce import (CompressedAllReduce, adafactor_request,  # noqa: E402
                                                 uncompressed_allreduce_sgd)
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer  # noqa: E402
from fpga_ai_nic_amd.parallel.transport import ThreadFabric  # noqa: E402
from fpga_ai_nic_amd.utils import checkpoint  # noqa: E402

ROWS, COLS, TAIL, N, LR, WD = 12, 32, 9, 12 * 32 + 9, 5e-2, 1e-2


def _textbook(w, g, R, C, V, step, lr, wd, d=1.0, eps1=1e-30):
    """Adafactor (Shazeer & Stern 2018, Algorithm 4 without a first moment, absolute lr, decoupled decay), float64."""
    b2 = 1.0 - step ** -0.8
    W, G = w[: ROWS * COLS].reshape(ROWS, COLS), g[: ROWS * COLS].reshape(ROWS, COLS)
    R = b2 * R + (1 - b2) * (G * G + eps1).mean(1)
    C = b2 * C + (1 - b2) * (G * G + eps1).mean(0)
    V = b2 * V + (1 - b2) * (g[ROWS * COLS:] ** 2 + eps1)
    U = G / np.sqrt(np.outer(R, C) / R.mean())
    ut = g[ROWS * COLS:] / np.sqrt(V)
    U = U / max(1.0, np.sqrt((U * U).mean()) / d)
    ut = ut / max(1.0, np.sqrt((ut * ut).mean()) / d)
    return np.concatenate([(W * (1 - lr * wd) - lr * U).reshape(-1), w[ROWS * COLS:] * (1 - lr * wd) - lr * ut]), R, C, V


def test_oracle_against_textbook_float64():
    """A noisy quadratic 0.5 |w - t|^2, 40 steps. Per step the oracle rounds to f32: g * grad_scale, each state element,
    a and b (+ the state's half power each), u's two products, the scale (+ the state's through the rms), then the decay
    product and the fma on |w| <= 4: <= 12 roundings of 2^-24 on lr * |u| <= lr * sqrt(ROWS * COLS), 2 on |w|. That the
    steps' errors add up without growing (w -> w' contracts on this quadratic) is assumed, not derived; the bound is
    steps * 2^-24 * (12 * lr * sqrt(n) + 2 * 4). The losses' tolerance, 1e-4 relative, is a chosen number."""
    rng = np.random.default_rng(0)
    t = rng.standard_normal(N)
    w64 = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    w32 = w64.astype(np.float32)
    R, C, V = np.zeros(ROWS), np.zeros(COLS), np.zeros(TAIL)
    fac = np.zeros(ROWS + COLS + TAIL, np.float32)
    steps = 40
    for step in range(1, steps + 1):
        noise = 0.1 * rng.standard_normal(N)
        g = ((w32.astype(np.float64) - t) + noise).astype(np.float32)  # one gradient for both: the f32 run's
        w32, fac, words, _ = O.adafactor(w32, g, fac, ROWS, COLS, O.adafactor_scalars(LR, WD, step))
        w64, R, C, V = _textbook(w64, g.astype(np.float64), R, C, V, step, LR, WD)
    bound = steps * 2.0 ** -24 * (12 * LR * np.sqrt(ROWS * COLS) + 8)
    assert np.abs(w32 - w64).max() <= bound
    ref = np.concatenate([R, C, V])
    assert np.all(np.abs(fac - ref) <= steps * 2.0 ** -24 * ref + 1e-30)
    loss = [0.5 * np.sum((x - t) ** 2) for x in (w32.astype(np.float64), w64)]
    assert abs(loss[0] - loss[1]) <= 1e-4 * loss[1] and loss[1] < 0.5 * np.sum((rng.standard_normal(N) - t) ** 2)
    assert words[0] <= np.float32(LR) and O.adafactor_scalars(LR, WD, 1).beta2 == 0.0
    g[5], g[-1] = np.nan, np.nan  # a non-finite gradient propagates NaN into its tensor's state and weights
    wn, fn, _, _ = O.adafactor(w32, g, fac, ROWS, COLS, O.adafactor_scalars(LR, WD, steps + 1))
    assert np.isnan(wn).all() and np.isnan(fn[[0, ROWS + 5, -1]]).all()


@pytest.mark.parametrize("world", [1, 2])
def test_python_engine_against_the_oracle(world):
    rng = np.random.default_rng(world)
    w0 = rng.standard_normal(N).astype(np.float32)
    grads = [[rng.standard_normal(N).astype(np.float32) * (1 + r) for r in range(world)] for _ in range(2)]
    res = [None] * world

    def rank(t):
        eng = CompressedAllReduce(t, codec="bfp_rne")
        L = eng.layout(N)
        w = torch.zeros(L.n_pad)
        w[:N] = torch.from_numpy(w0)
        lp = torch.zeros(L.n_pad, dtype=torch.bfloat16)
        fac, words = torch.zeros(ROWS + COLS + TAIL), torch.zeros(4)
        snaps = []
        for step in (1, 2):
            g = torch.zeros(L.n_pad)
            g[:N] = torch.from_numpy(grads[step - 1][t.rank])
            eng.allreduce_sgd(g, w, lp, n_valid=N, lr=LR, weight_decay=WD, grad_scale=1.0 / world, opt="adafactor",
                              fac=fac, rows=ROWS, cols=COLS, step=step, adafactor_out=words).wait()
            snaps.append((w.numpy().copy(), fac.numpy().copy(), words.numpy().copy(), lp.clone()))
        res[t.rank] = (snaps, L)

    ThreadFabric(world, timeout_s=60).run(rank)
    snaps, L = res[0]
    w, fac = w0, np.zeros(ROWS + COLS + TAIL, np.float32)
    for step in (1, 2):
        red = sim.mesh_allreduce([np.pad(g, (0, L.n_pad - N)) for g in grads[step - 1]], L.shard, "bfp_rne")
        w, fac, words, _ = O.adafactor(w, red[:N], fac, ROWS, COLS, O.adafactor_scalars(LR, WD, step), 1.0 / world)
        for r in range(world):
            gw, gf, gwords, glp = res[r][0][step - 1]
            assert np.array_equal(gw[:N], w) and np.array_equal(gf, fac) and np.array_equal(gwords, words)
            assert np.all(gw[N:] == 0) and torch.equal(glp[:N], torch.from_numpy(w).to(torch.bfloat16))


def test_refusals():
    eng = CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne")
    L = eng.layout(N)
    g, w, m = torch.zeros(L.n_pad), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
    fac = torch.zeros(ROWS + COLS + TAIL)
    ok = dict(n_valid=N, lr=LR, opt="adafactor", fac=fac, rows=ROWS, cols=COLS, step=1)
    eng.allreduce_sgd(g, w, None, **ok).wait()
    for kw, match in ((dict(cols=24, rows=16), "multiple of 16"), (dict(rows=ROWS + 1), "exceeds n_valid"),
                      (dict(fac=fac.double()), "contiguous float32"), (dict(fac=fac.repeat(2)[::2]), "contiguous"),
                      (dict(fac=fac[:-1]), "exactly rows"), (dict(fac=None), "needs its state"),
                      (dict(var=m), "no moment plane"), (dict(momentum=0.9), "belong to SGD"),
                      (dict(nesterov=True), "belong to SGD"), (dict(betas=(0.9, 0.99)), "betas belong"),
                      (dict(trust_ratio=True), "flag of opt='adamw'"),
                      (dict(moment_codec="bfp8", moment_seed=1), "AdamW only"),
                      (dict(clip=torch.zeros(4), defer=True), "clip / max_grad_norm"), (dict(step=0), "1-based"),
                      (dict(step=None), "needs step"), (dict(lr=float("nan")), "must be finite"),
                      (dict(weight_decay=float("inf")), "must be finite")):
        with pytest.raises(ValueError, match=match):
            eng.allreduce_sgd(g, w, None, **{**ok, **kw})
    with pytest.raises(ValueError, match="belong to opt='adafactor'"):
        eng.allreduce_sgd(g, w, None, n_valid=N, lr=LR, fac=fac)
    for ekw, match in ((dict(algo="ring"), "mesh schedule only"), (dict(compat_owner_fp32=True), "compat_owner_fp32")):
        with pytest.raises(ValueError, match=match):
            CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", **ekw).allreduce_sgd(g, w, None, **ok)
    for kw, match in ((dict(chunks=2), "chunked layout"), (dict(sharded=True), "sharded update"),
                      (dict(mom=m), "no moment plane")):
        with pytest.raises(ValueError, match=match):  # (layouts and engines the Python engine cannot build on a CPU)
            adafactor_request(fac, ROWS, COLS, N, lr=LR, weight_decay=0.0, step=1, **kw)
    with pytest.raises(ValueError, match="compressed engines"):
        uncompressed_allreduce_sgd(ThreadFabric(1).transport(0), g, w, n_valid=N, lr=LR, opt="adafactor")
    with pytest.raises(ValueError, match="max_grad_norm"):
        DataParallelTrainer(MLP([32, 32, 16], dtype=torch.float32), None, optimizer="adafactor", max_grad_norm=1.0)
    with pytest.raises(TypeError, match="adafactor_scalars"):
        wire.adafactor(torch.zeros(272, dtype=torch.uint8), 256, 1, w, fac, codec="bfp_rne", rows=ROWS, cols=COLS,
                       scalars=O.lion_scalars(LR, 0, 0.9, 0.99), n_valid=N)


def test_checkpoint_round_trip(tmp_path):
    """Three steps straight through against two steps, save, load into a fresh model, one more step: bit-identical."""
    sizes, mb = [32, 48, 16], 8
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(mb, sizes[0], generator=gen) * 2 - 1
    y = torch.randint(0, sizes[-1], (mb,), generator=gen, dtype=torch.int32)
    a = MLP(sizes, dtype=torch.float32, seed=5)
    ta = DataParallelTrainer(a, None, lr=LR, weight_decay=WD, optimizer="adafactor")
    for _ in range(2):
        ta.step(x, y)
        ta.finish()
    path = str(tmp_path / "ck")
    checkpoint.save(path, a, iteration=2, optimizer="adafactor", opt_step=ta.opt_step)
    ta.step(x, y)
    ta.finish()
    b = MLP(sizes, dtype=torch.float32, seed=9)
    info = checkpoint.load(path, b, optimizer="adafactor")
    assert info["optimizer"] == "adafactor" and info["opt_step"] == 2
    tb = DataParallelTrainer(b, None, lr=LR, weight_decay=WD, optimizer="adafactor")
    tb.opt_step = info["opt_step"]
    tb.step(x, y)
    tb.finish()
    for la, lb in zip(a.layers, b.layers):
        assert torch.equal(la.master, lb.master) and torch.equal(la.fac, lb.fac) and bool(la.fac.abs().sum() > 0)
    with pytest.raises(ValueError, match="written under optimizer='adafactor'"):
        checkpoint.load(path, MLP(sizes, dtype=torch.float32), optimizer="sgd")
