"""Lion in the all-reduce epilogue, on CPU: the scalars, the oracle against a textbook float64 Lion, its edge cases
(c == 0, NaN), the Python engine over virtual ranks against the spec simulator, every refusal, and the CLI's
checkpoint / resume round trip.

The float64 reference (``_lion64``) takes the request's scalars as the oracle does — computed in float64 and rounded
once to f32 (``lion_scalars``; that rounding is checked by itself in ``test_scalars_are_float64_rounded_once``) — and
then works in float64 throughout. Per step it starts from the f32 trajectory's state, so one differing sign decision
cannot spread into the later steps' comparisons; a second, free-running float64 trajectory gives the final loss.

Seeds of the noisy quadratic: data 2023 (curvature, optimum, start), noise 7. The guard leaves out an element whose
interpolated momentum cancels to below 2^-20 of its two terms; with these seeds the float64 reference's own guarded
share is 0 of 4096 at every one of the 50 steps (printed), under the 0.1 % the test allows."""
import io
import json
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fpga_ai_nic_amd.cli import mlp_mpi
from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import sim
from fpga_ai_nic_amd.parallel.allreduce import (OPTIMIZERS, CompressedAllReduce, resolve_betas,
                                                uncompressed_allreduce_sgd)
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

LR, WD, B1, B2 = 1e-3, 1e-2, 0.9, 0.99
DENORM = float(np.float32(2.0 ** -149))


def test_scalars_are_float64_rounded_once():
    s = O.lion_scalars(LR, WD, B1, B2)
    assert isinstance(s, O.LionScalars) and O.LionScalars.FIELDS == ("beta1", "omb1", "beta2", "omb2", "lr", "decay",
                                                                    "wd")
    assert all(isinstance(x, np.float32) for x in s)
    assert s.beta1 == np.float32(B1) and s.beta2 == np.float32(B2)
    assert s.omb1 == np.float32(1 - B1) and s.omb2 == np.float32(1 - B2)
    # rounded once from float64: not 1 - f32(beta), not 1 - f32(lr) * f32(wd)
    assert s.omb2 != np.float32(1) - np.float32(B2)
    assert s.lr == np.float32(LR) and s.wd == np.float32(WD)
    assert s.decay == np.float32(1 - LR * WD)
    assert s.kernel_args() == [float(x) for x in s] and len(s.kernel_args()) == 7
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(lr=float("inf")),
                dict(lr=float("nan")), dict(wd=float("inf")), dict(wd=float("nan"))):
        kw = {**dict(lr=LR, wd=WD, beta1=B1, beta2=B2), **bad}
        with pytest.raises(ValueError, match="Lion"):
            O.lion_scalars(**kw)
    assert "lion" in OPTIMIZERS
    assert resolve_betas("lion", None) == (0.9, 0.99) and resolve_betas("adamw", None) == (0.9, 0.999)
    assert resolve_betas("sgd", None) == (0.9, 0.999) and resolve_betas("lion", (0.5, 0.6)) == (0.5, 0.6)


def _lion64(w, g, m, s):
    """Textbook Lion in float64 from the request's scalars: (w', m', c, base)."""
    f = np.float64
    w, g, m = w.astype(f), g.astype(f), m.astype(f)
    c = f(s.beta1) * m + f(s.omb1) * g
    base = w * f(s.decay) if s.wd != 0 else w
    return base - f(s.lr) * np.sign(c), f(s.beta2) * m + f(s.omb2) * g, c, base


def test_oracle_against_float64_lion():
    n, steps = 4096, 50
    rng = np.random.default_rng(2023)
    h = np.exp(rng.standard_normal(n))          # curvatures over about two decades
    w_star = rng.standard_normal(n)
    w_start = w_star + rng.standard_normal(n)
    noise = np.random.default_rng(7).standard_normal((steps, n)) * 0.3
    s = O.lion_scalars(LR, WD, B1, B2)

    def loss(w):
        return float(0.5 * np.sum(h * (w.astype(np.float64) - w_star) ** 2))

    w32, m32 = w_start.astype(np.float32), np.zeros(n, np.float32)
    w64, m64 = w_start.copy(), np.zeros(n)
    worst_m = worst_w = 0.0
    for k in range(steps):
        g32 = (h.astype(np.float32) * (w32 - w_star.astype(np.float32)) + noise[k].astype(np.float32)).astype(np.float32)
        rw, rm, c, base = _lion64(w32, g32, m32, s)
        guard = np.abs(c) > 2.0 ** -20 * (np.abs(np.float64(s.beta1) * m32) + np.abs(np.float64(s.omb1) * g32))
        share = 1.0 - guard.mean()
        w2, m2 = O.lion(w32, g32, m32, s)
        moved = np.sign(w2.astype(np.float64) - base)  # the oracle's decision: which way the weight left w * decay
        assert np.array_equal(moved[guard], -np.sign(c)[guard]), f"step {k}: a sign decision differs"
        # relative to the two terms' magnitude, the scale of the guard: the f32 product omb2 * g and the fma each round
        # once (2^-24 of |omb2 g| and of |m'|), whatever cancels between the terms
        mag = np.abs(np.float64(s.beta2) * m32) + np.abs(np.float64(s.omb2) * g32)
        em = np.abs(m2.astype(np.float64) - rm) / (2.0 ** -22 * mag + DENORM)
        # base is rounded to f32 once (half an ulp of base) and the fma once more (half an ulp of w'): together one ulp
        # of the larger of the two
        ulp = np.spacing(np.maximum(np.abs(w2), np.abs(base).astype(np.float32))).astype(np.float64)
        ew = np.abs(np.abs(w2.astype(np.float64) - base) - np.float64(s.lr)) / ulp
        worst_m, worst_w = max(worst_m, float(em[guard].max())), max(worst_w, float(ew[guard].max()))
        print(f"step {k}: guarded share {share:.5f}, m' err/bound {em[guard].max():.3f}, "
              f"||w' - base| - lr| {ew[guard].max():.3f} ulp")
        assert share <= 1e-3
        assert np.all(em[guard] <= 1.0)
        assert np.all(ew[guard] <= 1.0)
        w32, m32 = w2, m2
        g64 = h * (w64 - w_star) + noise[k]
        w64, m64, _, _ = _lion64(w64, g64, m64, s)
    l32, l64 = loss(w32), loss(w64)
    print(f"final loss f32 {l32:.6f}, f64 {l64:.6f}, ratio {l32 / l64:.6f}; start {loss(w_start):.3f}; "
          f"worst m' {worst_m:.3f} of the bound, worst w' {worst_w:.3f} ulp")
    assert l64 < loss(w_start) and l32 < loss(w_start)


def test_zero_momentum_and_gradient_keep_the_weight_on_its_decay():
    s = O.lion_scalars(LR, WD, B1, B2)
    w = np.random.default_rng(3).standard_normal(64).astype(np.float32)
    z = np.zeros(64, np.float32)
    w2, m2 = O.lion(w, z, z, s)
    assert np.array_equal(w2, (w * s.decay).astype(np.float32)) and np.array_equal(m2, z)
    w2, m2 = O.lion(w, -z, z, s)  # c == -0
    assert np.array_equal(w2, (w * s.decay).astype(np.float32)) and np.all(m2 == 0)
    w2, _ = O.lion(w, z, z, O.lion_scalars(LR, 0.0, B1, B2))
    assert np.array_equal(w2, w)


def test_nan_gradient_propagates():
    s = O.lion_scalars(LR, WD, B1, B2)
    w = np.ones(8, np.float32)
    g = np.zeros(8, np.float32)
    g[3] = np.nan
    w2, m2 = O.lion(w, g, np.zeros(8, np.float32), s)
    assert np.isnan(w2[3]) and np.isnan(m2[3])
    assert np.isfinite(np.delete(w2, 3)).all() and np.isfinite(np.delete(m2, 3)).all()


def test_wire_lion_cpu_shards_skip_and_tail():
    n_s, N = 1024, 4
    n, n_valid = n_s * N, n_s * N - 77
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n).astype(np.float32)
    w0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    s = O.lion_scalars(LR, WD, B1, B2)
    buf = torch.zeros(O.shard_bytes("bfp_rne", n_s) * N, dtype=torch.uint8)
    wire.pack(torch.from_numpy(g), buf, n_s, "bfp_rne")
    w, m = (torch.from_numpy(x.copy()) for x in (w0, m0))
    lp0 = torch.full((n,), 7.0, dtype=torch.bfloat16)
    lp = lp0.clone()
    wire.lion(buf, n_s, N, w, codec="bfp_rne", mom=m, scalars=s, lp=lp, grad_scale=0.5, n_valid=n_valid,
              skip_shard=1, skip_period=4)
    rw, rm = O.lion(w0, O.quantize(g, "bfp_rne"), m0, s, 0.5)
    keep = np.zeros(n, bool)
    keep[n_valid:] = True
    keep[n_s:2 * n_s] = True
    for got, ref, old in ((w, rw, w0), (m, rm, m0)):
        assert np.array_equal(got.numpy()[keep], old[keep])
        assert np.array_equal(got.numpy()[~keep], ref[~keep])
    k = torch.from_numpy(keep)
    assert torch.equal(lp[k], lp0[k])
    assert torch.equal(lp[~k], torch.from_numpy(rw).to(torch.bfloat16)[~k])
    words = torch.tensor([0.37, 0, 0, 0])
    a, b = [torch.from_numpy(x.copy()) for x in (w0, m0)], [torch.from_numpy(x.copy()) for x in (w0, m0)]
    wire.lion(buf, n_s, N, a[0], codec="bfp_rne", mom=a[1], scalars=s, grad_scale=0.5, clip=words)
    wire.lion(buf, n_s, N, b[0], codec="bfp_rne", mom=b[1], scalars=s, grad_scale=O.clip_scale(0.5, words.numpy()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="moment plane"):
        wire.lion(buf, n_s, N, w, codec="bfp_rne", mom=None, scalars=s)
    with pytest.raises(TypeError, match="lion_scalars"):
        wire.lion(buf, n_s, N, w, codec="bfp_rne", mom=m, scalars=O.adamw_scalars(LR, WD, B1, B2, 1e-8, 1))


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
@pytest.mark.parametrize("codec", ["bfp_rne", "bfp4_rne"])
def test_python_engine_virtual_ranks(N, algo, codec):
    n = 3000
    rng = np.random.default_rng(N * 7 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = ThreadFabric(N, timeout_s=60)

    def fn(t):
        eng = CompressedAllReduce(t, codec=codec, algo=algo, max_slice_elems=512, device="cpu")
        L = eng.layout(n)
        w, m = torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        lp = torch.zeros(L.n_pad, dtype=torch.bfloat16)
        w[:n] = torch.from_numpy(w0)
        for step in (1, 2):
            g = torch.zeros(L.n_pad)
            g[:n] = torch.from_numpy(grads[step - 1][t.rank])
            # step is ignored when given; betas left unset resolve to Lion's (0.9, 0.99)
            eng.allreduce_sgd(g, w, lp, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N, opt="lion",
                              step=step if step == 2 else None).synchronize()
        return w.numpy().copy(), m.numpy().copy(), lp.clone(), L, eng.orders

    res = fabric.run(fn)
    L, orders = res[0][3], res[0][4]
    rw, rm = w0, np.zeros(n, np.float32)
    s = O.lion_scalars(LR, WD, 0.9, 0.99)
    for step in (1, 2):
        gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step - 1]]
        red = sim.mesh_allreduce(gin, L.shard, codec) if algo == "mesh" else \
            sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, codec)[0]
        rw, rm = O.lion(rw, red[:n], rm, s, 1.0 / N)
    assert np.any(rm != 0) and not np.array_equal(rw, w0)
    for r in range(N):
        for got, ref in zip(res[r][:2], (rw, rm)):
            assert np.array_equal(got[:n], ref)
            assert np.all(got[n:] == 0), "padding untouched"
        assert torch.equal(res[r][2][:n], torch.from_numpy(rw).to(torch.bfloat16))
        assert torch.all(res[r][2][n:] == 0)
        for a, b in zip(res[r][:2], res[0][:2]):
            assert np.array_equal(a, b), "ranks identical"


def test_engine_refusals():
    t = ThreadFabric(1).transport(0)
    eng = CompressedAllReduce(t, device="cpu")
    n = eng.layout(100).n_pad
    g, w, m, v = (torch.zeros(n) for _ in range(4))
    ok = dict(n_valid=100, lr=LR, opt="lion")
    eng.allreduce_sgd(g, w, None, m, **ok).synchronize()
    for mom, kw, match in ((None, {}, "needs its moment plane"),
                           (m.double(), {}, "contiguous float32"),
                           (torch.zeros(2 * n)[::2], {}, "contiguous float32"),
                           (m, dict(var=v), "var must be None"),
                           (m, dict(momentum=0.9), "belong to SGD"),
                           (m, dict(nesterov=True), "belong to SGD"),
                           (m, dict(trust_ratio=True), "flag of opt='adamw'"),
                           (m, dict(n_adapt=10), "trust_ratio"),
                           (m, dict(moment_codec="bfp8", moment_seed=1), "AdamW only"),
                           (m, dict(betas=(1.0, 0.99)), r"\[0, 1\)"),
                           (m, dict(lr=float("nan")), "finite"),
                           (m, dict(weight_decay=float("inf")), "finite")):
        with pytest.raises(ValueError, match=match):
            eng.allreduce_sgd(g, w, None, mom, **{**ok, **kw})
    with pytest.raises(ValueError, match="uncompressed baseline"):
        uncompressed_allreduce_sgd(t, g, w, None, m, lr=LR, opt="lion")
    # the defaults of the other optimizers are today's
    eng.allreduce_sgd(g, w, None, m, n_valid=100, lr=LR, opt="adamw", var=v, step=1).synchronize()
    ref = O.adamw(np.zeros(100, np.float32), np.zeros(100, np.float32), np.zeros(100, np.float32),
                  np.zeros(100, np.float32), O.adamw_scalars(LR, 0.0, 0.9, 0.999, 1e-8, 1))
    assert np.array_equal(v.numpy()[:100], ref[2])


def test_trainer_refusals_and_engine_less_update():
    sizes = [32, 64, 32]
    with pytest.raises(ValueError, match=r"MLP\(\.\.\., momentum=True\)"):
        DataParallelTrainer(MLP(sizes, dtype=torch.float32), None, optimizer="lion")
    with pytest.raises(ValueError, match="momentum=True"):
        DataParallelTrainer(MLP(sizes, dtype=torch.float32, adam=True), None, optimizer="lion")
    mk = lambda: MLP(sizes, dtype=torch.float32, seed=3, momentum=True)  # noqa: E731
    for kw, match in ((dict(trust_ratio=True), "flag of optimizer='adamw'"),
                      (dict(moment_codec="bfp8"), "optimizer='adamw' only"),
                      (dict(momentum=0.9), "belong to SGD"), (dict(nesterov=True), "belong to SGD"),
                      (dict(betas=(0.9, 1.0)), r"\[0, 1\)")):
        with pytest.raises(ValueError, match=match):
            DataParallelTrainer(mk(), None, optimizer="lion", **kw)
    model = mk()
    tr = DataParallelTrainer(model, None, lr=1e-2, weight_decay=WD, optimizer="lion")
    assert tr.betas == (0.9, 0.99) and tr.fused_update is False
    adam = MLP(sizes, dtype=torch.float32, adam=True)
    assert DataParallelTrainer(adam, None, optimizer="adamw").betas == (0.9, 0.999)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(16, sizes[0], generator=g) * 2 - 1
    Y = torch.randint(0, sizes[-1], (16,), generator=g, dtype=torch.int32)
    s = O.lion_scalars(1e-2, WD, 0.9, 0.99)
    for _ in range(2):
        prev = [(l.master.numpy().copy(), l.mom.numpy().copy()) for l in model.layers]
        tr.step(X, Y)
        tr.finish()
        for l, (w0, m0) in zip(model.layers, prev):
            rw, rm = O.lion(w0[: l.n], l.grad.numpy()[: l.n], m0[: l.n], s)
            assert np.array_equal(l.master.numpy()[: l.n], rw) and np.array_equal(l.mom.numpy()[: l.n], rm)
            assert np.any(rm != 0)
    assert tr.fused_updates == 0
    # with clipping, error feedback and stochastic rounding: they act before the update
    for kw in (dict(max_grad_norm=0.5), dict(error_feedback=True), dict(stochastic_rounding=True, sr_seed=3)):
        t2 = DataParallelTrainer(mk(), None, lr=1e-2, optimizer="lion", **kw)
        assert np.isfinite(float(t2.step(X, Y).mean()))
        t2.finish()


_CLI = ["32", "0", "A", "1", "1", "1", "128", "256", "128", "--device", "cpu", "--dtype", "f32", "--warmup", "0",
        "--optimizer", "lion", "--lr", "1e-3", "--weight-decay", "1e-2"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cli_worker(rank, world, port, argv, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    try:
        r = mlp_mpi.run(argv, out=io.StringIO())
        q.put((rank, float(r["loss"]) if r and "loss" in r else None, None))
    except BaseException as e:  # noqa: BLE001 - reported to the parent, which must never wait for a missing result
        q.put((rank, None, repr(e)))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _run2(argv, world=2):
    """The CLI over ``world`` gloo ranks (one process each)."""
    q = mp.get_context("spawn").SimpleQueue()
    pc = mp.start_processes(_cli_worker, args=(world, _free_port(), argv, q), nprocs=world, join=False,
                            start_method="spawn")
    got, deadline = [], time.monotonic() + 120
    while len(got) < world:
        if not q.empty():
            got.append(q.get())
        elif pc.join(0.05):
            while not q.empty():
                got.append(q.get())
            break
        assert time.monotonic() < deadline, "CLI ranks hung"
    while not pc.join(0.05):
        assert time.monotonic() < deadline, "CLI ranks hung"
    assert len(got) == world and not [e for _, _, e in got if e], got
    return got


def test_cli_lion_checkpoint_resume_bit_identical(tmp_path):
    """Two gloo ranks: checkpoint at iteration 3, resume, iteration 4 equals the uninterrupted run's bit for bit."""
    full, part, rest = (str(tmp_path / k) for k in ("full", "part", "rest"))
    _run2(["4"] + _CLI + ["--checkpoint", full])
    _run2(["3"] + _CLI + ["--checkpoint", part])
    _run2(["1"] + _CLI + ["--resume", part, "--checkpoint", rest])
    from safetensors.torch import load_file

    a, b = load_file(full + ".safetensors"), load_file(rest + ".safetensors")
    assert sorted(a) == sorted(b)
    assert {"fc0.momentum", "fc1.momentum"} <= set(a) and not any("exp_avg" in k for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["fc0.momentum"].abs().max()) > 0
    ia, ip, ib = (json.load(open(p + ".json")) for p in (full, part, rest))
    assert ia["optimizer"] == "lion" and ip["optimizer"] == "lion" and ib["iteration"] == 4
    with pytest.raises(ValueError, match="written under optimizer='lion'"):
        mlp_mpi.run(["1"] + [x if x != "lion" else "adamw" for x in _CLI] + ["--resume", part], out=io.StringIO())
    with pytest.raises(ValueError, match="written under optimizer='lion'"):
        mlp_mpi.run(["1"] + [x if x != "lion" else "sgd" for x in _CLI] + ["--momentum", "0.9", "--resume", part],
                    out=io.StringIO())
