"""AdamW in the all-reduce epilogue, on CPU: the oracle against torch.optim.AdamW, wire.adamw's shard / skip / tail
handling, the Python engine over virtual ranks against the spec simulator, the trainer over gloo, the CLI's
checkpoint / resume round trip, and argument validation."""
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
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce, uncompressed_allreduce_sgd
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
from fpga_ai_nic_amd.parallel.transport import ThreadFabric, TorchDistTransport
from fpga_ai_nic_amd.utils import checkpoint

LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8


def test_scalars_are_float64_rounded_once():
    s = O.adamw_scalars(LR, WD, B1, B2, EPS, 7)
    assert all(isinstance(x, np.float32) for x in s)
    assert s.step_size == np.float32(LR / (1 - B1 ** 7))
    assert s.rsbc2 == np.float32(1 / np.sqrt(1 - B2 ** 7))
    assert s.decay == np.float32(1 - LR * WD)
    assert s.omb1 == np.float32(1 - B1) and s.omb2 == np.float32(1 - B2)
    assert s.kernel_args() == [float(x) for x in s[:8]]


def test_oracle_against_torch_adamw():
    """The oracle stays within 4x the error torch's own float32 AdamW has against float64 (the operation order
    differs: lerp and addcdiv in torch, fma here)."""
    n, steps = 4096, 20
    g = torch.Generator().manual_seed(11)
    w0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(steps)]

    def run_torch(dtype):
        p = torch.nn.Parameter(w0.to(dtype).clone())
        opt = torch.optim.AdamW([p], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
        for gr in grads:
            p.grad = gr.to(dtype).clone()
            opt.step()
        return p.detach().to(torch.float64).numpy()

    truth = run_torch(torch.float64)
    yardstick = np.abs(run_torch(torch.float32) - truth).max()
    w = w0.numpy().copy()
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    for t, gr in enumerate(grads, 1):
        w, m, v = O.adamw(w, gr.numpy(), m, v, O.adamw_scalars(LR, WD, B1, B2, EPS, t))
    err = np.abs(w.astype(np.float64) - truth).max()
    print(f"torch f32 vs f64: {yardstick:.3e}; oracle vs f64: {err:.3e}")
    assert yardstick > 0
    assert err <= 4 * yardstick


def test_wire_adamw_cpu_shards_skip_and_tail():
    n_s, N = 1024, 4
    n, n_valid = n_s * N, n_s * N - 77
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n).astype(np.float32)
    w0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v0 = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    s = O.adamw_scalars(LR, WD, B1, B2, EPS, 3)
    buf = torch.zeros(O.shard_bytes("bfp_rne", n_s) * N, dtype=torch.uint8)
    wire.pack(torch.from_numpy(g), buf, n_s, "bfp_rne")
    w, m, v = (torch.from_numpy(x.copy()) for x in (w0, m0, v0))
    lp0 = torch.full((n,), 7.0, dtype=torch.bfloat16)
    lp = lp0.clone()
    wire.adamw(buf, n_s, N, w, codec="bfp_rne", mom=m, var=v, scalars=s, lp=lp, grad_scale=0.5, n_valid=n_valid,
               skip_shard=1, skip_period=4)
    rw, rm, rv = O.adamw(w0, O.quantize(g, "bfp_rne"), m0, v0, s, 0.5)
    keep = np.zeros(n, bool)
    keep[n_valid:] = True        # the tail past n_valid
    keep[n_s:2 * n_s] = True     # the skipped shard
    for got, ref, old in ((w, rw, w0), (m, rm, m0), (v, rv, v0)):
        assert np.array_equal(got.numpy()[keep], old[keep])
        assert np.array_equal(got.numpy()[~keep], ref[~keep])
    assert torch.equal(lp[torch.from_numpy(keep)], lp0[torch.from_numpy(keep)])
    assert torch.equal(lp[torch.from_numpy(~keep)], torch.from_numpy(rw).to(torch.bfloat16)[torch.from_numpy(~keep)])
    # zero gradient on zero state: exactly no update, no NaN out of 0 / eps
    z = [torch.zeros(n) for _ in range(3)]
    zb = torch.zeros(O.shard_bytes("bfp_rne", n_s) * N, dtype=torch.uint8)
    wire.pack(torch.zeros(n), zb, n_s, "bfp_rne")
    wire.adamw(zb, n_s, N, z[0], codec="bfp_rne", mom=z[1], var=z[2], scalars=s)
    assert all(torch.equal(t, torch.zeros(n)) for t in z)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
@pytest.mark.parametrize("codec", ["bfp_rne", "raw_f32"])
def test_python_engine_virtual_ranks(N, algo, codec):
    n = 3000
    rng = np.random.default_rng(N * 7 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = ThreadFabric(N, timeout_s=60)

    def fn(t):
        eng = CompressedAllReduce(t, codec=codec, algo=algo, max_slice_elems=512, device="cpu")
        L = eng.layout(n)
        w, m, v = torch.zeros(L.n_pad), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        w[:n] = torch.from_numpy(w0)
        for step in (1, 2):
            g = torch.zeros(L.n_pad)
            g[:n] = torch.from_numpy(grads[step - 1][t.rank])
            eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N, opt="adamw",
                              var=v, betas=(B1, B2), eps=EPS, step=step).synchronize()
        return w.numpy().copy(), m.numpy().copy(), v.numpy().copy(), L, eng.orders

    res = fabric.run(fn)
    L, orders = res[0][3], res[0][4]
    rw, rm, rv = w0, np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in (1, 2):
        gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step - 1]]
        red = sim.mesh_allreduce(gin, L.shard, codec) if algo == "mesh" else \
            sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, codec)[0]
        rw, rm, rv = O.adamw(rw, red[:n], rm, rv, O.adamw_scalars(LR, WD, B1, B2, EPS, step), 1.0 / N)
    for r in range(N):
        for got, ref in zip(res[r][:3], (rw, rm, rv)):
            assert np.array_equal(got[:n], ref)
            assert np.all(got[n:] == 0), "padding untouched"
        for a, b in zip(res[r][:3], res[0][:3]):
            assert np.array_equal(a, b), "ranks identical"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _trainer_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    try:
        sizes = [32, 64, 32]
        t = TorchDistTransport()
        eng = make_engine(t, "bfp", device="cpu")
        model = MLP(sizes, dtype=torch.float32, device="cpu", pad_fn=lambda n: eng.layout(n).n_pad, seed=3,
                    adam=True)
        for l in model.layers:
            t.broadcast_(l.master, 0)
        tr = DataParallelTrainer(model, eng, lr=1e-2, weight_decay=WD, optimizer="adamw", betas=(B1, B2), eps=EPS)
        g = torch.Generator().manual_seed(100)
        X = torch.rand(16, sizes[0], generator=g) * 2 - 1
        Y = torch.randint(0, sizes[-1], (16,), generator=g, dtype=torch.int32)
        mb = 16 // world
        x, y = X[rank * mb:(rank + 1) * mb], Y[rank * mb:(rank + 1) * mb]
        losses = [float(tr.step(x, y).mean()) for _ in range(3)]
        tr.finish()
        planes = [torch.cat([getattr(l, k) for l in model.layers]).numpy() for k in ("master", "mom", "var")]
        q.put((rank, planes, losses, tr.opt_step))
    except Exception as e:  # noqa: BLE001 - reported to the parent, which must never wait for a result that won't come
        q.put((rank, None, repr(e), None))
    finally:
        dist.destroy_process_group()


@pytest.mark.slow
def test_trainer_gloo_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    pc = mp.start_processes(_trainer_worker, args=(world, _free_port(), q), nprocs=world, join=False,
                            start_method="spawn")
    got, deadline = [], time.monotonic() + 120
    while len(got) < world:
        if not q.empty():
            got.append(q.get())
        elif pc.join(0.05):  # every worker has ended (a worker that died raises here): take what they left
            while not q.empty():
                got.append(q.get())
            break
        assert time.monotonic() < deadline, "trainer workers hung"
    while not pc.join(0.05):
        assert time.monotonic() < deadline, "trainer workers hung"
    assert len(got) == world, got
    failed = [(r, l) for r, p, l, s in got if p is None]
    assert not failed, failed
    res = {r: (p, l, s) for r, p, l, s in got}
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b), "replicas must stay bit-identical"
    assert res[0][2] == 3 and res[1][2] == 3
    assert np.any(res[0][0][2] > 0), "second moment accumulated"
    for r in range(world):
        assert np.isfinite(res[r][1]).all()
    mean = [sum(res[r][1][k] for r in range(world)) / world for k in range(3)]
    assert mean[-1] < mean[0]


_CLI = ["32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0",
        "--optimizer", "adamw", "--lr", "1e-3", "--weight-decay", "1e-2"]


def test_cli_adamw_checkpoint_resume_bit_identical(tmp_path):
    full, half, rest = (str(tmp_path / k) for k in ("full", "half", "rest"))
    mlp_mpi.run(["4"] + _CLI + ["--checkpoint", full], out=io.StringIO())
    mlp_mpi.run(["2"] + _CLI + ["--checkpoint", half], out=io.StringIO())
    mlp_mpi.run(["2"] + _CLI + ["--resume", half, "--checkpoint", rest], out=io.StringIO())
    from safetensors.torch import load_file

    a, b = load_file(full + ".safetensors"), load_file(rest + ".safetensors")
    assert sorted(a) == sorted(b)
    assert {"fc0.exp_avg", "fc0.exp_avg_sq", "fc1.exp_avg", "fc1.exp_avg_sq"} <= set(a)
    assert not any(k.endswith(".momentum") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a["fc0.exp_avg_sq"].max()) > 0
    ia, ih, ib = (json.load(open(p + ".json")) for p in (full, half, rest))
    assert ia["optimizer"] == "adamw" and (ia["opt_step"], ih["opt_step"], ib["opt_step"]) == (4, 2, 4)
    assert ib["iteration"] == 4


def test_momentum_sgd_checkpoint_still_loads(tmp_path):
    """A checkpoint in the format from before AdamW (fc{i}.momentum, no optimizer / opt_step in the index)."""
    m = MLP([64, 64, 32], dtype=torch.float32, seed=5, momentum=True)
    for l in m.layers:
        l.mom[: l.n] = torch.arange(l.n, dtype=torch.float32)
    p = str(tmp_path / "old")
    checkpoint.save(p, m, iteration=3)
    info = json.load(open(p + ".json"))
    assert "optimizer" not in info and "opt_step" not in info
    m2 = MLP([64, 64, 32], dtype=torch.float32, seed=9, momentum=True)
    assert checkpoint.load(p, m2)["iteration"] == 3
    for l, l2 in zip(m.layers, m2.layers):
        assert torch.equal(l.master[: l.n], l2.master[: l.n]) and torch.equal(l.mom[: l.n], l2.mom[: l.n])
    r = mlp_mpi.run(["1", "32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32",
                     "--warmup", "0", "--momentum", "0.9", "--resume", p], out=io.StringIO())
    assert np.isfinite(r["loss"])
    # and into an AdamW run: the weights load, the moments start from zero, the update count from 0
    r = mlp_mpi.run(["1"] + _CLI + ["--resume", p], out=io.StringIO())
    assert np.isfinite(r["loss"])


def test_validation_errors():
    t = ThreadFabric(1).transport(0)
    eng = CompressedAllReduce(t, device="cpu")
    n = eng.layout(100).n_pad
    g, w, m, v = (torch.zeros(n) for _ in range(4))
    ok = dict(n_valid=100, lr=LR, opt="adamw", var=v, step=1)
    eng.allreduce_sgd(g, w, None, m, **ok).synchronize()
    for bad in (dict(eps=0.0), dict(step=0), dict(momentum=0.9), dict(nesterov=True), dict(var=None),
                dict(step=None), dict(opt="lamb")):
        with pytest.raises(ValueError):
            eng.allreduce_sgd(g, w, None, m, **{**ok, **bad})
    with pytest.raises(ValueError):
        eng.allreduce_sgd(g, w, None, None, **ok)
    with pytest.raises(ValueError):
        uncompressed_allreduce_sgd(t, g, w, None, m, lr=LR, opt="adamw", var=v, step=1, eps=-1.0)
    with pytest.raises(ValueError):
        O.adamw_scalars(LR, WD, B1, B2, 0.0, 1)
    with pytest.raises(ValueError):
        O.adamw_scalars(LR, WD, B1, B2, EPS, 0)
    model = MLP([32, 32], dtype=torch.float32, adam=True)
    with pytest.raises(ValueError):
        DataParallelTrainer(model, None, optimizer="adamw", momentum=0.9)
    with pytest.raises(ValueError):
        DataParallelTrainer(model, None, optimizer="adamw", eps=0.0)
    with pytest.raises(ValueError):
        DataParallelTrainer(MLP([32, 32], dtype=torch.float32), None, optimizer="adamw")


def test_trainer_without_engine_honours_adamw():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, adam=True)
    tr = DataParallelTrainer(model, None, lr=1e-2, weight_decay=WD, optimizer="adamw")
    g = torch.Generator().manual_seed(1)
    X = torch.rand(16, sizes[0], generator=g) * 2 - 1
    Y = torch.randint(0, sizes[-1], (16,), generator=g, dtype=torch.int32)
    prev = [(l.master.numpy().copy(), l.mom.numpy().copy(), l.var.numpy().copy()) for l in model.layers]
    tr.step(X, Y)
    tr.finish()
    assert tr.opt_step == 1
    s = O.adamw_scalars(1e-2, WD, 0.9, 0.999, 1e-8, 1)
    for l, (w0, m0, v0) in zip(model.layers, prev):
        rw, rm, rv = O.adamw(w0[: l.n], l.grad.numpy()[: l.n], m0[: l.n], v0[: l.n], s)
        assert np.array_equal(l.master.numpy()[: l.n], rw)
        assert np.array_equal(l.mom.numpy()[: l.n], rm) and np.array_equal(l.var.numpy()[: l.n], rv)


def test_model_planes_and_repad():
    m = MLP([32, 64, 32], dtype=torch.float32, seed=1, adam=True)
    assert all(l.mom is not None and l.var is not None and l.var.shape == l.master.shape for l in m.layers)
    assert all(l.var is None for l in MLP([32, 64, 32], dtype=torch.float32, momentum=True).layers)
    l = m.layers[0]
    l.var[: l.n] = 2.0
    n_pad = l.n_pad + 256
    m.repad(0, n_pad)
    assert l.var.numel() == n_pad and l.mom.numel() == n_pad and l.master.numel() == n_pad
    assert torch.all(l.var[: l.n] == 2.0) and torch.all(l.var[l.n:] == 0)
