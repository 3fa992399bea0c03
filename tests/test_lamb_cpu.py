"""AdamW with the layer-wise trust ratio (LAMB) in the all-reduce epilogue, on CPU: the oracle against an independent
float64 LAMB, wire.lamb_*'s shard / skip / tail / n_adapt handling, the Python engine over virtual ranks against the
spec simulator, the trainer over gloo, the CLI's checkpoint / resume round trip, and the refusals."""
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

LR, WD, B1, B2, EPS = 1e-3, 1e-2, 0.9, 0.999, 1e-8


def ulp_diff(a, b):
    """Distance in f32 units in the last place between finite same-sign values."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def lamb_f64(w, g, m, v, s, n_adapt, phi=None):
    """The update's formulas (pass 1, ratio, pass 2) evaluated in float64 throughout, with no intermediate rounding,
    from the step's scalars ``s`` (``lamb_scalars``: the rounded-once f32 values are the formulas' scalars).
    phi: forced when given. Returns (w', phi)."""
    f = np.float64
    w, g, m, v = (np.asarray(x, f) for x in (w, g, m, v))
    m2 = f(s.beta1) * m + f(s.omb1) * g
    v2 = f(s.beta2) * v + f(s.omb2) * g * g
    u = m2 / (np.sqrt(v2) * f(s.rsbc2) + f(s.eps))
    r = f(s.wd) * w + u * f(s.rbc1)
    if phi is None:
        sw, sr = np.sum(w[:n_adapt] ** 2), np.sum(r[:n_adapt] ** 2)
        phi = np.sqrt(sw / sr) if sw > 0 and sr > 0 else 1.0
    scale = np.where(np.arange(w.size) < n_adapt, f(s.lr) * phi, f(s.lr))
    return w - scale * r, phi


def test_scalars_extend_adamw():
    a, s = O.adamw_scalars(LR, WD, B1, B2, EPS, 7), O.lamb_scalars(LR, WD, B1, B2, EPS, 7)
    assert all(isinstance(x, np.float32) for x in s)
    for k in ("beta1", "omb1", "beta2", "omb2", "rsbc2", "eps"):
        assert getattr(s, k) == getattr(a, k)
    assert s.rbc1 == np.float32(1 / (1 - B1 ** 7)) and s.wd == np.float32(WD) and s.lr == np.float32(LR)
    assert O.AdamWScalars.FIELDS == ("beta1", "omb1", "beta2", "omb2", "step_size", "rsbc2", "eps", "decay", "wd")
    assert len(s.kernel_args()) == 9


def within(got, ref, what):
    """|got - ref| <= 1e-6 * |ref| for every element; a failure names the worst element."""
    err = np.abs(got.astype(np.float64) - ref)
    i = int(np.argmax(err - 1e-6 * np.abs(ref)))
    rel = float((err / np.abs(ref)).max())
    print(f"{what}: max relative error {rel:.3e}")
    assert np.all(err <= 1e-6 * np.abs(ref)), f"{what}: element {i}: got {got[i]!r}, float64 {ref[i]!r}"


@pytest.mark.parametrize("wd", [WD, 0.0])
def test_oracle_against_float64_lamb(wd):
    """Each w' within 1e-6 relative of the float64 value, |got - ref| <= 1e-6 * |ref| element by element, over five
    steps; and, with phi forced to 1 and n_adapt = 0, within the same bound of float64 AdamW (the same formulas with
    every scale equal to lr). The float64 side takes the step's f32-rounded scalars, as the formulas do: against
    hyper-parameters left unrounded (lr = 1e-3 is 4.75e-8 away from its f32 value) the AdamW comparison of these
    inputs reaches 1.07e-6 at one element of step 2, where a weight of 1e-3 and its step cancel to -9.3e-5 — the
    rounding of lr that the scalars specify, not an error of the update. Measured here: at most 8.4e-7."""
    n, n_adapt = 4096, 3001
    rng = np.random.default_rng(3)
    w = rng.standard_normal(n).astype(np.float32)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    for t in range(1, 6):
        g = rng.standard_normal(n).astype(np.float32)
        s = O.lamb_scalars(LR, wd, B1, B2, EPS, t)
        m2, v2, r = O.lamb_moments(w, g, m, v, s)
        words = O.lamb_ratio(w, r, n_adapt, LR)
        ref, phi = lamb_f64(w, g, m, v, s, n_adapt)
        got = O.lamb_apply(w, m2, v2, s, words, n_adapt)
        assert abs(float(words[2]) - phi) <= 1e-6 * phi
        assert words[0] == np.float32(LR) * words[2] and words[1] == np.float32(LR)
        within(got, ref, f"step {t} LAMB")
        # phi forced to 1 and nothing adapted: float64 AdamW
        one = np.array([LR, LR, 1.0], np.float32)
        within(O.lamb_apply(w, m2, v2, s, one, 0), lamb_f64(w, g, m, v, s, 0, phi=1.0)[0], f"step {t} AdamW")
        # the moments are AdamW's statements: the same bits
        _, am, av = O.adamw(w, g, m, v, O.adamw_scalars(LR, wd, B1, B2, EPS, t))
        assert np.array_equal(m2, am) and np.array_equal(v2, av)
        w, m, v = got, m2, v2


def test_scalar_classes_do_not_mix():
    """LambScalars is no AdamWScalars: the AdamW update refuses it instead of reading wrong scalars."""
    s = O.lamb_scalars(LR, WD, B1, B2, EPS, 1)
    assert not isinstance(s, O.AdamWScalars) and not hasattr(s, "step_size") and not hasattr(s, "decay")
    z = torch.zeros(256)
    with pytest.raises(TypeError):
        wire.adamw(torch.zeros(1024, dtype=torch.uint8), 256, 1, z, codec="raw_f32", mom=z.clone(), var=z.clone(),
                   scalars=s)


def test_ratio_degenerate_sums():
    z, one = np.zeros(64, np.float32), np.ones(64, np.float32)
    assert np.array_equal(O.lamb_ratio(z, one, 64, LR), np.array([LR, LR, 1.0], np.float32))
    assert np.array_equal(O.lamb_ratio(one, z, 64, LR), np.array([LR, LR, 1.0], np.float32))
    assert np.array_equal(O.lamb_ratio(one, one, 0, LR), np.array([LR, LR, 1.0], np.float32))
    bad = one.copy()
    bad[3] = np.inf
    assert O.lamb_ratio(one, bad, 64, LR)[2] == 1.0
    assert O.lamb_ratio(2 * one, one, 64, LR)[2] == 2.0


@pytest.mark.parametrize("codec", ["bfp_rne", "raw_f32"])
def test_wire_lamb_cpu_shards_skip_tail_and_adapt(codec):
    n_s, N = 1024, 4
    n, n_valid, n_adapt = n_s * N, n_s * N - 77, 3001  # 3001 = 187 * 16 + 9: inside a 16-value group
    rng = np.random.default_rng(5)
    g = rng.standard_normal(n).astype(np.float32)
    w0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v0 = (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)
    s = O.lamb_scalars(LR, WD, B1, B2, EPS, 3)
    buf = torch.zeros(O.shard_bytes(codec, n_s) * N, dtype=torch.uint8)
    wire.pack(torch.from_numpy(g), buf, n_s, codec)
    w, m, v = (torch.from_numpy(x.copy()) for x in (w0, m0, v0))
    lp0 = torch.full((n,), 7.0, dtype=torch.bfloat16)
    lp = lp0.clone()
    partials = torch.zeros(8, dtype=torch.float64)
    words = torch.zeros(3)
    kw = dict(n_valid=n_valid, n_adapt=n_adapt, skip_shard=1, skip_period=4)
    k = wire.lamb_moments(buf, n_s, N, w, codec=codec, mom=m, var=v, scalars=s, partials=partials, grad_scale=0.5, **kw)
    assert k == wire.lamb_partials_for(w, n_s) == 1
    assert np.array_equal(w.numpy(), w0) and torch.equal(lp, lp0), "pass 1 leaves the weights alone"
    keep = np.zeros(n, bool)
    keep[n_valid:] = True        # the tail past n_valid
    keep[n_s:2 * n_s] = True     # the skipped shard
    rm, rv, rr = O.lamb_moments(w0, O.quantize(g, codec), m0, v0, s, 0.5)
    for got, ref, old in ((m, rm, m0), (v, rv, v0)):
        assert np.array_equal(got.numpy()[keep], old[keep]) and np.array_equal(got.numpy()[~keep], ref[~keep])
    adapted = ~keep & (np.arange(n) < n_adapt)
    wire.lamb_ratio(partials, k, LR, words)
    ref_words = O.lamb_ratio(w0[adapted], rr[adapted], int(adapted.sum()), LR)
    assert np.array_equal(words.numpy(), ref_words)
    wire.lamb_apply(w, n_s, mom=m, var=v, scalars=s, words=words, lp=lp, **kw)
    rw = O.lamb_apply(w0, rm, rv, s, ref_words, n_adapt)
    assert np.array_equal(w.numpy()[keep], w0[keep]) and np.array_equal(w.numpy()[~keep], rw[~keep])
    kt = torch.from_numpy(keep)
    assert torch.equal(lp[kt], lp0[kt]) and torch.equal(lp[~kt], torch.from_numpy(rw).to(torch.bfloat16)[~kt])
    # the ratio really differs from 1 here and the tail past n_adapt really takes lr alone
    assert words[2] != 1.0
    tail = ~keep & (np.arange(n) >= n_adapt)
    assert np.array_equal(w.numpy()[tail], O.lamb_apply(w0, rm, rv, s, np.array([LR, LR, 1], np.float32), 0)[tail])
    # two complementary launches (all but shard 1, then shard 1 alone) form one ratio from two partial regions
    w2, m2, v2 = (torch.from_numpy(x.copy()) for x in (w0, m0, v0))
    p2 = torch.zeros(8, dtype=torch.float64)
    k1 = wire.lamb_moments(buf, n_s, N, w2, codec=codec, mom=m2, var=v2, scalars=s, partials=p2, grad_scale=0.5, **kw)
    sb = O.shard_bytes(codec, n_s)
    k2 = wire.lamb_moments(buf[sb:2 * sb], n_s, 1, w2[n_s:2 * n_s], codec=codec, mom=m2[n_s:2 * n_s],
                           var=v2[n_s:2 * n_s], scalars=s, partials=p2, partials_base=k1, grad_scale=0.5)
    wire.lamb_ratio(p2, k1 + k2, LR, words)
    both = np.arange(n) < min(n_adapt, n_valid)
    full = O.lamb_ratio(w0[both], rr[both], int(both.sum()), LR)
    assert np.all(ulp_diff(words.numpy(), full) <= 1)
    with pytest.raises(ValueError):
        wire.lamb_moments(buf, n_s, N, w, codec=codec, mom=m, var=v, scalars=s, partials=partials, n_valid=n_valid,
                          n_adapt=n_valid + 1)


@pytest.mark.parametrize("N", [1, 2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
@pytest.mark.parametrize("codec", ["bfp_rne", "raw_f32"])
def test_python_engine_virtual_ranks(N, algo, codec):
    """Two steps against sim + oracle. The engine sums each region's squares exactly and then the regions' sums, the
    oracle all squares at once: the scale words may differ in the last place (<= 2 ulp as on the GPU), so the planes
    are compared with the oracle fed each step's own words, bit for bit."""
    n, n_adapt = 3000, 2841
    rng = np.random.default_rng(N * 7 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for _ in range(2)]
    w0 = rng.standard_normal(n).astype(np.float32)
    fabric = ThreadFabric(N, timeout_s=60)

    def fn(t):
        eng = CompressedAllReduce(t, codec=codec, algo=algo, max_slice_elems=512, device="cpu")
        L = eng.layout(n)
        w, m, v = torch.zeros(L.n_pad), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        w[:n] = torch.from_numpy(w0)
        words = torch.zeros(2, 3)
        for step in (1, 2):
            g = torch.zeros(L.n_pad)
            g[:n] = torch.from_numpy(grads[step - 1][t.rank])
            eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=1.0 / N, opt="adamw",
                              var=v, betas=(B1, B2), eps=EPS, step=step, trust_ratio=True, n_adapt=n_adapt,
                              trust_out=words[step - 1], defer=step == 2).synchronize()
        return w.numpy().copy(), m.numpy().copy(), v.numpy().copy(), words.numpy().copy(), L, eng.orders

    res = fabric.run(fn)
    L, orders = res[0][4], res[0][5]
    rw, rm, rv = w0, np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in (1, 2):
        gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step - 1]]
        red = sim.mesh_allreduce(gin, L.shard, codec) if algo == "mesh" else \
            sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, codec)[0]
        s = O.lamb_scalars(LR, WD, B1, B2, EPS, step)
        rm, rv, rr = O.lamb_moments(rw, red[:n], rm, rv, s, 1.0 / N)
        words = res[0][3][step - 1]
        assert np.all(ulp_diff(words, O.lamb_ratio(rw, rr, n_adapt, LR)) <= 2)
        assert words[2] != 1.0
        rw = O.lamb_apply(rw, rm, rv, s, words, n_adapt)
    for r in range(N):
        for got, ref in zip(res[r][:3], (rw, rm, rv)):
            assert np.array_equal(got[:n], ref)
            assert np.all(got[n:] == 0), "padding untouched"
        for a, b in zip(res[r][:4], res[0][:4]):
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
        tr = DataParallelTrainer(model, eng, lr=1e-2, weight_decay=WD, optimizer="adamw", betas=(B1, B2), eps=EPS,
                                 trust_ratio=True)
        g = torch.Generator().manual_seed(100)
        X = torch.rand(16, sizes[0], generator=g) * 2 - 1
        Y = torch.randint(0, sizes[-1], (16,), generator=g, dtype=torch.int32)
        mb = 16 // world
        x, y = X[rank * mb:(rank + 1) * mb], Y[rank * mb:(rank + 1) * mb]
        losses = [float(tr.step(x, y).mean()) for _ in range(3)]
        tr.finish()
        planes = [torch.cat([getattr(l, k) for l in model.layers]).numpy() for k in ("master", "mom", "var")]
        planes.append(tr.trust_ratios.numpy().copy())
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
    ratios = res[0][0][3]
    assert ratios.shape == (2, 3) and np.isfinite(ratios).all()
    assert np.all(ratios[:, 1] == np.float32(1e-2)) and np.all(ratios[:, 2] != 1.0)
    assert np.array_equal(ratios[:, 0], ratios[:, 1] * ratios[:, 2])
    for r in range(world):
        assert np.isfinite(res[r][1]).all()


_CLI = ["32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0",
        "--optimizer", "adamw", "--trust-ratio", "--lr", "1e-3", "--weight-decay", "1e-2"]


def test_cli_trust_ratio_checkpoint_resume_bit_identical(tmp_path):
    full, half, rest, plain = (str(tmp_path / k) for k in ("full", "half", "rest", "plain"))
    mlp_mpi.run(["4"] + _CLI + ["--checkpoint", full], out=io.StringIO())
    mlp_mpi.run(["2"] + _CLI + ["--checkpoint", half], out=io.StringIO())
    mlp_mpi.run(["2"] + _CLI + ["--resume", half, "--checkpoint", rest], out=io.StringIO())
    mlp_mpi.run(["4"] + [x for x in _CLI if x != "--trust-ratio"] + ["--checkpoint", plain], out=io.StringIO())
    from safetensors.torch import load_file

    a, b, c = (load_file(p + ".safetensors") for p in (full, rest, plain))
    assert sorted(a) == sorted(b) == sorted(c), "no new checkpoint state"
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["fc0.weight"], c["fc0.weight"]), "the flag changes the run"
    ia, ib = (json.load(open(p + ".json")) for p in (full, rest))
    assert ia["optimizer"] == "adamw" and (ia["opt_step"], ib["opt_step"]) == (4, 4)


def test_trainer_without_engine_matches_oracle():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, adam=True, bias=True)
    tr = DataParallelTrainer(model, None, lr=1e-2, weight_decay=WD, optimizer="adamw", trust_ratio=True)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(16, sizes[0], generator=g) * 2 - 1
    Y = torch.randint(0, sizes[-1], (16,), generator=g, dtype=torch.int32)
    prev = [(l.master.numpy().copy(), l.mom.numpy().copy(), l.var.numpy().copy()) for l in model.layers]
    tr.step(X, Y)
    tr.finish()
    s = O.lamb_scalars(1e-2, WD, 0.9, 0.999, 1e-8, 1)
    for i, (l, (w0, m0, v0)) in enumerate(zip(model.layers, prev)):
        na = l.cin * l.cout
        assert na < l.n, "the bucket ends in a bias segment"
        rm, rv, rr = O.lamb_moments(w0[: l.n], l.grad.numpy()[: l.n], m0[: l.n], v0[: l.n], s)
        words = O.lamb_ratio(w0, rr, na, 1e-2)
        assert np.array_equal(tr.trust_ratios[i].numpy(), words) and words[2] != 1.0
        assert np.array_equal(l.master.numpy()[: l.n], O.lamb_apply(w0[: l.n], rm, rv, s, words, na))
        assert np.array_equal(l.mom.numpy()[: l.n], rm) and np.array_equal(l.var.numpy()[: l.n], rv)


def test_trainer_equal_shaped_layers_keep_their_own_rows():
    model = MLP([32, 32, 32, 32], dtype=torch.float32, seed=4, adam=True)
    tr = DataParallelTrainer(model, None, lr=1e-2, optimizer="adamw", trust_ratio=True)
    g = torch.Generator().manual_seed(2)
    tr.step(torch.rand(8, 32, generator=g), torch.randint(0, 32, (8,), generator=g, dtype=torch.int32))
    tr.finish()
    r = tr.trust_ratios.numpy()
    assert r.shape == (3, 3) and np.all(r[:, 2] > 0) and len({float(x) for x in r[:, 2]}) == 3


@pytest.mark.parametrize("algo", ["mesh", "ring"])
def test_empty_request_still_writes_its_words(algo):
    """n_valid == 0: no region, no pass 1; the ratio sums nothing and the words are {lr, lr, 1}, not stale."""
    eng = CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu", algo=algo)
    n = eng.layout(0).n_pad
    g, w, m, v = (torch.zeros(n) for _ in range(4))
    out = torch.full((3,), float("nan"))
    eng.allreduce_sgd(g, w, None, m, n_valid=0, lr=LR, opt="adamw", var=v, step=1, trust_ratio=True,
                      trust_out=out).synchronize()
    assert np.array_equal(out.numpy(), np.array([LR, LR, 1.0], np.float32))
    assert all(torch.equal(t, torch.zeros(n)) for t in (w, m, v))


def test_refusals():
    t = ThreadFabric(1).transport(0)
    eng = CompressedAllReduce(t, device="cpu")
    n = eng.layout(100).n_pad
    g, w, m, v = (torch.zeros(n) for _ in range(4))
    ok = dict(n_valid=100, lr=LR, opt="adamw", var=v, step=1, trust_ratio=True)
    eng.allreduce_sgd(g, w, None, m, **ok).synchronize()
    eng.allreduce_sgd(g, w, None, m, **ok, n_adapt=0).synchronize()
    eng.allreduce_sgd(g, w, None, m, **ok, n_adapt=100).synchronize()
    for bad in (dict(opt="sgd", var=None, step=None), dict(n_adapt=101), dict(n_adapt=-1), dict(opt="lamb"),
                dict(var=None), dict(step=None)):
        with pytest.raises(ValueError):
            eng.allreduce_sgd(g, w, None, m, **{**ok, **bad})
    with pytest.raises(ValueError):
        eng.allreduce_sgd(g, w, None, m, n_valid=100, lr=LR, opt="lamb")
    ring = CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu", algo="ring", compat_owner_fp32=True)
    with pytest.raises(ValueError, match="compat_owner_fp32"):
        ring.allreduce_sgd(torch.zeros(ring.layout(100).n_pad), w, None, m, **ok)
    with pytest.raises(ValueError, match="trust_ratio"):
        uncompressed_allreduce_sgd(t, g, w, None, m, lr=LR, opt="adamw", var=v, step=1, trust_ratio=True)
    model = MLP([32, 32], dtype=torch.float32, adam=True)
    with pytest.raises(ValueError):
        DataParallelTrainer(model, None, optimizer="sgd", trust_ratio=True)

    class Sharded:  # what the trainer reads of a sharded-update engine
        world, shard_update = 2, True

    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, Sharded(), optimizer="adamw", trust_ratio=True)
    assert DataParallelTrainer(model, None, optimizer="adamw").trust_ratios is None
