"""Global-norm gradient clipping in the all-reduce epilogues, on CPU: the oracle against torch's clip_grad_norm_, the
Python engine's clip groups over virtual ranks against the spec simulators, the trainer, the CLI flag and the
refusals."""
import io
import math

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.cli import mlp_mpi
from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import sim
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

LR, WD, MOM = 0.05, 1e-2, 0.9
LIMIT = "a clip group holds at most 8 deferred requests"


@pytest.mark.parametrize("max_norm", [0.5, 10.0, 1e6])
def test_oracle_against_torch(max_norm):
    n = 4096
    g = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    p = torch.nn.Parameter(torch.zeros(n))
    p.grad = torch.from_numpy(g.copy())
    total = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
    words = O.clip_words(O.clip_sumsq(g), 1.0, max_norm)
    assert words.dtype == np.float32 and words.shape == (4,)
    # torch sums the squares in f32 (n additions, 2^-24 each); the oracle's fp64 sum is the tighter of the two
    tol = n * 2.0 ** -24
    ref_coef = min(1.0, max_norm / (total + 1e-6))
    assert abs(float(words[0]) - ref_coef) <= tol * ref_coef
    assert abs(float(words[1]) - total) <= tol * total
    assert words[2] == np.float32(max_norm) and words[3] == 0
    assert (words[0] == 1.0) == (max_norm >= 1e6)
    gs = O.clip_scale(1.0, words)
    assert gs == float(words[0])
    assert np.allclose(p.grad.numpy(), g * np.float32(gs), rtol=4 * tol, atol=0)
    # the f32 grad_scale is the one the kernels apply: the norm is that of the scaled gradient
    w2 = O.clip_words(O.clip_sumsq(g), -1.0 / 3, max_norm)
    assert abs(float(w2[1]) - total * float(np.float32(1.0 / 3))) <= tol * total
    assert O.clip_scale(-1.0 / 3, w2) == float(np.float32(-1.0 / 3) * w2[0])


def test_oracle_degenerate_inputs():
    z = O.clip_words(O.clip_sumsq(np.zeros(64, np.float32)), 1.0, 1.0)
    assert z[0] == 1.0 and z[1] == 0.0 and z[3] == 0.0
    g = np.ones(64, np.float32)
    g[7] = np.inf
    w = O.clip_words(O.clip_sumsq(g), 1.0, 1.0)
    assert math.isnan(w[0]) and w[3] == 1.0 and w[2] == 1.0
    assert math.isnan(O.clip_scale(0.5, w))
    g[7] = np.nan
    w = O.clip_words(O.clip_sumsq(g), 1.0, 1.0)
    assert math.isnan(w[0]) and w[3] == 1.0
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_norm"):
            O.clip_words(1.0, 1.0, bad)
    # exactly 1 up to the boundary total + 1e-6 <= max_norm
    assert O.clip_words(9.0, 1.0, 3.0 + 1e-6)[0] == 1.0
    assert O.clip_words(9.0, 1.0, 2.0)[0] == np.float32(2.0 / (3.0 + 1e-6))
    # a coefficient of 1 leaves grad_scale's bits
    assert O.clip_scale(1.0 / 3, z) == float(np.float32(1.0 / 3))


@pytest.mark.parametrize("codec", ["bfp_rne", "bfp_trunc", "raw_f32", "raw_bf16"])
def test_wire_sumsq_and_clip_coef(codec):
    n_s, N = 256, 4
    n, n_valid = n_s * N, n_s * N - 77
    g = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    buf = torch.zeros(O.shard_bytes(codec, n_s) * N, dtype=torch.uint8)
    wire.pack(torch.from_numpy(g), buf, n_s, codec)
    dec = O.quantize(g, codec) if codec.startswith("bfp") else O.unpack(buf.numpy(), n, n_s, codec)
    part = torch.full((4,), math.nan, dtype=torch.float64)
    assert wire.sumsq_partials_for(buf, n_s) == 1
    assert wire.sumsq(buf, n_s, N, codec=codec, partials=part, partials_base=1, n_valid=n_valid) == 1
    assert float(part[1]) == O.clip_sumsq(dec[:n_valid]) and torch.isnan(part[[0, 2, 3]]).all()
    keep = np.ones(n, bool)
    keep[n_valid:] = False
    keep[n_s:2 * n_s] = False
    wire.sumsq(buf, n_s, N, codec=codec, partials=part, partials_base=2, n_valid=n_valid, skip_shard=1, skip_period=4)
    assert float(part[2]) == O.clip_sumsq(dec[keep])
    words = torch.zeros(4)
    wire.clip_coef([(part, 1, 1), (part, 0, 0), (part, 2, 1)], 2.0, 0.5, words)
    ref = O.clip_words(math.fsum([float(part[1]), float(part[2])]), 0.5, 2.0)
    assert np.array_equal(words.numpy(), ref) and 0 < ref[0] < 1
    with pytest.raises(ValueError, match="max_norm"):
        wire.clip_coef([(part, 1, 1)], 0.0, 1.0, words)
    with pytest.raises(ValueError, match="at most 8"):
        wire.clip_coef([(part, 1, 1)] * 9, 1.0, 1.0, words)


def test_wire_updates_take_the_clip_words():
    n_s, N, codec = 256, 2, "bfp_rne"
    n = n_s * N
    rng = np.random.default_rng(9)
    g = rng.standard_normal(n).astype(np.float32)
    w0 = rng.standard_normal(n).astype(np.float32)
    buf = torch.zeros(O.shard_bytes(codec, n_s) * N, dtype=torch.uint8)
    wire.pack(torch.from_numpy(g), buf, n_s, codec)
    words = torch.tensor([0.37, 5.0, 1.0, 0.0])
    gs = O.clip_scale(0.5, words.numpy())
    assert gs == float(np.float32(0.5) * np.float32(0.37))

    def run(fn, clip, scale):
        w, m, v = torch.from_numpy(w0.copy()), torch.zeros(n), torch.zeros(n)
        fn(w, m, v, clip, scale)
        return w.numpy(), m.numpy(), v.numpy()

    def sgd(w, m, v, clip, scale):
        wire.sgd(buf, n_s, N, w, codec=codec, mom=m, lr=LR, grad_scale=scale, weight_decay=WD, momentum=MOM, clip=clip)

    def adamw(w, m, v, clip, scale):
        wire.adamw(buf, n_s, N, w, codec=codec, mom=m, var=v, scalars=O.adamw_scalars(LR, WD, 0.9, 0.999, 1e-8, 2),
                   grad_scale=scale, clip=clip)

    def lamb(w, m, v, clip, scale):
        s = O.lamb_scalars(LR, WD, 0.9, 0.999, 1e-8, 2)
        part, tw = torch.zeros(2, dtype=torch.float64), torch.zeros(3)
        k = wire.lamb_moments(buf, n_s, N, w, codec=codec, mom=m, var=v, scalars=s, partials=part, grad_scale=scale,
                              clip=clip)
        wire.lamb_ratio(part, k, LR, tw)
        wire.lamb_apply(w, n_s, mom=m, var=v, scalars=s, words=tw)

    one = torch.tensor([1.0, 0.0, 1.0, 0.0])
    for fn in (sgd, adamw, lamb):
        for a, b in zip(run(fn, words, 0.5), run(fn, None, gs)):
            assert np.array_equal(a, b)
        for a, b in zip(run(fn, one, 0.5), run(fn, None, 0.5)):
            assert np.array_equal(a, b)
        assert not np.array_equal(run(fn, words, 0.5)[0], run(fn, None, 0.5)[0])


SIZES = (3000, 1200, 333)  # the smallest: n_valid no multiple of 16


def _reduced(N, algo, codec, grads, L, orders):
    gin = [np.pad(g, (0, L.n_pad - g.size)) for g in grads]
    if algo == "mesh":
        return sim.mesh_allreduce(gin, L.shard, codec)
    return sim.ring_allreduce(gin, orders, L.slice_elems, L.blocks, codec)[0]


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
def test_python_engine_clip_group(N, algo):
    codec, max_norm = "bfp_rne", 1.0
    rng = np.random.default_rng(N * 11 + len(algo))
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(N)] for n in SIZES]
    w0 = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    m0 = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in SIZES]
    fabric = ThreadFabric(N, timeout_s=60)

    def fn(t):
        eng = CompressedAllReduce(t, codec=codec, algo=algo, rings=2, max_slice_elems=512, device="cpu")
        words = torch.full((4,), math.nan)
        hs, planes, Ls = [], [], []
        for b, n in enumerate(SIZES):
            L = eng.layout(n)
            g, w, m = torch.zeros(L.n_pad), torch.zeros(L.n_pad), torch.zeros(L.n_pad)
            g[:n] = torch.from_numpy(grads[b][t.rank])
            w[:n] = torch.from_numpy(w0[b])
            m[:n] = torch.from_numpy(m0[b])
            hs.append(eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, grad_scale=1.0 / N, weight_decay=WD,
                                        momentum=MOM, defer=True, clip=words, name=f"b{b}"))
            planes.append((w, m))
            Ls.append(L)
        assert all(np.array_equal(w.numpy()[:n], w0[b]) for b, ((w, _), n) in enumerate(zip(planes, SIZES)))
        assert torch.isnan(words).all(), "no word before the group commits"
        eng.commit_group(hs, max_norm=max_norm, grad_scale=1.0 / N)
        for h in hs:
            h.synchronize()
        return [(w.numpy().copy(), m.numpy().copy()) for w, m in planes], words.numpy().copy(), Ls, eng.orders

    res = fabric.run(fn)
    Ls, orders = res[0][2], res[0][3]
    red = [_reduced(N, algo, codec, grads[b], Ls[b], orders)[:n] for b, n in enumerate(SIZES)]
    ref_words = O.clip_words(O.clip_sumsq(np.concatenate(red)), 1.0 / N, max_norm)
    assert 0 < ref_words[0] < 1 and ref_words[3] == 0
    gs = O.clip_scale(1.0 / N, ref_words)
    for r in range(N):
        assert np.array_equal(res[r][1], ref_words)
        for b, n in enumerate(SIZES):
            rw, rm = O.sgd(w0[b], red[b], LR, gs, WD, MOM, m0[b])
            w, m = res[r][0][b]
            assert np.array_equal(w[:n], rw) and np.array_equal(m[:n], rm)
            assert np.all(w[n:] == 0) and np.all(m[n:] == 0), "padding untouched"


@pytest.mark.parametrize("opt", ["adamw", "lamb"])
def test_python_engine_clip_group_adamw_lamb(opt):
    N, algo, codec, max_norm = 2, "mesh", "bfp_rne", 0.5
    rng = np.random.default_rng(17)
    sizes = SIZES[1:]
    grads = [[rng.standard_normal(n).astype(np.float32) for _ in range(N)] for n in sizes]
    w0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    fabric = ThreadFabric(N, timeout_s=60)
    okw = dict(opt="adamw", betas=(0.9, 0.999), eps=1e-8, step=1, trust_ratio=opt == "lamb")

    def fn(t):
        eng = CompressedAllReduce(t, codec=codec, algo=algo, device="cpu")
        words, hs, planes, Ls = torch.zeros(4), [], [], []
        for b, n in enumerate(sizes):
            L = eng.layout(n)
            g, w, m, v = (torch.zeros(L.n_pad) for _ in range(4))
            g[:n] = torch.from_numpy(grads[b][t.rank])
            w[:n] = torch.from_numpy(w0[b])
            hs.append(eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=LR, grad_scale=1.0 / N, weight_decay=WD, var=v,
                                        defer=True, clip=words, **okw))
            planes.append((w, m, v))
            Ls.append(L)
        eng.commit_group(hs, max_norm=max_norm, grad_scale=1.0 / N)
        for h in hs:
            h.synchronize()
        return [tuple(x.numpy().copy() for x in p) for p in planes], words.numpy().copy(), Ls

    res = fabric.run(fn)
    red = [_reduced(N, algo, codec, grads[b], res[0][2][b], None)[:n] for b, n in enumerate(sizes)]
    ref_words = O.clip_words(O.clip_sumsq(np.concatenate(red)), 1.0 / N, max_norm)
    gs = O.clip_scale(1.0 / N, ref_words)
    assert 0 < ref_words[0] < 1
    for r in range(N):
        assert np.array_equal(res[r][1], ref_words)
        for b, n in enumerate(sizes):
            z = np.zeros(n, np.float32)
            if opt == "adamw":
                rw, rm, rv = O.adamw(w0[b], red[b], z, z, O.adamw_scalars(LR, WD, 0.9, 0.999, 1e-8, 1), gs)
            else:
                s = O.lamb_scalars(LR, WD, 0.9, 0.999, 1e-8, 1)
                rm, rv, rr = O.lamb_moments(w0[b], red[b], z, z, s, gs)
                rw = O.lamb_apply(w0[b], rm, rv, s, O.lamb_ratio(w0[b], rr, n, LR), n)
            for got, ref in zip(res[r][0][b], (rw, rm, rv)):
                assert np.array_equal(got[:n], ref)


def _data(sizes, rows=16, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rows, sizes[0], generator=g) * 2 - 1,
            torch.randint(0, sizes[-1], (rows,), generator=g, dtype=torch.int32))


def _train(engine_kind, max_grad_norm, steps=3, **kw):
    sizes = [32, 64, 32]
    eng = None
    if engine_kind == "python":
        eng = CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu")
    pad = (lambda n: eng.layout(n).n_pad) if eng is not None else None
    adam = kw.get("optimizer") == "adamw"
    model = MLP(sizes, dtype=torch.float32, device="cpu", seed=3, bias=True, pad_fn=pad, momentum=not adam, adam=adam)
    tr = DataParallelTrainer(model, eng, lr=LR, weight_decay=WD, momentum=0.0 if adam else MOM,
                             max_grad_norm=max_grad_norm, **kw)
    x, y = _data(sizes)
    norms = []
    for _ in range(steps):
        tr.step(x, y)
        tr.finish()
        if tr.grad_norm is not None:
            norms.append(tr.grad_norm.numpy().copy())
    return model, tr, norms


@pytest.mark.parametrize("engine_kind", ["none", "python"])
@pytest.mark.parametrize("kw", [dict(), dict(optimizer="adamw"), dict(optimizer="adamw", trust_ratio=True)],
                         ids=["sgd", "adamw", "lamb"])
def test_trainer_unclipped_step_is_bit_identical(engine_kind, kw):
    plain, tp, _ = _train(engine_kind, None, **kw)
    big, tb, norms = _train(engine_kind, 1e30, **kw)
    assert tp.grad_norm is None and tb.grad_norm.shape == (4,)
    for a, b in zip(plain.layers, big.layers):
        assert torch.equal(a.master, b.master) and torch.equal(a.mom, b.mom)
    assert all(w[0] == 1.0 and w[1] > 0 and w[2] == np.float32(1e30) and w[3] == 0 for w in norms)
    small, _, norms = _train(engine_kind, float(norms[0][1]) / 2, **kw)
    assert 0.49 < norms[0][0] < 0.5
    assert not any(torch.equal(a.master, b.master) for a, b in zip(plain.layers, small.layers))


def test_trainer_without_engine_matches_oracle():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True, momentum=True)
    tr = DataParallelTrainer(model, None, lr=LR, weight_decay=WD, momentum=MOM, max_grad_norm=0.05)
    prev = [(l.master.numpy().copy(), l.mom.numpy().copy()) for l in model.layers]
    tr.step(*_data(sizes))
    tr.finish()
    grads = [l.grad.numpy()[: l.n] for l in model.layers]
    words = O.clip_words(O.clip_sumsq(np.concatenate(grads[::-1])), 1.0, 0.05)
    assert np.array_equal(tr.grad_norm.numpy(), words) and 0 < words[0] < 1
    gs = O.clip_scale(1.0, words)
    for l, g, (w0, m0) in zip(model.layers, grads, prev):
        rw, rm = O.sgd(w0[: l.n], g, LR, gs, WD, MOM, m0[: l.n])
        assert np.array_equal(l.master.numpy()[: l.n], rw) and np.array_equal(l.mom.numpy()[: l.n], rm)


def test_cli_flag():
    args = ["2", "32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0"]
    out = io.StringIO()
    mlp_mpi.run(args + ["--clip-grad-norm", "0.01"], out=out)
    assert out.getvalue()


def _eng(**kw):
    return CompressedAllReduce(ThreadFabric(1).transport(0), device="cpu", **kw)


def _ordinary(eng, n=100):
    """An ordinary request still completes on the engine."""
    L = eng.layout(n)
    g, w = torch.ones(L.n_pad), torch.zeros(L.n_pad)
    eng.allreduce_sgd(g, w, n_valid=n, lr=1.0).synchronize()
    assert torch.all(w[:n] == -1.0)


def test_refusals():
    eng = _eng()
    n = 100
    L = eng.layout(n)
    g, w = torch.ones(L.n_pad), torch.zeros(L.n_pad)
    words = torch.zeros(4)
    ok = dict(n_valid=n, lr=1.0, defer=True, clip=words)
    with pytest.raises(ValueError, match="must be deferred"):
        eng.allreduce_sgd(g, w, **{**ok, "defer": False})
    with pytest.raises(ValueError, match="four f32 words"):
        eng.allreduce_sgd(g, w, **{**ok, "clip": torch.zeros(3)})
    with pytest.raises(ValueError, match="four f32 words"):
        eng.allreduce_sgd(g, w, **{**ok, "clip": torch.zeros(4, dtype=torch.float64)})
    _ordinary(eng)
    ring = _eng(algo="ring", compat_owner_fp32=True)
    with pytest.raises(ValueError, match="compat_owner_fp32"):
        ring.allreduce_sgd(torch.ones(ring.layout(n).n_pad), w, **ok)
    _ordinary(ring)
    # a lone commit / wait / synchronize of a clipped request
    h = eng.allreduce_sgd(g, w, **ok)
    for call in (h.commit, h.commit_after_current, h.synchronize):
        with pytest.raises(ValueError, match=LIMIT):
            call()
    assert h.pending and torch.all(w == 0), "refused: nothing was updated"
    # commit_group's checks
    other = eng.allreduce_sgd(g, w, **{**ok, "clip": torch.zeros(4)})
    plain = eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, defer=True)
    with pytest.raises(ValueError, match="same clip words"):
        eng.commit_group([h, other], max_norm=1.0)
    with pytest.raises(ValueError, match="not submitted with clip"):
        eng.commit_group([h, plain], max_norm=1.0)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_norm"):
            eng.commit_group([h], max_norm=bad)
    with pytest.raises(ValueError, match="no request"):
        eng.commit_group([], max_norm=1.0)
    with pytest.raises(ValueError, match=LIMIT):
        eng.commit_group([h] * 9, max_norm=1.0)
    with pytest.raises(ValueError, match="named twice"):
        eng.commit_group([h, h], max_norm=1.0)
    with pytest.raises(ValueError, match="another engine"):
        _eng().commit_group([h], max_norm=1.0)
    plain.commit()
    eng.commit_group([other], max_norm=1e30)
    eng.commit_group([h], max_norm=1e30)
    with pytest.raises(ValueError, match="not pending"):
        eng.commit_group([h], max_norm=1.0)
    assert torch.all(w[:n] == -3.0) and words[0] == 1.0
    _ordinary(eng)


def test_ninth_deferred_clipped_request_is_refused():
    eng = _eng()
    n = 100
    L = eng.layout(n)
    words = torch.zeros(4)
    bufs = [(torch.ones(L.n_pad), torch.zeros(L.n_pad)) for _ in range(9)]
    hs = [eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, defer=True, clip=words) for g, w in bufs[:8]]
    with pytest.raises(ValueError, match=LIMIT):
        eng.allreduce_sgd(*bufs[8], n_valid=n, lr=1.0, defer=True, clip=words)
    with pytest.raises(ValueError, match=LIMIT):  # an unclipped request would force the same commit
        eng.allreduce_sgd(*bufs[8], n_valid=n, lr=1.0)
    assert all(h.pending for h in hs) and all(torch.all(w == 0) for _, w in bufs), "never a stale coefficient"
    eng.commit_group(hs, max_norm=1e30)
    assert all(torch.all(w[:n] == -1.0) for _, w in bufs[:8]) and torch.all(bufs[8][1] == 0)
    _ordinary(eng)


def test_trainer_refusals():
    with pytest.raises(ValueError, match="at most 8"):
        DataParallelTrainer(MLP([16] * 10, dtype=torch.float32), None, max_grad_norm=1.0)
    model = MLP([32, 32], dtype=torch.float32)
    for bad in (0.0, -2.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_grad_norm"):
            DataParallelTrainer(model, None, max_grad_norm=bad)

    class Sharded:  # what the trainer reads of a sharded-update engine
        world, shard_update = 2, True

    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, Sharded(), max_grad_norm=1.0)
    assert DataParallelTrainer(model, None).grad_norm is None
