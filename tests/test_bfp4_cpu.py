"""The 4-bit-mantissa BFP wire codec ``bfp4_rne`` (id 4), CPU side: the NumPy oracle, error feedback through it, the
simulators, the Python engine over ThreadFabric, the trainer and the CLI flag.

Definition (group of 16, E = max biased f32 exponent): q = clamp(rint(x * 2^(129-E)), -7, 7), decode q * 2^(E-129),
E = 255 -> NaN; byte i of a group's 8 mantissa bytes holds value 2i in bits [3:0] and value 2i+1 in bits [7:4]; a
shard of n_s elements is [nib[n_s/2]][exp[n_s/16]]."""
import io

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.cli import mlp_mpi
from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import gate, sim
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

C4 = "bfp4_rne"
T = 64


def _issue_input():
    """tests/test_error_feedback_cpu.py::_issue_input: normal values under a log-normal scale."""
    rng = np.random.default_rng(0)
    n = 4096
    return (rng.standard_normal(n) * np.exp(rng.standard_normal(n) * 2)).astype(np.float32)


def _group_max(g):
    return np.repeat(np.abs(g).reshape(-1, 16).max(axis=1), 16).astype(np.float64)


def _fields(buf, n_s, shards=1):
    """(q int [shards * n_s], E int [shards * n_s / 16]) read straight from the bytes, independent of O.unpack."""
    sb = 9 * n_s // 16
    qs, Es = [], []
    for s in range(shards):
        sh = np.asarray(buf[s * sb:(s + 1) * sb], np.uint8)
        nib = sh[: n_s // 2].astype(np.int32)
        q = np.stack([nib & 0xF, nib >> 4], 1).reshape(-1)
        qs.append(np.where(q >= 8, q - 16, q))
        Es.append(sh[n_s // 2:].astype(np.int32))
    return np.concatenate(qs), np.concatenate(Es)


# --------------------------------------------------------------------------- oracle
def test_codec_id_and_shard_bytes():
    assert O.CODECS[C4] == 4 and O.codec_id(C4) == 4 and O.CODEC_NAMES[4] == C4
    for n_s in (256, 512, 4352, 1 << 20):
        assert O.shard_bytes(C4, n_s) == 9 * n_s // 16 == wire.shard_bytes(4, n_s)
        assert O.shard_bytes(C4, n_s) % 16 == 0, "every shard start and exponent plane stays 16-B aligned"
    assert not wire.is_raw(C4)
    # today's codecs keep their sizes
    assert [O.shard_bytes(c, 256) for c in range(4)] == [272, 272, 1024, 512]


def test_pack_unpack_is_quantize_and_the_definition():
    rng = np.random.default_rng(1)
    n_s, shards = 512, 3
    x = (rng.standard_normal(n_s * shards) * np.exp(rng.standard_normal(n_s * shards) * 3)).astype(np.float32)
    buf = O.pack(x, n_s, C4)
    assert buf.dtype == np.uint8 and buf.size == shards * 9 * n_s // 16
    dec = O.unpack(buf, x.size, n_s, C4)
    assert np.array_equal(dec.view(np.uint32), O.quantize(x, C4).view(np.uint32))
    q, E = _fields(buf, n_s, shards)
    assert np.abs(q).max() <= 7
    assert np.array_equal(E, (np.abs(x).view(np.uint32).reshape(-1, 16).max(axis=1) >> 23))
    exp = np.ldexp(q.astype(np.float64), np.repeat(E, 16) - 129)
    assert np.array_equal(dec.astype(np.float64), exp), "every decoded value is q * 2^(E-129), exactly"
    # q is the nearest integer (ties to even), clamped
    s = np.ldexp(x.astype(np.float64), 129 - np.repeat(E, 16))
    assert np.array_equal(q, np.clip(np.rint(s), -7, 7).astype(np.int64))
    # the error bound of the definition: half a unit, or up to one unit where the clamp bites (|s| in (7.5, 8))
    assert (np.abs(s - q) <= np.where(np.abs(s) > 7.5, 1.0, 0.5)).all()
    assert np.array_equal(O.quantize(dec, C4).view(np.uint32), dec.view(np.uint32)), "quantize is idempotent"


def test_nibble_order_on_a_hand_written_group():
    # E = 129: one unit is 1.0
    g = np.array([1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6, 7, -7, 0, 1], np.float32)
    x = np.zeros(256, np.float32)
    x[:16] = g
    buf = O.pack(x, 256, C4)
    assert buf.size == 144
    assert list(buf[:8]) == [0xF1, 0xE2, 0xD3, 0xC4, 0xB5, 0xA6, 0x97, 0x10]
    assert not buf[8:128].any() and buf[128] == 129 and not buf[129:].any()
    assert np.array_equal(O.unpack(buf, 256, 256, C4)[:16], g)
    assert np.array_equal(O.unpack_nibbles(O.pack_nibbles(np.arange(-8, 8, dtype=np.int8))), np.arange(-8, 8))


def test_special_groups():
    x = np.zeros(256, np.float32)
    x[16:32] = np.linspace(-1, 1, 16)
    x[20] = np.nan                          # group 1: NaN
    x[32:48] = 1.0
    x[33] = np.inf                          # group 2: +Inf
    x[49] = -np.inf                         # group 3: -Inf among zeros
    x[64:80] = np.float32(1e-40) * np.arange(-8, 8)   # group 4: denormals
    x[80] = -0.0                            # group 5: -0.0 among zeros
    x[96:112] = [8, 7.5, 7.75, -7.5, -7.9, 6.5, 5.5, -6.5, 0.5, -0.5, 1.5, -1.5, 2.5, 0.49, -0.51, 15.9]  # group 6
    buf = O.pack(x, 256, C4)
    dec = O.unpack(buf, 256, 256, C4)
    q, E = _fields(buf, 256)
    assert not dec[:16].any() and E[0] == 0 and not q[:16].any() and not np.signbit(dec[:16]).any(), "exact zeros"
    for grp in (1, 2, 3):
        assert E[grp] == 255 and np.isnan(dec[16 * grp:16 * grp + 16]).all()
    assert q[20] == -7 and q[33] == 7 and q[49] == -7 and q[32] == 0, "NaN -> -7, +-Inf -> +-7, finite -> 0"
    # denormals: E = 0, unit 2^-129 = 1.47e-39; the values are k * 1e-40 = k * 0.068 units: -8 rounds to -1, the rest to 0
    assert E[4] == 0 and list(q[64:80]) == [-1] + [0] * 15
    assert np.array_equal(dec[64:80].astype(np.float64), np.ldexp(q[64:80].astype(np.float64), -129))
    big = np.zeros(256, np.float32)
    big[:16] = np.ldexp(np.float32(1), -127) * np.array([1, -1, 0.75, 0.25, -0.5, 0.5, 0.625, 0] * 2, np.float32)
    qb, Eb = _fields(O.pack(big, 256, C4), 256)
    assert Eb[0] == 0 and list(qb[:8]) == [4, -4, 3, 1, -2, 2, 2, 0], "denormal group: unit 2^-129, ties to even"
    assert np.array_equal(O.quantize(big, C4)[:16].astype(np.float64), np.ldexp(qb[:16].astype(np.float64), -129))
    # -0.0 among zeros: E = 0, q = 0, decodes to zero
    assert E[5] == 0 and not q[80:96].any() and not dec[80:96].any()
    # group 6: max 15.9 -> E = 130, unit 2.0: s = [4, 3.75, 3.875, -3.75, -3.95, 3.25, 2.75, -3.25, .25, -.25, .75,
    # -.75, 1.25, .245, -.255, 7.95]
    assert E[6] == 130 and list(q[96:112]) == [4, 4, 4, -4, -4, 3, 3, -3, 0, 0, 1, -1, 1, 0, 0, 7]
    # values that round to +-8 are clamped to +-7; +-7.5 units tie to 8 and clamp too
    c = np.zeros(256, np.float32)
    c[:8] = [15.9, -15.9, 15.0, -15.0, 14.0, -14.0, 13.0, 1.0]   # unit 2: 7.95, -7.95, 7.5, -7.5, 7, -7, 6.5, .5
    qc, Ec = _fields(O.pack(c, 256, C4), 256)
    assert Ec[0] == 130 and list(qc[:8]) == [7, -7, 7, -7, 7, -7, 6, 0]
    assert list(O.quantize(c, C4)[:8]) == [14, -14, 14, -14, 14, -14, 12, 0]


# --------------------------------------------------------------------------- error feedback
def test_ef_zero_plane_gives_packs_bytes():
    rng = np.random.default_rng(2)
    s, N = 512, 3
    g = rng.standard_normal(s * N).astype(np.float32)
    zero = np.zeros(s * N, np.float32)
    for self_shard in (-1, 1):
        w, e = O.ef_pack(g, zero, s, C4, self_shard)
        assert np.array_equal(w, O.pack(g, s, C4)) and not zero.any()
        exp = (g - O.quantize(g, C4)).astype(np.float32)
        if self_shard >= 0:
            exp[self_shard * s:(self_shard + 1) * s] = 0
        assert np.array_equal(e, exp)
    sb = O.shard_bytes(C4, s)
    packed = O.pack(g, s, C4)
    slots = [packed[r * sb:(r + 1) * sb] for r in range(N)]
    local = rng.standard_normal(s).astype(np.float32)
    for self_pos in range(N):
        w, e = O.ef_reduce(slots, local, self_pos, zero[:s], C4, s)
        acc = O.reduce_slots(slots, local, self_pos, C4, s)
        assert np.array_equal(w, O.pack(acc, s, C4))
        assert np.array_equal(e, (acc - O.quantize(acc, C4)).astype(np.float32))
    # the CPU wire ops follow the oracle
    e_t = torch.zeros(s * N)
    out = torch.zeros(sb * N, dtype=torch.uint8)
    wire.pack_ef(torch.from_numpy(g), e_t, out, s, C4, self_shard=1)
    w_ref, e_ref = O.ef_pack(g, zero, s, C4, 1)
    assert np.array_equal(out.numpy(), w_ref) and np.array_equal(e_t.numpy(), e_ref)
    er, o1 = torch.zeros(s), torch.zeros(sb, dtype=torch.uint8)
    wire.reduce_ef(torch.from_numpy(packed.copy()), N, 2, torch.from_numpy(local), er, o1, s, C4)
    w_ref, e_ref = O.ef_reduce(slots, local, 2, zero[:s], C4, s)
    assert np.array_equal(o1.numpy(), w_ref) and np.array_equal(er.numpy(), e_ref)


def _iterate(g, steps, via):
    """tests/test_error_feedback_cpu.py::_iterate for the new codec."""
    n = g.size
    e = np.zeros(n, np.float32)
    hist = []
    for _ in range(steps):
        x = (g + e).astype(np.float32)
        if via == "pack":
            w, e2 = O.ef_pack(g, e, n, C4, -1)
            q = O.unpack(w, n, n, C4)
        elif via == "reduce":
            w, e2 = O.ef_reduce([np.zeros(0, np.uint8)], g, 0, e, C4, n)
            q = O.unpack(w, n, n, C4)
        else:
            q, planes = sim.mesh_allreduce_ef([g], [e], n, C4)
            e2 = planes[0]
        assert e2.dtype == np.float32 and e2.shape == (n,) and q.shape == (n,)
        hist.append((x, q, e))
        e = e2
    return hist, e


@pytest.mark.parametrize("via", ["pack", "reduce", "sim"])
def test_convergence(via):
    """max over all elements of |mean_t q_t - g| / group max |g| at T = 64 is at most 1/16 of the same quantity without
    feedback, and every stored residual is the exact float64 difference x - q."""
    g = _issue_input()
    gm = _group_max(g)
    base = (np.abs(O.quantize(g, C4).astype(np.float64) - g) / gm).max()
    hist, e_T = _iterate(g, T, via)
    assert np.array_equal(hist[0][1], O.quantize(g, C4)), "step 1 (zero plane) is the codec without feedback"
    nxt = [h[2] for h in hist[1:]] + [e_T]
    for (x, q, _), e2 in zip(hist, nxt):
        assert np.array_equal(e2.astype(np.float64), x.astype(np.float64) - q.astype(np.float64))
    for steps in (16, 64):
        mean = np.mean(np.stack([q.astype(np.float64) for _, q, _ in hist[:steps]]), axis=0)
        fed = (np.abs(mean - g) / gm).max()
        print(f"{C4} via {via}: no feedback {base:.3e}, T={steps} {fed:.3e}, ratio 1/{base / fed:.1f}")
    assert fed <= base / 16, (fed, base)


def test_four_rank_accumulated_sum():
    """Fresh gradients per step on 4 ranks: the 64-step accumulated decoded sum against the float64 sum."""
    rng = np.random.default_rng(1)
    N, shard, steps = 4, 256, 64
    n = shard * N
    base = [(rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32) for _ in range(N)]
    planes = [np.zeros(n, np.float32) for _ in range(N)]
    exact, acc_ef, acc_plain = np.zeros(n), np.zeros(n), np.zeros(n)
    for _ in range(steps):
        grads = [(b + 0.3 * rng.standard_normal(n) * np.abs(b)).astype(np.float32) for b in base]
        out, planes = sim.mesh_allreduce_ef(grads, planes, shard, C4)
        acc_ef += out.astype(np.float64)
        acc_plain += sim.mesh_allreduce(grads, shard, C4).astype(np.float64)
        exact += np.sum([g.astype(np.float64) for g in grads], axis=0)
    err_ef = np.linalg.norm(acc_ef - exact) / np.linalg.norm(exact)
    err_plain = np.linalg.norm(acc_plain - exact) / np.linalg.norm(exact)
    print(f"{C4} 4-rank 64-step accumulated sum: relative L2 error {err_plain:.3e} without feedback, {err_ef:.3e} "
          f"with, ratio 1/{err_plain / err_ef:.1f}")
    assert err_ef <= err_plain / 8, (err_ef, err_plain)


# --------------------------------------------------------------------------- the Python engine
STEPS = 3
ADAM = dict(lr=0.01, weight_decay=0.1, betas=(0.9, 0.99), eps=1e-6)


def _grads(N, n, seed):
    return [gate.seeded_gradients(n, N, seed + t) for t in range(STEPS)]


def _engine_run(t, grads, n, algo, opt, ef, force):
    eng = CompressedAllReduce(t, codec=C4, algo=algo, rings=2 if algo == "ring" else 1, device="cpu",
                              force_comm=force, max_slice_elems=256)
    L = eng.layout(n)
    rng = np.random.default_rng(99)
    w = torch.zeros(L.n_pad)
    w[:n] = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    w0 = w.numpy().copy()
    m, v = torch.zeros(L.n_pad), torch.zeros(L.n_pad)
    e = torch.zeros(L.n_pad) if ef else None
    sums, hist = [], []
    for step in range(STEPS):
        g, out = torch.zeros(L.n_pad), torch.zeros(L.n_pad)
        g[:n] = torch.from_numpy(grads[step][t.rank])
        if ef:  # the planes advance once per step: the sum-only request is this step's request
            kw = dict(residual=e)
            e_before = e.clone()
            eng.allreduce(g, out, n_valid=n, **kw).synchronize()
            e_after = e.clone()
            e.copy_(e_before)
        else:
            kw = {}
            eng.allreduce(g, out, n_valid=n).synchronize()
        if opt == "adamw":
            eng.allreduce_sgd(g, w, None, m, n_valid=n, opt="adamw", var=v, step=step + 1, grad_scale=1.0 / t.world,
                              **ADAM, **kw).synchronize()
        else:
            eng.allreduce_sgd(g, w, None, m, n_valid=n, lr=0.05, momentum=0.9, grad_scale=1.0 / t.world,
                              **kw).synchronize()
        if ef:
            assert torch.equal(e, e_after), "the update request feeds back what the sum-only request did"
        sums.append(out.numpy().copy())
        hist.append((w.numpy().copy(), m.numpy().copy(), v.numpy().copy(), None if e is None else e.numpy().copy()))
    return dict(sums=sums, hist=hist, w0=w0, L=L, eng_orders=eng.orders, algo=algo)


def _check_engine(res, grads, n, N, algo, opt, ef):
    L = res[0]["L"]

    class Spec:  # what gate.reference_sum reads of an engine
        codec, world = C4, N
        orders = res[0]["eng_orders"]

        def layout(self, _n):
            return L

    Spec.algo = algo
    planes = [np.zeros(L.n_pad, np.float32) for _ in range(N)]
    for r in range(N):
        w, m, v = res[r]["w0"][:n].copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
        pl = [p.copy() for p in planes]
        for step in range(STEPS):
            if ef:
                gin = [np.pad(g, (0, L.n_pad - n)) for g in grads[step]]
                ref, pl = sim.mesh_allreduce_ef(gin, pl, L.shard, C4)
                assert np.array_equal(res[r]["hist"][step][3], pl[r]), (r, step)
            else:
                ref = gate.reference_sum(Spec(), grads[step], n, r)
            assert np.array_equal(res[r]["sums"][step].view(np.uint32), ref.view(np.uint32)), (r, step)
            if opt == "adamw":
                sc = O.adamw_scalars(ADAM["lr"], ADAM["weight_decay"], *ADAM["betas"], ADAM["eps"], step + 1)
                w, m, v = O.adamw(w, ref[:n], m, v, sc, 1.0 / N)
            else:
                w, m = O.sgd(w, ref[:n], 0.05, 1.0 / N, 0.0, 0.9, m)
            gw, gm, gv, _ = res[r]["hist"][step]
            assert np.array_equal(gw[:n].view(np.uint32), w.view(np.uint32)), (r, step)
            assert np.array_equal(gm[:n].view(np.uint32), m.view(np.uint32)), (r, step)
            if opt == "adamw":
                assert np.array_equal(gv[:n].view(np.uint32), v.view(np.uint32)), (r, step)
    for r in range(1, N):
        assert np.array_equal(res[r]["hist"][-1][0], res[0]["hist"][-1][0]), "replicas stay bit-identical"


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("algo,ef", [("mesh", False), ("mesh", True), ("ring", False)])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_python_engine_threadfabric(N, algo, ef, opt):
    n = 2000
    grads = _grads(N, n, 500 + N)
    res = ThreadFabric(N, timeout_s=60).run(lambda t: _engine_run(t, grads, n, algo, opt, ef, force=N == 1))
    _check_engine(res, grads, n, N, algo, opt, ef)
    if algo == "ring":
        assert res[0]["L"].blocks > 1, "more than one slice block per ring part"


def test_python_engine_existing_refusals_hold():
    eng = CompressedAllReduce(ThreadFabric(1).transport(0), codec=C4, algo="ring", device="cpu")
    L = eng.layout(100)
    with pytest.raises(ValueError, match="ring schedule"):
        eng.allreduce_sgd(torch.ones(L.n_pad), torch.zeros(L.n_pad), n_valid=100, lr=1.0,
                          residual=torch.zeros(L.n_pad))


# --------------------------------------------------------------------------- trainer and CLI
def _data(sizes, mb=16):
    g = torch.Generator().manual_seed(5)
    return (torch.rand(mb, sizes[0], generator=g) * 2 - 1,
            torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32))


def test_trainer_local_step_matches_oracle():
    sizes = [32, 64, 32]
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True)
    tr = DataParallelTrainer(model, None, lr=0.05, error_feedback=True, error_feedback_codec=C4)
    assert tr.ef_codec == C4
    x, y = _data(sizes)
    planes = [np.zeros(l.n_pad, np.float32) for l in model.layers]
    for _ in range(2):
        prev = [l.master.numpy().copy() for l in model.layers]
        tr.step(x, y)
        tr.finish()
        for i, l in enumerate(model.layers):
            yv = (l.grad.numpy() + planes[i]).astype(np.float32)
            q = O.quantize(yv, C4)
            planes[i] = (yv - q).astype(np.float32)
            w, _ = O.sgd(prev[i][: l.n], q[: l.n], 0.05)
            assert np.array_equal(l.master.numpy()[: l.n], w)
            assert np.array_equal(tr.residuals[i].numpy(), planes[i]) and planes[i].any()


def test_trainer_with_python_engine_and_error_feedback():
    sizes = [32, 64, 32]
    eng = make_engine(ThreadFabric(1).transport(0), "bfp4", device="cpu")
    assert eng.codec == C4 and eng.codec_id == 4 and not getattr(eng, "prepack", False)
    model = MLP(sizes, dtype=torch.float32, seed=3, bias=True, pad_fn=lambda n: eng.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=0.05, error_feedback=True)
    assert tr.ef_codec == C4 and not tr.prepack and not tr.fused_update
    local = MLP(sizes, dtype=torch.float32, seed=3, bias=True, pad_fn=lambda n: eng.layout(n).n_pad)
    tl = DataParallelTrainer(local, None, lr=0.05, error_feedback=True, error_feedback_codec=C4)
    x, y = _data(sizes)
    for _ in range(2):
        for t in (tr, tl):
            t.step(x, y)
            t.finish()
    for a, b in zip(model.layers, local.layers):
        assert torch.equal(a.master, b.master)
    for a, b in zip(tr.residuals, tl.residuals):
        assert torch.equal(a, b) and a.any()


def test_make_engine_and_cli_flag():
    with pytest.raises(ValueError, match="bfp4"):
        make_engine(ThreadFabric(1).transport(0), "bfp4", rounding="trunc", device="cpu")
    assert make_engine(ThreadFabric(1).transport(0), "bfp", rounding="trunc", device="cpu").codec == "bfp_trunc"
    args = ["1", "32", "0", "A", "1", "1", "1", "64", "64", "32", "--device", "cpu", "--dtype", "f32", "--warmup", "0"]
    parse = lambda *f: mlp_mpi.config_from_args(mlp_mpi.build_parser().parse_args(args + list(f)))  # noqa: E731
    assert parse("--compress", "bfp4").compress == "bfp4" and parse().compress == "bfp"
    with pytest.raises(ValueError, match="bfp4"):
        parse("--compress", "bfp4", "--rounding", "trunc")
    out = io.StringIO()
    r = mlp_mpi.run(["2"] + args[1:] + ["--compress", "bfp4", "--error-feedback"], out=out)
    assert out.getvalue() and r["trainer"].engine.codec == C4 and r["trainer"].ef_codec == C4
    assert all(bool(e.any()) for e in r["trainer"].residuals)
    with pytest.raises(ValueError, match="bfp4"):
        mlp_mpi.run(args + ["--compress", "bfp4", "--rounding", "trunc"], out=io.StringIO())
