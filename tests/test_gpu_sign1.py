"""The 1-bit sign wire codec ``sign1`` on the GPU: every wire op against the NumPy oracle byte for byte and bit for bit
(NaNs matched by position), the C++ engine over virtual ranks against the mesh simulator, and the refusals."""
import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.models.mlp import MLP
from fpga_ai_nic_amd.ops import bfp_oracle as O, wire
from fpga_ai_nic_amd.parallel import gate, sim
from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
from fpga_ai_nic_amd.parallel.transport import ThreadFabric
from test_gpu_bfp4 import EF_STEPS, N_ELEMS, _ef_steps, _same, _sentinel_ok, _threads, _values, _wire_buf

pytestmark = pytest.mark.gpu

DEV, S1 = "cuda", "sign1"
# (shard elements, shards): the smallest legal shard; sign and exponent gathers across a wave and a shard boundary
SHAPES = [(256, 1), (4096 + 256, 3)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_pack_unpack_pack_range(C, n_s, n_sh, dtype):
    n, sb = n_s * n_sh, wire.shard_bytes(S1, n_s)
    x = _values(n, dtype, n_s)[1]  # (zero, denormal, Inf / NaN and -0.0 groups included)
    # two groups at the E = 0 / 1 boundary: a_j = 2^23 - 1 and 0.5 denormal units; the half unit must round away
    # before the add (S = (2^23 - 1) * 2^-149, E = 0), a fused multiply-add keeps it (S = 2^-126, E = 1)
    x[144:176] = 0.0
    x[[144, 161]], x[[145, 160]] = np.ldexp(np.float32(8), -149), np.ldexp(np.float32(2 ** 27 - 16), -149)
    x_dev = torch.from_numpy(x).to(dtype).to(DEV)
    x = x_dev.float().cpu().numpy()
    ref, out = O.pack(x, n_s, S1), _wire_buf(S1, n_s, n_sh)
    assert sb == 3 * n_s // 16 and (dtype == torch.bfloat16 or list(ref[n_s // 8 + 9: n_s // 8 + 11]) == [0, 0])
    wire.pack(x_dev, out, n_s, S1)
    assert np.array_equal(out.cpu().numpy()[: sb * n_sh], ref) and _sentinel_ok(out, sb * n_sh)
    for odt in DTYPES:
        dec = torch.full((n + 16,), 7.0, dtype=odt, device=DEV)
        wire.unpack(out[: sb * n_sh], dec[:n], n_s, S1)
        assert _same(dec[:n].float().cpu().numpy(), O.unpack(ref, n, n_s, S1)) and bool((dec[n:] == 7.0).all())
    # the pair-of-lanes form: two flat ranges that meet inside the last shard (across the boundary when there is one)
    got = _wire_buf(S1, n_s, n_sh)
    for begin, end in ((n - 48, n), (0, n - 48)):
        C.wire_pack_range(x_dev, got, n_s, begin, end, 5)
    assert np.array_equal(got.cpu().numpy()[: sb * n_sh], ref) and _sentinel_ok(got, sb * n_sh)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("n_s", [256, 4096 + 256])
def test_reduce(n_s, n_slots, dtype):
    sb = wire.shard_bytes(S1, n_s)
    packed = O.pack(_values(n_slots * n_s, torch.float32, 11 * n_slots + n_s)[1], n_s, S1)
    # (a finite local operand: every NaN of the sum then comes from a decoded slot and is positive)
    l_dev, l_np = _values(n_s, dtype, n_slots + n_s + 1, special=False)
    acc = O.reduce_slots([packed[r * sb:(r + 1) * sb] for r in range(n_slots)], l_np, n_slots - 1, S1, n_s)
    ow, of = _wire_buf(S1, n_s, 1), torch.zeros(n_s, device=DEV)
    wire.reduce(torch.from_numpy(packed).to(DEV), n_slots, n_slots - 1, l_dev, ow[:sb], of, n_s, S1)
    assert np.array_equal(ow.cpu().numpy()[:sb], O.pack(acc, n_s, S1)) and _sentinel_ok(ow, sb)
    assert _same(of.cpu().numpy(), acc)


@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_pack_ef_and_reduce_ef(n_s, n_sh):
    """Two consecutive trips of each stage: the second consumes the residual the first left."""
    n, sb = n_s * n_sh, wire.shard_bytes(S1, n_s)
    e_ref, e = np.zeros(n, np.float32), torch.zeros(n, device=DEV)
    o_ref, o = np.zeros(n_s, np.float32), torch.zeros(n_s, device=DEV)
    self_shard = n_sh - 1 if n_sh > 1 else -1
    for trip in range(2):
        g_dev, g = _values(n, DTYPES[1 - trip], n_s + trip, special=trip == 1)  # (f32: every NaN is positive)
        out, ow = _wire_buf(S1, n_s, n_sh), _wire_buf(S1, n_s, 1)
        wire.pack_ef(g_dev, e, out, n_s, S1, self_shard=self_shard)
        w_ref, e_ref = O.ef_pack(g, e_ref, n_s, S1, self_shard)
        assert np.array_equal(out.cpu().numpy()[: sb * n_sh], w_ref) and _sentinel_ok(out, sb * n_sh)
        assert _same(e.cpu().numpy(), e_ref) and e_ref.any() and (n_sh == 1 or not e_ref[n - n_s:].any())
        wire.reduce_ef(out[: sb * n_sh], n_sh, 0, g_dev[:n_s], o, [ow[:sb]], n_s, S1)
        w_ref, o_ref = O.ef_reduce([w_ref[r * sb:(r + 1) * sb] for r in range(n_sh)], g[:n_s], 0, o_ref, S1, n_s)
        assert np.array_equal(ow.cpu().numpy()[:sb], w_ref) and _sentinel_ok(ow, sb) and _same(o.cpu().numpy(), o_ref)


@pytest.mark.parametrize("kind", ["sgd", "adamw", "lion"])
def test_update_kernels(kind):
    """n_valid inside a group; the oracle's update of the oracle's decoded values, bit for bit (the bfp4 tests' bound)."""
    n_s, n_sh = SHAPES[1]
    n, nv = n_s * n_sh, n_s * n_sh - 16 - 5
    buf = O.pack(_values(n, torch.float32, 5, special=False)[1], n_s, S1)
    g, rng = O.unpack(buf, n, n_s, S1)[:nv], np.random.default_rng(6)
    p0 = [(rng.standard_normal(n) * s).astype(np.float32) ** k for s, k in ((1, 1), (0.1, 1), (0.1, 2))]
    w, m, v = (torch.from_numpy(p.copy()).to(DEV) for p in p0)
    wt, (w0, m0, v0) = torch.from_numpy(buf).to(DEV), (p[:nv] for p in p0)
    if kind == "sgd":
        wire.sgd(wt, n_s, n_sh, w, codec=S1, mom=m, n_valid=nv, lr=0.05, grad_scale=0.5, weight_decay=0.01, momentum=0.9)
        ref = O.sgd(w0, g, 0.05, 0.5, 0.01, 0.9, m0)
    elif kind == "adamw":
        sc = O.adamw_scalars(0.01, 0.1, 0.9, 0.99, 1e-6, 3)
        wire.adamw(wt, n_s, n_sh, w, codec=S1, mom=m, var=v, scalars=sc, grad_scale=0.5, n_valid=nv)
        ref = O.adamw(w0, g, m0, v0, sc, 0.5)
    else:
        sc = O.lion_scalars(0.01, 0.1, 0.9, 0.99)
        wire.lion(wt, n_s, n_sh, w, codec=S1, mom=m, scalars=sc, grad_scale=0.5, n_valid=nv)
        ref = O.lion(w0, g, m0, sc, 0.5)
    for got, r, old in zip((w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()), ref, p0):
        assert _same(got[:nv], r) and np.array_equal(got[nv:], old[nv:]), kind


@pytest.mark.parametrize("N", [2, 3])
def test_native_engine_loopback_error_feedback(C, N):
    """test_gpu_bfp4's steps (an allreduce and an allreduce_sgd per step, a plane each) against the simulator."""
    grads = [gate.seeded_gradients(N_ELEMS, N, 700 + 10 * t + N) for t in range(EF_STEPS)]
    w = np.random.default_rng(12).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engs = [NativeAllReduce(None, codec=S1, comm=fabric.comm(r)) for r in range(N)]
    assert all(e.codec_id == 5 and e.prepack is False for e in engs)
    res = _threads(N, lambda r: _ef_steps(engs[r], r, grads, w))
    L = engs[0].layout(N_ELEMS)
    planes = [np.zeros(L.n_pad, np.float32) for _ in range(N)]
    for t in range(EF_STEPS):
        gin = [np.pad(g, (0, L.n_pad - N_ELEMS)) for g in grads[t]]
        ref, planes = sim.mesh_allreduce_ef(gin, planes, L.shard, S1)
        w, _ = O.sgd(w, ref[:N_ELEMS], 0.5)
        for r in range(N):  # (every replica against the one reference: bit-identical)
            out, wg, ea, eb = res[r][t]
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (r, t, "decoded result")
            assert np.array_equal(ea, planes[r]) and np.array_equal(eb, planes[r]) and ea.any(), (r, t, "plane")
            assert np.array_equal(wg[:N_ELEMS].view(np.uint32), w.view(np.uint32)), (r, t, "weights")


def test_refusals(C):
    n = 50000 - 48
    with pytest.raises(ValueError, match="sign"):
        make_engine(ThreadFabric(1).transport(0), "sign", rounding="trunc", impl="native")
    eng = make_engine(ThreadFabric(1).transport(0), "sign", impl="native")
    assert eng.codec == S1 and eng.prepack is False
    model = MLP([1024, 1024, 1024], dtype=torch.bfloat16, device=torch.device(DEV), pad_fn=lambda k: eng.layout(k).n_pad)
    for kw in (dict(), dict(stochastic_rounding=True)):
        with pytest.raises(ValueError, match="sign1 needs error feedback"):
            DataParallelTrainer(model, eng, lr=0.05, **kw)
    L = eng.layout(n)
    g, w, e = (torch.zeros(L.n_pad, device=DEV) for _ in range(3))
    with pytest.raises(ValueError, match="stochastic rounding"):
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, sr_seed=1)
    pre = torch.zeros(wire.shard_bytes(S1, L.n_pad), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="cannot take prepacked input"):
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, prepacked=(pre, 0))
    for kw, match in ((dict(algo="ring"), "ring schedule"), (dict(chunk_elems=8192), "chunked"),
                      (dict(shard_update=True), "sharded")):
        x = NativeAllReduce(None, codec=S1, comm=C.LoopbackFabric(2, 60.0).comm(0), **kw)
        gx, wx, ex = (torch.zeros(x.layout(n).n_pad, device=DEV) for _ in range(3))
        with pytest.raises(ValueError, match=match):
            x.allreduce_sgd(gx, wx, wx.to(torch.bfloat16), n_valid=n, lr=1.0, residual=ex)
    g.fill_(1.0)  # the engine's own requests take the codec with or without a plane; a group of ones is its own mean
    for kw in (dict(), dict(residual=e)):
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, **kw).synchronize(30)
    assert torch.all(w[:n] == -2.0) and not e[:n].any()
