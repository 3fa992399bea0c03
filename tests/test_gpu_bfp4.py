"""The 4-bit-mantissa BFP wire codec ``bfp4_rne`` on the GPU: every wire op against the NumPy oracle byte for byte and
bit for bit, the update kernels against the same kernels on a raw_f32 wire of the oracle's decoded values, the C++
engine over virtual ranks (LoopbackFabric) on every schedule against the simulators, two processes on one GPU over the
direct P2P transport, and the refusals. Every comparison is exact: the kernels perform the oracle's operations per
value. A NaN's payload is not part of the definition: where an update or a residual turns NaN (an Inf/NaN group), the
NaN positions must agree and every other value's bits."""
import math
import os
import queue as _queue
import socket
import threading

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd import _ext
from fpga_ai_nic_amd.ops import bfp_oracle as O
from fpga_ai_nic_amd.ops import wire
from fpga_ai_nic_amd.parallel import gate, sim
from fpga_ai_nic_amd.parallel.allreduce import CompressedAllReduce
from fpga_ai_nic_amd.parallel.native_engine import NativeAllReduce
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

pytestmark = pytest.mark.gpu

DEV = "cuda"
C4 = "bfp4_rne"
PAD = 64            # sentinel bytes past the last shard
# (shard elements, shards): 16 active lanes; a second block that is almost empty
SHAPES = [(256, 1), (4096 + 256, 2)]
# one shard above the grid cap's 2048 blocks x 4096 elements (a group per lane; the update kernels' 8 values per lane
# wrap at half of that): the first lanes take a second trip (the geometry of test_pack_ef_second_trip)
BIG = 2048 * 4096 + 256
DTYPES = [torch.float32, torch.bfloat16]
SGD = dict(lr=0.05, grad_scale=0.5, weight_decay=1e-2, momentum=0.9, nesterov=True)
ADAM = (0.01, 0.1, 0.9, 0.99, 1e-6, 3)  # lr, wd, beta1, beta2, eps, step


def _same(a, b):
    """Bit equality of two f32 arrays, NaNs matched by position."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na],
                                                                            b.view(np.uint32)[~nb])


def _values(n, dtype, seed, special=True):
    """n values: normal under a log-normal scale, the first half with alternating signs inside every byte (an
    unmasked nibble OR or a missing sign extension shows there), and — ``special`` — groups of zeros, denormals,
    Inf / NaN, -0.0 and values at +-7.5 units (ties, and the clamp of what rounds to +-8). Returns the device tensor
    and the f32 values the kernels read."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(np.float32)
    half = n // 2 // 16 * 16
    x[:half] = np.abs(x[:half]) * np.tile(np.array([1, -1], np.float32), half // 2)
    if special:
        x[16:32] = 0.0
        x[32:48] = np.float32(1e-40) * np.arange(-8, 8)
        x[48:64] = np.ldexp(np.float32(1), -127) * np.array([1, -1, 0.75, 0.25, -0.5, 0.5, 0.625, 0] * 2, np.float32)
        x[64:80] = [15.9, -15.9, 15.0, -15.0, 14, -14, 13, 1, 3, -3, 5, -5, 1, -1, 0.5, -0.5]  # unit 2: +-7.5, ties
        x[80:96] = 0.0
        x[81] = -0.0
        x[100] = np.inf
        x[117] = -np.inf
        x[130] = np.nan
    t = torch.from_numpy(x).to(dtype)
    return t.to(DEV), t.to(torch.float32).numpy()


def _wire_buf(codec, n_s, n_sh):
    return torch.full((wire.shard_bytes(codec, n_s) * n_sh + PAD,), 0xA5, dtype=torch.uint8, device=DEV)


def _sentinel_ok(buf, used):
    return bool((buf[used:] == 0xA5).all())


# --------------------------------------------------------------------------- pack / unpack / pack_range
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_pack_unpack_pack_range(C, n_s, n_sh, dtype):
    n, sb = n_s * n_sh, wire.shard_bytes(C4, n_s)
    assert sb == 9 * n_s // 16
    x_dev, x = _values(n, dtype, n_s)
    ref = O.pack(x, n_s, C4)
    out = _wire_buf(C4, n_s, n_sh)
    wire.pack(x_dev, out, n_s, C4)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[: sb * n_sh], ref), "wire bytes"
    assert _sentinel_ok(out, sb * n_sh), "bytes past the last shard untouched"
    dec_ref = O.unpack(ref, n, n_s, C4)
    for odt in DTYPES:
        dec = torch.full((n + 16,), 7.0, dtype=odt, device=DEV)
        wire.unpack(out[: sb * n_sh], dec[:n], n_s, C4)
        torch.cuda.synchronize()
        exp = dec_ref if odt == torch.float32 else O.bf16_bits_to_f32(O.f32_to_bf16_bits(dec_ref))
        assert _same(dec[:n].float().cpu().numpy(), exp), f"decoded {odt}"
        assert bool((dec[n:] == 7.0).all())
    assert np.array_equal(dec_ref[16:32].view(np.uint32), np.zeros(16, np.uint32)), "a zero group: exact zeros"
    assert np.isnan(dec_ref[96:144]).all(), "Inf / NaN groups decode to NaN"
    # the pair-of-lanes form: flat ranges at 16-element offsets, across the shard boundary when there is one
    for begin, end in ((0, n), (16, 48), (n - 16, n), (n_s - 32, min(n, n_s + 48))):
        rng_out = _wire_buf(C4, n_s, n_sh)
        C.wire_pack_range(x_dev, rng_out, n_s, begin, end, 4)
        torch.cuda.synchronize()
        got = rng_out.cpu().numpy()
        exp = np.full(sb * n_sh, 0xA5, np.uint8)
        for g in range(begin // 16, end // 16):
            sh, gl = divmod(g * 16, n_s)
            gl //= 16
            exp[sh * sb + 8 * gl: sh * sb + 8 * gl + 8] = ref[sh * sb + 8 * gl: sh * sb + 8 * gl + 8]
            exp[sh * sb + n_s // 2 + gl] = ref[sh * sb + n_s // 2 + gl]
        assert np.array_equal(got[: sb * n_sh], exp), (begin, end)
        assert _sentinel_ok(rng_out, sb * n_sh)


# --------------------------------------------------------------------------- reduce
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n_slots", [1, 2, 3])
@pytest.mark.parametrize("n_s", [256, 4096 + 256])
def test_reduce(n_s, n_slots, dtype):
    sb = wire.shard_bytes(C4, n_s)
    _, vals = _values(n_slots * n_s, torch.float32, 11 * n_slots + n_s)
    packed = O.pack(vals, n_s, C4)
    slots = torch.from_numpy(packed).to(DEV)
    l_dev, l_np = _values(n_s, dtype, n_slots + n_s + 1)
    slot_list = [packed[r * sb:(r + 1) * sb] for r in range(n_slots)]
    for self_pos, local in ((n_slots - 1, l_dev), (0, l_dev), (-1, None)):
        acc = O.reduce_slots(slot_list, None if local is None else l_np, self_pos, C4, n_s)
        ow = _wire_buf(C4, n_s, 1)
        of = torch.zeros(n_s, device=DEV)
        wire.reduce(slots, n_slots, self_pos, local, ow[:sb], of, n_s, C4)
        torch.cuda.synchronize()
        assert np.array_equal(ow.cpu().numpy()[:sb], O.pack(acc, n_s, C4)), (self_pos, "wire")
        assert _sentinel_ok(ow, sb)
        assert _same(of.cpu().numpy(), acc), (self_pos, "f32 sum")


# --------------------------------------------------------------------------- update kernels
def _update_case(n_s, n_sh, dtype, seed, n_valid):
    n = n_s * n_sh
    _, g = _values(n, dtype, seed)
    buf = O.pack(g, n_s, C4)
    dec = O.unpack(buf, n, n_s, C4)
    rng = np.random.default_rng(seed + 1)
    planes = [rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32),
              (rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)]
    return buf, dec, planes, n_valid


def _run_update(kind, codec, wire_np, n_s, n_sh, planes, n_valid):
    w, m, v = (torch.from_numpy(p.copy()).to(DEV) for p in planes)
    lp = torch.full((w.numel(),), 3.0, dtype=torch.bfloat16, device=DEV)
    wt = torch.from_numpy(wire_np).to(DEV)
    if kind == "sgd":
        wire.sgd(wt, n_s, n_sh, w, codec=codec, lp=lp, mom=m, n_valid=n_valid, **SGD)
    else:
        wire.adamw(wt, n_s, n_sh, w, codec=codec, mom=m, var=v, scalars=O.adamw_scalars(*ADAM), lp=lp,
                   grad_scale=0.5, n_valid=n_valid)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (w, m, v)] + [lp.float().cpu().numpy()]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_update_kernels(n_s, n_sh, dtype, kind):
    """wire.sgd / wire.adamw on the 4-bit wire: the oracle's update of the oracle's decoded values, and the same
    kernel's bits on a raw_f32 wire holding those values. n_valid ends inside a group."""
    n = n_s * n_sh
    buf, dec, planes, nv = _update_case(n_s, n_sh, dtype, n_s + 5, n - 16 - 5)
    got = _run_update(kind, C4, buf, n_s, n_sh, planes, nv)
    raw = _run_update(kind, "raw_f32", dec.view(np.uint8), n_s, n_sh, planes, nv)
    for a, b, name in zip(got, raw, ("master", "mom", "var", "lp")):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: differs from the raw_f32 wire's bits"
    w0, m0, v0 = planes
    if kind == "sgd":
        w, m = O.sgd(w0[:nv], dec[:nv], SGD["lr"], SGD["grad_scale"], SGD["weight_decay"], SGD["momentum"], m0[:nv],
                     SGD["nesterov"])
        v = v0[:nv]
    else:
        w, m, v = O.adamw(w0[:nv], dec[:nv], m0[:nv], v0[:nv], O.adamw_scalars(*ADAM), 0.5)
    for a, ref, old, name in zip(got[:3], (w, m, v), planes, ("master", "mom", "var")):
        assert _same(a[:nv], ref), name
        assert np.array_equal(a[nv:].view(np.uint32), old[nv:].view(np.uint32)), f"{name}: the tail is untouched"
    assert _same(got[3][:nv], O.bf16_bits_to_f32(O.f32_to_bf16_bits(w))) and np.all(got[3][nv:] == 3.0)


@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_sumsq(n_s, n_sh):
    """Every decoded value is q * 2^(E-129) with |q| <= 7, so a square is an integer below 64 times 2^(2E-258); with
    the groups' exponents within 8 of each other (scales 2^[-4, 4)) any sum of up to 2^14 of them has fewer than
    6 + 16 + 14 = 36 significant bits: exact in fp64 in any order, so the device's sum is math.fsum's, bit for bit."""
    n = n_s * n_sh
    rng = np.random.default_rng(n_s)
    x = (rng.uniform(1, 2, n) * rng.choice([-1, 1], n)).astype(np.float32)
    x *= np.repeat(np.exp2(rng.integers(-4, 4, n // 16)), 16).astype(np.float32)
    buf = O.pack(x, n_s, C4)
    dec = O.unpack(buf, n, n_s, C4)
    nv = n - 16 - 5
    wt = torch.from_numpy(buf).to(DEV)
    blocks = wire.sumsq_partials_for(wt, n_s)
    part = torch.full((blocks + 4,), math.nan, dtype=torch.float64, device=DEV)
    assert wire.sumsq(wt, n_s, n_sh, codec=C4, partials=part, partials_base=2, n_valid=nv) == blocks
    p = part.cpu().numpy()
    assert np.isnan(p[:2]).all() and np.isnan(p[2 + blocks:]).all()
    assert math.fsum(p[2:2 + blocks]) == O.clip_sumsq(dec[:nv]) > 0


# --------------------------------------------------------------------------- error feedback
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n_s,n_sh", SHAPES)
def test_pack_ef_and_reduce_ef(n_s, n_sh, dtype):
    n, sb = n_s * n_sh, wire.shard_bytes(C4, n_s)
    g_dev, g = _values(n, dtype, n_s + 9)
    e0 = (np.random.default_rng(n_s).standard_normal(n) * 0.05).astype(np.float32)
    for self_shard in sorted({-1, n_sh - 1}):
        e = torch.from_numpy(e0.copy()).to(DEV)
        out = _wire_buf(C4, n_s, n_sh)
        wire.pack_ef(g_dev, e, out, n_s, C4, self_shard=self_shard)
        torch.cuda.synchronize()
        w_ref, e_ref = O.ef_pack(g, e0, n_s, C4, self_shard)
        assert np.array_equal(out.cpu().numpy()[: sb * n_sh], w_ref) and _sentinel_ok(out, sb * n_sh)
        assert _same(e.cpu().numpy(), e_ref), (self_shard, "residual")
    # zero plane: pack's bytes
    a, b = _wire_buf(C4, n_s, n_sh), _wire_buf(C4, n_s, n_sh)
    wire.pack(g_dev, a, n_s, C4)
    wire.pack_ef(g_dev, torch.zeros(n, device=DEV), b, n_s, C4)
    assert torch.equal(a, b)
    # owner stage
    for n_slots in (1, 2, 3):
        _, vals = _values(n_slots * n_s, torch.float32, n_slots + 40)
        packed = O.pack(vals, n_s, C4)
        slots = torch.from_numpy(packed).to(DEV)
        self_pos = n_slots // 2
        w_ref, e_ref = O.ef_reduce([packed[r * sb:(r + 1) * sb] for r in range(n_slots)], g[:n_s], self_pos,
                                   e0[:n_s], C4, n_s)
        e = torch.from_numpy(e0[:n_s].copy()).to(DEV)
        o1, o2 = _wire_buf(C4, n_s, 1), torch.zeros(sb, dtype=torch.uint8, device=DEV)
        wire.reduce_ef(slots, n_slots, self_pos, g_dev[:n_s], e, [o1[:sb], None, o2], n_s, C4)
        torch.cuda.synchronize()
        assert np.array_equal(o2.cpu().numpy(), w_ref) and torch.equal(o1[:sb], o2) and _sentinel_ok(o1, sb)
        assert _same(e.cpu().numpy(), e_ref), (n_slots, "residual")


# --------------------------------------------------------------------------- the second trip
_BIG = {}


def _big():
    """The big shape's inputs and oracle results, computed once for the two tests below."""
    if not _BIG:
        g_dev, g = _values(BIG, torch.float32, 6, special=False)
        buf = O.pack(g, BIG, C4)
        _BIG.update(g_dev=g_dev, g=g, buf=buf, dec=O.unpack(buf, BIG, BIG, C4))
    return _BIG


def test_second_trip_pack_unpack_reduce_ef():
    b = _big()
    sb = wire.shard_bytes(C4, BIG)
    out = _wire_buf(C4, BIG, 1)
    wire.pack(b["g_dev"], out, BIG, C4)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[:sb], b["buf"]) and _sentinel_ok(out, sb)
    dec = torch.zeros(BIG, device=DEV)
    wire.unpack(out[:sb], dec, BIG, C4)
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), b["dec"].view(np.uint32))
    # reduce of one slot and the local operand, with and without a residual (x + x: exact)
    acc = (b["dec"] + b["g"]).astype(np.float32)
    ow = _wire_buf(C4, BIG, 1)
    wire.reduce(out[:sb], 2, 1, b["g_dev"], ow[:sb], None, BIG, C4)
    torch.cuda.synchronize()
    ref = O.pack(acc, BIG, C4)
    assert np.array_equal(ow.cpu().numpy()[:sb], ref) and _sentinel_ok(ow, sb)
    e = torch.zeros(BIG, device=DEV)
    ow2 = _wire_buf(C4, BIG, 1)
    wire.reduce_ef(out[:sb], 2, 1, b["g_dev"], e, ow2[:sb], BIG, C4)
    torch.cuda.synchronize()
    assert torch.equal(ow2, ow), "zero plane: reduce's bytes"
    e_ref = (acc - O.unpack(ref, BIG, BIG, C4)).astype(np.float32)
    got = e.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), e_ref.view(np.uint32)) and got[-256:].any()
    e2 = torch.from_numpy(e_ref).to(DEV)
    pe = _wire_buf(C4, BIG, 1)
    wire.pack_ef(b["g_dev"], e2, pe, BIG, C4)
    torch.cuda.synchronize()
    w_ref, e2_ref = O.ef_pack(b["g"], e_ref, BIG, C4, -1)
    assert np.array_equal(pe.cpu().numpy()[:sb], w_ref) and _sentinel_ok(pe, sb)
    assert np.array_equal(e2.cpu().numpy().view(np.uint32), e2_ref.view(np.uint32))


def test_second_trip_updates_and_sumsq():
    b = _big()
    nv = BIG - 16 - 5
    rng = np.random.default_rng(8)
    planes = [rng.standard_normal(BIG).astype(np.float32), np.zeros(BIG, np.float32),
              np.zeros(BIG, np.float32)]
    got = _run_update("sgd", C4, b["buf"], BIG, 1, planes, nv)
    w, m = O.sgd(planes[0][:nv], b["dec"][:nv], SGD["lr"], SGD["grad_scale"], SGD["weight_decay"], SGD["momentum"],
                 planes[1][:nv], SGD["nesterov"])
    assert np.array_equal(got[0][:nv].view(np.uint32), w.view(np.uint32))
    assert np.array_equal(got[1][:nv].view(np.uint32), m.view(np.uint32))
    assert np.array_equal(got[0][nv:], planes[0][nv:]) and not got[1][nv:].any()
    got = _run_update("adamw", C4, b["buf"], BIG, 1, planes, nv)
    raw = _run_update("adamw", "raw_f32", b["dec"].view(np.uint8), BIG, 1, planes, nv)
    for x, y in zip(got, raw):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert not np.array_equal(got[0][-256:nv - BIG], planes[0][-256:nv - BIG]), "the second trip's elements moved"
    # the norm pass (fp64 sums in the device's order: within n * 2^-52 of the exact sum, relatively)
    wt = torch.from_numpy(b["buf"]).to(DEV)
    blocks = wire.sumsq_partials_for(wt, BIG)
    part = torch.zeros(blocks, dtype=torch.float64, device=DEV)
    assert wire.sumsq(wt, BIG, 1, codec=C4, partials=part, n_valid=nv) == blocks
    S, ref = math.fsum(part.cpu().numpy()), O.clip_sumsq(b["dec"][:nv])
    print(f"sumsq second trip: gpu {S!r} ref {ref!r}")
    assert abs(S - ref) <= nv * 2.0 ** -52 * ref


# --------------------------------------------------------------------------- the C++ engine over virtual ranks
def _threads(N, fn):
    out, errs = [None] * N, [None] * N

    def run(r):
        try:
            torch.cuda.set_device(0)
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


N_ELEMS = 6000 - 48
PATHS = {
    "mesh": dict(),
    "chunked": dict(chunk_elems=2048),
    "ring1": dict(algo="ring", rings=1, max_slice_elems=512),
    "ring2": dict(algo="ring", rings=2, max_slice_elems=512),
    "sharded": dict(shard_update=True),
}


def _plane(L, x):
    t = torch.zeros(L.n_pad, device=DEV)
    t[:N_ELEMS] = torch.from_numpy(x)
    return t


def _both_updates(eng, r, grads, w0, N):
    """One SGD + momentum request and one AdamW request of rank r's gradient; every plane gathered when sharded."""
    L = eng.layout(N_ELEMS)
    g = _plane(L, grads[r])
    res = {}
    for opt in ("sgd", "adamw"):
        w, m, v = _plane(L, w0), torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
        lp = torch.zeros(L.n_pad, dtype=torch.bfloat16, device=DEV)
        torch.cuda.synchronize()
        if opt == "sgd":
            h = eng.allreduce_sgd(g, w, lp, m, n_valid=N_ELEMS, lr=0.05, momentum=0.9, grad_scale=1.0 / N, defer=True)
        else:
            h = eng.allreduce_sgd(g, w, lp, m, n_valid=N_ELEMS, lr=ADAM[0], weight_decay=ADAM[1], grad_scale=1.0 / N,
                                  opt="adamw", var=v, betas=ADAM[2:4], eps=ADAM[4], step=ADAM[5], defer=True)
        h.commit_after_current()
        h.synchronize(60)
        torch.cuda.synchronize()
        for p in (w, m, v):
            eng.gather_owned(p, N_ELEMS)
        torch.cuda.synchronize()
        res[opt] = [t.float().cpu().numpy() for t in (w, m, v, lp)]
    out = torch.zeros(L.n_pad, device=DEV)
    if not eng.shard_update:
        eng.allreduce(g, out, n_valid=N_ELEMS).synchronize(60)
        torch.cuda.synchronize()
    res["sum"] = out.cpu().numpy()
    return res


def _check_updates(engs, res, grads, w0, N, codec):
    L = engs[0].layout(N_ELEMS)
    for r in range(N):
        red = gate.reference_sum(engs[r], grads, N_ELEMS, r)
        if not engs[r].shard_update:
            assert np.array_equal(res[r]["sum"].view(np.uint32), red.view(np.uint32)), (r, "decoded sum")
        z = np.zeros(N_ELEMS, np.float32)
        w, m = O.sgd(w0, red[:N_ELEMS], 0.05, 1.0 / N, 0.0, 0.9, z)
        for got, ref, name in zip(res[r]["sgd"], (w, m), ("master", "mom")):
            assert np.array_equal(got[:N_ELEMS].view(np.uint32), ref.view(np.uint32)), (r, "sgd", name)
            assert not got[N_ELEMS:].any(), "padding untouched"
        assert np.array_equal(res[r]["sgd"][3][:N_ELEMS], O.bf16_bits_to_f32(O.f32_to_bf16_bits(w))), (r, "sgd lp")
        aw = O.adamw(w0, red[:N_ELEMS], z, z, O.adamw_scalars(*ADAM), 1.0 / N)
        for got, ref, name in zip(res[r]["adamw"], aw, ("master", "mom", "var")):
            assert np.array_equal(got[:N_ELEMS].view(np.uint32), ref.view(np.uint32)), (r, "adamw", name)
        assert np.array_equal(res[r]["adamw"][3][:N_ELEMS], O.bf16_bits_to_f32(O.f32_to_bf16_bits(aw[0])))
        if engs[r].algo == "mesh":  # (a ring's ranks agree by the simulator: each decodes what the others do)
            for opt in ("sgd", "adamw"):
                for a, b in zip(res[r][opt], res[0][opt]):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "replicas must be bit-identical"
    return L


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("N", [2, 3, 4])
def test_native_engine_loopback(C, N, path):
    grads = gate.seeded_gradients(N_ELEMS, N, 300 + N)
    w0 = np.random.default_rng(9).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engs = [NativeAllReduce(None, codec=C4, comm=fabric.comm(r), **PATHS[path]) for r in range(N)]
    assert all(e.codec_id == 4 and e.prepack is False for e in engs)
    L = engs[0].layout(N_ELEMS)
    assert {"chunked": L.chunks > 1, "ring1": L.blocks > 1 and L.rings == 1, "ring2": L.rings == min(2, N - 1),
            "sharded": engs[0].shard_update}.get(path, True)
    res = _threads(N, lambda r: _both_updates(engs[r], r, grads, w0, N))
    _check_updates(engs, res, grads, w0, N, C4)
    if path == "sharded":
        assert all(e.counters()["sharded_updates"] == 2 for e in engs)


def test_bfp_rne_engine_in_the_same_process(C):
    """The 8-bit codec beside the new instantiations: one mesh check of a bfp_rne engine (and of a bfp4 one after it)."""
    N = 2
    grads = gate.seeded_gradients(N_ELEMS, N, 77)
    for codec in ("bfp_rne", C4):
        fabric = C.LoopbackFabric(N, 60.0)
        engs = [NativeAllReduce(None, codec=codec, comm=fabric.comm(r)) for r in range(N)]
        assert engs[0].prepack == (codec == "bfp_rne")

        def fn(r):
            L = engs[r].layout(N_ELEMS)
            out = torch.zeros(L.n_pad, device=DEV)
            engs[r].allreduce(_plane(L, grads[r]), out, n_valid=N_ELEMS).synchronize(60)
            torch.cuda.synchronize()
            return out.cpu().numpy()

        res = _threads(N, fn)
        for r in range(N):
            ref = gate.reference_sum(engs[r], grads, N_ELEMS, r)
            assert np.array_equal(res[r].view(np.uint32), ref.view(np.uint32)), (codec, r)


def _clip_group(eng, r, grads, w0, N):
    L = eng.layout(N_ELEMS)
    words = torch.full((4,), math.nan, device=DEV)
    planes = [(_plane(L, w0), torch.zeros(L.n_pad, device=DEV)) for _ in range(2)]
    gs = [_plane(L, grads[b][r]) for b in range(2)]
    torch.cuda.synchronize()
    hs = [eng.allreduce_sgd(gs[b], w, None, m, n_valid=N_ELEMS, lr=0.05, momentum=0.9, grad_scale=1.0 / N,
                            defer=True, clip=words, name=f"b{b}") for b, (w, m) in enumerate(planes)]
    eng.commit_group(hs, max_norm=1.0, grad_scale=1.0 / N)
    for h in hs:
        h.synchronize(60)
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in p] for p in planes], words.cpu().numpy()


def test_native_engine_loopback_clip_group(C):
    """One clip group of two SGD requests on the mesh: the device's words against the oracle's (one f32 ulp: the fp64
    sum's order), the updates bit for bit with the device's coefficient, and the Python engine's bits."""
    N = 2
    grads = [gate.seeded_gradients(N_ELEMS, N, 900 + b) for b in range(2)]
    grads = [[g * np.float32(64) for g in gb] for gb in grads]  # (a norm well above max_norm)
    w0 = np.random.default_rng(10).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engs = [NativeAllReduce(None, codec=C4, comm=fabric.comm(r)) for r in range(N)]
    res = _threads(N, lambda r: _clip_group(engs[r], r, grads, w0, N))
    pys = [None] * N

    def py_rank(t):
        torch.cuda.set_device(0)
        pys[t.rank] = _clip_group(CompressedAllReduce(t, codec=C4, device=DEV), t.rank, grads, w0, N)

    ThreadFabric(N, timeout_s=60).run(py_rank)
    red = [gate.reference_sum(engs[0], grads[b], N_ELEMS, 0) for b in range(2)]
    ref_words = O.clip_words(O.clip_sumsq(np.concatenate([x[:N_ELEMS] for x in red])), 1.0 / N, 1.0)
    for r in range(N):
        planes, words = res[r]
        ulp = np.abs(words[:3].view(np.int32).astype(np.int64) - ref_words[:3].view(np.int32).astype(np.int64))
        print(f"rank {r}: words gpu {words.tolist()} oracle {ref_words.tolist()}")
        assert ulp.max() <= 1 and 0 < words[0] < 1 and words[3] == 0, "the group was clipped"
        assert np.array_equal(words, res[0][1]) and np.array_equal(words, pys[r][1])
        for b in range(2):
            w, m = O.sgd(w0, red[b][:N_ELEMS], 0.05, O.clip_scale(1.0 / N, words), 0.0, 0.9,
                         np.zeros(N_ELEMS, np.float32))
            assert np.array_equal(planes[b][0][:N_ELEMS].view(np.uint32), w.view(np.uint32))
            assert np.array_equal(planes[b][1][:N_ELEMS].view(np.uint32), m.view(np.uint32))
            for x, y in zip(planes[b], pys[r][0][b]):
                assert np.array_equal(x, y), "native engine differs from the Python engine"


EF_STEPS = 3


def _ef_steps(eng, r, grads, w0):
    L = eng.layout(N_ELEMS)
    ea, eb = torch.zeros(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)
    w = _plane(L, w0)
    res = []
    for t in range(EF_STEPS):
        g, out = _plane(L, grads[t][r]), torch.zeros(L.n_pad, device=DEV)
        torch.cuda.synchronize()
        eng.allreduce(g, out, n_valid=N_ELEMS, residual=ea).synchronize(60)
        h = eng.allreduce_sgd(g, w, n_valid=N_ELEMS, lr=0.5, defer=True, residual=eb)
        h.commit_after_current()
        h.synchronize(60)
        torch.cuda.synchronize()
        res.append(tuple(x.cpu().numpy().copy() for x in (out, w, ea, eb)))
    return res


@pytest.mark.parametrize("N", [2, 3, 4])
def test_native_engine_loopback_error_feedback(C, N):
    grads = [gate.seeded_gradients(N_ELEMS, N, 700 + 10 * t + N) for t in range(EF_STEPS)]
    w0 = np.random.default_rng(12).standard_normal(N_ELEMS).astype(np.float32)
    fabric = C.LoopbackFabric(N, 60.0)
    engs = [NativeAllReduce(None, codec=C4, comm=fabric.comm(r)) for r in range(N)]
    res = _threads(N, lambda r: _ef_steps(engs[r], r, grads, w0))
    L = engs[0].layout(N_ELEMS)
    planes = [np.zeros(L.n_pad, np.float32) for _ in range(N)]
    w = w0
    for t in range(EF_STEPS):
        gin = [np.pad(g, (0, L.n_pad - N_ELEMS)) for g in grads[t]]
        ref, planes = sim.mesh_allreduce_ef(gin, planes, L.shard, C4)
        w, _ = O.sgd(w, ref[:N_ELEMS], 0.5)
        for r in range(N):
            out, wg, ea, eb = res[r][t]
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (r, t, "decoded result")
            assert np.array_equal(ea, planes[r]) and np.array_equal(eb, planes[r]), (r, t, "plane")
            assert np.array_equal(wg[:N_ELEMS].view(np.uint32), w.view(np.uint32)), (r, t, "weights")
    assert all(p.any() for p in planes)
    plain = sim.mesh_allreduce([np.pad(g, (0, L.n_pad - N_ELEMS)) for g in grads[1]], L.shard, C4)
    assert not np.array_equal(res[0][1][0], plain), "the second step already differs from the engine without feedback"


# --------------------------------------------------------------------------- direct P2P, two processes on one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _p2p_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from fpga_ai_nic_amd.parallel.transport import make_p2p_comm

        torch.cuda.set_device(0)
        comm = make_p2p_comm(rank, world, 0, slot_bytes=4 << 20)
        m = 30000
        grads = gate.seeded_gradients(m, world, 11)
        ok = {}
        for algo in ("mesh", "ring"):
            eng = NativeAllReduce(None, codec=C4, algo=algo, max_slice_elems=2048, comm=comm)
            L = eng.layout(m)
            g = torch.zeros(L.n_pad, device="cuda")
            g[:m] = torch.from_numpy(grads[rank]).cuda()
            out = torch.zeros(L.n_pad, device="cuda")
            eng.allreduce(g, out, n_valid=m).synchronize(30)
            torch.cuda.synchronize()
            ref = gate.reference_sum(eng, grads, m, rank)
            ok[f"{algo}_sum"] = bool(np.array_equal(out.cpu().numpy()[:m].view(np.uint32), ref[:m].view(np.uint32)))
            ok[f"{algo}_direct_rounds"] = eng.counters()["direct_rounds"] >= 2
            ok[f"{algo}_no_prepack"] = eng.prepack is False
        q.put((rank, ok, comm.sequence))
    except Exception as ex:  # noqa: BLE001
        q.put((rank, {"error": repr(ex)}, -1))
    finally:
        dist.destroy_process_group()


def test_p2p_two_processes_one_gpu():
    import torch.multiprocessing as mp

    world = 2
    q = mp.get_context("spawn").Queue()
    pc = mp.start_processes(_p2p_worker, args=(world, _free_port(), q), nprocs=world, join=False, start_method="spawn")
    res = {}
    try:
        for _ in range(world):
            rank, ok, seq = q.get(timeout=180)
            res[rank] = (ok, seq)
    except _queue.Empty:
        for p in pc.processes:
            p.kill()
        pytest.fail("p2p workers did not report within 180 s")
    while not pc.join(60):
        pass
    for rank, (ok, _) in res.items():
        assert "error" not in ok, ok
        assert all(ok.values()), f"rank {rank}: {ok}"
    assert res[0][1] == res[1][1], "ranks issued different numbers of rounds"


# --------------------------------------------------------------------------- refusals
def test_refusals(C):
    n = 50000 - 48
    eng = NativeAllReduce(None, codec=C4)
    assert eng.prepack is False and tuple(eng.C.prepack_shape(n)) == (0, 0, -1)
    L = eng.layout(n)
    g, w, e = (torch.zeros(L.n_pad, device=DEV) for _ in range(3))
    assert eng.prepack_target(g, n) is None
    pre = torch.zeros(wire.shard_bytes(C4, L.n_pad), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="cannot take prepacked input"):  # (the binding: before a slot is taken)
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, prepacked=(pre, 0))
    with pytest.raises(RuntimeError, match="cannot take prepacked input"):
        eng.allreduce(g, w, n_valid=n, prepacked=(pre, 0))
    with pytest.raises(ValueError, match="prepacked"):
        eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, prepacked=(pre, 0), residual=e)
    # the residual's existing refusals
    for kw, match in ((dict(algo="ring"), "ring schedule"), (dict(chunk_elems=8192), "chunked"),
                      (dict(shard_update=True), "sharded")):
        x = NativeAllReduce(None, codec=C4, comm=C.LoopbackFabric(2, 60.0).comm(0), **kw)
        Lx = x.layout(n)
        gx, wx, ex = (torch.zeros(Lx.n_pad, device=DEV) for _ in range(3))
        with pytest.raises(ValueError, match=match):
            x.allreduce_sgd(gx, wx, wx.to(torch.bfloat16), n_valid=n, lr=1.0, residual=ex)
        with pytest.raises(RuntimeError, match=match):
            x.C.submit(gx, wx, wx.to(torch.bfloat16), None, n, 1.0, residual=ex)
    # the GEMM wire epilogue stays 8-bit, and truncation has no 4-bit form
    from fpga_ai_nic_amd.parallel.dp import make_engine

    with pytest.raises(ValueError, match="bfp4"):
        make_engine(ThreadFabric(1).transport(0), "bfp4", rounding="trunc", impl="native")
    assert make_engine(ThreadFabric(1).transport(0), "bfp4", impl="native").codec == C4
    # an ordinary request with a plane still completes
    g.fill_(1.0)
    eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, residual=e).synchronize(30)
    torch.cuda.synchronize()
    assert torch.all(w[:n] == -1.0) and not e.any(), "1.0 is exactly representable: nothing dropped"
