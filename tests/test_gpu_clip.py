"""Global-norm gradient clipping on the GPU: the norm kernel and the coefficient kernel against the oracle, the update
kernels' device-side scale, clip groups on the native engine over virtual ranks (LoopbackFabric) against the Python
engine and the spec simulators, the inline engine and the trainer at world 1 and through the forced multi-rank path,
and the refusals.

Bounds:
  * wire_sumsq: every square is exact in fp64 and every term non-negative, so a sum of n of them in any order is within
    n * 2^-53 of the exact sum, relatively; doubled for the block tree: |S_gpu - S_ref| <= n * 2^-52 * S_ref, S_ref the
    math.fsum of the exact squares of the oracle-decoded values.
  * clip_coef: the fp64 error of the sum, sqrt, product and division is far below half an f32 ulp, so the words are
    within 1 f32 ulp of bfp_oracle.clip_words fed the exact fp64 sum (a rounding-boundary flip), words[2] exactly.
  * the updates with clip= are bit-identical to the same update with grad_scale = f32(grad_scale) * f32(words[0]).
"""
import math
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
from fpga_ai_nic_amd.parallel.transport import NativeTransport, ThreadFabric

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, WD, MOM, B1, B2, EPS = 0.05, 1e-2, 0.9, 0.9, 0.999, 1e-8
CODECS = ["bfp_trunc", "bfp_rne", "raw_f32", "raw_bf16"]
LIMIT = "a clip group holds at most 8 deferred requests"
N_S, N_SH = 1024, 4
N_VALID = N_S * N_SH - 77


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _wire(codec, n_s, n_sh, seed=2, stride_pad=0):
    """A packed wire of n_sh shards on the GPU (optionally its shards `stride_pad` bytes further apart, the gaps
    filled with 0xFF) and the oracle's decoding of the packed bytes."""
    n = n_s * n_sh
    g = (np.random.default_rng(seed).standard_normal(n) * 3).astype(np.float32)
    sb = O.shard_bytes(codec, n_s)
    buf = torch.zeros(sb * n_sh, dtype=torch.uint8, device=DEV)
    wire.pack(torch.from_numpy(g).to(DEV), buf, n_s, codec)
    dec = O.unpack(buf.cpu().numpy(), n, n_s, codec)
    if stride_pad:
        wide = torch.full(((sb + stride_pad) * n_sh,), 255, dtype=torch.uint8, device=DEV)
        wide.view(n_sh, sb + stride_pad)[:, :sb] = buf.view(n_sh, sb)
        buf = wide
    return buf, dec, sb + stride_pad if stride_pad else 0


def _check_sumsq(codec, n_s, n_sh, n_valid, stride_pad=0, skip=(-1, 0)):
    buf, dec, stride = _wire(codec, n_s, n_sh, stride_pad=stride_pad)
    blocks = wire.sumsq_partials_for(buf, n_s)
    part = torch.full((blocks + 5,), math.nan, dtype=torch.float64, device=DEV)
    kw = dict(codec=codec, partials=part, partials_base=2, n_valid=n_valid, skip_shard=skip[0], skip_period=skip[1],
              shard_stride=stride)
    assert wire.sumsq(buf, n_s, n_sh, **kw) == blocks
    first = part.cpu().numpy().copy()
    assert np.isfinite(first[2:2 + blocks]).all() and np.all(first[2:2 + blocks] >= 0), "every block wrote its partial"
    assert np.isnan(first[:2]).all() and np.isnan(first[2 + blocks:]).all(), "nothing outside [base, base + blocks)"
    keep = np.arange(n_s * n_sh) < n_valid
    if skip[0] >= 0:
        keep &= (np.arange(n_s * n_sh) // n_s) % skip[1] != skip[0]
    ref = O.clip_sumsq(dec[keep])
    got = math.fsum(first[2:2 + blocks])
    n = int(keep.sum())
    print(f"{codec} n_s {n_s} blocks {blocks} n {n}: S gpu {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e} "
          f"bound {n * 2.0 ** -52:.3e}")
    assert abs(got - ref) <= n * 2.0 ** -52 * ref
    part.fill_(math.nan)
    wire.sumsq(buf, n_s, n_sh, **kw)
    assert np.array_equal(part.cpu().numpy()[2:2 + blocks], first[2:2 + blocks]), "two runs, the same bits"
    return blocks


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("stride_pad", [0, 160])
@pytest.mark.parametrize("skip", [(-1, 0), (1, 4)], ids=["all", "skip1of4"])
def test_wire_sumsq(codec, stride_pad, skip):
    _check_sumsq(codec, N_S, N_SH, N_VALID, stride_pad, skip)


@pytest.mark.parametrize("codec", CODECS)
def test_wire_sumsq_several_blocks(codec):
    n_s = 256
    while wire.sumsq_partials_for(torch.zeros(1, device=DEV), n_s) < 3:
        n_s += 256
    n_s += 256  # (the last block is not full)
    assert _check_sumsq(codec, n_s, 2, 2 * n_s - 77) >= 3


def test_wire_sumsq_refuses_an_empty_region():
    C = _ext.require()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    part = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError):
        C.wire_sumsq(buf, 256, 0, -1, 0, 0, part, 0, 1)
    with pytest.raises(RuntimeError, match="partials"):
        C.wire_sumsq(buf, 256, 1, -1, 0, 256, part, 4, 1)
    with pytest.raises(RuntimeError, match="too small"):
        C.wire_sumsq(buf, 256, 100, -1, 0, 256, part, 0, 1)


def _coef_case(segs, max_norm, grad_scale=1.0):
    """segs: lists of float64 partials, one per segment; returns (device words, oracle words)."""
    part = torch.tensor([x for s in segs for x in s] + [math.nan], dtype=torch.float64, device=DEV)
    triples, base = [], 0
    for s in segs:
        triples.append((part, base, len(s)))
        base += len(s)
    words = torch.full((6,), math.nan, device=DEV)
    wire.clip_coef(triples, max_norm, grad_scale, words)
    got = words.cpu().numpy()
    assert np.isnan(got[4:]).all(), "four words"
    flat = [x for s in segs for x in s]
    S = math.fsum(flat) if all(math.isfinite(x) for x in flat) else float(np.sum(flat))
    return got[:4], O.clip_words(S, grad_scale, max_norm)


@pytest.mark.parametrize("n_seg", [1, 3, 8])
def test_clip_coef_segments(n_seg):
    rng = np.random.default_rng(n_seg)
    segs = [list(rng.random(1 + 300 * k) * 10) for k in range(n_seg)]
    if n_seg == 3:
        segs[1] = []  # a segment of count 0 contributes nothing
    got, ref = _coef_case(segs, 0.3, -0.5)  # (below every case's total: a clipped case)
    print(f"{n_seg} segments: gpu {got.tolist()} oracle {ref.tolist()}")
    assert np.all(_ulps(got, ref) <= 1) and 0 < got[0] < 1 and got[3] == 0
    assert got[2] == np.float32(0.3)


def test_clip_coef_edges():
    got, ref = _coef_case([[0.0, 0.0], [0.0]], 1.0)
    assert np.array_equal(got, ref) and got[0] == 1.0 and got[1] == 0.0, "S = 0"
    # coef is exactly 1 up to total + 1e-6 <= max_norm, and below 1 right past it
    got, _ = _coef_case([[4.0, 5.0]], 3.0 + 1e-6)
    assert got[0] == 1.0 and got[1] == 3.0 and got[2] == np.float32(3.0 + 1e-6)
    got, ref = _coef_case([[4.0, 5.0]], 3.0 - 1e-3)
    assert got[0] < 1.0 and np.all(_ulps(got, ref) <= 1)
    got, ref = _coef_case([[1e-300] * 3], 0.1)
    assert got[0] == 1.0 and np.all(_ulps(got, ref) <= 1)
    # a non-finite partial: NaN coefficient, the flag, max_norm still there
    for bad in (math.inf, math.nan):
        got, _ = _coef_case([[1.0], [bad, 2.0]], 0.7)
        assert math.isnan(got[0]) and got[3] == 1.0 and got[2] == np.float32(0.7)
    with pytest.raises(ValueError, match="max_norm"):
        _coef_case([[1.0]], 0.0)
    with pytest.raises(ValueError, match="at most 8"):
        _coef_case([[1.0]] * 9, 1.0)
    C = _ext.require()
    p, w = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match="max_norm"):
        C.clip_coef([p], [0], [4], math.nan, 1.0, w)
    with pytest.raises(RuntimeError, match="segment"):
        C.clip_coef([p], [2], [3], 1.0, 1.0, w)


def _planes(n, seed=4):
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
    m = torch.from_numpy((rng.standard_normal(n) * 0.1).astype(np.float32)).to(DEV)
    v = torch.from_numpy((rng.standard_normal(n) ** 2 * 0.01).astype(np.float32)).to(DEV)
    return w, m, v, torch.zeros(n, dtype=torch.bfloat16, device=DEV)


def _upd_sgd(buf, codec, clip, scale, mom, lp):
    w, m, _, l = _planes(N_S * N_SH)
    wire.sgd(buf, N_S, N_SH, w, codec=codec, lp=l if lp else None, mom=m if mom else None, lr=LR, grad_scale=scale,
             weight_decay=WD, momentum=MOM if mom else 0.0, nesterov=mom, n_valid=N_VALID, skip_shard=1,
             skip_period=4, clip=clip)
    return w, m, l


def _upd_adamw(buf, codec, clip, scale, mom, lp):
    w, m, v, l = _planes(N_S * N_SH)
    wire.adamw(buf, N_S, N_SH, w, codec=codec, mom=m, var=v, lp=l if lp else None, grad_scale=scale, n_valid=N_VALID,
               scalars=O.adamw_scalars(LR, WD, B1, B2, EPS, 3), skip_shard=1, skip_period=4, clip=clip)
    return w, m, v, l


def _upd_lamb(buf, codec, clip, scale, mom, lp):
    w, m, v, l = _planes(N_S * N_SH)
    s = O.lamb_scalars(LR, WD, B1, B2, EPS, 3)
    part = torch.zeros(2 * wire.lamb_partials_for(w, N_S), dtype=torch.float64, device=DEV)
    tw = torch.zeros(3, device=DEV)
    kw = dict(n_valid=N_VALID, n_adapt=3001, skip_shard=1, skip_period=4)
    k = wire.lamb_moments(buf, N_S, N_SH, w, codec=codec, mom=m, var=v, scalars=s, partials=part, grad_scale=scale,
                          clip=clip, **kw)
    wire.lamb_ratio(part, k, LR, tw)
    wire.lamb_apply(w, N_S, mom=m, var=v, scalars=s, words=tw, lp=l if lp else None, **kw)
    return w, m, v, l, tw


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("upd,mom,lp", [(_upd_sgd, False, False), (_upd_sgd, True, False), (_upd_sgd, False, True),
                                        (_upd_sgd, True, True), (_upd_adamw, True, True), (_upd_adamw, True, False),
                                        (_upd_lamb, True, True)],
                         ids=["sgd", "sgd-mom", "sgd-lp", "sgd-mom-lp", "adamw-lp", "adamw", "lamb"])
def test_update_kernels_device_scale(codec, upd, mom, lp):
    buf, _, _ = _wire(codec, N_S, N_SH, seed=6)
    words = torch.tensor([0.37, 11.0, 4.0, 0.0], device=DEV)
    scale = 1.0 / 3
    premul = float(np.float32(scale) * np.float32(0.37))
    assert premul == O.clip_scale(scale, words.cpu().numpy())
    clipped, ref, plain = upd(buf, codec, words, scale, mom, lp), upd(buf, codec, None, premul, mom, lp), \
        upd(buf, codec, None, scale, mom, lp)
    for a, b in zip(clipped, ref):
        assert torch.equal(a, b), "clip= differs from the premultiplied grad_scale"
    assert not torch.equal(clipped[0], plain[0])
    one = torch.tensor([1.0, 0.0, 4.0, 0.0], device=DEV)
    for a, b in zip(upd(buf, codec, one, scale, mom, lp), plain):
        assert torch.equal(a, b), "a coefficient of 1 changes the update's bits"
    assert torch.equal(words.cpu(), torch.tensor([0.37, 11.0, 4.0, 0.0])), "the words are read only"


# ------------------------------------------------------------------------------------------ engines
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


SIZES = (50000 - 48, 12000, 333)  # the smallest: n_valid no multiple of 16
MAX_NORM = 2.0
_OPT = {"sgd": dict(momentum=MOM), "adamw": dict(opt="adamw", betas=(B1, B2), eps=EPS, step=2),
        "lamb": dict(opt="adamw", betas=(B1, B2), eps=EPS, step=2, trust_ratio=True)}


def _group(eng, nranks, r, opt, inputs, clip, grad_scale):
    """One step over the three buckets on rank r's engine: a clip group (clip=True) or plain deferred requests with
    the given grad_scale. Returns the planes, the bf16 copies and the clip words."""
    grads, w0, m0 = inputs
    words = torch.full((4,), math.nan, device=DEV) if clip else None
    hs, planes = [], []
    for b, n in enumerate(SIZES):
        L = eng.layout(n)
        g, w, m, v = (torch.zeros(L.n_pad, device=DEV) for _ in range(4))
        lp = torch.zeros(L.n_pad, device=DEV, dtype=torch.bfloat16)
        g[:n] = torch.from_numpy(grads[b][r])
        w[:n] = torch.from_numpy(w0[b])
        m[:n] = torch.from_numpy(m0[b])
        kw = dict(_OPT[opt], **({"var": v} if opt != "sgd" else {}), **({"clip": words} if clip else {}))
        torch.cuda.synchronize()
        hs.append(eng.allreduce_sgd(g, w, lp, m, n_valid=n, lr=LR, weight_decay=WD, grad_scale=grad_scale, defer=True,
                                    name=f"b{b}", **kw))
        planes.append((w, m, v, lp))
    if clip:
        eng.commit_group(hs, max_norm=MAX_NORM, grad_scale=grad_scale)
    else:
        for h in hs:
            h.commit_after_current()
    for h in hs:
        h.synchronize(60)
    torch.cuda.synchronize()
    return [tuple(x.cpu() for x in p) for p in planes], None if words is None else words.cpu().numpy()


def _same_planes(a, b):
    return all(torch.equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))


def _inputs(nranks, seed):
    rng = np.random.default_rng(seed)
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + r) for r in range(nranks)] for n in SIZES]
    w0 = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    m0 = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in SIZES]
    return grads, w0, m0


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("algo", ["mesh", "ring"])
@pytest.mark.parametrize("opt", ["sgd", "adamw", "lamb"])
def test_native_engine_loopback_clip_group(nranks, algo, opt):
    C = _ext.require()
    inputs = _inputs(nranks, nranks * 100 + len(algo))
    gs = 1.0 / nranks
    ekw = dict(codec="bfp_rne", algo=algo, rings=2, max_slice_elems=8192)

    def engines():
        fabric = C.LoopbackFabric(nranks, 60.0)
        return [NativeAllReduce(None, comm=fabric.comm(r), **ekw) for r in range(nranks)]

    engs = engines()
    res = _threads(nranks, lambda r: _group(engs[r], nranks, r, opt, inputs, True, gs))
    words = res[0][1]
    for r in range(1, nranks):
        assert np.array_equal(res[r][1], words), "the words are identical on every rank"
        assert _same_planes(res[r][0], res[0][0]), "replicas must be bit-identical"
    # the oracle's words over the simulator's reduced wire
    red = []
    for b, n in enumerate(SIZES):
        L = engs[0].layout(n)
        gin = [np.pad(g, (0, L.n_pad - n)) for g in inputs[0][b]]
        red.append((sim.mesh_allreduce(gin, L.shard, "bfp_rne") if algo == "mesh" else
                    sim.ring_allreduce(gin, engs[0].orders, L.slice_elems, L.blocks, "bfp_rne")[0])[:n])
    ref = O.clip_words(O.clip_sumsq(np.concatenate(red)), gs, MAX_NORM)
    print(f"N={nranks} {algo} {opt}: words gpu {words.tolist()} oracle {ref.tolist()} ulp {_ulps(words, ref).tolist()}")
    assert np.all(_ulps(words, ref) <= 1) and 0 < words[0] < 1 and words[3] == 0 and words[2] == np.float32(MAX_NORM)
    # SGD against the oracle update with the device's coefficient (the other optimizers: through the two runs below)
    if opt == "sgd":
        for b, n in enumerate(SIZES):
            rw, rm = O.sgd(inputs[1][b], red[b], LR, O.clip_scale(gs, words), WD, MOM, inputs[2][b])
            assert np.all(_ulps(res[0][0][b][0].numpy()[:n], rw) <= 1)
            assert np.all(res[0][0][b][0].numpy()[n:] == 0), "padding untouched"
    # a native run without clipping whose grad_scale is premultiplied by the device's own coefficient
    engs = engines()
    pre = _threads(nranks, lambda r: _group(engs[r], nranks, r, opt, inputs, False, O.clip_scale(gs, words)))
    assert _same_planes(pre[0][0], res[0][0]), "clipped run differs from the premultiplied unclipped run"
    # the Python engine issues the same launches on the same GPU tensors: the same bits
    pys = [None] * nranks

    def py_rank(t):
        torch.cuda.set_device(0)
        eng = CompressedAllReduce(t, device=DEV, **ekw)
        for n in SIZES:
            Lp, Ln = eng.layout(n), engs[0].layout(n)
            assert (Lp.n_pad, Lp.shard, Lp.slice_elems, Lp.blocks, Lp.rings) == \
                (Ln.n_pad, Ln.shard, Ln.slice_elems, Ln.blocks, Ln.rings)
        pys[t.rank] = _group(eng, nranks, t.rank, opt, inputs, True, gs)

    ThreadFabric(nranks, timeout_s=60).run(py_rank)
    assert np.array_equal(pys[0][1], words) and _same_planes(pys[0][0], res[0][0]), \
        "native engine differs from the Python engine"


def _train(engine, max_grad_norm, steps=3, **kw):
    sizes, mb = [64, 128, 64], 256
    eng = {"native": lambda: NativeAllReduce(None, codec="bfp_rne"),
           "python": lambda: CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", device=DEV),
           "forced": lambda: NativeAllReduce(_native_transport(), codec="bfp_rne", force_comm=True)}[engine]()
    model = MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3, momentum=True,
                pad_fn=lambda n, e=eng: e.layout(n).n_pad)
    tr = DataParallelTrainer(model, eng, lr=LR, momentum=MOM, weight_decay=WD, max_grad_norm=max_grad_norm, **kw)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=g) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=g, dtype=torch.int32).to(DEV)
    norms = []
    for _ in range(steps):
        tr.step(x, y)
        if tr.grad_norm is not None:
            tr.finish()
            norms.append(tr.grad_norm.cpu().numpy().copy())
    tr.finish()
    return [(l.master.cpu(), l.mom.cpu(), l.lp.cpu()) for l in model.layers], norms, tr


def test_trainer_world1_inline():
    plain, _, tp = _train("native", None, fused_update=False)
    big, norms, tb = _train("native", 1e30)
    assert tp.grad_norm is None and tb.grad_norm.is_cuda and tb.grad_norm.shape == (4,)
    assert tb.fused_update is False and tb.fused_updates == 0
    assert _same_planes(plain, big), "an unclipped step of a clipped trainer must keep the unclipped step's bits"
    assert all(w[0] == 1.0 and w[1] > 0 and w[3] == 0 for w in norms)
    total = float(norms[0][1])
    half, hn, th = _train("native", total / 2)
    ref = np.float32(0.5 * total / (total + 1e-6))
    print(f"first step: total {total!r} coef {hn[0][0]!r} ref {ref!r} ulp {_ulps(hn[0][:1], [ref]).tolist()}")
    assert _ulps(hn[0][:1], [ref])[0] <= 1 and hn[0][0] < 0.5
    assert not any(torch.equal(a[0], b[0]) for a, b in zip(plain, half)), "clipping changes the weights"
    assert th.fused_updates == 0
    # the Python engine: bit for bit, the words too
    py, pn, _ = _train("python", total / 2)
    assert _same_planes(py, half) and all(np.array_equal(a, b) for a, b in zip(pn, hn))


_NT = {}


class _Store(dict):
    def set(self, k, v):
        self[k] = v

    def get(self, k):
        return self[k]


def _native_transport():
    if "t" not in _NT:  # one 1-rank communicator for the whole module
        _NT["t"] = NativeTransport(rank=0, world=1, device=0, store=_Store(), force_collectives=True)
    return _NT["t"]


def test_trainer_forced_multirank_path():
    """World 1 through the multi-rank path (comm stream, epilogues on the compute stream, the last request on the
    producer): the clip group trains like the inline engine's, clipped or not."""
    ref, rn, _ = _train("native", 1e30)
    got, gn, tr = _train("forced", 1e30)
    assert tr.last_on_producer and tr.engine.epilogue_on_producer
    assert _same_planes(ref, got) and all(np.array_equal(a, b) for a, b in zip(rn, gn))
    total = float(rn[0][1])
    ref, rn, _ = _train("native", total / 2)
    got, gn, _ = _train("forced", total / 2)
    assert _same_planes(ref, got) and all(np.array_equal(a, b) for a, b in zip(rn, gn))
    assert gn[0][0] < 0.5


def _bufs(eng, n, k=1):
    L = eng.layout(n)
    return [(torch.ones(L.n_pad, device=DEV), torch.zeros(L.n_pad, device=DEV)) for _ in range(k)]


def _ordinary(eng, n=1000):
    """An ordinary request still completes on the engine."""
    (g, w), = _bufs(eng, n)
    eng.allreduce_sgd(g, w, n_valid=n, lr=1.0).synchronize(60)
    torch.cuda.synchronize()
    q = O.quantize(np.ones(eng.layout(n).n_pad, np.float32), "bfp_rne")[:n]
    assert np.array_equal(w.cpu().numpy()[:n], -q)


def test_refusals_at_submit():
    C = _ext.require()
    n = 50000 - 48
    words = torch.zeros(4, device=DEV)
    eng = NativeAllReduce(None, codec="bfp_rne")
    (g, w), = _bufs(eng, n)
    ok = dict(n_valid=n, lr=1.0, defer=True, clip=words)
    with pytest.raises(ValueError, match="must be deferred"):
        eng.allreduce_sgd(g, w, **{**ok, "defer": False})
    with pytest.raises(ValueError, match="four f32 words"):
        eng.allreduce_sgd(g, w, **{**ok, "clip": torch.zeros(3, device=DEV)})
    with pytest.raises(ValueError, match="the engine runs on"):
        eng.allreduce_sgd(g, w, **{**ok, "clip": torch.zeros(4)})
    # the engine itself refuses what the wrapper lets through: not deferred, and a sum-only request
    with pytest.raises(RuntimeError, match="must be deferred"):
        eng.C.submit(g, w, None, None, n, 1.0, defer=False, clip=words)
    with pytest.raises(RuntimeError, match="update requests only"):
        eng.C.submit(g, w, None, None, n, 1.0, defer=True, update=False, out_sum=w, clip=words)
    _ordinary(eng)
    # a sharded-update engine (request and trainer)
    eng = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), shard_update=True)
    (g, w), = _bufs(eng, n)
    with pytest.raises(ValueError, match="sharded"):
        eng.allreduce_sgd(g, w, w.to(torch.bfloat16), **ok)
    with pytest.raises(RuntimeError, match="sharded"):
        eng.C.submit(g, w, w.to(torch.bfloat16), None, n, 1.0, defer=True, clip=words)
    model = MLP([256, 256], dtype=torch.bfloat16, device=DEV, pad_fn=lambda k, e=eng: e.layout(k).n_pad)
    with pytest.raises(ValueError, match="sharded"):
        DataParallelTrainer(model, eng, max_grad_norm=1.0)
    # a chunked layout: a bucket above chunk_elems, and an explicit layout=(shard, chunks)
    eng = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0), chunk_elems=8192)
    assert eng.layout(n).chunks > 1
    (g, w), = _bufs(eng, n)
    with pytest.raises(ValueError, match="chunked"):
        eng.allreduce_sgd(g, w, **ok)
    with pytest.raises(RuntimeError, match="chunked"):
        eng.C.submit(g, w, None, None, n, 1.0, defer=True, clip=words)
    eng = NativeAllReduce(None, codec="bfp_rne", comm=C.LoopbackFabric(2, 60.0).comm(0))
    g = torch.ones(eng.layout(n, 8192, 4).n_pad, device=DEV)
    w = torch.zeros_like(g)
    with pytest.raises(ValueError, match="chunked"):
        eng.allreduce_sgd(g, w, layout=(8192, 4), **ok)
    # the ring's compat_owner_fp32
    eng = NativeAllReduce(None, codec="bfp_rne", algo="ring", comm=C.LoopbackFabric(2, 60.0).comm(0),
                          compat_owner_fp32=True)
    (g, w), = _bufs(eng, n)
    with pytest.raises(ValueError, match="compat_owner_fp32"):
        eng.allreduce_sgd(g, w, **ok)
    with pytest.raises(RuntimeError, match="compat_owner_fp32"):
        eng.C.submit(g, w, None, None, n, 1.0, defer=True, clip=words)
    # more than 8 layers
    with pytest.raises(ValueError, match="at most 8"):
        DataParallelTrainer(MLP([256] * 10, dtype=torch.bfloat16, device=DEV), NativeAllReduce(None),
                            max_grad_norm=1.0)


@pytest.mark.parametrize("impl", ["native", "python"])
def test_refusals_of_pending_clipped_requests(impl):
    n = 1000
    eng = NativeAllReduce(None, codec="bfp_rne") if impl == "native" else \
        CompressedAllReduce(ThreadFabric(1).transport(0), codec="bfp_rne", device=DEV)
    words = torch.zeros(4, device=DEV)
    bufs = _bufs(eng, n, 9)
    hs = [eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, defer=True, clip=words) for g, w in bufs[:8]]
    # the 9th deferred request would force-commit the first with a coefficient that does not exist yet
    with pytest.raises(ValueError, match=LIMIT):
        eng.allreduce_sgd(*bufs[8], n_valid=n, lr=1.0, defer=True, clip=words)
    with pytest.raises(ValueError, match=LIMIT):
        eng.allreduce_sgd(*bufs[8], n_valid=n, lr=1.0)
    # a lone commit / wait / synchronize
    for call in (hs[0].commit, hs[0].commit_after_current, hs[0].wait, hs[0].synchronize):
        with pytest.raises(ValueError, match=LIMIT):
            call()
    if impl == "native":
        for call in (lambda: eng.C.commit(hs[0].slot, True, hs[0].seq), lambda: eng.C.wait_stream(hs[0].slot, hs[0].seq),
                     lambda: eng.C.synchronize(hs[0].slot, 1.0, hs[0].seq), lambda: eng.C.commit(hs[0].slot)):
            with pytest.raises(RuntimeError, match=LIMIT):
                call()
        # commit_group's own checks, past the wrapper's
        with pytest.raises(RuntimeError, match="not pending any more, or its slot holds another"):
            eng.C.commit_group([hs[0].slot], [hs[0].seq + 100], 1.0)
        with pytest.raises(RuntimeError, match="named twice"):
            eng.C.commit_group([hs[0].slot] * 2, [hs[0].seq] * 2, 1.0)
        with pytest.raises(RuntimeError, match="max_norm"):
            eng.C.commit_group([hs[0].slot], [hs[0].seq], math.nan)
        with pytest.raises(RuntimeError, match=LIMIT):
            eng.C.commit_group([h.slot for h in hs] + [0], [h.seq for h in hs] + [hs[0].seq], 1.0)
    torch.cuda.synchronize()
    assert all(h.pending for h in hs) and all(torch.all(w == 0) for _, w in bufs), "never a stale coefficient"
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="max_norm"):
            eng.commit_group(hs, max_norm=bad)
    with pytest.raises(ValueError, match=LIMIT):
        eng.commit_group(hs + hs[:1], max_norm=1.0)
    with pytest.raises(ValueError, match="no request"):
        eng.commit_group([], max_norm=1.0)
    eng.commit_group(hs, max_norm=1e30)
    for h in hs:
        h.synchronize(60)
    torch.cuda.synchronize()
    q = O.quantize(np.ones(eng.layout(n).n_pad, np.float32), "bfp_rne")[:n]
    assert all(np.array_equal(w.cpu().numpy()[:n], -q) for _, w in bufs[:8]) and torch.all(bufs[8][1] == 0)
    assert words.cpu()[0] == 1.0
    with pytest.raises(ValueError, match="not pending"):
        eng.commit_group(hs[:1], max_norm=1.0)
    # two groups' words, and a request without clip
    (g, w), (g2, w2), (g3, w3) = _bufs(eng, n, 3)
    a = eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, defer=True, clip=words)
    b = eng.allreduce_sgd(g2, w2, n_valid=n, lr=1.0, defer=True, clip=torch.zeros(4, device=DEV))
    c = eng.allreduce_sgd(g3, w3, n_valid=n, lr=1.0, defer=True)
    with pytest.raises(ValueError, match="same clip words"):
        eng.commit_group([a, b], max_norm=1.0)
    with pytest.raises(ValueError, match="not submitted with clip"):
        eng.commit_group([a, c], max_norm=1.0)
    if impl == "native":
        with pytest.raises(RuntimeError, match="same clip words"):
            eng.C.commit_group([a.slot, b.slot], [a.seq, b.seq], 1.0)
        with pytest.raises(RuntimeError, match="not submitted with clip"):
            eng.C.commit_group([a.slot, c.slot], [a.seq, c.seq], 1.0)
    c.commit_after_current()
    eng.commit_group([a], max_norm=1e30)
    eng.commit_group([b], max_norm=1e30)
    for h in (a, b, c):
        h.synchronize(60)
    _ordinary(eng)


def test_refusal_of_two_epilogue_streams():
    """Epilogues on the comm stream beside an on-producer request's on the compute stream: one coefficient launch
    cannot precede both."""
    eng = NativeAllReduce(_native_transport(), codec="bfp_rne", force_comm=True)
    eng.epilogue_on_producer = False
    n = 1000
    words = torch.zeros(4, device=DEV)
    (g, w), (g2, w2) = _bufs(eng, n, 2)
    a = eng.allreduce_sgd(g, w, n_valid=n, lr=1.0, defer=True, clip=words)
    b = eng.allreduce_sgd(g2, w2, n_valid=n, lr=1.0, defer=True, clip=words, on_producer=True)
    with pytest.raises(ValueError, match="different streams"):
        eng.commit_group([a, b], max_norm=1e30)
    assert a.pending and b.pending
    eng.commit_group([a], max_norm=1e30)
    eng.commit_group([b], max_norm=1e30)
    a.synchronize(60)
    b.synchronize(60)
    _ordinary(eng)
    # the trainer keeps the last request off the producer stream on such an engine
    model = MLP([64, 128, 64], dtype=torch.bfloat16, device=DEV, pad_fn=lambda k, e=eng: e.layout(k).n_pad)
    assert DataParallelTrainer(model, eng, max_grad_norm=1.0).last_on_producer is False
    assert DataParallelTrainer(model, eng).last_on_producer is True
