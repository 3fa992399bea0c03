"""Count-sketch compression on the GPU: the kernels of csrc/sketch/sketch_kernels.hip and the keys-only select of
csrc/topk/topk_kernels.hip against the NumPy oracle, bit for bit; the two-rank reducer and one trainer step."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import sketch as SK
from fpga_ai_nic_amd.ops import sketch_oracle as O
from fpga_ai_nic_amd.parallel.sketch import SketchReducer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED = 0xC0FFEE_0000_0001
# one chunk, a tail inside a vector; four chunks; two column tiles, a wrap inside a tile; 18 chunks: two strips, ragged
SHAPES = [(1024, 1000, 1024, 1), (4096, 4090, 1024, 3), (6144, 6144, 2048, 3), (17920, 17461, 1024, 5)]
CLASSES = ["normal", "planted", "special"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@lru_cache(maxsize=None)
def planes(cls, n_pad, n):
    """(g, e); past n, g is huge and e a sentinel: neither may be read or written."""
    rng = np.random.default_rng(n + len(cls))
    g, e = rng.standard_normal(n_pad).astype(np.float32), (rng.standard_normal(n_pad) / 4).astype(np.float32)
    if cls == "planted":
        g[rng.choice(n, 16, replace=False)] = 64 * rng.choice([-1.0, 1.0], 16)
        e[:] = 0
    elif cls == "special":  # all inside chunk 0, whose elements never share a column: no Inf - Inf, no NaN + NaN,
        g[[3, 5, 990]] = np.nan, np.inf, -np.inf  # whose NaN differs between machines
        g[[7, 9, 11]], e[[7, 9, 11]] = (-0.0, 1e-40, -3e-42), (-0.0, 0.0, 0.0)
    g[n:], e[n:] = 1e30, 7.5
    g.setflags(write=False)
    e.setflags(write=False)
    return g, e


@lru_cache(maxsize=None)
def oracle(cls, n_pad, n, cols, rows):
    """The one-rank step in stages: (S, est, x, idx, est at idx, val, e', g')."""
    g, e = planes(cls, n_pad, n)
    k = SK.count(n, 0.01)
    S = O.sketch(g, e, n, rows, cols, SEED)
    est, x = O.estimate(g, e, S, n, SEED)
    idx, ev = O.select_keys(est, n, k)
    val, left = O.fetch(x, idx, k)
    return S, est, x, idx, ev, val, left, O.step([g], [e], n, k, rows, cols, SEED)[0]


def run_stages(cls, n_pad, n, cols, rows, max_blocks=None):
    g, e = planes(cls, n_pad, n)
    k = SK.count(n, 0.01)
    sk, part, words, nbytes = SK.layout(n_pad, k, rows, cols)
    gd, ed = torch.from_numpy(g.copy()).to(DEV), torch.from_numpy(e.copy()).to(DEV)
    S, P = (torch.full((m,), 3.5, device=DEV) for m in (sk, part))
    wire = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros(words, dtype=torch.int32, device=DEV)
    SK.sketch(gd, ed, S, P, n, rows, cols, SEED, max_blocks=max_blocks)
    assert np.array_equal(bits(gd.cpu().numpy()), bits(g)) and np.array_equal(bits(ed.cpu().numpy()), bits(e))
    SK.estimate_select(gd, ed, S, wire, scratch, n, k, rows, cols, SEED, max_blocks=max_blocks)
    kp = SK.k_pad(k)
    w = wire.cpu().numpy()
    out = [bits(S.cpu().numpy()), bits(gd.cpu().numpy()), bits(ed.cpu().numpy()), w[: 4 * kp].view(np.uint32).copy(),
           w[4 * kp:].view(np.uint32).copy()]
    val = SK.fetch(ed, wire, n, k, max_blocks=max_blocks)
    return out + [bits(val.cpu().numpy()), bits(ed.cpu().numpy())]


def check_stages(got, cls, n_pad, n, cols, rows):
    S, est, x, idx, ev, val, left, _ = oracle(cls, n_pad, n, cols, rows)
    for name, a, b in zip(("S", "est", "x", "idx", "est at idx", "val", "e"), got, (S, est, x, idx, ev, val, left)):
        assert np.array_equal(a, bits(b).reshape(-1)), name


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n_pad,n,cols,rows", SHAPES)
def test_stages(n_pad, n, cols, rows, cls):
    check_stages(run_stages(cls, n_pad, n, cols, rows), cls, n_pad, n, cols, rows)
    if cls == "special":  # the non-finite elements are selected, never hidden
        assert {3, 5, 990} <= set(oracle(cls, n_pad, n, cols, rows)[3].tolist())


def test_one_workgroup():
    check_stages(run_stages("normal", *SHAPES[3], max_blocks=1), "normal", *SHAPES[3])


@pytest.mark.parametrize("n,k", [(1000, 1), (4099, 40), (17461, 174), (17461, 17461)])
def test_select_keys_stable_sort(n, k):
    """Eighths in [-7/8, 7/8] (8 magnitudes, so the tie budget decides) against a stable descending sort of the keys;
    the plane is left alone."""
    from fpga_ai_nic_amd import _ext
    from fpga_ai_nic_amd.ops import topk as TK

    n_pad = (n + 255) // 256 * 256
    p = (np.random.default_rng(n + k).integers(-7, 8, n_pad) / 8).astype(np.float32)
    p[n:] = 1e30
    key = bits(p[:n]) & np.uint32(0x7FFFFFFF)
    want = np.sort(np.argsort(-key.astype(np.int64), kind="stable")[:k])
    pd = torch.from_numpy(p).to(DEV)
    wire = torch.full((TK.layout(n_pad, k)[2],), 0xAB, dtype=torch.uint8, device=DEV)
    _ext.require().topk.select_keys(pd, wire, torch.zeros(TK.layout(n_pad, k)[1], dtype=torch.int32, device=DEV), n, k)
    kp, w = TK.k_pad(k), wire.cpu().numpy()
    idx, val = w[: 4 * kp].view(np.uint32), w[4 * kp:].view(np.uint32)
    assert np.array_equal(idx[:k], want) and np.array_equal(val[:k], bits(p[want]))
    assert (idx[k:] == 0xFFFFFFFF).all() and not val[k:].any() and np.array_equal(bits(pd.cpu().numpy()), bits(p))


def test_reducer_two_ranks():
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    n_pad, n, cols, rows = SHAPES[3]
    gs = [planes("normal", n_pad, n)[0], planes("planted", n_pad, n)[0]]
    k = SK.count(n, 0.01)
    want_g, want_e, _, _ = O.step(gs, [np.zeros(n_pad, np.float32)] * 2, n, k, rows, cols, SEED)

    def rank_fn(transport):
        b = SimpleNamespace(n=n, grad=torch.from_numpy(gs[transport.rank].copy()).to(DEV))
        red = SketchReducer(transport, 0.01, rows=rows, cols=cols, seed=SEED)
        red.reduce(b)
        assert red.wire_bytes(b) == 4 * (rows * cols + SK.k_pad(k))
        return bits(b.grad.cpu().numpy()), bits(red.state_for(b).e.cpu().numpy())

    (ga, ea), (gb, eb) = ThreadFabric(2).run(rank_fn)
    assert np.array_equal(ga[:n], gb[:n]) and np.array_equal(ga[:n], bits(want_g[:n]))
    assert np.array_equal(ea, bits(want_e[0])) and np.array_equal(eb, bits(want_e[1]))
    assert np.array_equal(ga[n:], bits(gs[0][n:])) and np.array_equal(gb[n:], bits(gs[1][n:]))


def test_trainer_step():
    """One step of a 32-64-32 MLP with sketch=SketchReducer(None, 0.25, rows=3, cols=1024): every layer's grad and
    residual bit-identical to the oracle's step on the plain trainer's gradient, the weights to wire.sgd applied to
    that grad."""
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.ops import wire
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer

    sizes, mb, lr = [32, 64, 32], 16, 0.05
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=gen) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=gen, dtype=torch.int32).to(DEV)
    plain, sketched = (MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3) for _ in range(2))
    w0 = [l.master.clone() for l in sketched.layers]
    DataParallelTrainer(plain, None, lr=0.0).step(x, y)
    tr = DataParallelTrainer(sketched, None, lr=lr, sketch=SketchReducer(None, 0.25, rows=3, cols=1024, seed=SEED))
    tr.step(x, y)
    tr.finish()
    for l, ref, w, e in zip(sketched.layers, plain.layers, w0, tr.sketch_residuals):
        g0 = ref.grad.cpu().numpy()
        want_g, want_e, _, _ = O.step([g0], [np.zeros_like(g0)], l.n, SK.count(l.n, 0.25), 3, 1024, SEED)
        assert np.array_equal(bits(l.grad.cpu().numpy()), bits(want_g))
        assert np.array_equal(bits(e.cpu().numpy()), bits(want_e[0])) and bool(l.grad.any()) and bool(e.any())
        fed = torch.from_numpy(want_g).to(DEV)
        wire.sgd(wire.as_bytes(fed), l.n_pad, 1, w, codec="raw_f32", lr=lr, n_valid=l.n)
        assert torch.equal(l.master, w) and torch.equal(l.lp, l.master.to(torch.bfloat16))
