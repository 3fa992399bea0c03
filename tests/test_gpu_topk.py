"""Top-k sparsification on the GPU: the kernels of csrc/topk/topk_kernels.hip against the NumPy oracle, bit for bit;
the two-rank reducer and one trainer step."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import topk as TK
from fpga_ai_nic_amd.ops import topk_oracle as O
from fpga_ai_nic_amd.parallel.sparse import TopKReducer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NS = [16, 4096, 4099, 12304, 70000]  # one vector; one tile; a ragged tail; four tiles, ragged; 18 tiles, 69 hist tiles
CLASSES = ["normal", "eighths", "zeros", "special", "low_digits"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@lru_cache(maxsize=None)
def planes(cls, n):
    """(g, e) of n_pad = n rounded up to 256 elements; past n, g is huge and e a sentinel: neither may be read."""
    n_pad = (n + 255) // 256 * 256
    rng = np.random.default_rng(n + len(cls))
    g, e = rng.standard_normal(n_pad).astype(np.float32), (rng.standard_normal(n_pad) / 4).astype(np.float32)
    if cls == "eighths":  # 8 magnitudes: the threshold's ties span tiles and the tie budget decides
        g, e = (rng.integers(-7, 8, n_pad) / 8).astype(np.float32), np.zeros(n_pad, np.float32)
    elif cls == "zeros":
        g, e = np.zeros(n_pad, np.float32), np.zeros(n_pad, np.float32)
    elif cls == "special":  # (e stays finite beside a non-finite g: no Inf - Inf, whose NaN differs between machines)
        g[[3, 5, n - 1]] = np.nan, np.inf, -np.inf
        g[[7, 9, 11]], e[[7, 9, 11]] = (-0.0, 1e-40, -3e-42), (-0.0, 0.0, 0.0)
    elif cls == "low_digits":  # 1 + j * 2^-23: one top digit, passes 1 and 2 decide
        g, e = np.ones(n_pad, np.float32), (rng.permutation(n_pad) * 2.0 ** -23).astype(np.float32)
    g[n:], e[n:] = 1e30, 7.5
    g.setflags(write=False)
    e.setflags(write=False)
    return g, e


def run_select(g, e, n, k, max_blocks=None, scratch=None):
    wire = torch.full((TK.layout(g.size, k)[2],), 0xAB, dtype=torch.uint8, device=DEV)
    if scratch is None:
        scratch = torch.zeros(TK.layout(g.size, k)[1], dtype=torch.int32, device=DEV)
    ed = torch.from_numpy(e.copy()).to(DEV)
    TK.select(torch.from_numpy(g.copy()).to(DEV), ed, wire, scratch, n, k, max_blocks=max_blocks)
    kp = O.k_pad(k)
    w = wire.cpu().numpy()
    return w[: 4 * kp].view(np.uint32), w[4 * kp:].view(np.uint32), bits(ed.cpu().numpy())


CASES = [(c, n, k) for c in CLASSES for n in NS for k in sorted({1, 7, max(1, n // 100), n})]


@pytest.mark.parametrize("cls,n,k", CASES)
def test_select(cls, n, k):
    g, e = planes(cls, n)
    idx, val, en = O.select(g, e, n, k)
    got_idx, got_val, got_e = run_select(g, e, n, k)
    assert np.array_equal(got_idx, idx) and np.array_equal(got_val, bits(val)) and np.array_equal(got_e, bits(en))
    assert np.array_equal(got_e[n:], bits(e[n:]))
    if cls == "zeros":
        assert np.array_equal(idx[:k], np.arange(k))


@pytest.mark.parametrize("cls", ["normal", "eighths"])
def test_select_one_workgroup(cls):
    """A one-workgroup grid against the default, on one scratch (each select leaves it ready for the next)."""
    n, k = 12304, 123
    g, e = planes(cls, n)
    scratch = torch.zeros(TK.layout(g.size, k)[1], dtype=torch.int32, device=DEV)
    a, b = run_select(g, e, n, k, scratch=scratch), run_select(g, e, n, k, max_blocks=1, scratch=scratch)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def pack(wires):
    return torch.from_numpy(np.concatenate([np.concatenate([i.view(np.uint8), v.view(np.uint8)]) for i, v in wires]))


@pytest.mark.parametrize("max_blocks", [None, 1])
@pytest.mark.parametrize("world", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [4099, 12304])
def test_accumulate(n, world, max_blocks):
    """Indices overlap between the ranks (density 1/8 each), and rank 0 sends nothing past element 4095."""
    k = n // 8
    wires = []
    for r in range(world):
        g = planes("normal", n)[1 if r % 2 else 0] * np.float32(1 + r)
        if r == 0:
            g = np.where(np.arange(g.size) < 4096, g, np.float32(0))
        wires.append(O.select(g, np.zeros_like(g), n, k)[:2])
    assert not (wires[0][0][:k] >= 4096).any() and np.intersect1d(wires[0][0][:k], wires[-1][0][:k]).size > 0
    g0 = planes("normal", n)[0]
    inv = np.float32(1.0) / np.float32(world)
    gd = torch.from_numpy(g0.copy()).to(DEV)
    TK.accumulate(pack(wires).to(DEV), world, gd, n, k, float(inv), max_blocks=max_blocks)
    assert np.array_equal(bits(gd.cpu().numpy()), bits(O.accumulate(wires, g0, n, inv)))


def test_reducer_two_ranks():
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    n = 12304
    gs = [planes("normal", n)[0], planes("special", n)[0]]
    k = O.count(n, 0.01)
    want_g, want_e, _ = O.step(gs, [np.zeros_like(gs[0])] * 2, n, k)

    def rank_fn(transport):
        b = SimpleNamespace(n=n, grad=torch.from_numpy(gs[transport.rank].copy()).to(DEV))
        red = TopKReducer(transport, 0.01)
        red.reduce(b)
        assert red.wire_bytes(b) == 8 * O.k_pad(k) == 992
        return bits(b.grad.cpu().numpy()), bits(red.state_for(b).e.cpu().numpy())

    (ga, ea), (gb, eb) = ThreadFabric(2).run(rank_fn)
    assert np.array_equal(ga[:n], gb[:n]) and np.array_equal(ga[:n], bits(want_g[:n]))
    assert np.array_equal(ea, bits(want_e[0])) and np.array_equal(eb, bits(want_e[1]))
    assert np.array_equal(ga[n:], bits(gs[0][n:])) and np.array_equal(gb[n:], bits(gs[1][n:]))


def test_trainer_step():
    """One step of a 32-64-32 MLP with topk=TopKReducer(None, 0.25): every layer's grad and residual bit-identical to
    the stand-alone reduce of the plain trainer's gradient, the weights to wire.sgd applied to that grad."""
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.ops import wire
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer

    sizes, mb, lr = [32, 64, 32], 16, 0.05
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=gen) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=gen, dtype=torch.int32).to(DEV)
    plain, sparse = (MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3) for _ in range(2))
    w0 = [l.master.clone() for l in sparse.layers]
    DataParallelTrainer(plain, None, lr=0.0).step(x, y)
    tr = DataParallelTrainer(sparse, None, lr=lr, topk=TopKReducer(None, 0.25))
    tr.step(x, y)
    tr.finish()
    alone = TopKReducer(None, 0.25)
    for l, ref, w, e in zip(sparse.layers, plain.layers, w0, tr.topk_residuals):
        alone.reduce(ref)
        assert torch.equal(l.grad, ref.grad) and torch.equal(e, alone.state_for(ref).e)
        assert int((l.grad[: l.n] != 0).sum()) <= l.n // 4 and bool(l.grad.any()) and bool(e.any())
        wire.sgd(wire.as_bytes(ref.grad), l.n_pad, 1, w, codec="raw_f32", lr=lr, n_valid=l.n)
        assert torch.equal(l.master, w) and torch.equal(l.lp, l.master.to(torch.bfloat16))
    with pytest.raises(ValueError, match="lives on"):
        TK.select(torch.zeros(256, device=DEV), torch.zeros(256), torch.zeros(32, dtype=torch.uint8, device=DEV),
                  torch.zeros(TK.layout(256, 4)[1], dtype=torch.int32, device=DEV), 256, 4)
