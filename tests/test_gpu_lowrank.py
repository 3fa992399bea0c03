"""PowerSGD low-rank compression on the GPU: every kernel of csrc/lowrank/lowrank_kernels.hip against a plain fp64
reference or the NumPy oracle, the two-rank reducer and the trainer."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import lowrank as LR
from fpga_ai_nic_amd.ops import lowrank_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
# one fragment; exactly one project tile; ragged panel and strip; several column strips; several row strips and tiles
SHAPES = [(16, 16), (64, 512), (80, 528), (192, 1040), (528, 272)]


def gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("e_scale", [0.0, 0.125])
@pytest.mark.parametrize("rank", [1, 4, 16])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_products(rows, cols, rank, e_scale):
    """P = X Q and Qn = X^T P^ against the fp64 product of the same f32 X: per element within gamma_n sum_k |x||q|, n =
    the K length + the strip count + 1; output columns >= rank exactly 0."""
    gen = torch.Generator().manual_seed(rows * 7 + cols + rank)
    g, e = torch.randn(rows * cols, generator=gen), torch.randn(rows * cols, generator=gen) * e_scale
    q = torch.from_numpy(O.init_q(cols, rank, 3))
    x = (g + e).view(rows, cols).double()
    sp, sb, n_part = LR.layout(rows, cols)
    part = torch.full((n_part,), float("nan"), device=DEV)
    p = LR.project(g.to(DEV), e.to(DEV), q.to(DEV), part, torch.empty(rows, 16, device=DEV), rows, cols).cpu()
    assert bool(((p.double() - x @ q.double()).abs() <= gamma(cols + sp + 1) * (x.abs() @ q.double().abs())).all())
    assert not bool(p[:, rank:].any())
    ph = torch.from_numpy(O.orth(p.numpy(), rank))
    qn = LR.backproject(g.to(DEV), e.to(DEV), ph.to(DEV), part, torch.empty(cols, 16, device=DEV), rows, cols).cpu()
    assert bool(((qn.double() - x.t() @ ph.double()).abs()
                 <= gamma(rows + sb + 1) * (x.t().abs() @ ph.double().abs())).all())
    assert not bool(qn[:, rank:].any())


@pytest.mark.parametrize("rank", [1, 4, 16])
@pytest.mark.parametrize("rows", [64, 272])
def test_orth(rows, rank):
    """Against the oracle within (r+1)(r+2)/2 * 2^-24 * max|P^|: at most j + 1 f32 roundings on column j, plus the
    inherited errors of the earlier columns, each scaled by a projection coefficient below 1."""
    p = torch.randn(rows, 16, generator=torch.Generator().manual_seed(rows + rank)) * 3
    p[:, rank:] = 0
    ref = torch.from_numpy(O.orth(p.numpy(), rank))
    out = LR.orth(p.to(DEV), rank).cpu()
    assert float((out - ref).abs().max()) <= (rank + 1) * (rank + 2) / 2 * U * float(ref.abs().max())
    assert not bool(out[:, rank:].any())


@pytest.mark.parametrize("e_scale", [0.0, 0.125])
@pytest.mark.parametrize("rank", [1, 4, 16])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_reconstruct(rows, cols, rank, e_scale):
    gen = torch.Generator().manual_seed(rows + cols * 5 + rank)
    n = rows * cols
    g, e = torch.randn(n + 48, generator=gen), torch.randn(n, generator=gen) * e_scale
    ph, qn = torch.randn(rows, 16, generator=gen), torch.randn(cols, 16, generator=gen)
    ph[:, rank:], qn[:, rank:] = 0, 0
    ph = torch.from_numpy(O.orth(ph.numpy(), rank))
    inv = float(np.float32(1.0) / np.float32(3.0))
    gd, ed, qd = g.to(DEV), e.to(DEV), torch.full((cols, 16), float("nan"), device=DEV)
    LR.reconstruct(gd, ed, ph.to(DEV), qn.to(DEV), qd, inv, rows, cols)
    qm = qn * inv
    assert torch.equal(qd.cpu(), qm)
    gh = gd.cpu()[:n].view(rows, cols)
    ref, mag = ph.double() @ qm.double().t(), ph.double().abs() @ qm.double().abs().t()
    assert bool(((gh.double() - ref).abs() <= gamma(17) * mag).all())
    assert torch.equal(ed.cpu().view(rows, cols), (g[:n] + e).view(rows, cols) - gh)
    assert torch.equal(gd.cpu()[n:], g[n:])


def test_reducer_two_ranks():
    """Two virtual ranks on one GPU, the inputs of tests/test_lowrank_cpu.py::test_exact_rank_mean_is_reproduced: both
    end with bit-identical G, Q and tail, and the relative Frobenius error against the fp64 run of the algorithm is at
    most 4x the f32 oracle's (7.2e-07; the margin covers the matrix instruction's summation order). Measured on an
    MI355X: 7.7e-07 (profiles/lowrank.txt)."""
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    rows, cols, r = 80, 528, 4
    rng = np.random.default_rng(11)
    eighths = lambda *shape: np.round(rng.standard_normal(shape) * 8) / 8
    m = (eighths(rows, r) @ eighths(r, cols)).astype(np.float32)
    n = eighths(rows, cols).astype(np.float32)
    gs = [m + n, m - n]
    tails = [rng.standard_normal(cols).astype(np.float32) for _ in range(2)]
    zeros = [np.zeros((rows, cols), np.float32)] * 2
    g32 = O.step(gs, zeros, O.init_q(cols, r, 0), r)[0]
    g64 = O.step(gs, zeros, O.init_q(cols, r, 0), r, dtype=np.float64)[0]

    def rank_fn(transport):
        grad = torch.from_numpy(np.concatenate([gs[transport.rank].ravel(), tails[transport.rank]])).to(DEV)
        b = SimpleNamespace(cin=rows, cout=cols, n=grad.numel(), grad=grad)
        red = LowRankReducer(transport, r, seed=0)
        red.reduce(b)
        assert red.wire_bytes(b) == 4 * ((rows + cols) * r + cols)
        return grad.cpu(), red.state_for(b).q.cpu()

    (ga, qa), (gb, qb) = ThreadFabric(2).run(rank_fn)
    assert torch.equal(ga, gb) and torch.equal(qa, qb)
    assert np.array_equal(ga[rows * cols:].numpy(), (tails[0] + tails[1]) * np.float32(0.5))
    fro = np.linalg.norm
    got = ga[: rows * cols].view(rows, cols).numpy().astype(np.float64)
    err, ref_err = fro(got - g64) / fro(g64), fro(g32 - g64) / fro(g64)
    print(f"reducer: GPU rel. Frobenius error {err:.3e}, f32 oracle {ref_err:.3e}")
    assert err <= 4 * ref_err


def test_trainer_step():
    """One step of a 32-64-32 MLP with lowrank=LowRankReducer(None, 16): every layer's grad and residual bit-identical
    to the stand-alone reduce of the plain trainer's gradient, the weights to wire.sgd applied to that grad."""
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.ops import wire
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer

    sizes, mb, lr = [32, 64, 32], 16, 0.05
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=gen) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=gen, dtype=torch.int32).to(DEV)
    plain, low = (MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3) for _ in range(2))
    w0 = [l.master.clone() for l in low.layers]
    DataParallelTrainer(plain, None, lr=0.0).step(x, y)
    tr = DataParallelTrainer(low, None, lr=lr, lowrank=LowRankReducer(None, 16, seed=5))
    tr.step(x, y)
    tr.finish()
    alone = LowRankReducer(None, 16, seed=5)
    for l, ref, w, e, q in zip(low.layers, plain.layers, w0, tr.lowrank_residuals, tr.lowrank_q):
        alone.reduce(ref)
        st = alone.state_for(ref)
        assert torch.equal(l.grad, ref.grad) and torch.equal(e, st.e) and torch.equal(q, st.q)
        assert bool(l.grad[: l.cin * l.cout].any()) and bool(e.any())
        wire.sgd(wire.as_bytes(ref.grad), l.n_pad, 1, w, codec="raw_f32", lr=lr, n_valid=l.n)
        assert torch.equal(l.master, w) and torch.equal(l.lp, l.master.to(torch.bfloat16))
    with pytest.raises(ValueError, match="rank"):
        LowRankReducer(None, 17)
    with pytest.raises(ValueError, match="multiples of 16"):
        LR.project(torch.zeros(24 * 16, device=DEV), torch.zeros(24 * 16, device=DEV), torch.zeros(16, 16, device=DEV),
                   torch.zeros(24 * 16, device=DEV), torch.zeros(24, 16, device=DEV), 24, 16)
    with pytest.raises(ValueError, match="float32"):
        LR.orth(torch.zeros(16, 16, device=DEV, dtype=torch.float64), 4)
    with pytest.raises(ValueError, match="lives on"):
        LR.project(torch.zeros(256, device=DEV), torch.zeros(256), torch.zeros(16, 16, device=DEV),
                   torch.zeros(256, device=DEV), torch.zeros(16, 16, device=DEV), 16, 16)
    with pytest.raises(ValueError, match="elements"):
        LR.project(torch.zeros(256, device=DEV), torch.zeros(128, device=DEV), torch.zeros(16, 16, device=DEV),
                   torch.zeros(256, device=DEV), torch.zeros(16, 16, device=DEV), 16, 16)
