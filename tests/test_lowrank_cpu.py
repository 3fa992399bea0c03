"""PowerSGD low-rank compression: the NumPy oracle (ops/lowrank_oracle.py) on the CPU."""
import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import lowrank_oracle as O

U = 2.0 ** -24


def test_exact_rank_mean_is_reproduced():
    """Two ranks whose gradients M + N and M - N are full rank but whose mean M has rank r: one reduction returns M.
    Prints the f32 oracle's relative Frobenius error against the fp64 run of the same algorithm (7.2e-07 on these
    inputs) — the reference figure of tests/test_gpu_lowrank.py::test_reducer_two_ranks. Bound: the f32 summation error
    of the longer of the two products, gamma_n with n = 528 + 2, once per product."""
    rows, cols, r = 80, 528, 4
    rng = np.random.default_rng(11)
    eighths = lambda *shape: np.round(rng.standard_normal(shape) * 8) / 8  # (M, M + N and M - N are exact in f32)
    m = (eighths(rows, r) @ eighths(r, cols)).astype(np.float32)
    n = eighths(rows, cols).astype(np.float32)
    gs, es = [m + n, m - n], [np.zeros((rows, cols), np.float32)] * 2
    tails = [rng.standard_normal(cols).astype(np.float32) for _ in range(2)]
    q = O.init_q(cols, r, 0)
    g32, e32, q32, t32 = O.step(gs, es, q, r, tails)
    g64, _, _, _ = O.step(gs, es, q, r, tails, dtype=np.float64)
    exact = (gs[0].astype(np.float64) + gs[1].astype(np.float64)) / 2
    fro = np.linalg.norm
    print(f"f32 oracle vs fp64 run: {fro(g32 - g64) / fro(g64):.3e}; fp64 run vs exact mean: "
          f"{fro(g64 - exact) / fro(exact):.3e}")
    # (the fp64 run is exact up to orth's 1e-8 beside norms in the hundreds: columns short of unit length by ~1e-10)
    assert g32.dtype == np.float32 and fro(g64 - exact) / fro(exact) < 1e-9
    assert fro(g32 - g64) / fro(g64) <= 2 * (530 * U) / (1 - 530 * U)
    assert np.array_equal(t32, (tails[0] + tails[1]) * np.float32(0.5))
    assert not q32[:, r:].any() and all(np.array_equal(e, (g + 0) - g32) for g, e in zip(gs, e32))


def test_constant_gradient_error_feedback_converges():
    """A constant full-rank gradient over T steps at rank 2: sum_t G^_t = T G - E_T telescopes, so mean_T(G^) -> G as
    long as E stays bounded. E_t = (I - P^ P^T) X_t is a projection of X_t = G + E_{t-1}, so ||E_t|| <= ||X_t||; it
    stops growing once a dropped direction has accumulated enough to enter the top r: asserted as no growth over the
    second half of the run."""
    rows, cols, r = 32, 48, 2
    g = np.random.default_rng(5).standard_normal((rows, cols)).astype(np.float32)
    e, q = np.zeros_like(g), O.init_q(cols, r, 0)
    acc, dist, enorm = np.zeros((rows, cols)), {}, []
    for t in range(1, 65):
        gh, (e,), q, _ = O.step([g], [e], q, r)
        acc += gh
        dist[t] = np.linalg.norm(acc / t - g)
        enorm.append(np.linalg.norm(e))
    assert np.isfinite(enorm).all() and max(enorm[32:]) <= 1.25 * max(enorm[:32])
    assert dist[64] < dist[4]


@pytest.mark.parametrize("rows,cols,rank", [(80, 528, 0), (80, 528, 17), (80, 520, 4), (72, 528, 4), (16, 32, True)])
def test_refused_shapes(rows, cols, rank):
    with pytest.raises(ValueError):
        O.check_shape(rows, cols, rank)


def test_cpu_reducer_and_trainer_refusals():
    """The reducer on CPU tensors runs the oracle; the trainer refuses lowrank with an engine or another residual."""
    from types import SimpleNamespace

    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    rows, cols, r = 32, 48, 4
    g0 = torch.randn(rows * cols + cols + 16, generator=torch.Generator().manual_seed(2))
    b = SimpleNamespace(cin=rows, cout=cols, n=rows * cols + cols, grad=g0.clone())
    red = LowRankReducer(None, r, seed=7)
    red.reduce(b)
    gm = g0[: rows * cols].view(rows, cols).numpy()
    gh, (e,), qm, _ = O.step([gm], [np.zeros_like(gm)], O.init_q(cols, r, 7), r)
    st = red.state_for(b)
    assert np.array_equal(b.grad[: rows * cols].view(rows, cols).numpy(), gh)
    assert np.array_equal(st.e.view(rows, cols).numpy(), e) and np.array_equal(st.q.numpy(), qm)
    assert torch.equal(b.grad[rows * cols:], g0[rows * cols:]) and red.wire_bytes(b) == 0
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError):
            LowRankReducer(None, bad)
    model = MLP([32, 48, 16], dtype=torch.float32, device="cpu")
    eng = make_engine(ThreadFabric(1).transport(0), "bfp", device="cpu")
    for kw in (dict(engine=eng), dict(error_feedback=True), dict(stochastic_rounding=True)):
        with pytest.raises(ValueError, match="lowrank"):
            DataParallelTrainer(model, kw.pop("engine", None), lowrank=LowRankReducer(None, r), **kw)
    with pytest.raises(ValueError, match="multiples of 16"):
        DataParallelTrainer(MLP([32, 40, 16], dtype=torch.float32, device="cpu"), None, lowrank=LowRankReducer(None, r))
