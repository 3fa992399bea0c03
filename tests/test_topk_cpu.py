"""Top-k sparsification with memory: the NumPy oracle (ops/topk_oracle.py), the CPU ops and the reducer."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import topk as TK
from fpga_ai_nic_amd.ops import topk_oracle as O
from fpga_ai_nic_amd.parallel.sparse import TopKReducer


def planes(n, n_pad, seed, ties=False):
    rng = np.random.default_rng(seed)
    if ties:  # eighths in [-7/8, 7/8]: 15 values, 8 magnitudes
        return (rng.integers(-7, 8, n_pad) / 8).astype(np.float32), np.zeros(n_pad, np.float32)
    return rng.standard_normal(n_pad).astype(np.float32), (rng.standard_normal(n_pad) / 4).astype(np.float32)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n,k", [(16, 1), (16, 16), (4099, 7), (4099, 40), (12304, 123), (12304, 12304)])
def test_select_matches_stable_sort(n, k, ties):
    """The threshold form of the oracle picks what a stable descending sort of the keys picks first."""
    n_pad = (n + 255) // 256 * 256
    g, e = planes(n, n_pad, n + k, ties)
    idx, val, en = O.select(g, e, n, k)
    x = g + e
    key = x[:n].view(np.uint32) & np.uint32(0x7FFFFFFF)
    want = np.sort(np.argsort(-key.astype(np.int64), kind="stable")[:k])
    assert np.array_equal(idx[:k], want) and np.array_equal(val[:k].view(np.uint32), x[want].view(np.uint32))
    assert (idx[k:] == O.PAD_IDX).all() and not val[k:].view(np.uint32).any() and idx.size == O.k_pad(k)
    left = np.concatenate([x[:n], e[n:]])  # (past n the residual is not touched)
    left[want] = 0
    assert np.array_equal(en.view(np.uint32), left.view(np.uint32))


@pytest.mark.parametrize("n,k", [(4099, 1), (4099, 40), (12304, 3076)])
def test_contraction(n, k):
    """||x - sent||^2 <= (1 - k/n) ||x||^2 in float64: the k removed squares are the largest, so their mean is at
    least the overall mean."""
    g, e = planes(n, (n + 3) // 4 * 4, n)
    idx, val, en = O.select(g, e, n, k)
    x = (g + e)[:n].astype(np.float64)
    assert np.sum(en[:n].astype(np.float64) ** 2) <= (1 - k / n) * np.sum(x ** 2)


def test_error_feedback_converges():
    """A constant g over T steps: sum_t sent_t = T g - e_T up to the accumulate adds' rounding, and ||e_T|| <=
    rho / (1 - rho) ||g|| with rho = sqrt(1 - k/n) (the contraction above, summed as a geometric series). So
    ||mean of sent - g||_2 <= rho / (1 - rho) ||g||_2 / T + sqrt(n) 2^-24 max_t |x_t| (each step rounds x_t = g + e
    once per element: T roundings of at most 2^-24 max|x_t|, divided by T). Measured at n = 4096, k = 409:
    T = 16: 1.565e+01, T = 64: 4.086e+00, T = 256: 1.038e+00 against bounds 7.423e+01, 1.856e+01, 4.639e+00."""
    n, k = 4096, 409
    g = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    rho = np.sqrt(1 - k / n)
    e, acc, xmax = np.zeros(n, np.float32), np.zeros(n), 0.0
    norm = np.linalg.norm(g.astype(np.float64))
    for t in range(1, 257):
        xmax = max(xmax, float(np.abs(g + e).max()))
        idx, val, e = O.select(g, e, n, k)
        acc[idx[:k]] += val[:k]
        if t in (16, 64, 256):
            dist = np.linalg.norm(acc / t - g)
            bound = rho / (1 - rho) * norm / t + np.sqrt(n) * 2.0 ** -24 * xmax
            print(f"T = {t}: ||mean of sent - g|| = {dist:.3e}, bound {bound:.3e}")
            assert dist <= bound


def test_two_ranks_on_cpu_fabric():
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    n, n_pad = 4099, 4352
    gs, es = zip(*(planes(n, n_pad, 20 + r) for r in range(2)))
    k = O.count(n, 0.01)
    want_g, want_e, _ = O.step(gs, [np.zeros(n_pad, np.float32)] * 2, n, k)
    want2_g, want2_e, _ = O.step(gs, want_e, n, k)

    def rank_fn(transport):
        b = SimpleNamespace(n=n, grad=torch.from_numpy(gs[transport.rank].copy()))
        red = TopKReducer(transport, 0.01)
        red.reduce(b)
        first = b.grad.clone()
        b.grad.copy_(torch.from_numpy(gs[transport.rank]))
        red.reduce(b)  # (the second step sends what the first left in the residual)
        assert red.wire_bytes(b) == 8 * O.k_pad(k)
        return first.numpy(), b.grad.numpy(), red.state_for(b).e.numpy()

    out = ThreadFabric(2).run(rank_fn)
    for r in range(2):
        assert np.array_equal(out[r][0][:n].view(np.uint32), want_g[:n].view(np.uint32))
        assert np.array_equal(out[r][1][:n].view(np.uint32), want2_g[:n].view(np.uint32))
        assert np.array_equal(out[r][2].view(np.uint32), want2_e[r].view(np.uint32))
        assert np.array_equal(out[r][0][n:], gs[r][n:])


def test_refusals():
    from fpga_ai_nic_amd.cli.mlp_mpi import build_parser
    from fpga_ai_nic_amd.config import config_from_args
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    for bad in (0.0, -0.5, 1.5, True, "1"):
        with pytest.raises(ValueError, match="density"):
            TopKReducer(None, bad)
    with pytest.raises(ValueError, match="16 ranks"):
        TopKReducer(SimpleNamespace(world=17), 0.5)
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt)
    wire, scratch = z(8 * 4, torch.uint8), z(TK.layout(256, 4)[1], torch.int32)
    for args in ((z(256, torch.float64), z(256), wire, scratch, 256, 4),    # not f32
                 (z(512)[::2], z(256), wire, scratch, 256, 4),              # not contiguous
                 (z(256), z(252), wire, scratch, 256, 4),                   # e of the wrong length
                 (z(256), z(256), wire[:-1], scratch, 256, 4),              # wire of the wrong length
                 (z(256), z(256), wire, scratch[:-1], 256, 4),              # scratch of the wrong length
                 (z(254), z(254), wire, scratch, 254, 4),                   # n_pad % 4
                 (z(256), z(256), wire, scratch, 257, 4),                   # n above n_pad
                 (z(256), z(256), wire, scratch, 256, 0),                   # k outside 1..n
                 (z(256), z(256), wire, scratch, 3, 4)):
        with pytest.raises(ValueError, match="topk"):
            TK.select(*args)
    with pytest.raises(ValueError, match="max_blocks"):
        TK.select(z(256), z(256), wire, scratch, 256, 4, max_blocks=0)
    with pytest.raises(ValueError, match="below 2\\^31"):
        O.check_shape(2 ** 31, 16, 1)
    with pytest.raises(ValueError, match="ranks"):
        TK.accumulate(z(17 * 32, torch.uint8), 17, z(256), 256, 4, 1.0)
    with pytest.raises(ValueError, match="wires"):
        TK.accumulate(z(2 * 32 - 8, torch.uint8), 2, z(256), 256, 4, 0.5)
    model = MLP([32, 48, 16], dtype=torch.float32, device="cpu")
    eng = make_engine(ThreadFabric(1).transport(0), "bfp", device="cpu")
    for kw in (dict(engine=eng), dict(error_feedback=True), dict(stochastic_rounding=True),
               dict(lowrank=LowRankReducer(None, 4))):
        with pytest.raises(ValueError, match="topk"):
            DataParallelTrainer(model, kw.pop("engine", None), topk=TopKReducer(None, 0.1), **kw)
    for argv in (["--compress", "topk", "--density", "0"], ["--compress", "topk", "--error-feedback"]):
        with pytest.raises(ValueError, match="topk|density"):
            config_from_args(build_parser().parse_args(["1", "32"] + argv))
