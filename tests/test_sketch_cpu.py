"""Count-sketch compression: the NumPy oracle (ops/sketch_oracle.py), the CPU ops and the reducer."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import sketch as SK
from fpga_ai_nic_amd.ops import sketch_oracle as O
from fpga_ai_nic_amd.ops.bfp_oracle import sr_hash, sr_key
from fpga_ai_nic_amd.parallel.sketch import SketchReducer


def planted(n, n_pad, seed, amp=64.0, count=16):
    """Unit normal noise with `count` planted elements of amplitude `amp` and random sign: (g, the planted indices)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n_pad).astype(np.float32)
    where = np.sort(rng.choice(n, count, replace=False))
    g[where] = amp * rng.choice([-1.0, 1.0], count)
    return g, where


@pytest.mark.parametrize("n_pad,n,cols,rows", [(1024, 1000, 1024, 1), (6144, 6144, 2048, 3), (17920, 17461, 1024, 5)])
def test_definition(n_pad, n, cols, rows):
    """Small integers, so every f32 sum is exact: the sketch and the estimate against the definition restated element by
    element in float64 (a scatter by column and signed add; a sort for the median)."""
    rng = np.random.default_rng(n)
    g, e = (rng.integers(-8, 9, n_pad).astype(np.float32) for _ in range(2))
    seed = 0x1234_5678_9ABC_DEF0 + n
    x = g.astype(np.float64) + e
    want = np.zeros((rows, cols))
    col, sgn = np.zeros((rows, n), dtype=np.int64), np.zeros((rows, n))
    for j in range(rows):
        for i in range(n):
            off = 4 * (int(sr_hash(*sr_key(seed, j, 0), i // cols)) % (cols // 4))
            col[j, i] = (i % cols + off) % cols
            sgn[j, i] = -1.0 if (int(sr_hash(*sr_key(seed, j, 1), i >> 5)) >> (i & 31)) & 1 else 1.0
            want[j, col[j, i]] += sgn[j, i] * x[i]
    S = O.sketch(g, e, n, rows, cols, seed)
    assert np.array_equal(S.astype(np.float64), want)
    est, left = O.estimate(g, e, S, n, seed)
    med = np.sort(np.stack([sgn[j] * want[j, col[j]] for j in range(rows)]), axis=0)[rows // 2]
    assert np.array_equal(est[:n].astype(np.float64), med) and np.array_equal(left[:n].astype(np.float64), x[:n])
    assert np.array_equal(est[n:], g[n:]) and np.array_equal(left[n:], e[n:])


def test_recovery():
    """n = 16384, C = 2048, R = 5, k = 16: a row's estimate error has standard deviation at most ||x|| / sqrt(C) =
    sqrt(16384 + 16 * 64^2) / sqrt(2048) = 6.3, a tenth of the planted amplitude 64, so the 16 planted elements are
    exactly what is selected. Measured: the worst |est - x| over all elements is printed (6.651 at this seed)."""
    n, cols, rows, k = 16384, 2048, 5, 16
    g, where = planted(n, n, 7)
    S = O.sketch(g, np.zeros_like(g), n, rows, cols, 11)
    est, x = O.estimate(g, np.zeros_like(g), S, n, 11)
    print(f"worst |est - x| = {np.abs(est.astype(np.float64) - x).max():.3f}")
    idx, _ = O.select_keys(est, n, k)
    assert np.array_equal(idx, where)


def test_two_ranks_on_cpu_fabric():
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    n, n_pad, rows, cols, seed = 17461, 17920, 3, 1024, 5
    gs = [planted(n, n_pad, 20 + r)[0] for r in range(2)]
    k = SK.count(n, 0.01)

    def rank_fn(transport):
        b = SimpleNamespace(n=n, grad=torch.from_numpy(gs[transport.rank].copy()))
        red = SketchReducer(transport, 0.01, rows=rows, cols=cols, seed=seed)
        red.reduce(b)
        assert red.wire_bytes(b) == 4 * (rows * cols + SK.k_pad(k))
        st = red.state_for(b)
        return b.grad.numpy(), st.e.numpy(), st.wire[: 4 * k].view(torch.int32).numpy()

    (ga, ea, ia), (gb, eb, ib) = ThreadFabric(2).run(rank_fn)
    assert np.array_equal(ga[:n].view(np.uint32), gb[:n].view(np.uint32)) and np.array_equal(ia, ib)
    mean = ((gs[0] + gs[1]) * np.float32(0.5))[ia]  # (the residuals start at zero: x = g)
    assert np.array_equal(ga[ia], mean) and np.count_nonzero(ga[:n]) == np.count_nonzero(mean)
    for g, e in zip(gs, (ea, eb)):
        left = g.copy()
        left[ia] = 0
        assert np.array_equal(e[:n].view(np.uint32), left[:n].view(np.uint32)) and not e[n:].any()
    want_g, want_e, _, _ = O.step(gs, [np.zeros(n_pad, np.float32)] * 2, n, k, rows, cols, seed)
    assert np.array_equal(ga.view(np.uint32), want_g.view(np.uint32))
    assert np.array_equal(ea.view(np.uint32), want_e[0].view(np.uint32))


def test_refusals():
    from fpga_ai_nic_amd.cli.mlp_mpi import build_parser
    from fpga_ai_nic_amd.config import config_from_args
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
    from fpga_ai_nic_amd.parallel.sparse import TopKReducer
    from fpga_ai_nic_amd.parallel.transport import ThreadFabric

    for kw, what in ((dict(density=0.0), "density"), (dict(density=0.5, rows=2), "rows"),
                     (dict(density=0.5, cols=1000), "cols"), (dict(density=0.5, cols=1 << 23), "cols"),
                     (dict(density=0.5, seed=-1), "seed"), (dict(density=0.5, seed=1 << 64), "seed")):
        with pytest.raises(ValueError, match=what):
            SketchReducer(None, **kw)
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt)
    sk, part, words, nbytes = SK.layout(2048, 4, 3, 1024)
    S, P, wire, scratch = z(sk), z(part), z(nbytes, torch.uint8), z(words, torch.int32)
    for args in ((z(2048, torch.float64), z(2048), S, P, 2048, 3, 1024, 0),   # not f32
                 (z(4096)[::2], z(2048), S, P, 2048, 3, 1024, 0),             # not contiguous
                 (z(2048), z(2044), S, P, 2048, 3, 1024, 0),                  # e of the wrong length
                 (z(2048), z(2048), S[:-4], P, 2048, 3, 1024, 0),             # S of the wrong length
                 (z(2048), z(2048), S, P[:-4], 2048, 3, 1024, 0),             # part of the wrong length
                 (z(2046), z(2046), S, P, 2046, 3, 1024, 0),                  # n_pad % 4
                 (z(2048), z(2048), S, P, 2049, 3, 1024, 0),                  # n above n_pad
                 (z(2048), z(2048), S, P, 2048, 4, 1024, 0),                  # rows
                 (z(2048), z(2048), S, P, 2048, 3, 1536 + 8, 0),              # cols
                 (z(2048), z(2048), S, P, 2048, 3, 1024, -1)):                # seed
        with pytest.raises(ValueError, match="sketch"):
            SK.sketch(*args)
    g = z(2048)
    with pytest.raises(ValueError, match="of their own"):
        SK.sketch(g, g, S, P, 2048, 3, 1024, 0)
    with pytest.raises(ValueError, match="max_blocks"):
        SK.sketch(z(2048), z(2048), S, P, 2048, 3, 1024, 0, max_blocks=0)
    with pytest.raises(ValueError, match="sketch: k must"):
        SK.estimate_select(z(2048), z(2048), S, wire, scratch, 2048, 0, 3, 1024, 0)
    with pytest.raises(ValueError, match="wire"):
        SK.estimate_select(z(2048), z(2048), S, wire[:-1], scratch, 2048, 4, 3, 1024, 0)
    with pytest.raises(ValueError, match="wire"):
        SK.fetch(z(2048), wire[:-1], 2048, 4)
    model = MLP([32, 48, 16], dtype=torch.float32, device="cpu")
    eng = make_engine(ThreadFabric(1).transport(0), "bfp", device="cpu")
    for kw in (dict(engine=eng), dict(error_feedback=True), dict(stochastic_rounding=True),
               dict(lowrank=LowRankReducer(None, 4)), dict(topk=TopKReducer(None, 0.1))):
        with pytest.raises(ValueError, match="sketch"):
            DataParallelTrainer(model, kw.pop("engine", None), sketch=SketchReducer(None, 0.1, cols=1024), **kw)
    for argv in (["--compress", "sketch", "--density", "0"], ["--compress", "sketch", "--error-feedback"],
                 ["--compress", "sketch", "--sketch-cols", "1000"], ["--compress", "topk", "--sketch-rows", "3"],
                 ["--sketch-cols", "2048"], ["--sketch-seed", "3"]):
        with pytest.raises(ValueError, match="sketch|density"):
            config_from_args(build_parser().parse_args(["1", "32"] + argv))
    cfg = config_from_args(build_parser().parse_args(["1", "32", "--compress", "sketch", "--sketch-rows", "3"]))
    assert (cfg.sketch_rows, cfg.sketch_cols, cfg.sketch_seed) == (3, 65536, 0)
