"""Rotated one-bit compression: the NumPy oracle (ops/rht_oracle.py), the CPU ops and the reducer."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import bfp_oracle
from fpga_ai_nic_amd.ops import rht as RH
from fpga_ai_nic_amd.ops import rht_oracle as O
from fpga_ai_nic_amd.parallel.rotated import RotatedSignReducer
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

B = O.B


def inputs(kind, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_t(2, n) if kind == "student" else rng.standard_normal(n)
    if kind == "spikes":
        x, x[::16] = x * 0.01, rng.choice([-1.0, 1.0], n // 16)
    return x.astype(np.float32)


def one_bit(y):
    """The decoded one-bit value of the rotated blocks y, in float64."""
    y = y.astype(np.float64).reshape(-1, B)
    return (np.where(y < 0, -1.0, 1.0) * np.abs(y).mean(axis=1, keepdims=True)).reshape(-1)


def test_contraction():
    """||y - dec||^2 = ||y||^2 - ||y||_1^2 / 4096 per block. s is the minimiser, so its rounding enters squared; e' is
    rounded to f32 per element, 2^-24 relative, 2^-23 on its square: 2^-22 * ||y||^2 covers both."""
    g = inputs("student", 3 * B, 3)
    y = O.transform(g, 9).astype(np.float64).reshape(3, B)
    _, _, left = O.encode(g, np.zeros(3 * B, np.float32), 3 * B, 9)
    got = (left.astype(np.float64).reshape(3, B) ** 2).sum(axis=1)
    want = (y ** 2).sum(axis=1) - np.abs(y).sum(axis=1) ** 2 / B
    print("kept energy per block:", 1 - got / (y ** 2).sum(axis=1))
    assert (np.abs(got - want) <= 2.0 ** -22 * (y ** 2).sum(axis=1)).all()


def test_round_trip_table():
    """Relative L2 error of one round trip on 65536 values: sign1 against rotate, one bit and a scale, rotate back."""
    err = {}
    for kind in ("normal", "student", "spikes"):
        x = inputs(kind, 65536, 11)
        back = O.transform(one_bit(O.transform(x, 4)).astype(np.float32), 4, inverse=True)
        rel = lambda q: np.linalg.norm(q.astype(np.float64) - x) / np.linalg.norm(x.astype(np.float64))  # noqa: E731
        err[kind] = rel(bfp_oracle.quantize(x, "sign1")), rel(back)
        print(f"{kind}: sign1 {err[kind][0]:.3f} rotated {err[kind][1]:.3f}")
    assert err["student"][1] < err["student"][0] and err["spikes"][1] < err["spikes"][0]


def test_error_feedback():
    """A constant Student-t gradient, one block: sum_t dec_t = T y0 - e_T, so the mean of the decoded blocks misses
    y0 = rht(g) by ||e_T|| / T. The contraction identity makes step t a contraction by rho_t = sqrt(1 - c_t), c_t the
    share of ||y_t||^2 kept, so ||e_T|| <= rho / (1 - rho) ||y0|| with rho = max rho_t = sqrt(1 - 2/pi + slack) and
    slack = 2/pi - min c_t from a float64 restatement of the recursion: y_t = y0 + e_(t-1) is not Gaussian, c_t falls
    from 0.65 to 0.044 and the error decays like 1 / sqrt(T): 0.594 / 0.182 / 0.089 / 0.046 at T = 1 / 16 / 64 / 256."""
    g = inputs("student", B, 1)
    y0 = O.transform(g, 5).astype(np.float64)
    e64, cmin = np.zeros(B), 1.0
    e, total = np.zeros(B, np.float32), np.zeros(B)
    for t in range(1, 257):
        y = y0 + e64
        cmin = min(cmin, np.abs(y).sum() ** 2 / B / (y ** 2).sum())
        e64 = y - one_bit(y)
        sign, scale, e = O.encode(g, e, B, 5)
        total += np.where(np.unpackbits(sign, bitorder="little") != 0, -1.0, 1.0) * scale[0]
        if t in (1, 16, 64, 256):
            rho = np.sqrt(1 - cmin)  # = sqrt(1 - 2/pi + slack)
            got = np.linalg.norm(total / t - y0) / np.linalg.norm(y0)
            print(f"T = {t}: error {got:.4f}, slack {2 / np.pi - cmin:.3f}, bound {rho / (1 - rho) / t:.4f}")
            assert got <= rho / (1 - rho) / t
            assert abs(got - np.linalg.norm(e64) / t / np.linalg.norm(y0)) < 1e-3  # the f32 path follows the f64 one


def test_two_ranks_on_cpu_fabric():
    n, n_pad, seed = 17461, 20480, 5
    gs = [inputs(kind, n_pad, 20 + r) for r, kind in enumerate(("normal", "student"))]
    want_g, want_e, wires = O.step(gs, [np.zeros(5 * B, np.float32)] * 2, n, seed)

    def rank_fn(transport):
        b = SimpleNamespace(n=n, grad=torch.from_numpy(gs[transport.rank].copy()))
        red = RotatedSignReducer(transport, seed=seed)
        red.reduce(b)
        assert red.wire_bytes(b) == 5 * 512 + 4 * 8 == wires[0][0].size + 4 * wires[0][1].size
        return b.grad.numpy().view(np.uint32), red.state_for(b).e.numpy().view(np.uint32)

    (ga, ea), (gb, eb) = ThreadFabric(2).run(rank_fn)
    assert np.array_equal(ga[:n], gb[:n]) and np.array_equal(ga[:n], want_g[:n].view(np.uint32))
    assert np.array_equal(ea, want_e[0].view(np.uint32)) and np.array_equal(eb, want_e[1].view(np.uint32))
    assert np.array_equal(ga[n:], gs[0][n:].view(np.uint32)) and np.array_equal(gb[n:], gs[1][n:].view(np.uint32))


def test_refusals():
    from fpga_ai_nic_amd.cli.mlp_mpi import build_parser
    from fpga_ai_nic_amd.config import config_from_args
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer, make_engine
    from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
    from fpga_ai_nic_amd.parallel.sketch import SketchReducer
    from fpga_ai_nic_amd.parallel.sparse import TopKReducer

    for kw, what in ((dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(seed=0.5), "seed"),
                     (dict(transport=SimpleNamespace(world=17)), "at most 16")):
        with pytest.raises(ValueError, match=what):
            RotatedSignReducer(kw.pop("transport", None), **kw)
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt)  # noqa: E731
    g, wire = z(8192), z(RH.layout(8192, 4097)[2], torch.uint8)
    # not f32; not contiguous; e, wire of the wrong length; n_pad % 4; n outside 1 .. n_pad; the seed; a shared plane
    for args in ((z(8192, torch.float64), z(8192), wire, 4097, 0), (z(16384)[::2], z(8192), wire, 4097, 0),
                 (g, z(4096), wire, 4097, 0), (g, z(8192), wire[:-4], 4097, 0), (z(8190), z(8192), wire, 4097, 0),
                 (g, z(8192), wire, 8193, 0), (g, z(8192), wire, 0, 0), (g, z(8192), wire, 4097, 1 << 64),
                 (g, g, wire, 4097, 0)):
        with pytest.raises(ValueError, match="rht"):
            RH.encode(*args)
    for what, call in (("max_blocks", lambda: RH.encode(g, z(8192), wire, 4097, 0, max_blocks=0)),
                       ("world", lambda: RH.decode(wire, 17, g, 4097, 0)),
                       ("wires", lambda: RH.decode(wire, 2, g, 4097, 0)),
                       ("inverse", lambda: RH.transform(z(4100), 0, inverse=True))):
        with pytest.raises(ValueError, match=what):
            call()
    model = MLP([32, 48, 16], dtype=torch.float32, device="cpu")
    eng = make_engine(ThreadFabric(1).transport(0), "bfp", device="cpu")
    for kw in (dict(engine=eng), dict(error_feedback=True), dict(stochastic_rounding=True),
               dict(lowrank=LowRankReducer(None, 4)), dict(topk=TopKReducer(None, 0.1)),
               dict(sketch=SketchReducer(None, 0.1, cols=1024))):
        with pytest.raises(ValueError, match="rotated"):
            DataParallelTrainer(model, kw.pop("engine", None), rotated=RotatedSignReducer(None), **kw)
    for argv in (["--compress", "drive", "--error-feedback"], ["--compress", "drive", "--stochastic-rounding"],
                 ["--compress", "drive", "--drive-seed", "-1"], ["--compress", "topk", "--drive-seed", "3"],
                 ["--drive-seed", "3"]):
        with pytest.raises(ValueError, match="drive"):
            config_from_args(build_parser().parse_args(["1", "32"] + argv))
    cfg = config_from_args(build_parser().parse_args(["1", "32", "--compress", "drive", "--drive-seed", "7"]))
    assert (cfg.compress, cfg.drive_seed) == ("drive", 7)
