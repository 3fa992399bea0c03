"""The kernels of csrc/rht/rht_kernels.hip against the NumPy oracle: bit for bit where every f32 sum is exact, within
the transform's rounding bound otherwise; the two-rank reducer and one trainer step."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import rht as RH
from fpga_ai_nic_amd.ops import rht_oracle as O
from fpga_ai_nic_amd.parallel.rotated import RotatedSignReducer
from fpga_ai_nic_amd.parallel.transport import ThreadFabric

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEED = 0xD21E_0000_0000_0001
B, U = O.B, 2.0 ** -24
SHAPES = [(4096, 4096), (4096, 1000), (8192, 4097), (20480, 17461)]
WORLDS = [1, 2, 3, 16]
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)  # noqa: E731


@lru_cache(maxsize=None)
def plane(kind, n_pad, n, seed=0):
    """Eighths in [-7/8, 7/8] ("grid": every sum is exact), normal or Student-t values; past n a huge canary."""
    rng = np.random.default_rng(n + len(kind) + seed)
    g = {"grid": lambda: rng.integers(-7, 8, n_pad) / 8, "normal": lambda: rng.standard_normal(n_pad),
         "student": lambda: rng.standard_t(2, n_pad)}[kind]().astype(np.float32)
    g[n:] = 1e30
    g.setflags(write=False)
    return g


def blocksum(x, n):
    """sum|x[:n]| of each block, repeated over the block's 4096 elements, in float64."""
    p = np.zeros(-(-n // B) * B)
    p[:n] = np.abs(np.asarray(x[:n], dtype=np.float64))
    return np.repeat(p.reshape(-1, B).sum(axis=1), B)


@lru_cache(maxsize=None)
def wires_for(n, world, grid):
    """`world` ranks' (sign, scale) with random bits and scales on the grid of eighths or in [0.5, 1.5)."""
    rng, nb = np.random.default_rng(world), -(-n // B)
    return [(rng.integers(0, 256, 512 * nb).astype(np.uint8),
             np.pad(rng.integers(1, 8, nb) / 8 if grid else rng.random(nb) + 0.5, (0, -nb % 4)).astype(np.float32))
            for _ in range(world)]


def gpu_encode(g, e, n, max_blocks=None):
    nb, _, nbytes = RH.layout(g.size, n)
    gd, ed, wire = dev(g), dev(e), torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    RH.encode(gd, ed, wire, n, SEED, max_blocks=max_blocks)
    assert np.array_equal(bits(gd.cpu().numpy()), bits(g))
    w = wire.cpu().numpy()
    return w[: 512 * nb], w[512 * nb:].view(np.float32), ed.cpu().numpy(), wire


def gpu_decode(wires, g, n, max_blocks=None):
    flat = np.concatenate([np.concatenate([s, c.view(np.uint8)]) for s, c in wires])
    return RH.decode(dev(flat), len(wires), dev(g), n, SEED, max_blocks=max_blocks).cpu().numpy()


def check_grid(n_pad, n, max_blocks=None):
    g = plane("grid", n_pad, n)
    y = O.transform(g, SEED, n=n)
    assert blocksum(O.rht64(g, n, SEED).reshape(-1), y.size).max() < 2 ** 15
    yd = RH.transform(dev(g), SEED, n=n, max_blocks=max_blocks)
    assert np.array_equal(bits(yd.cpu().numpy()), bits(y))
    back = RH.transform(yd, SEED, inverse=True, n=n, max_blocks=max_blocks).cpu().numpy()
    assert np.array_equal(bits(back), bits(O.transform(y, SEED, inverse=True, n=n)))
    sign, scale, left, _ = gpu_encode(g, np.zeros(y.size, np.float32), n, max_blocks)
    for name, a, b in zip(("sign", "scale", "e"), (sign, scale, left), O.encode(g, np.zeros(y.size, np.float32), n, SEED)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert n < B or (y == 0).any()  # exact zeros: bit 0, which the sign plane above has checked
    for world in WORLDS:
        w = wires_for(n, world, True)
        assert np.array_equal(bits(gpu_decode(w, g, n, max_blocks)), bits(O.decode(w, g, n, SEED))), world


@pytest.mark.parametrize("n_pad,n,max_blocks", [s + (None,) for s in SHAPES] + [SHAPES[3] + (1,)])
def test_grid_bit_exact(n_pad, n, max_blocks):
    check_grid(n_pad, n, max_blocks)


@pytest.mark.parametrize("kind", ["normal", "student"])
@pytest.mark.parametrize("n_pad,n", SHAPES)
def test_rounding_bounds(n_pad, n, kind):
    """50 * 2^-24 * sum_block|x| / 64 per element of the transform (three rounds of 16-term +-1 dot products, one scale,
    one rounding); 4098 * 2^-24 relative on the scale; a sign bit may differ only inside the transform bound of y."""
    g = plane(kind, n_pad, n)
    y64 = O.rht64(g, n, SEED).reshape(-1)
    tb = 50 * U * blocksum(g, n) / 64
    yd = RH.transform(dev(g), SEED, n=n)
    assert (np.abs(yd.cpu().numpy() - y64) <= tb).all()
    y32 = y64.astype(np.float32)
    back = RH.transform(dev(y32), SEED, inverse=True, n=n).cpu().numpy()
    assert (np.abs(back - O.irht64(y32, SEED)[:n]) <= (50 * U * blocksum(y32, y32.size) / 64)[:n]).all()
    e = np.zeros(y64.size, np.float32)
    for step in range(2):  # the second step starts from the kernel's own non-zero e'
        want_sign, want_scale, _ = O.encode(g, e, n, SEED)
        yref = O.transform(g, SEED, n=n).astype(np.float64) + e
        ytol = tb + 2 * U * np.abs(yref)  # (the f32 add of e)
        near = (np.abs(yref) < ytol).reshape(-1, B).sum(axis=1)
        assert near.max() < B / 1000, "the input itself must stay under the cap"
        sign, scale, left, _ = gpu_encode(g, e, n)
        nb = near.size
        assert (np.abs(scale[:nb] - want_scale[:nb]) <= 4098 * U * want_scale[:nb]).all() and not scale[nb:].any()
        bit, want_bit = (np.unpackbits(s, bitorder="little") != 0 for s in (sign, want_sign))
        assert (np.abs(yref[bit != want_bit]) < ytol[bit != want_bit]).all()
        s_rep = np.repeat(want_scale[:nb].astype(np.float64), B)
        want_left = yref - np.where(bit, -s_rep, s_rep)
        assert (np.abs(left - want_left) <= ytol + 4098 * U * s_rep + 2 * U * np.abs(want_left)).all(), step
        e = left
    for world in WORLDS:
        w = wires_for(n, world, False)
        acc = sum(np.where(np.unpackbits(s, bitorder="little") != 0, -1.0, 1.0) * np.repeat(c[:nb].astype(np.float64), B)
                  for s, c in w)  # (any f32 order of this sum is within world * 2^-24 * sum|acc| of it after H / 64)
        want = O.irht64(acc.astype(np.float32), SEED)[:n] * float(np.float32(1.0) / np.float32(world))
        got = gpu_decode(w, g, n)
        tol = (50 + world) * U * blocksum(acc, acc.size)[:n] / 64
        assert (np.abs(got[:n] - want) <= tol).all() and np.array_equal(bits(got[n:]), bits(g[n:])), world


def test_non_finite_block():
    """NaN, Inf, -0.0 and a denormal in block 1: a NaN scale and an all-NaN decode for that block only."""
    n_pad, n = SHAPES[3]
    clean = plane("normal", n_pad, n)
    g = clean.copy()
    g[[4100, 5000, 6000, 8191]] = np.nan, np.inf, -0.0, 1e-40
    z = np.zeros(5 * B, np.float32)
    (sa, ca, ea, _), (sb, cb, eb, wire) = gpu_encode(clean, z, n), gpu_encode(g, z, n)
    other = np.arange(5) != 1
    assert np.isnan(cb[1]) and np.isnan(eb[B:2 * B]).all() and np.array_equal(bits(ca[:5][other]), bits(cb[:5][other]))
    assert np.array_equal(sa.reshape(5, 512)[other], sb.reshape(5, 512)[other])
    assert np.array_equal(bits(ea).reshape(5, B)[other], bits(eb).reshape(5, B)[other])
    ga, gb = (gpu_decode([(s, c)], clean, n) for s, c in ((sa, ca), (sb, cb)))
    assert np.isnan(gb[B:2 * B]).all() and np.array_equal(bits(gb[2 * B:]), bits(ga[2 * B:]))
    assert np.array_equal(bits(gb[:B]), bits(ga[:B])) and np.array_equal(bits(gb[n:]), bits(clean[n:]))


def test_reducer_two_ranks():
    """Grid inputs: exact residuals; the scales are means, off the grid: the decode bound, |acc| <= s_0 + s_1."""
    n_pad, n = SHAPES[3]
    gs = [plane("grid", n_pad, n, r) for r in range(2)]
    want_g, want_e, wires = O.step(gs, [np.zeros(5 * B, np.float32)] * 2, n, SEED)
    tol = 52 * U * 64 * np.repeat(wires[0][1][:5].astype(np.float64) + wires[1][1][:5], B)[:n]

    def rank_fn(transport):
        b = SimpleNamespace(n=n, grad=dev(gs[transport.rank]))
        red = RotatedSignReducer(transport, seed=SEED)
        red.reduce(b)
        assert red.wire_bytes(b) == 5 * 512 + 4 * 8
        return bits(b.grad.cpu().numpy()), bits(red.state_for(b).e.cpu().numpy())

    (ga, ea), (gb, eb) = ThreadFabric(2).run(rank_fn)
    assert np.array_equal(ga[:n], gb[:n]) and (np.abs(ga[:n].view(np.float32) - want_g[:n]) <= tol).all()
    assert np.array_equal(ea, bits(want_e[0])) and np.array_equal(eb, bits(want_e[1]))
    assert np.array_equal(ga[n:], bits(gs[0][n:])) and np.array_equal(gb[n:], bits(gs[1][n:]))


def test_trainer_step():
    """One step of a 32-64-32 MLP: scale and residual within the bounds of the oracle's encode of the plain trainer's
    gradient, the grad within the decode bound of the kernel's own wire, the weights wire.sgd applied to that grad."""
    from fpga_ai_nic_amd.models.mlp import MLP
    from fpga_ai_nic_amd.ops import wire
    from fpga_ai_nic_amd.parallel.dp import DataParallelTrainer

    sizes, mb, lr = [32, 64, 32], 16, 0.05
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(mb, sizes[0], generator=gen) * 2 - 1).to(DEV, torch.bfloat16)
    y = torch.randint(0, sizes[-1], (mb,), generator=gen, dtype=torch.int32).to(DEV)
    plain, rotated = (MLP(sizes, dtype=torch.bfloat16, device=DEV, seed=3) for _ in range(2))
    w0 = [l.master.clone() for l in rotated.layers]
    DataParallelTrainer(plain, None, lr=0.0).step(x, y)
    red = RotatedSignReducer(None, seed=SEED)
    tr = DataParallelTrainer(rotated, None, lr=lr, rotated=red)
    tr.step(x, y)
    tr.finish()
    for l, ref, w, e in zip(rotated.layers, plain.layers, w0, tr.rotated_residuals):
        g0, nb = ref.grad.cpu().numpy(), -(-l.n // B)
        sent = red.state_for(l).wire.cpu().numpy()
        sign, scale = sent[: 512 * nb], sent[512 * nb:].view(np.float32)
        want_sign, want_scale, want_e = O.encode(g0, np.zeros(nb * B, np.float32), l.n, SEED)
        tb = 50 * U * blocksum(g0, l.n) / 64
        assert (np.abs(scale - want_scale) <= 4098 * U * want_scale).all() and bool(scale.any())
        same = np.unpackbits(sign, bitorder="little") == np.unpackbits(want_sign, bitorder="little")
        assert (~same).sum() < nb * B / 1000
        s_rep = np.repeat(want_scale[:nb].astype(np.float64), B)
        assert (np.abs(e.cpu().numpy() - want_e) <= tb + 4098 * U * s_rep + 4 * U * (np.abs(want_e) + 2 * s_rep))[same].all()
        got = l.grad.cpu().numpy()
        want = O.decode([(sign, scale)], g0, l.n, SEED)
        assert (np.abs(got - want)[: l.n] <= 51 * U * np.repeat(scale[:nb].astype(np.float64), B)[: l.n] * 64).all()
        wire.sgd(wire.as_bytes(dev(got)), l.n_pad, 1, w, codec="raw_f32", lr=lr, n_valid=l.n)
        assert torch.equal(l.master, w) and torch.equal(l.lp, l.master.to(torch.bfloat16))
