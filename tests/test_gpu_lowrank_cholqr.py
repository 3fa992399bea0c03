"""CholeskyQR2 orthogonalisation on the GPU (lowrank_gram_kernel, lowrank_cholqr_apply_kernel) against the NumPy oracle
and the fp64 measures of tests/test_lowrank_cholqr_cpu.py, on its inputs (idle waves, a 16-row last strip, 5 strips)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.ops import lowrank as LR
from fpga_ai_nic_amd.ops import lowrank_oracle as O
from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer
from fpga_ai_nic_amd.parallel.transport import ThreadFabric
from test_lowrank_cholqr_cpu import CASES, U, check_against, inputs, measures, twin

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def gpu_orth(p, rank):
    part = torch.full((4 * -(-p.shape[0] // O.ORTH_STRIP) * 256,), float("nan"), device=DEV)  # (written before read)
    return LR.orth(torch.tensor(p, device=DEV), rank, method="cholqr2", part=part).cpu().numpy()


@pytest.mark.parametrize("rows,rank,fam", CASES)
def test_orth_cholqr2(rows, rank, fam):
    """Per element against the oracle. With A1 = P, A2 = the oracle's first-pass result and Rinv1, Rinv2 its factors,
    the two differ by (1) the order of each 16-term f32 sum, gamma_16 sum_k |A||Rinv|; (2) a last bit of Rinv (the
    fp64 Gram sums inside a strip are ordered differently, which can move its one rounding to f32), 2^-24 of the same
    sum: 17 * 2^-24 together; (3) the first pass's difference carried through the second, (|A1||Rinv1|)|Rinv2|, and
    through the second Gram matrix into Rinv2: the factor 4. Measured on an MI355X: at most 9.7e-08, 0.06 of the bound,
    33 of the 45 cases bit-identical. The fp64 measures: at most 4x the f32 oracle's own, floored alike."""
    p, dead = inputs(rows, rank, fam)
    out1, rinv1, a1 = O.cholqr_pass(p, rank)
    ref, rinv2, a2 = O.cholqr_pass(out1, rank)
    got = gpu_orth(p, rank)
    absd = lambda x: np.abs(x.astype(np.float64))  # noqa: E731
    err, bound = absd(got.astype(np.float64) - ref), 4 * 17 * U * (absd(a2) + absd(a1) @ absd(rinv1)) @ absd(rinv2)
    print(f"{rows} r{rank} {fam}: max |gpu - oracle| {err.max():.3e}, of the bound {np.max(err / (bound + 1e-300)):.3f}")
    assert (err <= bound).all() and not got[:, rank:].any() and (dead is None or not got[:, dead].any())
    check_against(measures(got, p, rank, dead), measures(ref, p, rank, dead), f"gpu {rows} r{rank} {fam}")
    if fam in "bd":  # (bit for bit the result of the well-conditioned twin, as in the oracle)
        assert np.array_equal(got, gpu_orth(twin(rows, rank, fam), rank))


def test_reducer_two_ranks():
    """The two-rank scenario of tests/test_gpu_lowrank.py through orth="cholqr2": bit-identical replicas, the error against
    the fp64 run of the same method at most 4x the f32 oracle's (7.8e-07 against 7.2e-07); orth="mgs" is the default."""
    rows, cols, r = 80, 528, 4
    rng = np.random.default_rng(11)
    eighths = lambda *shape: np.round(rng.standard_normal(shape) * 8) / 8  # noqa: E731
    m, n = (eighths(rows, r) @ eighths(r, cols)).astype(np.float32), eighths(rows, cols).astype(np.float32)
    gs, zeros = [m + n, m - n], [np.zeros((rows, cols), np.float32)] * 2
    g32, g64 = (O.step(gs, zeros, O.init_q(cols, r, 0), r, dtype=dt, orth_fn=O.orth_cholqr2)[0]
                for dt in (np.float32, np.float64))

    def rank_fn(transport):
        outs = []
        for kw in (dict(orth="cholqr2"), dict(orth="mgs"), dict()):
            b = SimpleNamespace(cin=rows, cout=cols, n=rows * cols, grad=torch.tensor(gs[transport.rank], device=DEV).view(-1))
            red = LowRankReducer(transport, r, seed=0, **kw)
            red.reduce(b)
            outs.append(torch.cat([b.grad, red.state_for(b).q.view(-1)]).cpu())
        return outs

    ra, rb = ThreadFabric(2).run(rank_fn)
    assert all(torch.equal(a, b) for a, b in zip(ra, rb)) and torch.equal(ra[1], ra[2]) and not torch.equal(ra[0], ra[1])
    got, fro = ra[0][: rows * cols].view(rows, cols).numpy().astype(np.float64), np.linalg.norm
    err, ref_err = fro(got - g64) / fro(g64), fro(g32 - g64) / fro(g64)
    print(f"cholqr2 reducer: GPU rel. Frobenius error {err:.3e}, f32 oracle {ref_err:.3e}")
    assert err <= 4 * ref_err


def test_refused():
    for match, part in (("part", None), ("elements", torch.zeros(2047, device=DEV)), ("lives on", torch.zeros(2048))):
        with pytest.raises(ValueError, match=match):
            LR.orth(torch.zeros(272, 16, device=DEV), 4, method="cholqr2", part=part)
