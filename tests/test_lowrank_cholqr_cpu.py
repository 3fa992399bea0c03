"""CholeskyQR2 orthogonalisation (ops/lowrank_oracle.py: orth_cholqr2) on the CPU, measured in fp64 against the
modified Gram-Schmidt oracle on the same inputs. tests/test_gpu_lowrank_cholqr.py reuses the inputs and the measures."""
import argparse

import numpy as np
import pytest
import torch

from fpga_ai_nic_amd.config import add_named_flags, config_from_args
from fpga_ai_nic_amd.ops import lowrank as LR
from fpga_ai_nic_amd.ops import lowrank_oracle as O
from fpga_ai_nic_amd.parallel.lowrank import LowRankReducer

U, FLOOR = 2.0 ** -24, 32 * 2.0 ** -24
# rows: one k-step group; a 16-row last strip; 5 strips (more than a workgroup has waves). Families: a normal entries,
# b columns scaled 2^-20 .. 2^20, c one exactly zero column, d one column an exact copy of column 0 (not at rank 1)
CASES = [(m, r, f) for m in (16, 272, 1040) for r in (1, 3, 4, 16) for f in "abcd" if not (f == "d" and r == 1)]


def inputs(rows, rank, fam):
    """(P[rows][16] f32 with zero columns >= rank, the index of its dead column or None)."""
    p = np.zeros((rows, 16), np.float32)
    p[:, :rank] = np.random.default_rng(rows * 31 + rank).standard_normal((rows, rank)).astype(np.float32)
    dead = {"c": rank // 2, "d": max(1, rank // 2)}.get(fam)
    if fam == "b":
        p[:, :rank] *= np.float32(2.0) ** np.round(np.linspace(-20, 20, rank)).astype(np.float32)
    elif fam in "cd":
        p[:, dead] = p[:, 0] if fam == "d" else 0
    return p, dead


def measures(ph, p, rank, dead):
    """fp64 measures of P^ = orth(P): (orthonormality defect over the live columns; without a dead column also the
    largest below-diagonal entry of P^^T P over ||P_k|| and the distance to the sign-fixed np.linalg.qr of P)."""
    live = [j for j in range(rank) if j != dead]
    h, a = ph[:, live].astype(np.float64), p[:, live].astype(np.float64)
    defect = np.abs(h.T @ h - np.eye(len(live))).max(initial=0.0)  # (rank 1 with its column dead: nothing live)
    if dead is not None:
        return (defect,)
    r, (q, rr) = h.T @ a, np.linalg.qr(a)
    assert (np.diagonal(r) > 0).all()
    return (defect, np.abs(np.tril(r, -1) / np.linalg.norm(a, axis=0)[None, :]).max(),
            np.abs(h - q * np.sign(np.diagonal(rr))[None, :]).max())


def check_against(got, ref, what):
    """At most 4x the yardstick's, floored at 32 * 2^-24 (where the yardstick is exact, as at rank 1, no ratio holds)."""
    print(what, " ".join(f"{g:.3e} (yardstick {r:.3e})" for g, r in zip(got, ref)))
    assert all(g <= max(4 * r, FLOOR) for g, r in zip(got, ref))


def twin(rows, rank, fam):
    """The input whose result (b) or (d) reproduces bit for bit: a power-of-two column scale passes exactly through W,
    s, Rinv and the apply (a's result); the copy dies at its pivot and reaches no other column (that column zeroed).
    No ratio check there: Gram-Schmidt's own defect is 5e-3 on (b) (1e-8 beside a norm of 4e-6), up to 0.2 on (d)."""
    p, dead = inputs(rows, rank, fam)
    return inputs(rows, rank, "a")[0] if fam == "b" else np.where(np.arange(16) == dead, np.float32(0), p)


@pytest.mark.parametrize("rows,rank,fam", CASES)
def test_orth_cholqr2(rows, rank, fam):
    p, dead = inputs(rows, rank, fam)
    ph = O.orth_cholqr2(p, rank)
    assert ph.dtype == np.float32 and not ph[:, rank:].any() and (dead is None or not ph[:, dead].any())
    if fam in "bd":
        assert np.array_equal(ph, O.orth_cholqr2(twin(rows, rank, fam), rank))
    else:
        check_against(measures(ph, p, rank, dead), measures(O.orth(p, rank), p, rank, dead), f"{rows} r{rank} {fam}")
    assert measures(O.orth_cholqr2(p.astype(np.float64), rank), p, rank, dead)[0] <= 2.0 ** -40  # (the same in double)


def test_method_plumbing():
    p = inputs(272, 4, "a")[0]
    assert np.array_equal(LR.orth(torch.tensor(p), 4, method="cholqr2").numpy(), O.orth_cholqr2(p, 4))
    assert np.array_equal(LR.orth(torch.tensor(p), 4).numpy(), O.orth(p, 4))
    for bad in (lambda: LR.orth(torch.tensor(p), 4, method="qr"), lambda: LowRankReducer(None, 4, orth="qr")):
        with pytest.raises(ValueError, match="orth"):
            bad()
    cli = lambda *a: config_from_args(add_named_flags(argparse.ArgumentParser()).parse_args(a))  # noqa: E731
    assert [cli("--compress", "powersgd", *f).lowrank_orth for f in ((), ("--lowrank-orth", "cholqr2"))] == ["mgs", "cholqr2"]
    with pytest.raises(ValueError, match="powersgd"):
        cli("--lowrank-orth", "cholqr2")
