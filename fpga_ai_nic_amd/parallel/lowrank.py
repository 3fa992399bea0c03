"""PowerSGD low-rank gradient reduction (``ops/lowrank_oracle.py`` is the definition): a layer's rows x cols gradient
crosses the transport as rows x r plus cols x r f32 numbers, summed by two plain all-reduces (the wire is linear), and
comes back as the rank-averaged rank-r approximation in the layer's own f32 gradient plane — what the engine-less
update of :class:`~fpga_ai_nic_amd.parallel.dp.DataParallelTrainer` already consumes as ``raw_f32``. What the
approximation drops stays in a per-rank residual plane and is added to the next step's gradient; Q is warm-started
from the previous step. The two all-reduces are synchronous on the transport (no overlap with the backward)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import lowrank as LR
from .transport import Transport


@dataclass
class LowRankState:
    rows: int
    cols: int
    e: torch.Tensor     # residual plane, rows * cols
    q: torch.Tensor     # [cols][16], columns >= rank zero
    p: torch.Tensor     # [rows][16] scratch: P, then P^
    qn: torch.Tensor    # [cols][16] scratch
    part: torch.Tensor  # strip partials of both products


class LowRankReducer:
    def __init__(self, transport: Transport | None, rank: int, seed: int = 0, orth: str = "mgs"):
        """``transport=None``: one rank, no collective. ``rank``: 1..16. ``seed``: of every bucket's initial Q (bucket
        number b, in the order of first use, draws from ``seed + b``): the same on every rank. ``orth``: ``"mgs"``
        (modified Gram-Schmidt, one workgroup) or ``"cholqr2"`` (CholeskyQR2 spread over 256-row strips; other bits)."""
        if orth not in ("mgs", "cholqr2"):
            raise ValueError(f"lowrank: unknown orth method {orth!r}; mgs or cholqr2")
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= LR.RANK_PAD:
            raise ValueError(f"lowrank: the rank must be an int in 1..{LR.RANK_PAD}, got {rank!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
            raise ValueError(f"lowrank: the seed must be a non-negative int, got {seed!r}")
        self.transport = transport
        self.world = transport.world if transport is not None else 1
        self.rank, self.seed, self.orth = rank, seed, orth
        self.inv = float(np.float32(1.0) / np.float32(self.world))
        self._states: list[tuple[object, LowRankState]] = []  # (bucket, state), found by identity

    def state_for(self, bucket) -> LowRankState:
        """The bucket's E, Q and scratch, allocated on first use (E zeroed, Q from the seed)."""
        for b, st in self._states:
            if b is bucket:
                return st
        rows, cols = bucket.cin, bucket.cout
        LR.O.check_shape(rows, cols, self.rank)
        g = bucket.grad
        if not (g.dtype == torch.float32 and g.is_contiguous() and g.numel() >= bucket.n >= rows * cols):
            raise ValueError("lowrank: the bucket's gradient must be a contiguous float32 plane of at least n elements")
        dev = g.device
        q = torch.from_numpy(LR.O.init_q(cols, self.rank, self.seed + len(self._states))).to(dev)
        n_part = LR.layout(rows, cols)[2]
        if self.orth == "cholqr2":  # two 16 x 16 fp64 Gram matrices per strip: more than the products need only
            n_part = max(n_part, 4 * -(-rows // LR.O.ORTH_STRIP) * 256)  # where a strip is mostly empty
        st = LowRankState(rows, cols, torch.zeros(rows * cols, dtype=torch.float32, device=dev), q,
                          torch.zeros(rows, LR.RANK_PAD, dtype=torch.float32, device=dev),
                          torch.zeros(cols, LR.RANK_PAD, dtype=torch.float32, device=dev),
                          torch.zeros(n_part, dtype=torch.float32, device=dev))
        self._states.append((bucket, st))
        return st

    def _all_reduce(self, t: torch.Tensor):
        """Sum the first ``rank`` columns of t[*][16] over the ranks (the others are zero on every rank)."""
        if self.world == 1:
            return
        if self.rank == LR.RANK_PAD:
            self.transport.all_reduce_(t)
            return
        w = t[:, : self.rank].contiguous()
        self.transport.all_reduce_(w)
        t[:, : self.rank].copy_(w)

    def reduce(self, bucket) -> None:
        """One reduction of the bucket's gradient in place, on the current stream; collective over the transport."""
        st = self.state_for(bucket)
        rows, cols, g = st.rows, st.cols, bucket.grad
        LR.project(g, st.e, st.q, st.part, st.p, rows, cols)
        self._all_reduce(st.p)
        LR.orth(st.p, self.rank, self.orth, st.part)
        LR.backproject(g, st.e, st.p, st.part, st.qn, rows, cols)
        self._all_reduce(st.qn)
        LR.reconstruct(g, st.e, st.p, st.qn, st.q, self.inv, rows, cols)
        if bucket.n > rows * cols:  # the tail (the bias) is not compressed
            tail = g[rows * cols: bucket.n]
            if self.world > 1:
                self.transport.all_reduce_(tail)
                tail.mul_(self.inv)

    def wire_bytes(self, bucket) -> int:
        """Bytes one rank contributes to the all-reduces of one reduction (0 with one rank)."""
        if self.world == 1:
            return 0
        return 4 * ((bucket.cin + bucket.cout) * self.rank + bucket.n - bucket.cin * bucket.cout)
