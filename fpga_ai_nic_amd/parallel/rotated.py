"""Rotated one-bit gradient compression (``ops/rht_oracle.py`` is the definition; DRIVE, Vargaftik et al., NeurIPS
2021): each rank rotates its gradient by a randomised Hadamard transform in blocks of 4096, adds its residual (kept in
rotated coordinates), and sends one sign bit per value and one f32 scale per block; one ``all_gather`` per bucket moves
the wires, and every rank adds them in rank order, rotates back and writes the rank mean into the bucket's own f32
gradient plane — what the engine-less update of :class:`~fpga_ai_nic_amd.parallel.dp.DataParallelTrainer` already
consumes as ``raw_f32``. The all-gather is synchronous on the transport (no overlap with the backward); its received
bytes grow with the world size."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import rht as RH
from .transport import Transport


@dataclass
class RotatedState:
    n_pad: int
    n: int
    e: torch.Tensor      # residual plane in rotated coordinates, blocks * 4096 f32
    wire: torch.Tensor   # this rank's wire
    wires: torch.Tensor  # every rank's wire in rank order (the wire itself with one rank)


class RotatedSignReducer:
    def __init__(self, transport: Transport | None, seed: int = 0):
        """``transport=None``: one rank, no collective. ``seed``: of the rotation's signs, in [0, 2^64), the same on
        every rank and fixed for the reducer's lifetime (the residuals live in the rotated coordinates it defines)."""
        self.seed = RH.O.check_seed(seed)
        self.transport = transport
        self.world = transport.world if transport is not None else 1
        if self.world > RH.MAX_WORLD:
            raise ValueError(f"rht: at most {RH.MAX_WORLD} ranks, got {self.world}")
        self._states: list[tuple[object, RotatedState]] = []  # (bucket, state), found by identity

    def state_for(self, bucket) -> RotatedState:
        """The bucket's residual and wires, allocated on first use (the residual zeroed)."""
        for b, st in self._states:
            if b is bucket:
                return st
        g = bucket.grad
        if not (isinstance(g, torch.Tensor) and g.dtype == torch.float32 and g.is_contiguous()):
            raise ValueError("rht: the bucket's gradient must be a contiguous float32 plane")
        n_pad, n = g.numel(), bucket.n
        _, rot, nbytes = RH.layout(n_pad, n)
        wire = torch.zeros(nbytes, dtype=torch.uint8, device=g.device)
        wires = wire if self.world == 1 else torch.zeros(self.world * nbytes, dtype=torch.uint8, device=g.device)
        st = RotatedState(n_pad, n, torch.zeros(rot, dtype=torch.float32, device=g.device), wire, wires)
        self._states.append((bucket, st))
        return st

    def reduce(self, bucket) -> None:
        """One reduction of the bucket's gradient in place, on the current stream; collective over the transport."""
        st = self.state_for(bucket)
        RH.encode(bucket.grad, st.e, st.wire, st.n, self.seed)
        if self.world > 1:
            self.transport.all_gather(st.wire, st.wires)
        RH.decode(st.wires, self.world, bucket.grad, st.n, self.seed)

    def wire_bytes(self, bucket) -> int:
        """Bytes one rank sends in one reduction (0 with one rank); it receives ``world - 1`` times as many."""
        return 0 if self.world == 1 else int(self.state_for(bucket).wire.numel())
