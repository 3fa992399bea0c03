"""Top-k gradient sparsification with memory (``ops/topk_oracle.py`` is the definition): each rank sends the k
largest-magnitude components of gradient + residual as ``[u32 idx[k_pad]][f32 val[k_pad]]``, one ``all_gather`` per
bucket moves the wires, and every rank adds them in rank order into the bucket's own f32 gradient plane — the rank mean
of the sparse contributions, what the engine-less update of
:class:`~fpga_ai_nic_amd.parallel.dp.DataParallelTrainer` already consumes as ``raw_f32``. What a rank does not send
stays in its residual plane and is added to the next step's gradient. The all-gather is synchronous on the transport
(no overlap with the backward); its received bytes grow with the world size, unlike an all-reduce's."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import topk as TK
from .transport import Transport


@dataclass
class TopKState:
    n_pad: int
    n: int
    k: int
    e: torch.Tensor        # residual plane, n_pad f32
    wire: torch.Tensor     # this rank's wire, 8 * k_pad bytes
    wires: torch.Tensor    # every rank's wire in rank order (the wire itself with one rank)
    scratch: torch.Tensor  # the select's histogram, state words and per-tile counts


class TopKReducer:
    def __init__(self, transport: Transport | None, density: float):
        """``transport=None``: one rank, no collective. ``density``: in (0, 1]; a bucket of n valid elements sends
        ``k = max(1, min(n, int(n * density)))``."""
        TK.count(1, density)  # (refuses a density outside (0, 1])
        self.transport = transport
        self.world = transport.world if transport is not None else 1
        if self.world > TK.MAX_WORLD:
            raise ValueError(f"topk: at most {TK.MAX_WORLD} ranks, got {self.world}")
        self.density = float(density)
        self.inv = float(np.float32(1.0) / np.float32(self.world))
        self._states: list[tuple[object, TopKState]] = []  # (bucket, state), found by identity

    def state_for(self, bucket) -> TopKState:
        """The bucket's residual, wires and scratch, allocated on first use (the residual zeroed)."""
        for b, st in self._states:
            if b is bucket:
                return st
        g = bucket.grad
        if not (isinstance(g, torch.Tensor) and g.dtype == torch.float32 and g.is_contiguous()):
            raise ValueError("topk: the bucket's gradient must be a contiguous float32 plane")
        n_pad, n = g.numel(), bucket.n
        k = TK.count(n, self.density)
        TK.O.check_shape(n_pad, n, k)
        _, words, nbytes = TK.layout(n_pad, k)
        dev = g.device
        wire = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        wires = wire if self.world == 1 else torch.zeros(self.world * nbytes, dtype=torch.uint8, device=dev)
        st = TopKState(n_pad, n, k, torch.zeros(n_pad, dtype=torch.float32, device=dev), wire, wires,
                       torch.zeros(words, dtype=torch.int32, device=dev))
        self._states.append((bucket, st))
        return st

    def reduce(self, bucket) -> None:
        """One reduction of the bucket's gradient in place, on the current stream; collective over the transport."""
        st = self.state_for(bucket)
        g = bucket.grad
        TK.select(g, st.e, st.wire, st.scratch, st.n, st.k)
        if self.world > 1:
            self.transport.all_gather(st.wire, st.wires)
        TK.accumulate(st.wires, self.world, g, st.n, st.k, self.inv)

    def wire_bytes(self, bucket) -> int:
        """Bytes one rank sends in one reduction (0 with one rank); it receives ``world - 1`` times as many."""
        return 0 if self.world == 1 else int(self.state_for(bucket).wire.numel())
