"""Count-sketch gradient compression (``ops/sketch_oracle.py`` is the definition; Ivkin et al., NeurIPS 2019, two
rounds): each rank sketches gradient + residual into ``rows x cols`` f32, one ``all_reduce_`` sums the sketches, every
rank recovers the same k indices from the same summed sketch, a second ``all_reduce_`` sums the exact values at those
indices, and the bucket's own f32 gradient plane becomes their rank mean — what the engine-less update of
:class:`~fpga_ai_nic_amd.parallel.dp.DataParallelTrainer` already consumes as ``raw_f32``. What is not sent stays in the
rank's residual plane. Both all-reduces are synchronous on the transport (no overlap with the backward); their bytes
do not depend on the world size."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import sketch as SK
from ..ops import topk as TK
from .transport import Transport


@dataclass
class SketchState:
    n_pad: int
    n: int
    k: int
    e: torch.Tensor        # residual plane, n_pad f32
    S: torch.Tensor        # the sketch, rows * cols f32
    part: torch.Tensor     # the accumulate's per-strip slabs
    wire: torch.Tensor     # the agreed indices and their values, 8 * k_pad bytes
    scratch: torch.Tensor  # the select's histogram, state words and per-tile counts


class SketchReducer:
    def __init__(self, transport: Transport | None, density: float, rows: int = 5, cols: int = 65536, seed: int = 0):
        """``transport=None``: one rank, no collective. ``density``: in (0, 1]; a bucket of n valid elements recovers
        ``k = max(1, min(n, int(n * density)))`` components. ``rows``: 1, 3 or 5; ``cols``: a multiple of 1024 in
        1024 .. 2^22; ``seed``: of the hashes, in [0, 2^64), the same on every rank."""
        TK.count(1, density)  # (refuses a density outside (0, 1])
        SK.O.check_params(rows, cols, seed)
        self.transport = transport
        self.world = transport.world if transport is not None else 1
        self.density, self.rows, self.cols, self.seed = float(density), rows, cols, int(seed)
        self.inv = float(np.float32(1.0) / np.float32(self.world))
        self._states: list[tuple[object, SketchState]] = []  # (bucket, state), found by identity

    def state_for(self, bucket) -> SketchState:
        """The bucket's residual, sketch, wire and scratch, allocated on first use (the residual zeroed)."""
        for b, st in self._states:
            if b is bucket:
                return st
        g = bucket.grad
        if not (isinstance(g, torch.Tensor) and g.dtype == torch.float32 and g.is_contiguous()):
            raise ValueError("sketch: the bucket's gradient must be a contiguous float32 plane")
        n_pad, n = g.numel(), bucket.n
        k = TK.count(n, self.density)
        TK.O.check_shape(n_pad, n, k)
        sk, part, words, nbytes = SK.layout(n_pad, k, self.rows, self.cols)
        z = lambda m, dt: torch.zeros(m, dtype=dt, device=g.device)  # noqa: E731
        st = SketchState(n_pad, n, k, z(n_pad, torch.float32), z(sk, torch.float32), z(part, torch.float32),
                         z(nbytes, torch.uint8), z(words, torch.int32))
        self._states.append((bucket, st))
        return st

    def reduce(self, bucket) -> None:
        """One reduction of the bucket's gradient in place, on the current stream; collective over the transport."""
        st = self.state_for(bucket)
        g = bucket.grad
        SK.sketch(g, st.e, st.S, st.part, st.n, self.rows, self.cols, self.seed)
        if self.world > 1:
            self.transport.all_reduce_(st.S)
        SK.estimate_select(g, st.e, st.S, st.wire, st.scratch, st.n, st.k, self.rows, self.cols, self.seed)
        val = SK.fetch(st.e, st.wire, st.n, st.k)
        if self.world > 1:
            self.transport.all_reduce_(val)
        TK.accumulate(st.wire, 1, g, st.n, st.k, self.inv)

    def wire_bytes(self, bucket) -> int:
        """Bytes one rank contributes to the two all-reduces of one reduction (0 with one rank)."""
        if self.world == 1:
            return 0
        return 4 * (self.rows * self.cols + TK.k_pad(self.state_for(bucket).k))
