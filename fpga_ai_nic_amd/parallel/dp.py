"""Data-parallel trainer: per-layer gradient all-reduce overlapped with backward on a side HIP stream.

Reference schedule (sw/mlp_mpi_example_f32.cpp:701-787): forward all layers; softmax fwd/bwd; for layer
i = L-1..0: backward, then issue the NIC all-reduce(+SGD) of layer i asynchronously while layer i-1's
backward runs. MI355X mapping:

* main stream: fwd GEMMs (bias+ReLU fused), softmax-xent, bwd-weight GEMM of layer i, then bwd-data GEMM;
* comm stream (high priority): as soon as dW_i is written, the engine packs + exchanges layer i's bucket
  (overlapping the bwd-data GEMM of layer i and the whole backward of layers < i);
* the fused SGD epilogue of layer i waits (GPU-side event) for the bwd-data GEMM that still reads W_i;
* the NEXT step's forward of layer i waits (GPU-side event) for that epilogue — the host never blocks.
"""
from __future__ import annotations

import math
import os
import time

import torch

from ..models.mlp import MLP
from ..ops import gemm as G
from ..ops import gemm_tune, wire
from ..utils import tracing
from ..config import wire_codec
from .allreduce import (MAX_PEERS, NUM_SLOTS, OPTIMIZERS, CompressedAllReduce, Handle, _round_up,
                        resolve_betas)
from .transport import Transport


class RcclAllReduce(CompressedAllReduce):
    """Uncompressed baseline: transport all-reduce (RCCL ring/tree) + a separate SGD kernel
    (BASELINE config 2; the reference's commented MPI_Iallreduce path, sw:615-647)."""

    def __init__(self, transport: Transport, **kw):
        kw.pop("codec", None)
        kw.pop("algo", None)
        super().__init__(transport, codec="raw_f32", algo="mesh", **kw)
        self.algo = "rccl"

    def layout(self, n):
        from .allreduce import BucketLayout

        n_pad = _round_up(max(n, 1), 256 * self.world)
        return BucketLayout(n=n, n_pad=n_pad, algo="rccl", world=self.world, shard=n_pad)

    def wire_bytes(self, L):
        N = self.world
        return 0 if N == 1 else int(2 * (N - 1) / N * L.n_pad * 4)

    def _run(self, L, grad, finish, owner_fp32, allow_compat=True, residual=None, sr_seed=None):
        g = grad.view(-1)[: L.n_pad]
        self.transport.all_reduce_(g)
        return [lambda: finish(wire.as_bytes(g), L.n_pad, 1, 0, L.n_pad)]


def make_engine(transport: Transport | None, kind: str = "bfp", *, rounding: str = "rne", algo: str = "mesh",
                rings: int = 1, max_slice_elems: int = 1 << 22, compat_owner_fp32: bool = False,
                timeout_s: float = 600.0, force_comm: bool = False, impl: str = "python", comm=None,
                side_stream: bool = False, ring_sub: int = 0, shard_update: bool | None = None, device=None):
    """``device`` (Python engines): where the engine keeps its buffers; None: the current GPU when there is one. A
    CPU run on a machine that has a GPU must name it, or the engine's scratch lands on the GPU beside CPU gradients.
    kind: 'bfp' (compressed engine), 'bfp4' (the same with 4-bit mantissas, codec bfp4_rne: ``rounding`` must be 'rne'),
    'raw' (engine, uncompressed fp32 wire), 'rccl' (baseline),
    'local' (no communication: world 1). impl: 'python' (request path issued from Python over any
    transport) or 'native' (C++ engine over its own RCCL communicator, or over ``comm``, e.g. the direct P2P
    communicator of :func:`~fpga_ai_nic_amd.parallel.transport.make_p2p_comm`; GPU only)."""
    if kind == "local" or transport is None:
        return None
    if kind == "rccl":
        return RcclAllReduce(transport, timeout_s=timeout_s, force_comm=force_comm, device=device)
    codec = wire_codec(kind, rounding)
    if impl == "native":
        from .native_engine import NativeAllReduce

        return NativeAllReduce(transport, codec=codec, algo=algo, rings=rings, max_slice_elems=max_slice_elems,
                               compat_owner_fp32=compat_owner_fp32, timeout_s=timeout_s, force_comm=force_comm,
                               comm=comm, side_stream=side_stream, ring_sub=ring_sub, shard_update=shard_update)
    return CompressedAllReduce(transport, codec=codec, algo=algo, rings=rings, max_slice_elems=max_slice_elems,
                               compat_owner_fp32=compat_owner_fp32, timeout_s=timeout_s, force_comm=force_comm,
                               device=device)


class DataParallelTrainer:
    def __init__(self, model: MLP, engine: CompressedAllReduce | None, *, lr: float = 0.1,
                 weight_decay: float = 0.0, momentum: float = 0.0, nesterov: bool = False,
                 loss_scale: float = 1.0, average: bool = True, profile: bool = False, prepack: bool = True,
                 commit_at_end: bool | None = None, fused_update: bool | None = None,
                 gemm_inflight: str | None = None, wgrad_pair: bool | str | None = None, optimizer: str = "sgd",
                 betas=None, eps: float = 1e-8, trust_ratio: bool = False,
                 max_grad_norm: float | None = None, error_feedback: bool = False,
                 error_feedback_codec: str = "bfp_rne", stochastic_rounding: bool = False, sr_seed: int = 0,
                 moment_codec: str = "f32"):
        """``moment_codec``: 'f32' (the model's f32 moment planes) or 'bfp8' (AdamW only): both moments of every layer
        live in 8-bit block-floating-point planes (``wire.moment_plane``: 2.125 B per parameter instead of 8, the
        second holding sqrt(v)), which the trainer allocates zeroed in place of the model's ``mom`` / ``var`` unless
        the model already holds them (``MLP(..., adam=True, moment_codec="bfp8")``, a resumed run). Every layer's
        request carries ``moment_seed=bfp_oracle.sr_step_seed(sr_seed, opt_step, layer)``, under which the update
        stores the new moments with stochastic rounding (``bfp_oracle.adamw_q``); ``opt_step`` is already checkpointed,
        so a resumed run's next step is bit-identical. With ``stochastic_rounding``, ``error_feedback`` and
        ``max_grad_norm`` (they act before the update); not with ``trust_ratio`` or a sharded-update engine.

        ``stochastic_rounding``: stochastic rounding for the compressed mesh all-reduce — every layer's request
        carries ``sr_seed=bfp_oracle.sr_step_seed(sr_seed, sr_step, layer)``, under which this rank's two encoders round
        up with probability equal to the dropped fraction; ``sr_step`` is the trainer's update counter (1-based,
        advanced once per ``backward_pass``, checkpointed by the CLI). Stateless: no plane, no extra traffic; one
        encode has about twice round-to-nearest's variance and is unbiased. ``prepack`` and hence ``fused_update`` are
        off, as with ``error_feedback``. ``bfp_rne`` / ``bfp4_rne`` and the mesh schedule only; not with a
        sharded-update engine, a chunked layout or ``error_feedback`` (pick one). Without an engine the local update
        takes the gradient through the one-slot round trip (``wire.reduce_sr``) of ``error_feedback_codec``. A step
        cannot be captured into a graph (its seed is a by-value kernel argument).

        ``error_feedback``: error feedback (residual compensation) for the compressed mesh all-reduce — every layer
        bucket gets one zeroed f32 plane per rank (``residuals``), passed with the layer's request, in which this rank's
        encoders keep what they dropped and from which they add it to the next step's input. ``prepack`` and hence
        ``fused_update`` are off (the bwd-weight GEMM writes f32 and the engine packs: the GEMM's encoding carries no
        residual). BFP codecs and the mesh schedule only; not with a sharded-update engine or a chunked layout. Without
        an engine the local update takes the gradient through the one-slot round trip (``wire.reduce_ef``) of
        ``error_feedback_codec`` (an engine's own codec always wins).
        With any ``optimizer``, ``trust_ratio`` and ``max_grad_norm``. The planes are per-rank state and are not
        checkpointed: a resumed run restarts them at zero.

        ``max_grad_norm``: clip the step's reduced gradient — every layer's, as one vector, after the all-reduce and
        through the wire codec, times ``grad_scale`` — to this 2-norm (``torch.nn.utils.clip_grad_norm_``'s
        coefficient). The layers' requests form one clip group: each ends its communication phase with a norm pass
        over its gathered wire, and the step commits through ``engine.commit_group`` in the order L-1..0, whatever
        ``commit_at_end`` says; ``grad_norm`` (f32[4] on the model's device) holds the last step's {coef, total norm,
        max_grad_norm, nonfinite}, written on the device (no host sync). A group holds at most 8 requests, so at most
        8 layers; ``fused_update`` is off (the GEMM epilogue cannot wait for the group); not with a sharded-update
        engine. With any ``optimizer`` and with ``trust_ratio``.

        ``optimizer``: 'sgd', 'adamw' or 'lion'. AdamW (``betas``, ``eps``; the model holds the second-moment planes,
        ``MLP(..., adam=True)``). AdamW runs in the engine's decode + update epilogue — not in the bwd-weight GEMM's,
        so ``fused_update`` is off with it — with ``opt_step``, the 1-based update count, advanced once per
        ``backward_pass``. ``trust_ratio`` (AdamW): the layer-wise trust ratio (LAMB) — each layer's weight matrix
        steps by lr * ||W|| / ||update||, its bias by lr — through the engines' two-pass epilogue; ``trust_ratios``
        ([L, 3] f32 on the model's device) then holds every layer's {lr * phi, lr, phi} of the last step, written by
        the requests themselves (no host sync). Not with a sharded-update engine. 'lion': Lion (``bfp_oracle.lion``;
        ``betas`` default (0.9, 0.99), no ``eps``, no step count) on the model's momentum plane, ``MLP(...,
        momentum=True)`` — SGD-momentum's planes and bytes, in the engine's epilogue like AdamW, so ``fused_update`` is
        off with it; with ``max_grad_norm``, ``error_feedback``, ``stochastic_rounding`` and a sharded-update engine,
        not with ``trust_ratio`` or ``moment_codec='bfp8'``. ``betas`` left unset: (0.9, 0.999) for AdamW.

        ``fused_update`` (default env FAN_FUSED_UPDATE, else on): with a single-rank engine (world 1, requests
        inline: the all-reduce of one rank is the identity) and the GEMM-encoded wire, the bwd-weight GEMM's epilogue
        takes each encoded gradient group through its BFP round trip in registers and applies the SGD update to the
        layer's weights in place — the engine's decode + SGD pass over the whole bucket (master read + write, bf16
        copy write, wire read) disappears into the GEMM. Same operations in the same order: bit-identical weights
        to the unfused schedule. The layer's bwd-data GEMM (which reads the weights) is issued first.

        ``gemm_inflight`` (default env FAN_GEMM_INFLIGHT, else 'persistent'): the GEMM form while a request of this
        step is in flight on the side stream (multi-rank engines only). 'persistent': one 4-wave workgroup per CU
        looping over tiles — it holds every CU until it ends, so the comm stream's kernels start only at GEMM
        boundaries; 'grid': one workgroup per tile from the first submit to the end of backward, so comm kernels
        start at tile boundaries (the forced 1-rank path's comm phase took half the device time that way,
        profiles/r3_persist_vs_tile_grid_forced.txt). bench.py picks between them by timing both at world > 1.

        ``wgrad_pair`` (default env FAN_WGRAD_PAIR, else on; fused update only): the bwd-weight GEMMs whose plan is
        the planner rule's 256x256 split-K one (the narrow layers: too few tiles to fill the CUs unsplit) are
        postponed to the end of the backward and run as ONE grouped launch at a smaller common split with ONE slab
        reduce (models/mlp.py backward_weight_group). False: each in its layer's turn. 'single' (tests, A/B):
        postponed alike, but launched one by one at the group's split — the grouped launch is bit-identical to it."""
        self.m = model
        self.engine = engine
        self.world = engine.world if engine is not None else 1
        self.lr, self.wd, self.momentum, self.nesterov = lr, weight_decay, momentum, nesterov
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {optimizer!r}")
        betas = resolve_betas(optimizer, betas)
        self.optimizer, self.betas, self.eps = optimizer, (float(betas[0]), float(betas[1])), float(eps)
        self.opt_step = 0  # updates applied so far (AdamW's bias correction; checkpointed)
        if optimizer == "adamw":
            if momentum or nesterov:
                raise ValueError("momentum / nesterov belong to SGD: AdamW's first moment is governed by betas[0]")
            wire.O.adamw_scalars(lr, weight_decay, self.betas[0], self.betas[1], self.eps, 1)  # validates
            if moment_codec != "bfp8" and any(l.mom is None or l.var is None for l in model.layers):
                raise ValueError("optimizer='adamw' needs a model with both moment planes: MLP(..., adam=True)")
        if optimizer == "lion":
            if momentum or nesterov:
                raise ValueError("momentum / nesterov belong to SGD: Lion's moment is governed by betas")
            if trust_ratio:
                raise ValueError("trust_ratio is a flag of optimizer='adamw' (a trust ratio on Lion is not provided)")
            wire.O.lion_scalars(lr, weight_decay, self.betas[0], self.betas[1])  # validates
            if any(l.mom is None or l.mom.dtype != torch.float32 for l in model.layers):
                raise ValueError("optimizer='lion' needs a model with the f32 momentum plane: MLP(..., momentum=True)")
            if any(l.var is not None for l in model.layers):
                raise ValueError("optimizer='lion' keeps one moment plane: the model holds a second (adam=True); "
                                 "allocate it with MLP(..., momentum=True)")
        self.moment_codec = wire.O.moment_codec_check(moment_codec)
        if moment_codec == "bfp8":
            if optimizer == "lion":
                raise ValueError("moment_codec='bfp8': optimizer='adamw' only (Lion's one moment plane stays f32)")
            if optimizer != "adamw":
                raise ValueError("moment_codec='bfp8': optimizer='adamw' only (SGD keeps no second moment; its "
                                 "momentum stays f32)")
            if trust_ratio:
                raise ValueError("moment_codec='bfp8': not with trust_ratio (LAMB's pass 2 recomputes the direction "
                                 "from the stored moments)")
            if bool(getattr(engine, "shard_update", False)):
                raise ValueError("moment_codec='bfp8': not with a sharded-update engine (its owner kernels keep f32 "
                                 "moment shards)")
            for l in model.layers:
                n_pad = engine.layout(l.n).n_pad if engine is not None else l.n_pad
                nb = wire.O.moment_plane_bytes(n_pad)
                if not all(t is not None and t.dtype == torch.uint8 and t.numel() == nb for t in (l.mom, l.var)):
                    l.mom, l.var = wire.moment_plane(n_pad, model.device), wire.moment_plane(n_pad, model.device)
        elif any(t is not None and t.dtype == torch.uint8 for l in model.layers for t in (l.mom, l.var)):
            raise ValueError("the model holds 8-bit moment planes: moment_codec='bfp8'")
        self.trust_ratio = bool(trust_ratio)
        if self.trust_ratio and optimizer != "adamw":
            raise ValueError("trust_ratio is a flag of optimizer='adamw'")
        if self.trust_ratio and bool(getattr(engine, "shard_update", False)):
            raise ValueError("trust_ratio: not with a sharded-update engine (each owner updates its shard before the "
                             "bucket is reduced)")
        self.trust_ratios = (torch.zeros(model.L, 3, dtype=torch.float32, device=model.device)
                             if self.trust_ratio else None)
        self._trust_partials = None  # the engine-less update's norm partials
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self._clip_partials = None  # the engine-less update's norm partials, one segment per layer
        if self.max_grad_norm is not None:
            if not (self.max_grad_norm > 0 and math.isfinite(self.max_grad_norm)):
                raise ValueError(f"max_grad_norm must be finite and positive, got {max_grad_norm}")
            if model.L > NUM_SLOTS:
                raise ValueError(f"max_grad_norm: the model has {model.L} layers; a clip group holds at most "
                                 f"{NUM_SLOTS} deferred requests (one per layer)")
            if bool(getattr(engine, "shard_update", False)):
                raise ValueError("max_grad_norm: not with a sharded-update engine (each owner updates its shard before "
                                 "the bucket is reduced)")
            self.grad_norm = torch.zeros(4, dtype=torch.float32, device=model.device)
        self.error_feedback = bool(error_feedback)
        self.residuals = None
        self._ef_wire = None  # the engine-less trainer's one-slot wire, per layer
        self.ef_codec = getattr(engine, "codec", "bfp_rne") if engine is not None else error_feedback_codec
        if self.error_feedback:
            if wire.is_raw(self.ef_codec):
                raise ValueError(f"error_feedback: nothing to feed back with a raw codec ({self.ef_codec}); BFP codecs "
                                 f"only")
            if engine is not None and getattr(engine, "algo", "mesh") != "mesh":
                raise ValueError("error_feedback: mesh schedule only (the ring schedule is not supported yet)")
            if bool(getattr(engine, "shard_update", False)):
                raise ValueError("error_feedback: not with a sharded-update engine")
            if engine is not None and any(getattr(engine.layout(l.n), "chunks", 1) > 1 for l in model.layers):
                raise ValueError("error_feedback: not with a chunked layout (a bucket above the engine's chunk_elems)")
            self.residuals = [torch.zeros(l.n_pad, dtype=torch.float32, device=model.device) for l in model.layers]
            prepack = False
        self.stochastic_rounding = bool(stochastic_rounding)
        self.sr_seed = wire.O.sr_seed_check(sr_seed)
        self.sr_step = 0  # updates enqueued so far (the step of sr_step_seed; checkpointed with the flag on)
        if self.stochastic_rounding:
            if self.error_feedback:
                raise ValueError("stochastic_rounding: not together with error_feedback (pick one)")
            if wire.codec_id(self.ef_codec) not in wire.O.SR_CODECS:
                raise ValueError(f"stochastic_rounding: bfp_rne and bfp4_rne only, got {self.ef_codec!r} (bfp_trunc is "
                                 f"the reference's floor, a raw codec rounds nothing)")
            if engine is not None and getattr(engine, "algo", "mesh") != "mesh":
                raise ValueError("stochastic_rounding: mesh schedule only (the ring schedule is not supported yet)")
            if bool(getattr(engine, "shard_update", False)):
                raise ValueError("stochastic_rounding: not with a sharded-update engine")
            if engine is not None and any(getattr(engine.layout(l.n), "chunks", 1) > 1 for l in model.layers):
                raise ValueError("stochastic_rounding: not with a chunked layout (a bucket above the engine's "
                                 "chunk_elems)")
            if self.world > MAX_PEERS:
                raise ValueError(f"stochastic_rounding: at most {MAX_PEERS} ranks, got {self.world}")
            if any(l.n_pad >= wire.O.SR_MAX_ELEMS for l in model.layers):
                raise ValueError("stochastic_rounding: a padded bucket of 2^32 or more elements (element indices are "
                                 "32-bit)")
            prepack = False
        self.loss_scale = loss_scale
        # gradients are of the LOCAL mean loss; the all-reduce sums over ranks -> average with 1/N
        self.grad_scale = (1.0 / self.world) if average else 1.0
        self.pending: list[Handle | None] = [None] * model.L
        self.last_handle: Handle | None = None
        self.cuda = model.device.type == "cuda"
        self.profile = profile
        self.times = {"fwd": 0.0, "loss": 0.0, "bwd": 0.0, "bwd_first": 0.0, "steps": 0}
        self.step_count = 0
        # fuse the BFP encode into the bwd-weight GEMM when the engine accepts prepacked wire input
        # commit every request's epilogue after the whole backward is enqueued (required when the engine runs
        # epilogues on the compute stream: a per-layer commit would stall it on that layer's communication)
        self.commit_at_end = (bool(getattr(engine, "epilogue_on_producer", False)) if commit_at_end is None
                              else commit_at_end)
        self.prepack = (prepack and engine is not None and getattr(engine, "prepack", False) and self.cuda
                        and model.dtype == torch.bfloat16)
        fu = os.environ.get("FAN_FUSED_UPDATE", "1") != "0" if fused_update is None else bool(fused_update)
        # (the GEMM epilogue's update is SGD: AdamW takes the engine's decode + update pass; nor can it wait for a
        # clip group's coefficient)
        self.fused_update = (fu and self.prepack and bool(getattr(engine, "inline", False))
                             and getattr(engine, "codec", "") == "bfp_rne" and optimizer == "sgd"
                             and self.max_grad_norm is None)
        self.fused_updates = 0
        # fused update: the layers' bias-gradient reduces of unsplit bwd-weight plans are queued and run by the next
        # split-K wire reduce of the backward, or all in one grouped launch after it (FAN_DEFER_COLSUM=0: one launch
        # each, right after its GEMM; bit-identical either way)
        self.defer_colsum = os.environ.get("FAN_DEFER_COLSUM", "1") != "0"
        # a split-K classifier GEMM leaves its slabs to the softmax-xent kernel, which folds them (FAN_FOLD_LOGITS=0:
        # the GEMM's own slab reduce launch; bit-identical either way)
        self.fold_logits = os.environ.get("FAN_FOLD_LOGITS", "1") != "0"
        wp = os.environ.get("FAN_WGRAD_PAIR", "1") != "0" if wgrad_pair is None else wgrad_pair
        if wp not in (True, False, "single"):
            raise ValueError(f"wgrad_pair must be True|False|'single', got {wgrad_pair!r}")
        self.wgrad_pair = wp
        self.wgrad_groups = 0  # grouped bwd-weight launches so far
        self._wgrad_plan = (None, [], 0)
        # layer-chain launches (ops/gemm.py linear_chain, FAN_GEMM_CHAIN): the forward at every world size; the
        # bwd-data chain only with the fused world-1 update — with a multi-rank engine each layer's all-reduce is
        # issued right after its own bwd-weight GEMM and overlaps that layer's bwd-data GEMM, which a chain of the
        # bwd-data GEMMs would postpone
        self.chain_fwd = G.chain_enabled()
        self.chain_bwd = G.chain_enabled()
        gi = os.environ.get("FAN_GEMM_INFLIGHT", "persistent") if gemm_inflight is None else gemm_inflight
        if gi not in ("persistent", "grid"):
            raise ValueError(f"gemm_inflight must be persistent|grid, got {gi!r}")
        self.gemm_inflight = gi if (self.cuda and engine is not None and not getattr(engine, "inline", True)) \
            else "persistent"
        self._persist_saved = None
        # sharded-update engine (bf16 model): each request writes the layer's NEXT weight buffer (lp_next), which no
        # GEMM of this step reads, so it needs no ordering after the layer's bwd-data GEMM; the buffers swap once the
        # step's backward is enqueued (the next forward waits for its layer's request, _wait_layer)
        self.shard = bool(getattr(engine, "shard_update", False)) and self.cuda and model.dtype == torch.bfloat16
        self.lp_next = [l.lp.clone() if self.shard else None for l in model.layers]
        # multi-rank native engine: layer 0's request (the backward's last) on the compute stream itself
        # (FAN_LAST_ON_PRODUCER=0: on the comm stream like the others)
        self.last_on_producer = (self.cuda and engine is not None and not getattr(engine, "inline", True)
                                 and hasattr(engine, "C") and os.environ.get("FAN_LAST_ON_PRODUCER", "1") != "0")
        if self.max_grad_norm is not None and not bool(getattr(engine, "epilogue_on_producer", False)):
            # an on-producer request's epilogue runs on the compute stream; with the others' on the comm stream the
            # group's one coefficient launch could not precede them all
            self.last_on_producer = False

    def _opt_kw(self, l):
        """The optimizer, clip-group, error-feedback and stochastic-rounding arguments of layer l's request in the step
        being enqueued."""
        kw = {} if self.grad_norm is None else dict(clip=self.grad_norm)
        if self.residuals is not None:
            kw["residual"] = self.residuals[self._index(l)]
        if self.stochastic_rounding:
            kw["sr_seed"] = self._sr_seed_of(l)
        if self.optimizer == "lion":
            kw.update(opt="lion", betas=self.betas)
            return kw
        if self.optimizer != "adamw":
            return kw
        kw.update(opt="adamw", var=l.var, betas=self.betas, eps=self.eps, step=self.opt_step)
        if self.moment_codec == "bfp8":
            kw.update(moment_codec="bfp8", moment_seed=self._moment_seed_of(l))
        if self.trust_ratio:
            kw.update(trust_ratio=True, n_adapt=self._n_adapt(l), trust_out=self._trust_row(l))
        return kw

    def _trust_row(self, l):
        """Layer l's row of ``trust_ratios`` (found by identity: buckets of equal shape compare by their tensors)."""
        return self.trust_ratios[self._index(l)]

    def _index(self, l):
        return next(i for i, x in enumerate(self.m.layers) if x is l)

    def _local_src(self, l):
        """(wire bytes, their codec) the engine-less update of layer l reads: the f32 gradient itself as raw_f32, or
        with error feedback or stochastic rounding the one-slot wire ``_ef_local`` / ``_sr_local`` encoded this step."""
        if self.residuals is None and not self.stochastic_rounding:
            return wire.as_bytes(l.grad), "raw_f32"
        return self._ef_wire[self._index(l)], self.ef_codec

    def _local_wire(self, l):
        if self._ef_wire is None:
            self._ef_wire = [torch.zeros(wire.shard_bytes(self.ef_codec, x.n_pad), dtype=torch.uint8,
                                         device=x.grad.device) for x in self.m.layers]
        return self._ef_wire[self._index(l)]

    def _ef_local(self, l):
        """Engine-less error feedback: layer l's gradient plus its residual through the codec's round trip at one
        slot (the owner stage alone, as a one-rank engine)."""
        S = self._local_wire(l)
        wire.reduce_ef(S, 1, 0, l.grad, self.residuals[self._index(l)], S, l.n_pad, self.ef_codec)

    def _sr_seed_of(self, l):
        """The seed of layer l's request in the step being enqueued."""
        return wire.O.sr_step_seed(self.sr_seed, self.sr_step, self._index(l))

    def _moment_seed_of(self, l):
        """The seed of layer l's 8-bit state in the update being enqueued (``opt_step`` is its 1-based count)."""
        return wire.O.sr_step_seed(self.sr_seed, self.opt_step, self._index(l))

    def _sr_local(self, l):
        """Engine-less stochastic rounding: layer l's gradient through the stochastic round trip at one slot (the
        owner stage alone, as a one-rank engine)."""
        S = self._local_wire(l)
        wire.reduce_sr(S, 1, 0, l.grad, S, l.n_pad, self.ef_codec, self._sr_seed_of(l), 0)

    def _n_adapt(self, l):
        """The adapted tensor of layer l's bucket: its weight matrix; the bias segment behind it takes ratio 1."""
        return l.cin * l.cout if self.m.bias else l.n

    def _clip_local(self):
        """The engine-less clip group: every layer's norm pass over its f32 gradient, then the coefficient."""
        if self._clip_partials is None:
            self._clip_partials = [torch.zeros(wire.sumsq_partials_for(l.master, l.n_pad), dtype=torch.float64,
                                               device=l.master.device) for l in self.m.layers]
        segs = []
        for i in reversed(range(self.m.L)):
            l = self.m.layers[i]
            src, codec = self._local_src(l)
            k = wire.sumsq(src, l.n_pad, 1, codec=codec, partials=self._clip_partials[i], n_valid=l.n)
            segs.append((self._clip_partials[i], 0, k))
        wire.clip_coef(segs, self.max_grad_norm, self.grad_scale, self.grad_norm)

    def _sgd_local(self, l):
        clip = self.grad_norm
        src, codec = self._local_src(l)
        if self.trust_ratio:
            scalars = wire.O.lamb_scalars(self.lr, self.wd, self.betas[0], self.betas[1], self.eps, self.opt_step)
            if self._trust_partials is None:
                self._trust_partials = torch.zeros(2 * wire.lamb_partials_for(l.master, 1 << 40), dtype=torch.float64,
                                                   device=l.master.device)
            words, kw = self._trust_row(l), dict(n_valid=l.n, n_adapt=self._n_adapt(l))
            k = wire.lamb_moments(src, l.n_pad, 1, l.master, codec=codec, mom=l.mom, var=l.var,
                                  scalars=scalars, partials=self._trust_partials, grad_scale=self.grad_scale,
                                  clip=clip, **kw)
            wire.lamb_ratio(self._trust_partials, k, self.lr, words)
            wire.lamb_apply(l.master, l.n_pad, mom=l.mom, var=l.var, scalars=scalars, words=words, lp=l.lp, **kw)
            return
        if self.optimizer == "adamw":
            scalars = wire.O.adamw_scalars(self.lr, self.wd, self.betas[0], self.betas[1], self.eps, self.opt_step)
            if self.moment_codec == "bfp8":
                wire.adamw_q(src, l.n_pad, 1, l.master, codec=codec, lp=l.lp, mom_q=l.mom, var_q=l.var,
                             scalars=scalars, seed=self._moment_seed_of(l), grad_scale=self.grad_scale, n_valid=l.n,
                             clip=clip)
                return
            wire.adamw(src, l.n_pad, 1, l.master, codec=codec, lp=l.lp, mom=l.mom, var=l.var,
                       scalars=scalars, grad_scale=self.grad_scale, n_valid=l.n, clip=clip)
            return
        if self.optimizer == "lion":
            scalars = wire.O.lion_scalars(self.lr, self.wd, self.betas[0], self.betas[1])
            wire.lion(src, l.n_pad, 1, l.master, codec=codec, lp=l.lp, mom=l.mom, scalars=scalars,
                      grad_scale=self.grad_scale, n_valid=l.n, clip=clip)
            return
        wire.sgd(src, l.n_pad, 1, l.master, codec=codec, lp=l.lp, mom=l.mom, lr=self.lr,
                 grad_scale=self.grad_scale, weight_decay=self.wd, momentum=self.momentum, nesterov=self.nesterov,
                 n_valid=l.n, clip=clip)

    def step(self, x: torch.Tensor, labels: torch.Tensor):
        """One training iteration (reference type 'A': FWD + loss + BWD + all-reduce/UPD)."""
        self.forward_pass(x)
        self.backward_pass(labels)
        self.times["steps"] += 1
        self.step_count += 1
        return self.m.loss_rows

    def forward_pass(self, x: torch.Tensor):
        """Forward of every layer (reference type 'F' times this plus the loss forward)."""
        m = self.m
        m.alloc_activations(x.shape[0])
        m.act[0] = x
        t0 = time.perf_counter()
        with tracing.range("fwd"):
            # the whole forward as one layer-chain launch when it takes the model (every layer's update must have
            # landed first: layer 0's, the last request of the backward, is the one it waits on in practice)
            if self.cuda and self.chain_fwd:
                for i in range(m.L):
                    self._wait_layer(i)
                chained = m.forward_chain()
            else:
                chained = False
            if not chained:
                for i in range(m.L):
                    self._wait_layer(i)  # layer i's weights updated (reference: per-layer wait, sw:757-787)
                    m.forward_layer(i, fold_logits=self.fold_logits and self.cuda)
            self.last_handle = None
        if self.profile:
            self._sync()
            self.times["fwd"] += time.perf_counter() - t0

    def _wait_layer(self, i: int):
        """Layer i's weights must be updated before its forward reads them: a GPU-side wait on layer i's
        request(s) only (free when its epilogue already runs on this stream), so layer i's forward starts as soon
        as ITS update lands rather than after the whole step's (reference: the host waits per layer request,
        sw/mlp_mpi_example_f32.cpp:757-787)."""
        h = self.pending[i]
        if h is None:
            return
        for x in (h if isinstance(h, list) else [h]):
            if self.cuda:
                x.wait()
            else:
                x.synchronize()
        self.pending[i] = None

    def _wait_updates(self):
        """Every outstanding update has landed (GPU-side order on the current stream; host waits on CPU)."""
        for i in range(self.m.L):
            self._wait_layer(i)
        self.last_handle = None

    def backward_pass(self, labels: torch.Tensor):
        """Loss fwd+bwd, then per layer L-1..0: dW -> async all-reduce+SGD -> dX (reference type 'B')."""
        m = self.m
        prof = self.profile
        if self.optimizer == "adamw" and self.cuda and torch.cuda.is_current_stream_capturing():
            # the step's scalars are by-value kernel arguments: a captured graph would replay step 1's for ever
            raise RuntimeError("an AdamW step cannot be captured into a graph (its per-step scalars would be frozen)")
        if self.stochastic_rounding and self.cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a stochastically rounded step cannot be captured into a graph (its seed would be frozen)")
        self.opt_step += 1
        self.sr_step += 1
        self._wait_updates()  # no-op after forward_pass; needed when backward passes run back to back
        t0 = time.perf_counter()
        with tracing.range("loss"):
            m.loss_backward(labels, grad_scale=self.loss_scale / m.act[0].shape[0])
        if prof:
            self._sync()
            t1 = time.perf_counter()
            self.times["loss"] += t1 - t0
            t0 = t1
        # world 1 with the fused update on every layer: the bwd-data GEMMs of layers L-1 .. 1 as one layer-chain
        # launch first (each layer's weights are read there before its bwd-weight GEMM updates them in place)
        tgts = [(self.engine.prepack_target(l.grad, l.n, None if m.bias else l.cin * l.cout)
                 if self.prepack and l.cout % 16 == 0 else None) for l in m.layers]
        chained = (self.fused_update and self.chain_bwd and all(t is not None for t in tgts)
                   and m.backward_data_chain())
        # (with or without the bwd-data chain: the two schedules stay bit-identical, tests/test_gpu_gemm_chain.py)
        post, split = self._wgrad_postponed(tgts)
        late = []  # the postponed layers' (i, wire, update), in the backward's order
        try:
            for i in reversed(range(m.L)):
                l = m.layers[i]
                with tracing.range(f"bwd{i}"):
                    # the bwd-weight GEMM encodes dW (and the fused bias gradient) straight into the wire buffer;
                    # the zero tail (padding, or the bias segment of a bias-free model) is encoded once
                    # (the wire epilogue encodes whole 16-column groups: output widths that are multiples of 16)
                    tgt = tgts[i]
                    if tgt is not None and self.fused_update:
                        # single-rank engine: bwd-data first (it reads W_i), then dW's BFP round trip + SGD in the
                        # bwd-weight epilogue
                        if not chained:
                            m.backward_data(i)
                        upd = G.LocalUpdate(l.master, l.lp, l.mom, lr=self.lr, grad_scale=self.grad_scale,
                                            weight_decay=self.wd, momentum=self.momentum, nesterov=self.nesterov)
                        # (the bwd-weight GEMMs of layers >= 1 on a second stream, beside the next GEMM, measured 1.5-2 %
                        # slower: profiles/r3_fused_update_ab.txt)
                        if i in post:
                            late.append((i, tgt, upd))
                        else:
                            m.backward_weight(i, wire=tgt, update=upd, defer_colsum=self.defer_colsum)
                        self.fused_updates += 1
                    else:
                        m.backward_weight(i, wire=tgt)
                        h = None
                        if self.engine is not None:
                            kw = {"prepacked": (tgt[0], l.n_pad)} if tgt is not None else {}
                            lp_out = self.lp_next[i] if self.shard else l.lp
                            if i == 0 and self.last_on_producer:
                                # the backward's last request: nothing left to overlap it with, so it runs on this
                                # stream (no hand-off to the comm stream and back before the next forward)
                                kw["on_producer"] = True
                            h = self.engine.allreduce_sgd(l.grad, l.master, lp_out, l.mom, n_valid=l.n, lr=self.lr,
                                                          grad_scale=self.grad_scale, weight_decay=self.wd,
                                                          momentum=self.momentum, nesterov=self.nesterov, defer=True,
                                                          name=f"fc{i}", **kw, **self._opt_kw(l))
                            self._gemm_grid(True)
                        elif self.residuals is not None:
                            self._ef_local(l)
                        elif self.stochastic_rounding:
                            self._sr_local(l)
                        m.backward_data(i)
                        if h is not None:
                            clipped = self.grad_norm is not None  # (commits with its group, below)
                            self.pending[i] = h if self.commit_at_end or clipped else h.commit_after_current()
                            self.last_handle = self.pending[i]
                        elif self.grad_norm is None:
                            self._sgd_local(l)
                if prof and i == m.L - 1:
                    self._sync()
                    t1 = time.perf_counter()
                    self.times["bwd_first"] += t1 - t0
                    self.times["bwd"] += t1 - t0
                    t0 = t1
            if late and self.wgrad_pair == "single":
                for i, tgt, upd in late:
                    m.backward_weight(i, wire=tgt, update=upd, split_k=split, tile=(256, 256))
            elif late:
                # every layer's bwd-data GEMM is enqueued (the updates are in place); the reduce of this launch also
                # runs the bias-gradient reduces the unsplit layers queued
                with tracing.range("bwd_wgrad_group"):
                    m.backward_weight_group(late, split)
                self.wgrad_groups += 1
        finally:
            # the bias updates still queued (every layer's lands before the next forward; after an exception too, so
            # no queued reduce is left for an unrelated later GEMM of the stream to run)
            if self.fused_updates and self.defer_colsum and self.cuda:
                G.flush_colsum()
            # the grid GEMM form must not outlive this backward (an exception in between would leave every later
            # GEMM of the process on one workgroup per tile while records report the persistent form)
            self._gemm_grid(False)
        if self.shard:  # this step's requests write lp_next: it holds the weights the next forward uses
            for i, l in enumerate(m.layers):
                l.lp, self.lp_next[i] = self.lp_next[i], l.lp
        if self.grad_norm is not None and self.engine is None:
            # no weight moves before the norm over every layer exists: the updates wait for the end of the backward
            self._clip_local()
            for i in reversed(range(m.L)):
                self._sgd_local(m.layers[i])
        elif self.grad_norm is not None:
            self.engine.commit_group([self.pending[i] for i in reversed(range(m.L))], max_norm=self.max_grad_norm,
                                     grad_scale=self.grad_scale)
        elif self.commit_at_end:  # issue order L-1..0: the epilogues run in the order their all-reduces finish
            for i in reversed(range(m.L)):
                h = self.pending[i]
                for x in (h if isinstance(h, list) else [] if h is None else [h]):
                    x.commit_after_current()
        if prof:
            self._sync()
            self.times["bwd"] += time.perf_counter() - t0

    def _wgrad_postponed(self, tgts):
        """The layers whose bwd-weight GEMM is postponed into the grouped launch that ends the backward, and its
        common split (([], 0): none). World 1 with the fused update only — with a multi-rank engine a postponed layer
        would delay its all-reduce. A layer qualifies when its GEMM would run the planner rule's 256x256 split-K plan
        (ops/gemm.py wgrad_static_split); the group needs two or more of them and a common split within the
        planner's limits (wgrad_group_split), which holds from 4096 rows upward for 1024-wide layers."""
        m = self.m
        if not (self.wgrad_pair and self.fused_update and self.cuda and m.bias):
            return [], 0
        # (decided once per batch size and state of the tuner's decisions, not per step)
        T = gemm_tune.tuner()
        key = (m.act[0].shape[0], tuple(t is not None for t in tgts), id(T), T.enabled, len(T.plans))
        if self._wgrad_plan[0] != key:
            post = [i for i in range(m.L) if tgts[i] is not None and G.wgrad_static_split(*m.wgrad_problem(i)) > 1]
            split = G.wgrad_group_split([m.wgrad_problem(i) for i in post])
            self._wgrad_plan = (key, post if split else [], split)
        return self._wgrad_plan[1:]

    def _gemm_grid(self, on: bool):
        """gemm_inflight='grid': GEMMs enqueued while a request is in flight run one workgroup per tile."""
        if self.gemm_inflight != "grid":
            return
        from .. import _ext

        C = _ext.require()
        if on and self._persist_saved is None:
            self._persist_saved = C.gemm_persist()
            C.gemm_set_persist(0)
        elif not on and self._persist_saved is not None:
            C.gemm_set_persist(self._persist_saved)
            self._persist_saved = None

    def _sync(self):
        if self.cuda:
            torch.cuda.synchronize()

    def finish_async(self):
        """GPU-side: order the current stream after every outstanding update (no host wait; usable while
        capturing a HIP graph)."""
        self._wait_updates()

    def gather_state(self):
        """Sharded-update engine: collect every layer's owner-sharded master (and moments) onto every rank, so the
        planes are whole again (checkpoint, replica check). Collective; a no-op for other engines."""
        if not self.shard:
            return
        self.finish()
        for l in self.m.layers:
            self.engine.gather_owned(l.master, l.n)
            if l.mom is not None:
                self.engine.gather_owned(l.mom, l.n)
            if l.var is not None:
                self.engine.gather_owned(l.var, l.n)

    def finish(self, timeout: float | None = None):
        """Wait (host) for every outstanding all-reduce/update."""
        self._gemm_grid(False)
        for i, h in enumerate(self.pending):
            if h is not None:
                for x in (h if isinstance(h, list) else [h]):
                    x.synchronize(timeout)
                self.pending[i] = None
        self.last_handle = None
        self._sync()
