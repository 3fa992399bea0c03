"""Compressed all-reduce engine with the SGD weight update fused into the all-gather epilogue.

This is the MI355X-native replacement for the reference NIC (hw/all_reduce.sv + hw/weight_update.sv +
hw/bfp_adapter.sv) and its host driver (sw/mlp_mpi_example_f32.cpp:65-180):

* request API ``allreduce_sgd(grad, weights, ...) -> Handle`` mirrors ``all_reduce(buf, weight_out, flags,
  done, count)`` + ``wait(done)`` (sw:114-180); completion slots round-robin 0..7 like the NIC's 3-bit
  ``done_id`` (hw/all_reduce.sv:1228, 1373). ``Handle.synchronize(timeout)`` replaces the reference's
  unbounded busy-spin (sw:163-168) with a bounded wait + diagnostics.
* weights live in HBM next to the gradients; the epilogue decodes the reduced gradient and applies
  ``w = fma(-lr, g, w)`` (hw/weight_update.sv:442-451) in place — with lr / grad scaling / momentum /
  weight decay as runtime parameters instead of the hard-coded 0.1.
* every rank applies the update to the SAME decoded values (owner included), so replicas stay
  bit-identical (the reference's owner used the un-quantised sum: SURVEY.md §2.6 quirk; available as
  ``compat_owner_fp32=True`` on the ring algorithm).

Algorithms
----------
``mesh`` (default on xGMI): pack -> all-to-all -> owner sums its shard (local contribution un-quantised)
-> re-encode -> all-gather -> fused decode+SGD. On a fully connected 8-GPU xGMI node every link carries
traffic at once, and every contribution is quantised once (instead of N-1 re-quantisations in a ring).

``ring``: the reference schedule (SEND_LOCAL, REDUCE x(N-2), REDUCE_OUTPUT, FORWARD_OUTPUT x(N-2)),
planned natively (``_C.ring_plan``), generalised to any N >= 1 and to R arc-disjoint directed rings
(``_C.ring_orders``: 7 rings on 8 GPUs so each of the 7 xGMI links of a GPU carries one ring). Each hop is
one fused HIP kernel (decode recv + add local + re-encode); all-gather hops forward the encoded bytes
untouched (re-encoding a decoded group is idempotent).
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field

import torch

from .. import _ext
from ..ops import wire
from ..utils import faults
from .transport import Transport

NUM_SLOTS = 8  # reference: 3-bit done_id


class CommTimeoutError(RuntimeError):
    pass


class ChecksumError(RuntimeError):
    """A message failed verification (debug ``verify`` mode): corrupted payload or out-of-order request."""


def _checksum(rows: torch.Tensor) -> torch.Tensor:
    """Per-row Fletcher-style checksum of byte rows [k, nbytes] (nbytes % 4 == 0) -> int64 [k, 2]."""
    w = rows.contiguous().view(torch.int32).to(torch.int64)
    idx = torch.arange(1, w.shape[1] + 1, device=w.device, dtype=torch.int64)
    return torch.stack([w.sum(1), (w * idx).sum(1)], 1)


def _cdiv(a, b):
    return (a + b - 1) // b


def _round_up(a, b):
    return _cdiv(a, b) * b


OPTIMIZERS = ("sgd", "adamw", "lion")
DEFAULT_BETAS = {"sgd": (0.9, 0.999), "adamw": (0.9, 0.999), "lion": (0.9, 0.99)}


def resolve_betas(opt, betas):
    """``betas`` left unset: AdamW's (0.9, 0.999) for ``sgd`` (which ignores them) and ``adamw``, Lion's (0.9, 0.99)
    for ``lion`` (Chen et al. 2023)."""
    return DEFAULT_BETAS.get(opt, (0.9, 0.999)) if betas is None else betas
CLIP_GROUP_LIMIT = f"a clip group holds at most {NUM_SLOTS} deferred requests"


def clip_request(clip, defer, device=None):
    """Validate one request's ``clip=`` words (global-norm clipping, see ``commit_group``)."""
    if clip is None:
        return
    if not (isinstance(clip, torch.Tensor) and clip.dtype == torch.float32 and clip.numel() >= 4
            and clip.is_contiguous()):
        raise ValueError("clip: the group's four f32 words (a contiguous float32 tensor of 4 elements)")
    if device is not None and clip.device.type != torch.device(device).type:
        raise ValueError(f"clip: the words live on {clip.device}, the engine runs on {device}")
    if not defer:
        raise ValueError("a clipped request must be deferred (defer=True): no weight may move before the norm over "
                         "every request of the group exists")


def clip_group_check(handles, max_norm):
    """The checks of ``commit_group`` both engines share; returns the group's words tensor."""
    handles = list(handles)
    if not handles:
        raise ValueError("commit_group: no request")
    if len(handles) > NUM_SLOTS:
        raise ValueError(f"commit_group: {len(handles)} requests: {CLIP_GROUP_LIMIT}")
    max_norm = float(max_norm)
    if not (max_norm > 0 and math.isfinite(max_norm)):
        raise ValueError(f"commit_group: max_norm must be finite and positive, got {max_norm}")
    if len({id(h) for h in handles}) != len(handles):
        raise ValueError("commit_group: a request named twice")
    for h in handles:
        if getattr(h, "_clip", None) is None:
            raise ValueError(f"commit_group: request '{h.name}' was not submitted with clip=")
        if not h.pending:
            raise ValueError(f"commit_group: request '{h.name}' (slot {h.slot}) is not pending any more")
    words = handles[0]._clip["words"]
    for h in handles[1:]:
        w = h._clip["words"]
        if w.data_ptr() != words.data_ptr() or w.device != words.device:
            raise ValueError("commit_group: every request of a clip group names the same clip words")
    return words


MAX_PEERS = 16  # csrc/bfp/bfp_format.h kMaxPeers: the destination table of the kernels that store per shard


def residual_request(residual, L, *, codec_id, algo, world, device, prepacked=False, sharded=False):
    """Validate one request's ``residual=`` plane (error feedback: the f32 plane of ``L.n_pad`` elements that keeps
    what this rank's encoders dropped, zeroed by the caller before the bucket's first request and updated in place by
    every request). Returns the flat plane, or None without one."""
    if residual is None:
        return None
    if codec_id == 2:
        raise ValueError("error feedback: nothing to feed back with the raw codec (raw_f32 drops nothing)")
    if codec_id == 3:
        raise ValueError("error feedback: raw_bf16 is not supported yet (BFP codecs only)")
    if prepacked:
        raise ValueError("error feedback: not with prepacked input (the GEMM's encoding carries no residual)")
    if algo != "mesh":
        raise ValueError("error feedback: mesh schedule only (the ring schedule is not supported yet)")
    if L.chunks > 1:
        raise ValueError("error feedback: not with a chunked layout")
    if sharded:
        raise ValueError("error feedback: not with a sharded-update engine")
    if world > MAX_PEERS:
        raise ValueError(f"error feedback: at most {MAX_PEERS} ranks (one destination per shard), got {world}")
    if not (isinstance(residual, torch.Tensor) and residual.dtype == torch.float32):
        raise ValueError("error feedback: the residual plane is a float32 tensor (whatever the gradient's dtype)")
    if not residual.is_contiguous():
        raise ValueError("error feedback: the residual plane must be contiguous")
    if residual.device.type != torch.device(device).type or (
            residual.device.type == "cuda" and torch.device(device).index not in (None, residual.device.index)):
        raise ValueError(f"error feedback: the residual plane lives on {residual.device}, the engine runs on {device}")
    if residual.numel() < L.n_pad:
        raise ValueError(f"error feedback: the residual plane has {residual.numel()} elements; the layout needs "
                         f"{L.n_pad} (engine.layout(n).n_pad)")
    return residual.view(-1)


def sr_request(sr_seed, L, *, codec_id, algo, world, prepacked=False, sharded=False, residual=None):
    """Validate one request's ``sr_seed=`` (stochastic rounding: this rank's two encoders of the mesh schedule round up
    with probability equal to the dropped fraction, drawing from a hash of the 64-bit request seed, the rank, the stage
    and the element's index in the padded bucket). Returns the seed as an int, or None without one."""
    if sr_seed is None:
        return None
    if residual is not None:
        raise ValueError("stochastic rounding: not together with error feedback (sr_seed and residual: pick one)")
    if codec_id not in wire.O.SR_CODECS:
        raise ValueError(f"stochastic rounding: bfp_rne and bfp4_rne only, got {wire.O.CODEC_NAMES.get(codec_id, codec_id)!r}"
                         f" (bfp_trunc is the reference's floor, a raw codec rounds nothing)")
    if prepacked:
        raise ValueError("stochastic rounding: not with prepacked input (the GEMM's encoding rounds to nearest)")
    if algo != "mesh":
        raise ValueError("stochastic rounding: mesh schedule only (the ring schedule is not supported yet)")
    if L.chunks > 1:
        raise ValueError("stochastic rounding: not with a chunked layout")
    if sharded:
        raise ValueError("stochastic rounding: not with a sharded-update engine")
    if world > MAX_PEERS:
        raise ValueError(f"stochastic rounding: at most {MAX_PEERS} ranks (one destination per shard), got {world}")
    if L.n_pad >= wire.O.SR_MAX_ELEMS:
        raise ValueError(f"stochastic rounding: a padded bucket of 2^32 or more elements ({L.n_pad}; element indices "
                         f"are 32-bit)")
    return wire.O.sr_seed_check(sr_seed)


def moment_request(moment_codec, moment_seed, mom, var, L, master, *, opt, trust_ratio=False, sharded=False):
    """Validate one request's ``moment_codec=`` (``"f32"``: today's planes, returns None; ``"bfp8"``: AdamW's two
    moments live in 8-bit block-floating-point planes, ``mom`` holding m and ``var`` sqrt(v), each a uint8 tensor of
    exactly ``L.n_pad * 17 / 16`` bytes — ``wire.moment_plane`` — stored with stochastic rounding under the 64-bit
    request seed ``moment_seed``, which every rank passes alike). Returns the seed as an int."""
    wire.O.moment_codec_check(moment_codec)
    if moment_codec == "f32":
        if moment_seed is not None:
            raise ValueError("moment_seed belongs to moment_codec='bfp8'")
        return None
    if opt == "lion":
        raise ValueError("moment_codec='bfp8': AdamW only (opt='lion' keeps its one moment plane in f32)")
    if opt != "adamw":
        raise ValueError("moment_codec='bfp8': AdamW only (opt='sgd' keeps no second moment; its momentum stays f32)")
    if trust_ratio:
        raise ValueError("moment_codec='bfp8': not with trust_ratio (LAMB's pass 2 recomputes the direction from the "
                         "stored moments)")
    if sharded:
        raise ValueError("moment_codec='bfp8': not with a sharded-update engine (its owner kernels keep f32 moment "
                         "shards)")
    if L.n_pad >= wire.O.SR_MAX_ELEMS:
        raise ValueError(f"moment_codec='bfp8': a padded bucket of 2^32 or more elements ({L.n_pad}; element indices "
                         f"are 32-bit)")
    if moment_seed is None:
        raise ValueError("moment_codec='bfp8' needs moment_seed, an int in [0, 2^64)")
    seed = wire.O.sr_seed_check(moment_seed)
    wire.moment_check(mom, master, L.n_pad, what="first-moment plane (mom)")
    wire.moment_check(var, master, L.n_pad, what="second-moment plane (var)")
    return seed


def lion_request(mom, var, *, lr, weight_decay, momentum, nesterov, betas, trust_ratio=False, device=None):
    """Validate one ``opt="lion"`` request; its ``bfp_oracle.LionScalars``. ``mom`` is Lion's one moment plane (f32,
    contiguous, laid out as master, on ``device`` where one is given); there is no second plane, no ``step`` (no bias
    correction; a value given is ignored) and no trust ratio."""
    if trust_ratio:
        raise ValueError("trust_ratio is a flag of opt='adamw' (a trust ratio on Lion is not provided)")
    if momentum or nesterov:
        raise ValueError("momentum / nesterov belong to SGD: Lion's moment is governed by betas")
    if var is not None:
        raise ValueError("Lion keeps one moment plane (mom): var must be None")
    if mom is None:
        raise ValueError("Lion needs its moment plane: mom (f32, laid out as master)")
    if mom.dtype != torch.float32 or not mom.is_contiguous():
        raise ValueError(f"Lion: mom must be a contiguous float32 tensor, got {mom.dtype}"
                         f"{'' if mom.is_contiguous() else ', not contiguous'}")
    if device is not None and (mom.device.type != torch.device(device).type or (
            mom.device.type == "cuda" and torch.device(device).index not in (None, mom.device.index))):
        raise ValueError(f"Lion: mom must be on the engine's device {device}, got {mom.device}")
    betas = resolve_betas("lion", betas)
    return wire.O.lion_scalars(lr, weight_decay, betas[0], betas[1])


def adamw_request(opt, mom, var, *, lr, weight_decay, momentum, nesterov, betas, eps, step, trust_ratio=False,
                  n_adapt=None, n_valid=None, device=None):
    """Validate one request's optimizer arguments; the step's ``bfp_oracle.AdamWScalars`` for ``opt="adamw"``
    (``mom`` the first moment, ``var`` the second, ``step`` the bucket's 1-based update count), the request's
    ``bfp_oracle.LionScalars`` for ``opt="lion"`` (:func:`lion_request`), None for SGD.
    ``trust_ratio`` (AdamW only): the layer-wise trust ratio (LAMB) over the bucket's first ``n_adapt`` of ``n_valid``
    elements; the scalars are then ``bfp_oracle.LambScalars``."""
    if opt not in OPTIMIZERS:
        raise ValueError(f"unknown optimizer {opt!r} (one of {OPTIMIZERS})")
    if opt == "lion":
        if n_adapt is not None:
            raise ValueError("n_adapt belongs to trust_ratio=True, a flag of opt='adamw'")
        return lion_request(mom, var, lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                            betas=betas, trust_ratio=trust_ratio, device=device)
    betas = resolve_betas(opt, betas)
    if trust_ratio and opt != "adamw":
        raise ValueError("trust_ratio is a flag of opt='adamw' (LARS on the SGD path is not provided)")
    if n_adapt is not None and not trust_ratio:
        raise ValueError("n_adapt belongs to trust_ratio=True")
    if trust_ratio and n_adapt is not None and not 0 <= int(n_adapt) <= int(n_valid):
        raise ValueError(f"n_adapt must lie in [0, n_valid = {n_valid}], got {n_adapt}")
    if opt == "sgd":
        return None
    if momentum or nesterov:
        raise ValueError("momentum / nesterov belong to SGD: AdamW's first moment is governed by betas[0]")
    if step is None:
        raise ValueError("AdamW needs step, the 1-based update count of the bucket")
    scalars = (wire.O.lamb_scalars if trust_ratio else wire.O.adamw_scalars)(lr, weight_decay, betas[0], betas[1],
                                                                               eps, step)
    if mom is None or var is None:
        raise ValueError("AdamW needs both moment planes: mom (first) and var (second)")
    return scalars


# ------------------------------------------------------------------------------------------ planning
def ring_geometry(n: int, world: int, max_slice_elems: int):
    C = _ext.load()
    if C is not None:
        return tuple(C.ring_geometry(int(n), int(world), int(max_slice_elems)))
    ms = max(256, max_slice_elems // 256 * 256)
    nn = max(n, 1)
    blocks = _cdiv(nn, world * ms)
    sl = _round_up(_cdiv(nn, world * blocks), 256)
    return (n, sl, blocks, blocks * world * sl)


def ring_plan(world: int, position: int, blocks: int):
    """List of [send_slice, send_src, recv_slice, recv_full, owned] rows (see csrc/comm/planner.h)."""
    C = _ext.load()
    if C is not None:
        return [list(r) for r in C.ring_plan(int(world), int(position), int(blocks))]
    return _py_ring_plan(world, position, blocks)


def _py_ring_plan(N, p, blocks):  # identical to csrc/comm/planner.cpp (used only without the extension)
    out = []
    for b in range(blocks):
        base = b * N
        if N == 1:
            out.append([base, 0, -1, 0, base])
            continue
        out.append([base + p % N, 0, base + (p + 1) % N, 0, -1])
        for k in range(1, N - 1):
            out.append([base + (p + k) % N, 1, base + (p + k + 1) % N, 0, -1])
        out.append([base + (p - 1) % N, 1, base + p % N, 1, base + (p - 1) % N])
        for i in range(1, N - 1):
            out.append([base + (p + i - 1) % N, 2, base + (p + i) % N, 1, -1])
    return out


def ring_orders(world: int, max_rings: int, links=None):
    """Arc-disjoint directed Hamiltonian rings (native planner); ``links[a][b]`` truthy: rank a has a direct link
    to rank b (None: fully connected)."""
    C = _ext.load()
    if C is not None:
        lk = None if links is None else [[int(bool(x)) for x in row] for row in links]
        return [list(o) for o in C.ring_orders(int(world), int(max_rings), lk)]
    return [list(range(world))]


@dataclass
class BucketLayout:
    n: int
    n_pad: int
    algo: str
    world: int
    shard: int = 0          # mesh: shard elements
    slice_elems: int = 0    # ring: slice elements
    blocks: int = 0         # ring: blocks per ring part
    rings: int = 1
    part: int = 0           # ring: padded elements per ring part
    chunks: int = 1         # mesh (C++ engine): chunks of `world` shards streamed through the collectives
    sub: int = 1            # ring (C++ engine, direct P2P): sub-slices per hop message (streamed hops)

    @property
    def key(self):
        return (self.n_pad, self.algo, self.world, self.shard, self.slice_elems, self.blocks, self.rings)


class Handle:
    """Async completion of one all-reduce request (reference: a done slot, sw:157-180)."""

    def __init__(self, engine, slot: int, event, name: str, pending=None):
        self.engine = engine
        self.slot = slot
        self.event = event
        self.name = name
        self.t_issue = time.time()
        self._pending = pending  # deferred epilogue thunks (see CompressedAllReduce.allreduce_sgd(defer=True))
        self._clip = None  # member of a clip group: dict(words, partials, count), see allreduce_sgd(clip=)

    def commit(self, update_after=None):
        """Enqueue the deferred weight-update epilogue, after ``update_after`` (an event on the producer
        stream marking the last read of the old weights, e.g. the bwd-data GEMM)."""
        if self._pending is None:
            return self
        if self._clip is not None:
            # its update needs the group's coefficient, which only commit_group computes: never a stale one
            raise ValueError(f"all-reduce '{self.name}' (slot {self.slot}) is a clipped request: it commits with its "
                             f"group through engine.commit_group ({CLIP_GROUP_LIMIT})")
        thunks, self._pending = self._pending, None
        self.event = self.engine._run_thunks(thunks, update_after)
        return self

    def commit_after_current(self):
        """commit() ordered after everything enqueued so far on the current stream."""
        ev = None
        if self._pending is not None and self.engine.cuda and not self.engine.inline:
            ev = self.engine._event()
            ev.record()
        return self.commit(update_after=ev)

    @property
    def pending(self) -> bool:
        """The deferred epilogue is not committed yet."""
        return self._pending is not None

    def done(self) -> bool:
        if self._pending is not None:
            return False
        return self.event is None or self.event.query()

    def latency_ms(self) -> float | None:
        """Device-side latency of the request (start of its comm phase -> end of the epilogue); requires
        ``engine.timing = True`` (the reference's get_all_reduce_latency(), sw/mlp_mpi_example_f32.cpp:100-106)."""
        t = getattr(self, "_timing", None)
        if t is None or self._pending is not None:
            return None
        t[1].synchronize()
        return t[0].elapsed_time(t[1])

    def wait(self, stream=None):
        """GPU-side wait: make ``stream`` (default: current) wait for completion; host does not block."""
        self.commit()
        if self.event is not None:
            (stream or torch.cuda.current_stream()).wait_event(self.event)

    def synchronize(self, timeout: float | None = None):
        """Host wait with a bounded timeout and diagnostics (never spins forever)."""
        self.commit()
        if self.event is None:
            return
        timeout = self.engine.timeout_s if timeout is None else timeout
        t0 = time.time()
        sleep = 1e-5
        while not self.event.query():
            err = self.engine.transport.async_error()
            if err:
                raise CommTimeoutError(f"all-reduce '{self.name}' (slot {self.slot}) failed: {err}")
            if time.time() - t0 > timeout:
                diag = self.engine.diagnostics(self)
                self.engine.transport.abort()
                raise CommTimeoutError(f"all-reduce '{self.name}' timed out after {timeout:.1f}s: {diag}")
            time.sleep(sleep)
            sleep = min(sleep * 2, 1e-3)


@dataclass
class _Scratch:
    tensors: dict = field(default_factory=dict)


class CompressedAllReduce:
    """Compressed (or raw) all-reduce + fused SGD over a :class:`Transport`."""

    def __init__(self, transport: Transport, *, codec: str = "bfp_rne", algo: str = "mesh", rings: int = 1,
                 max_slice_elems: int = 1 << 22, device=None, compat_owner_fp32: bool = False,
                 timeout_s: float = 600.0, stream=None, stream_priority: int = -1, force_comm: bool = False,
                 verify: bool | None = None):
        if algo not in ("mesh", "ring"):
            raise ValueError(f"unknown algo {algo!r}")
        self.transport = transport
        self.rank, self.world = transport.rank, transport.world
        self.codec = codec
        self.codec_id = wire.codec_id(codec)
        self.algo = algo
        self.max_slice_elems = max_slice_elems
        self.compat_owner_fp32 = compat_owner_fp32
        self.timeout_s = timeout_s
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        self.cuda = self.device.type == "cuda"
        self.orders = ring_orders(self.world, rings) if algo == "ring" else [list(range(self.world))]
        self.rings = len(self.orders)
        # world 1: nothing to overlap -> run inline on the caller's stream (no side stream, no event packets).
        # force_comm keeps the multi-rank code path (side stream, collectives) even at world 1.
        self.force_comm = force_comm
        self.inline = self.world == 1 and not force_comm
        if self.cuda and not self.inline:
            self.stream = stream or torch.cuda.Stream(device=self.device, priority=stream_priority)
        else:
            self.stream = None
        self._events: list = []
        self.timing = False  # per-request device timestamps (Handle.latency_ms)
        self._scratch: dict = {}
        self._cur_slot = 0
        self._slot = 0
        self._slot_owner: list = [None] * NUM_SLOTS  # last request issued on each slot
        self.fault = faults.FaultInjector.from_env()
        self.stats = {"requests": 0, "wire_bytes": 0, "logical_bytes": 0}
        # debug mode: every message travels with a checksum + the request sequence number,
        # verified on arrival (host-synchronous: for bisecting corruption / desync, not for speed)
        self.verify = bool(int(os.environ.get("FAN_VERIFY", "0"))) if verify is None else verify

    # -------------------------------------------------------------------------------- layout
    def layout(self, n: int) -> BucketLayout:
        N = self.world
        if self.algo == "mesh":
            shard = _round_up(max(_cdiv(n, N), 1), 256)
            return BucketLayout(n=n, n_pad=shard * N, algo="mesh", world=N, shard=shard)
        R = self.rings
        chunk = _cdiv(max(n, 1), R)
        _, sl, blocks, part = ring_geometry(chunk, N, self.max_slice_elems)
        return BucketLayout(n=n, n_pad=part * R, algo="ring", world=N, slice_elems=sl, blocks=blocks, rings=R,
                            part=part)

    def wire_bytes(self, L: BucketLayout) -> int:
        """Bytes this rank sends for one request (for bus-bandwidth accounting)."""
        N = self.world
        if N == 1:
            return 0
        if L.algo == "mesh":
            return 2 * (N - 1) * wire.shard_bytes(self.codec_id, L.shard)
        return L.rings * L.blocks * 2 * (N - 1) * wire.shard_bytes(self.codec_id, L.slice_elems)

    def _buf(self, L: BucketLayout, name: str, nbytes: int, dtype=torch.uint8, per_slot: bool = False):
        """Persistent scratch per bucket layout. ``per_slot``: a buffer a deferred epilogue reads — one per
        request slot, so a later same-size request cannot overwrite it before this request commits."""
        key = (L.key, name, self._cur_slot) if per_slot else (L.key, name)
        t = self._scratch.get(key)
        if t is None:
            t = torch.zeros(nbytes // torch.empty(0, dtype=dtype).element_size(), dtype=dtype, device=self.device)
            self._scratch[key] = t
        return t

    # -------------------------------------------------------------------------------- requests
    def allreduce_sgd(self, grad: torch.Tensor, master: torch.Tensor, lp: torch.Tensor | None = None,
                      mom: torch.Tensor | None = None, *, n_valid: int | None = None, lr: float,
                      grad_scale: float = 1.0, weight_decay: float = 0.0, momentum: float = 0.0,
                      nesterov: bool = False, update_after=None, defer: bool = False,
                      name: str = "bucket", opt: str = "sgd", var: torch.Tensor | None = None,
                      betas=None, eps: float = 1e-8, step: int | None = None, trust_ratio: bool = False,
                      n_adapt: int | None = None, trust_out: torch.Tensor | None = None,
                      clip: torch.Tensor | None = None, residual: torch.Tensor | None = None,
                      sr_seed: int | None = None, moment_codec: str = "f32",
                      moment_seed: int | None = None) -> Handle:
        """All-reduce ``grad`` (flat, padded to ``layout(n).n_pad``) and apply SGD to ``master`` (+bf16 ``lp``).
        ``opt="adamw"``: AdamW instead, ``mom`` / ``var`` the first / second moment planes (both required), ``step``
        the bucket's 1-based update count. ``trust_ratio`` (AdamW): scale the step of the bucket's first ``n_adapt``
        elements (default all ``n_valid``; the rest, a bias segment, take ratio 1) by ||w|| / ||update|| (LAMB): the
        epilogue becomes two passes around one norm reduction, and ``trust_out`` (3 f32, optional) receives
        {lr * phi, lr, phi}. ``clip`` (four f32 words on the engine's device; ``defer=True`` required): the request
        joins the clip group of those words — its communication phase ends with the norm pass over its reduced
        gradient, and ``commit_group`` computes the group's coefficient and commits its members. ``residual`` (f32,
        ``layout(n).n_pad`` elements, zeroed before the bucket's first request): error feedback — this rank's encoders
        (the sender's pack and the owner's re-encode) add it to their input and store what they dropped back into it;
        the gathered wire keeps its format, so every epilogue runs unchanged. Mesh schedule and BFP codecs only.
        ``sr_seed`` (an int in [0, 2^64); not with ``residual``): stochastic rounding — the same two encoders round up
        with probability equal to the dropped fraction (``bfp_oracle.sr_pack`` / ``sr_reduce``), stateless; every rank
        passes the same seed. Mesh schedule, ``bfp_rne`` / ``bfp4_rne`` only. ``moment_codec="bfp8"`` (AdamW): ``mom`` /
        ``var`` are 8-bit moment planes (``wire.moment_plane(layout(n).n_pad, device)``; ``var`` holds sqrt(v)) updated
        by ``wire.adamw_q`` under the request seed ``moment_seed``, on every schedule; not with ``trust_ratio``.
        ``opt="lion"``: Lion (``bfp_oracle.lion``), ``mom`` its one f32 moment plane (required; no ``var``, ``step``
        ignored), on every schedule and the sharded update; no ``trust_ratio``, no ``moment_codec="bfp8"``. ``betas``
        left unset: (0.9, 0.999) for AdamW, (0.9, 0.99) for Lion."""
        clip_request(clip, defer, self.device)
        if clip is not None and self.compat_owner_fp32 and self.algo == "ring":
            raise ValueError("clip: not with compat_owner_fp32 (the owner's slices would be updated from another "
                             "gradient than the one the norm was taken over)")
        n_valid = int(n_valid if n_valid is not None else master.numel())
        scalars = adamw_request(opt, mom, var, lr=lr, weight_decay=weight_decay, momentum=momentum,
                                nesterov=nesterov, betas=betas, eps=eps, step=step, trust_ratio=trust_ratio,
                                n_adapt=n_adapt, n_valid=n_valid, device=self.device)
        lamb = isinstance(scalars, wire.O.LambScalars)
        lion = isinstance(scalars, wire.O.LionScalars)
        if lamb and self.compat_owner_fp32 and self.algo == "ring":
            raise ValueError("trust_ratio: not with compat_owner_fp32 (the owner's slices would be updated from "
                             "another gradient than the one the norms were taken over)")
        n_adapt = n_valid if n_adapt is None else int(n_adapt)
        L = self.layout(n_valid)
        self._check(grad, L)
        mq_seed = moment_request(moment_codec, moment_seed, mom, var, L, master, opt=opt, trust_ratio=trust_ratio,
                                 sharded=bool(getattr(self, "shard_update", False)))
        sr_seed = sr_request(sr_seed, L, codec_id=self.codec_id, algo=self.algo, world=self.world, residual=residual)
        residual = residual_request(residual, L, codec_id=self.codec_id, algo=self.algo, world=self.world,
                                    device=self.device)
        sgd_kw = dict(lr=lr, grad_scale=grad_scale, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov)
        tr = dict(pairs=0, regions=[])  # trust ratio: the regions pass 1 has run over, for the ratio and pass 2
        cl = None if clip is None else dict(words=clip.view(-1), partials=None, count=0, norm=True)

        def update(G, shard, n_shards, off, length, nv, codec, skip=(-1, 0)):
            if cl is not None and cl["norm"]:  # the norm pass over this region (at the tail of the comm phase)
                cl["count"] += wire.sumsq(G, shard, n_shards, codec=codec, partials=cl["partials"],
                                          partials_base=cl["count"], n_valid=nv, skip_shard=skip[0],
                                          skip_period=skip[1])
                return
            if mq_seed is not None:  # 8-bit state: the planes go whole, the region's offset addresses them
                wire.adamw_q(G, shard, n_shards, master.view(-1)[off:off + length], codec=codec, mom_q=mom.view(-1),
                             var_q=var.view(-1), scalars=scalars, seed=mq_seed,
                             lp=None if lp is None else lp.view(-1)[off:off + length], grad_scale=grad_scale,
                             n_valid=nv, skip_shard=skip[0], skip_period=skip[1],
                             clip=None if cl is None else cl["words"], elem_base=off)
                return
            planes = dict(lp=None if lp is None else lp.view(-1)[off:off + length],
                          mom=None if mom is None else mom.view(-1)[off:off + length],
                          clip=None if cl is None else cl["words"])
            if lamb:
                adapt = max(0, min(n_adapt - off, nv))
                tr["pairs"] += wire.lamb_moments(G, shard, n_shards, master.view(-1)[off:off + length], codec=codec,
                                                 mom=planes["mom"], var=var.view(-1)[off:off + length],
                                                 scalars=scalars, partials=tr["partials"], partials_base=tr["pairs"],
                                                 grad_scale=grad_scale, n_valid=nv, n_adapt=adapt,
                                                 skip_shard=skip[0], skip_period=skip[1], clip=planes["clip"])
                tr["regions"].append((shard, off, length, nv, adapt, skip))
            elif lion:
                wire.lion(G, shard, n_shards, master.view(-1)[off:off + length], codec=codec, scalars=scalars,
                          grad_scale=grad_scale, n_valid=nv, skip_shard=skip[0], skip_period=skip[1], **planes)
            elif scalars is not None:
                wire.adamw(G, shard, n_shards, master.view(-1)[off:off + length], codec=codec,
                           var=var.view(-1)[off:off + length], scalars=scalars, grad_scale=grad_scale, n_valid=nv,
                           skip_shard=skip[0], skip_period=skip[1], **planes)
            else:
                wire.sgd(G, shard, n_shards, master.view(-1)[off:off + length], codec=codec, n_valid=nv,
                         skip_shard=skip[0], skip_period=skip[1], **planes, **sgd_kw)

        def finish(G, shard, n_shards, off, length, skip=(-1, 0)):
            nv = max(0, min(n_valid - off, length))
            if nv == 0:
                return
            update(G, shard, n_shards, off, length, nv, self.codec_id, skip)

        def owner_fp32(buf, off, length):  # compat: owner applies the update from the un-quantised fp32 sum
            nv = max(0, min(n_valid - off, length))
            if nv:
                update(buf, length, 1, off, length, nv, "raw_f32")

        def lamb_finish():  # after every region's pass 1: one ratio over all their partials, then their pass 2
            wire.lamb_ratio(tr["partials"], tr["pairs"], lr, tr["words"])
            for shard, off, length, nv, adapt, skip in tr["regions"]:
                wire.lamb_apply(master.view(-1)[off:off + length], shard, mom=mom.view(-1)[off:off + length],
                                var=var.view(-1)[off:off + length], scalars=scalars, words=tr["words"],
                                lp=None if lp is None else lp.view(-1)[off:off + length], n_valid=nv, n_adapt=adapt,
                                skip_shard=skip[0], skip_period=skip[1])

        def clipped(thunks):
            # the region thunks run once now, as norm passes (one partials segment per region: one for mesh, one per
            # ring), on the stream of the communication phase; at commit they run again as the update
            cap = wire.sumsq_partials_for(master, 1 << 40)
            cl["partials"] = self._buf(L, "clip_partials", 8 * cap * max(1, self.rings), torch.float64, per_slot=True)
            for t in thunks:
                t()
            cl["norm"] = False
            return thunks

        def comm():
            if cl is not None:
                thunks = clipped(list(self._run(L, grad, finish, owner_fp32, residual=residual, sr_seed=sr_seed)))
                if not lamb:
                    return thunks
            elif not lamb:
                return self._run(L, grad, finish, owner_fp32, residual=residual, sr_seed=sr_seed)
            # one partials segment per region a schedule hands to finish(): one (mesh), or one per ring
            cap = wire.lamb_partials_for(master, 1 << 40)
            tr["partials"] = self._buf(L, "lamb_partials", 16 * cap * max(1, self.rings), torch.float64, per_slot=True)
            tr["words"] = trust_out.view(-1) if trust_out is not None else \
                self._buf(L, "lamb_words", 12, torch.float32, per_slot=True)
            if cl is not None:
                return thunks + [lamb_finish]
            return list(self._run(L, grad, finish, owner_fp32, residual=residual, sr_seed=sr_seed)) + [lamb_finish]

        h = self._launch(comm, name, L, defer, update_after)
        h._clip = cl
        return h

    def commit_group(self, handles, *, max_norm: float, grad_scale: float = 1.0, update_after=None):
        """Commit the clip group ``handles`` (deferred requests submitted with the same ``clip=`` words, at most 8,
        all of one optimizer step): one coefficient launch over the members' norm partials in the order given —
        ``words = {min(1, max_norm / (||g|| * |grad_scale| + 1e-6)), ||g|| * |grad_scale|, max_norm, nonfinite}`` with
        ||g|| the 2-norm of the reduced gradient over every member (``bfp_oracle.clip_words``) — then each member's
        update with ``grad_scale * words[0]``, after ``update_after`` (default: after everything enqueued so far on the
        current stream). ``grad_scale``: the members' common value."""
        handles = list(handles)
        words = clip_group_check(handles, max_norm)
        for h in handles:
            if h.engine is not self:
                raise ValueError("commit_group: a request of another engine")
        segments = [(h._clip["partials"], 0, h._clip["count"]) for h in handles]
        if update_after is None and self.cuda and not self.inline:
            # after everything enqueued so far on the current stream (the bwd-data GEMMs that still read the weights)
            update_after = self._event()
            update_after.record()

        def coef():
            wire.clip_coef(segments, max_norm, grad_scale, words)

        for i, h in enumerate(handles):
            thunks, h._pending = h._pending, None
            # one stream runs every member: the coefficient first, then the members in order
            h.event = self._run_thunks(([coef] if i == 0 else []) + list(thunks), update_after if i == 0 else None)
        return handles

    def allreduce(self, grad: torch.Tensor, out: torch.Tensor, *, n_valid: int | None = None,
                  name: str = "bucket", residual: torch.Tensor | None = None, sr_seed: int | None = None) -> Handle:
        """Sum-only all-reduce: decoded result written to ``out`` (f32 or bf16, same padded length). ``residual``: the
        bucket's error-feedback plane, ``sr_seed``: the request's stochastic-rounding seed, as :meth:`allreduce_sgd`."""
        n_valid = int(n_valid if n_valid is not None else grad.numel())
        L = self.layout(n_valid)
        self._check(grad, L)
        sr_seed = sr_request(sr_seed, L, codec_id=self.codec_id, algo=self.algo, world=self.world, residual=residual)
        residual = residual_request(residual, L, codec_id=self.codec_id, algo=self.algo, world=self.world,
                                    device=self.device)

        def finish(G, shard, n_shards, off, length, skip=(-1, 0)):
            wire.unpack(G, out.view(-1)[off:off + length], shard, self.codec_id)

        def owner_fp32(buf, off, length):
            pass

        return self._launch(lambda: self._run(L, grad, finish, owner_fp32, allow_compat=False, residual=residual,
                                              sr_seed=sr_seed), name, L, False, None)

    def _check(self, grad, L):
        if grad.numel() < L.n_pad:
            raise ValueError(f"gradient buffer has {grad.numel()} elements; layout needs {L.n_pad} (use "
                             f"engine.layout(n).n_pad to size flat buffers)")
        if grad.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("gradients must be f32 or bf16")

    def _launch(self, comm_fn, name, L, defer=False, update_after=None) -> Handle:
        slot = self._slot
        self._slot = (slot + 1) % NUM_SLOTS
        prev = self._slot_owner[slot]
        if prev is not None and prev._pending is not None:
            # more than NUM_SLOTS requests deferred: the slot's previous request must commit before its per-slot
            # scratch is reused (ordered after everything enqueued so far on the producer stream)
            if prev._clip is not None:  # (its coefficient does not exist yet: never update with a stale one)
                self._slot = slot
                raise ValueError(f"all-reduce '{name}': slot {slot} still holds the clipped request '{prev.name}': "
                                 f"{CLIP_GROUP_LIMIT}")
            prev.commit_after_current()
            self.stats["forced_commits"] = self.stats.get("forced_commits", 0) + 1
        self._cur_slot = slot  # per-slot scratch of the request comm_fn builds
        self.stats["requests"] += 1
        self.stats["wire_bytes"] += self.wire_bytes(L)
        self.stats["logical_bytes"] += L.n * 4
        if not self.cuda or self.inline:
            thunks = comm_fn()
            h = Handle(self, slot, None, name, pending=thunks)
            self._slot_owner[slot] = h
            return h if defer else h.commit()
        ready = self._event()
        ready.record(torch.cuda.current_stream(self.device))
        t_start = None
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ready)
            if self.timing:
                t_start = torch.cuda.Event(enable_timing=True)
                t_start.record(self.stream)
            thunks = comm_fn()
        if t_start is not None:
            t_end = torch.cuda.Event(enable_timing=True)
            thunks = list(thunks) + [lambda: t_end.record(self.stream)]
        h = Handle(self, slot, None, name, pending=thunks)
        self._slot_owner[slot] = h
        if t_start is not None:
            h._timing = (t_start, t_end)
        return h if defer else h.commit(update_after)

    def _event(self):
        """Events are recycled round-robin (a pool deeper than the requests in flight)."""
        if len(self._events) < 4 * NUM_SLOTS:
            e = torch.cuda.Event()
            self._events.append(e)
            return e
        e = self._events.pop(0)
        self._events.append(e)
        return e

    def _run_thunks(self, thunks, update_after=None):
        if not self.cuda or self.inline:
            for t in thunks:
                t()
            return None
        with torch.cuda.stream(self.stream):
            if update_after is not None:
                self.stream.wait_event(update_after)
            for t in thunks:
                t()
            done = self._event()
            done.record(self.stream)
        return done

    def _tag(self, rows: torch.Tensor) -> torch.Tensor:
        """[k, 3] int64: checksum of each byte row + the request sequence number."""
        seq = torch.full((rows.shape[0], 1), self.stats["requests"], dtype=torch.int64, device=rows.device)
        return torch.cat([_checksum(rows), seq], 1)

    def _verify_rows(self, rows, tags, peers, what):
        got = _checksum(rows).cpu()
        tags = tags.cpu()
        for i, peer in enumerate(peers):
            if int(tags[i, 2]) != self.stats["requests"]:
                raise ChecksumError(f"rank {self.rank}: {what}: message from peer {peer} belongs to request "
                                    f"#{int(tags[i, 2])}, expected #{self.stats['requests']} (out of order)")
            if not torch.equal(got[i], tags[i, :2]):
                raise ChecksumError(f"rank {self.rank}: {what}: message from peer {peer} is corrupted "
                                    f"(checksum {got[i].tolist()} != {tags[i, :2].tolist()}, request "
                                    f"#{self.stats['requests']})")

    def diagnostics(self, h: Handle) -> str:
        return (f"rank={self.rank} world={self.world} algo={self.algo} codec={self.codec} rings={self.rings} "
                f"slot={h.slot} elapsed={time.time() - h.t_issue:.1f}s transport={self.transport.name} "
                f"async_error={self.transport.async_error()!r}")

    # -------------------------------------------------------------------------------- execution
    def _run(self, L, grad, finish, owner_fp32, allow_compat=True, residual=None, sr_seed=None):
        """Issue the communication phase; returns the epilogue thunks (run now or at commit)."""
        if L.algo == "mesh":
            return self._mesh(L, grad, finish, residual, sr_seed)
        return self._ring(L, grad, finish, owner_fp32, allow_compat)

    def _mesh(self, L, grad, finish, residual=None, sr_seed=None):
        N, r, s, c = self.world, self.rank, L.shard, self.codec_id
        sb = wire.shard_bytes(c, s)
        g = grad.view(-1)[: L.n_pad]
        # Error feedback: `residual` (residual_request: f32, n_pad elements, a BFP codec) is read and written here
        # only, by the kernels of this request's communication phase on the stream it runs on — the comm stream, whose
        # order puts step t's owner-stage store before step t + 1's pack (CPU / inline: the caller's own order). The
        # sender stage writes every shard but r, the owner stage shard r: disjoint parts of the plane.
        e = residual
        # Stochastic rounding: `sr` (sr_request: an rne BFP codec, never with `residual`) swaps the same two encoders
        # for their stateless stochastic forms — sender r under key (sr, r, 0), owner r under key (sr, r, 1).
        sr = sr_seed
        S = self._buf(L, "mesh_S", sb, per_slot=N == 1 and not self.force_comm)
        if N == 1 and not self.force_comm:
            if e is not None:
                wire.reduce_ef(S, 1, 0, g[:s], e[:s], S, s, c)
            elif sr is not None:
                wire.reduce_sr(S, 1, 0, g[:s], S, s, c, sr, 0)
            else:
                wire.reduce(S, 1, 0, g[:s], S, None, s, c)
            return [lambda: finish(S, s, 1, 0, s)]
        if c == 2 and g.dtype == torch.float32:
            P = wire.as_bytes(g)
        elif c == 3 and g.dtype == torch.bfloat16:
            P = wire.as_bytes(g)
        else:
            P = self._buf(L, "mesh_P", sb * N)
            if e is not None:
                wire.pack_ef(g, e[: L.n_pad], P, s, c, self_shard=r)
            elif sr is not None:
                wire.pack_sr(g, P, s, c, sr, r, self_shard=r)
            else:
                wire.pack(g, P, s, c)
        cs = self._tag(P.view(N, sb)) if self.verify else None
        self.fault.maybe_corrupt("mesh_pack", P)
        R = self._buf(L, "mesh_R", sb * N)
        self.transport.all_to_all(P, R)
        if cs is not None:
            cs_r = torch.empty_like(cs)
            self.transport.all_to_all(cs, cs_r)
            self._verify_rows(R.view(N, sb), cs_r, list(range(N)), "mesh all_to_all")
        if e is not None:
            wire.reduce_ef(R, N, r, g[r * s:(r + 1) * s], e[r * s:(r + 1) * s], S, s, c)
        elif sr is not None:
            wire.reduce_sr(R, N, r, g[r * s:(r + 1) * s], S, s, c, sr, r, base=r * s)
        else:
            wire.reduce(R, N, r, g[r * s:(r + 1) * s], S, None, s, c)
        G = self._buf(L, "mesh_G", sb * N, per_slot=True)
        self.transport.all_gather(S, G)
        if self.verify:
            cs_g = torch.empty(N, 3, dtype=torch.int64, device=G.device)
            self.transport.all_gather(self._tag(S.view(1, sb)), cs_g)
            self._verify_rows(G.view(N, sb), cs_g, list(range(N)), "mesh all_gather")
        return [lambda: finish(G, s, N, 0, L.n_pad)]

    def _ring(self, L, grad, finish, owner_fp32, allow_compat):
        N, c = self.world, self.codec_id
        S = L.slice_elems
        sb = wire.shard_bytes(c, S)
        nsl = L.blocks * N
        g = grad.view(-1)
        compat = allow_compat and self.compat_owner_fp32 and N > 1
        rings = []
        for i, order in enumerate(self.orders):
            pos = order.index(self.rank)
            rings.append(dict(
                off=i * L.part,
                down=order[(pos - 1) % N], up=order[(pos + 1) % N], pos=pos,
                plan=ring_plan(N, pos, L.blocks),
                G=self._buf(L, f"ring_G{i}", sb * nsl, per_slot=True),
                send=self._buf(L, f"ring_send{i}", sb),
                recv=[self._buf(L, f"ring_recv{i}_0", sb), self._buf(L, f"ring_recv{i}_1", sb)],
                last_partial=None,
                fp32=self._buf(L, f"ring_fp32_{i}", 4 * S * L.blocks, torch.float32, per_slot=True) if compat else None,
            ))
        nrows = len(rings[0]["plan"])
        # group rows into communication rounds: a SEND_LOCAL row joins the previous round (OUTPUT_SEND overlap)
        rounds, cur = [], []
        for j in range(nrows):
            if cur and not (rings[0]["plan"][j][1] == 0 and j > 0):
                rounds.append(cur)
                cur = []
            cur.append(j)
        if cur:
            rounds.append(cur)

        def local(ring, x):
            o = ring["off"] + x * S
            return g[o:o + S]

        checks = []
        for ri, rnd in enumerate(rounds):
            sends, recvs = [], []
            for j in rnd:
                for ring in rings:
                    send_slice, src, recv_slice, recv_full, owned = ring["plan"][j]
                    Gs = lambda x, ring=ring: ring["G"][x * sb:(x + 1) * sb]  # noqa: E731
                    out = None
                    if src == 0:  # SEND_LOCAL
                        out = Gs(send_slice) if owned >= 0 else ring["send"]
                        wire.pack(local(ring, send_slice), out, S, c)
                    elif src == 1:  # REDUCE / REDUCE_OUTPUT
                        out = Gs(send_slice) if owned >= 0 else ring["send"]
                        f32 = None
                        if compat and owned >= 0:
                            blk = owned // N
                            f32 = ring["fp32"][blk * S:(blk + 1) * S]
                        wire.reduce(ring["last_partial"], 2, 1, local(ring, send_slice), out, f32, S, c)
                    elif src == 2:  # FORWARD (already-encoded full slice)
                        out = Gs(send_slice)
                    if out is not None and N > 1:
                        cs = self._tag(out.view(1, sb)) if self.verify else None
                        self.fault.maybe_corrupt("ring_send", out)
                        sends.append((out, ring["down"]))
                        if cs is not None:
                            sends.append((cs, ring["down"]))
                    if recv_slice >= 0:
                        if recv_full:
                            tgt = Gs(recv_slice)
                        else:
                            tgt = ring["recv"][j % 2]
                            ring["last_partial"] = tgt
                        recvs.append((tgt, ring["up"]))
                        if self.verify:
                            cs_r = torch.empty(1, 3, dtype=torch.int64, device=tgt.device)
                            recvs.append((cs_r, ring["up"]))
                            checks.append((tgt, cs_r, ring["up"], f"ring round {ri} slice {recv_slice}"))
            if N > 1:
                self.transport.sendrecv(sends, recvs)
                for tgt, cs_r, peer, what in checks:
                    self._verify_rows(tgt.view(1, sb), cs_r, [peer], what)
                checks.clear()
        thunks = []
        for i, ring in enumerate(rings):
            off = ring["off"]
            if compat:
                own = (ring["pos"] - 1) % N
                thunks.append(lambda ring=ring, off=off, own=own: finish(ring["G"], S, nsl, off, L.part,
                                                                        skip=(own, N)))
                for b in range(L.blocks):
                    x = b * N + own
                    thunks.append(lambda ring=ring, b=b, x=x, off=off: owner_fp32(
                        ring["fp32"][b * S:(b + 1) * S], off + x * S, S))
            else:
                thunks.append(lambda ring=ring, off=off: finish(ring["G"], S, nsl, off, L.part))
        return thunks


def uncompressed_allreduce_sgd(transport: Transport, grad, master, lp=None, mom=None, *, n_valid=None, lr,
                               grad_scale=1.0, weight_decay=0.0, momentum=0.0, nesterov=False, opt="sgd", var=None,
                               betas=(0.9, 0.999), eps=1e-8, step=None, trust_ratio=False):
    """Baseline: RCCL all-reduce (sum) of the raw gradients + a separate SGD (or AdamW) kernel (BASELINE config 2;
    the reference's commented MPI_Iallreduce + libxsmm opt path, sw:615-647)."""
    if trust_ratio:
        raise ValueError("trust_ratio belongs to the compressed engines' two-pass epilogue; the uncompressed baseline "
                         "has a single update kernel")
    if opt == "lion":
        raise ValueError("opt='lion' belongs to the compressed engines' epilogues; the uncompressed baseline offers "
                         "SGD and AdamW")
    scalars = adamw_request(opt, mom, var, lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                            betas=betas, eps=eps, step=step)
    transport.all_reduce_(grad)
    n_valid = master.numel() if n_valid is None else n_valid
    n = _round_up(n_valid, 256)
    codec = "raw_f32" if grad.dtype == torch.float32 else "raw_bf16"
    if scalars is not None:
        wire.adamw(wire.as_bytes(grad.view(-1)[:n]) if grad.numel() >= n else wire.as_bytes(grad), n, 1,
                   master.view(-1), codec=codec, lp=None if lp is None else lp.view(-1), mom=mom.view(-1),
                   var=var.view(-1), scalars=scalars, grad_scale=grad_scale, n_valid=n_valid)
        return
    wire.sgd(wire.as_bytes(grad.view(-1)[:n]) if grad.numel() >= n else wire.as_bytes(grad), n, 1,
             master.view(-1), codec=codec, lp=None if lp is None else lp.view(-1),
             mom=None if mom is None else mom.view(-1), lr=lr, grad_scale=grad_scale, weight_decay=weight_decay,
             momentum=momentum, nesterov=nesterov, n_valid=n_valid)
