"""Wire-format ops of the all-reduce engine: pack / unpack / reduce / fused SGD epilogue.

GPU tensors run the hand-written CDNA4 kernels of ``csrc/bfp/bfp_kernels.hip`` (a missing extension is
a hard error on GPU). CPU tensors run the bit-exact NumPy oracle (``bfp_oracle``) so that the gloo
multi-process tests exercise exactly the same numerics as the GPU path.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _ext
from . import bfp_oracle as O

CODEC_IDS = O.CODECS


def codec_id(codec) -> int:
    return O.codec_id(codec)


def is_raw(codec) -> bool:
    return codec_id(codec) in (2, 3)


def shard_bytes(codec, n_s: int) -> int:
    return O.shard_bytes(codec, n_s)


def _np_f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.float32).contiguous().view(-1).numpy()


def _np_u8(t: torch.Tensor) -> np.ndarray:
    return t.detach().contiguous().view(torch.uint8).view(-1).numpy()


def as_bytes(t: torch.Tensor) -> torch.Tensor:
    """uint8 view of a contiguous tensor (zero copy)."""
    return t.contiguous().view(torch.uint8).view(-1)


def pack(x: torch.Tensor, out: torch.Tensor, shard_elems: int, codec) -> torch.Tensor:
    """Encode dense x (f32/bf16, numel % shard_elems == 0) into ``out`` (uint8)."""
    c = codec_id(codec)
    if x.is_cuda:
        _ext.require().wire_pack(x, out, int(shard_elems), c)
        return out
    buf = O.pack(_np_f32(x), shard_elems, c)
    out.view(-1)[: buf.size].copy_(torch.from_numpy(buf))
    return out


def unpack(packed: torch.Tensor, out: torch.Tensor, shard_elems: int, codec) -> torch.Tensor:
    c = codec_id(codec)
    if out.is_cuda:
        _ext.require().wire_unpack(packed, out, int(shard_elems), c)
        return out
    v = O.unpack(_np_u8(packed), out.numel(), shard_elems, c)
    out.view(-1).copy_(torch.from_numpy(v).to(out.dtype))
    return out


def reduce(slots: torch.Tensor, n_slots: int, self_pos: int, local: torch.Tensor | None,
           out_wire: torch.Tensor | None, out_f32: torch.Tensor | None, shard_elems: int, codec):
    """Sum ``n_slots`` wire shards stored back to back in ``slots`` (slot ``self_pos`` replaced by the
    dense ``local`` operand when given) and write the result as wire (``out_wire``) and/or f32."""
    c = codec_id(codec)
    if slots.is_cuda:
        _ext.require().wire_reduce(slots, int(n_slots), int(self_pos), local, out_wire, out_f32,
                                   int(shard_elems), c)
        return
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(slots)
    slot_list = [raw[r * sb:(r + 1) * sb] for r in range(n_slots)]
    acc = O.reduce_slots(slot_list, None if local is None else _np_f32(local), self_pos, c, shard_elems)
    if out_f32 is not None:
        out_f32.view(-1)[:shard_elems].copy_(torch.from_numpy(acc))
    if out_wire is not None:
        buf = O.pack(acc, shard_elems, c)
        as_bytes(out_wire)[: buf.size].copy_(torch.from_numpy(buf))


def _ef_check(residual: torch.Tensor, need: int, ref: torch.Tensor, codec) -> int:
    c = codec_id(codec)
    if c not in O.BFP_CODECS:
        raise ValueError(f"error feedback: BFP codecs only, got {O.CODEC_NAMES.get(c, c)!r} (a raw codec drops "
                         f"nothing)")
    if not (isinstance(residual, torch.Tensor) and residual.dtype == torch.float32 and residual.is_contiguous()):
        raise ValueError("error feedback: the residual plane is a contiguous float32 tensor")
    if residual.device != ref.device:
        raise ValueError(f"error feedback: the residual plane lives on {residual.device}, the gradient on {ref.device}")
    if residual.numel() < need:
        raise ValueError(f"error feedback: the residual plane has {residual.numel()} elements, the request needs {need}")
    return c


def pack_ef(x: torch.Tensor, residual: torch.Tensor, out, shard_elems: int, codec, self_shard: int = -1):
    """:func:`pack` with error feedback (``bfp_oracle.ef_pack``): every shard but ``self_shard`` is encoded from
    ``x + residual`` and the f32 ``residual`` plane (x.numel() elements, updated in place) keeps what the codec dropped;
    shard ``self_shard`` is encoded from x alone and its residual slice is left alone. ``out``: one uint8 buffer
    (shards back to back), or a list with one uint8 buffer per shard — a ``None`` entry skips that shard entirely
    (neither encoded nor fed back; at most 16 shards either way on the GPU)."""
    n_shards = x.numel() // shard_elems
    if x.numel() % shard_elems:
        raise ValueError("numel must be a multiple of shard_elems")
    c = _ef_check(residual, x.numel(), x, codec)
    sb = O.shard_bytes(c, shard_elems)
    dsts = list(out) if isinstance(out, (list, tuple)) else [as_bytes(out)[q * sb:(q + 1) * sb] for q in range(n_shards)]
    if len(dsts) != n_shards:
        raise ValueError("one destination per shard")
    if x.is_cuda:
        _ext.require().wire_pack_ef(x, residual, dsts, int(shard_elems), c, int(self_shard))
        return out
    e = residual.view(-1).numpy()
    g = _np_f32(x)
    for q, d in enumerate(dsts):
        if d is None:
            continue
        sl = slice(q * shard_elems, (q + 1) * shard_elems)
        buf, e2 = O.ef_pack(g[sl], e[sl], shard_elems, c, 0 if q == self_shard else -1)
        e[sl] = e2
        as_bytes(d)[:sb].copy_(torch.from_numpy(buf))
    return out


def reduce_ef(slots: torch.Tensor, n_slots: int, self_pos: int, local: torch.Tensor, residual: torch.Tensor,
              out_wire, shard_elems: int, codec):
    """:func:`reduce` to wire with error feedback (``bfp_oracle.ef_reduce``): the slots' sum (slot ``self_pos`` from the
    dense ``local``, required) plus the f32 ``residual`` shard is encoded into ``out_wire`` — one uint8 buffer or a
    list of them (``None`` entries skipped), each receiving the same bytes — and ``residual`` (shard_elems elements,
    updated in place) keeps what that encode dropped."""
    if local is None:
        raise ValueError("reduce_ef: the dense local operand is required")
    c = _ef_check(residual, shard_elems, local, codec)
    dsts = list(out_wire) if isinstance(out_wire, (list, tuple)) else [out_wire]
    if slots.is_cuda:
        _ext.require().wire_reduce_ef(slots, int(n_slots), int(self_pos), local, residual, dsts, int(shard_elems), c)
        return
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(slots)
    slot_list = [raw[r * sb:(r + 1) * sb] for r in range(n_slots)]
    e = residual.view(-1).numpy()
    buf, e2 = O.ef_reduce(slot_list, _np_f32(local), self_pos, e[:shard_elems], c, shard_elems)
    e[:shard_elems] = e2
    for d in dsts:
        if d is not None:
            as_bytes(d)[:sb].copy_(torch.from_numpy(buf))


def _sr_check(codec, seed, rank: int, base: int, n: int) -> tuple[int, int]:
    c = O.sr_codec(codec)
    seed = O.sr_seed_check(seed)
    if not 0 <= int(rank) < 16:
        raise ValueError(f"stochastic rounding: rank in [0, 16), got {rank}")
    if base < 0 or base % 16 or base + n > O.SR_MAX_ELEMS:
        raise ValueError(f"stochastic rounding: elements [{base}, {base + n}) of a padded bucket of 2^32 or more "
                         f"elements (element indices are 32-bit, base a multiple of 16)")
    return c, seed


def pack_sr(x: torch.Tensor, out, shard_elems: int, codec, seed: int, rank: int, self_shard: int = -1, base: int = 0,
            peers: bool = False):
    """:func:`pack` with stochastic rounding (``bfp_oracle.sr_pack``; ``bfp_rne`` / ``bfp4_rne``): every shard but
    ``self_shard`` (plain rne) is encoded with key (seed, rank, 0); element j of x is element ``base + j`` of the
    padded bucket. ``out``: one uint8 buffer (shards back to back), or a list with one uint8 buffer per shard — a
    ``None`` entry skips that shard (at most 16 shards either way on the GPU). ``peers`` (GPU): launch as the
    direct-P2P engine does, under its grid cap and release mode; the bits do not depend on it."""
    n_shards = x.numel() // shard_elems
    if x.numel() % shard_elems:
        raise ValueError("numel must be a multiple of shard_elems")
    c, seed = _sr_check(codec, seed, rank, int(base), x.numel())
    sb = O.shard_bytes(c, shard_elems)
    dsts = list(out) if isinstance(out, (list, tuple)) else [as_bytes(out)[q * sb:(q + 1) * sb] for q in range(n_shards)]
    if len(dsts) != n_shards:
        raise ValueError("one destination per shard")
    if x.is_cuda:
        _ext.require().wire_pack_sr(x, dsts, int(shard_elems), c, seed, int(rank), int(self_shard), int(base),
                                    bool(peers))
        return out
    g = _np_f32(x)
    for q, d in enumerate(dsts):
        if d is None:
            continue
        sl = slice(q * shard_elems, (q + 1) * shard_elems)
        buf = O.sr_pack(g[sl], shard_elems, c, seed, rank, 0 if q == self_shard else -1, int(base) + q * shard_elems)
        as_bytes(d)[:sb].copy_(torch.from_numpy(buf))
    return out


def reduce_sr(slots: torch.Tensor, n_slots: int, self_pos: int, local: torch.Tensor, out_wire, shard_elems: int,
              codec, seed: int, rank: int, base: int = 0, peers: bool = False):
    """:func:`reduce` to wire with stochastic rounding (``bfp_oracle.sr_reduce``): the slots' sum (slot ``self_pos``
    from the dense ``local``, required) is encoded with key (seed, rank, 1) into ``out_wire`` — one uint8 buffer or a
    list of them (``None`` entries skipped), each receiving the same bytes. ``base``: the shard's first element in the
    padded bucket; ``peers`` as :func:`pack_sr`."""
    if local is None:
        raise ValueError("reduce_sr: the dense local operand is required")
    c, seed = _sr_check(codec, seed, rank, int(base), shard_elems)
    dsts = list(out_wire) if isinstance(out_wire, (list, tuple)) else [out_wire]
    if slots.is_cuda:
        _ext.require().wire_reduce_sr(slots, int(n_slots), int(self_pos), local, dsts, int(shard_elems), c, seed,
                                      int(rank), int(base), bool(peers))
        return
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(slots)
    slot_list = [raw[r * sb:(r + 1) * sb] for r in range(n_slots)]
    buf = O.sr_reduce(slot_list, _np_f32(local), self_pos, c, shard_elems, seed, rank, int(base))
    for d in dsts:
        if d is not None:
            as_bytes(d)[:sb].copy_(torch.from_numpy(buf))


def sgd(wire: torch.Tensor, shard_elems: int, n_shards: int, master: torch.Tensor, *, codec,
        lp: torch.Tensor | None = None, mom: torch.Tensor | None = None, lr: float, grad_scale: float = 1.0,
        weight_decay: float = 0.0, momentum: float = 0.0, nesterov: bool = False, n_valid: int | None = None,
        skip_shard: int = -1, skip_period: int = 0, clip: torch.Tensor | None = None):
    """Fused decode + SGD in place: master -= lr * (scale * g [+ wd * w], momentum); lp = bf16(master).
    ``clip``: a clip group's four f32 words (:func:`clip_coef`); the update then uses the one f32 product
    ``grad_scale * clip[0]`` (``bfp_oracle.clip_scale``) in place of ``grad_scale``."""
    c = codec_id(codec)
    n_valid = master.numel() if n_valid is None else int(n_valid)
    if master.is_cuda:
        _ext.require().wire_sgd(wire, int(shard_elems), int(n_shards), int(skip_shard), int(skip_period), master,
                                lp, mom, float(lr), float(grad_scale), float(weight_decay), float(momentum),
                                bool(nesterov), n_valid, c, clip)
        return
    if clip is not None:
        grad_scale = O.clip_scale(grad_scale, _np_f32(clip))
    n = shard_elems * n_shards
    g = O.unpack(_np_u8(wire), n, shard_elems, c)
    w = master.view(-1).numpy()
    m = mom.view(-1).numpy() if mom is not None else None
    period = skip_period if skip_period >= 1 else (1 << 30)
    for s in range(n_shards):
        if skip_shard >= 0 and s % period == skip_shard:
            continue
        lo, hi = s * shard_elems, min((s + 1) * shard_elems, n_valid)
        if hi <= lo:
            continue
        nw, nm = O.sgd(w[lo:hi], g[lo:hi], lr, grad_scale, weight_decay, momentum,
                       None if m is None else m[lo:hi], nesterov)
        w[lo:hi] = nw
        if m is not None and nm is not None:
            m[lo:hi] = nm
    if lp is not None:
        lp.view(-1)[:n_valid].copy_(master.view(-1)[:n_valid].to(lp.dtype))


def adamw(wire: torch.Tensor, shard_elems: int, n_shards: int, master: torch.Tensor, *, codec,
          mom: torch.Tensor, var: torch.Tensor, scalars: O.AdamWScalars, lp: torch.Tensor | None = None,
          grad_scale: float = 1.0, n_valid: int | None = None, skip_shard: int = -1, skip_period: int = 0,
          shard_stride: int = 0, clip: torch.Tensor | None = None):
    """Fused decode + AdamW in place (``bfp_oracle.adamw``'s arithmetic): ``mom`` / ``var`` are the first / second
    moment planes, ``scalars`` the step's ``bfp_oracle.adamw_scalars``; lp = bf16(master). ``shard_stride``: bytes
    between consecutive wire shards (0: packed). ``clip``: as :func:`sgd`."""
    c = codec_id(codec)
    if mom is None or var is None:
        raise ValueError("AdamW needs both moment planes (mom, var)")
    if not isinstance(scalars, O.AdamWScalars):
        raise TypeError(f"wire.adamw takes bfp_oracle.adamw_scalars, got {type(scalars).__name__}")
    n_valid = master.numel() if n_valid is None else int(n_valid)
    if master.is_cuda:
        _ext.require().wire_adamw(wire, int(shard_elems), int(n_shards), int(skip_shard), int(skip_period), master,
                                  lp, mom, var, scalars.kernel_args(), float(grad_scale), float(scalars.wd), n_valid,
                                  c, int(shard_stride), clip)
        return
    if clip is not None:
        grad_scale = O.clip_scale(grad_scale, _np_f32(clip))
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(wire)
    if shard_stride:
        raw = np.concatenate([raw[s * shard_stride: s * shard_stride + sb] for s in range(n_shards)])
    n = shard_elems * n_shards
    g = O.unpack(raw, n, shard_elems, c)
    w = master.view(-1).numpy()
    m = mom.view(-1).numpy()
    v = var.view(-1).numpy()
    period = skip_period if skip_period >= 1 else (1 << 30)
    for s in range(n_shards):
        if skip_shard >= 0 and s % period == skip_shard:
            continue
        lo, hi = s * shard_elems, min((s + 1) * shard_elems, n_valid)
        if hi <= lo:
            continue
        w[lo:hi], m[lo:hi], v[lo:hi] = O.adamw(w[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], scalars, grad_scale)
        if lp is not None:
            lp.view(-1)[lo:hi].copy_(master.view(-1)[lo:hi].to(lp.dtype))


def lion(wire: torch.Tensor, shard_elems: int, n_shards: int, master: torch.Tensor, *, codec,
         mom: torch.Tensor, scalars: O.LionScalars, lp: torch.Tensor | None = None, grad_scale: float = 1.0,
         n_valid: int | None = None, skip_shard: int = -1, skip_period: int = 0, shard_stride: int = 0,
         clip: torch.Tensor | None = None):
    """Fused decode + Lion in place (``bfp_oracle.lion``'s arithmetic): ``mom`` is the one moment plane (f32, laid out
    as master), ``scalars`` the request's ``bfp_oracle.lion_scalars``; lp = bf16(master). On the GPU master and mom hold
    ``n_valid`` rounded up to 8 elements (the kernel's lane trip). ``shard_stride`` and ``clip``: as :func:`adamw`."""
    c = codec_id(codec)
    if mom is None:
        raise ValueError("Lion needs its moment plane (mom)")
    if not isinstance(scalars, O.LionScalars):
        raise TypeError(f"wire.lion takes bfp_oracle.lion_scalars, got {type(scalars).__name__}")
    n_valid = master.numel() if n_valid is None else int(n_valid)
    if master.is_cuda:
        _ext.require().wire_lion(wire, int(shard_elems), int(n_shards), int(skip_shard), int(skip_period), master,
                                 lp, mom, scalars.kernel_args(), float(grad_scale), n_valid, c, int(shard_stride),
                                 clip)
        return
    if clip is not None:
        grad_scale = O.clip_scale(grad_scale, _np_f32(clip))
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(wire)
    if shard_stride:
        raw = np.concatenate([raw[s * shard_stride: s * shard_stride + sb] for s in range(n_shards)])
    n = shard_elems * n_shards
    g = O.unpack(raw, n, shard_elems, c)
    w = master.view(-1).numpy()
    m = mom.view(-1).numpy()
    period = skip_period if skip_period >= 1 else (1 << 30)
    for s in range(n_shards):
        if skip_shard >= 0 and s % period == skip_shard:
            continue
        lo, hi = s * shard_elems, min((s + 1) * shard_elems, n_valid)
        if hi <= lo:
            continue
        w[lo:hi], m[lo:hi] = O.lion(w[lo:hi], g[lo:hi], m[lo:hi], scalars, grad_scale)
        if lp is not None:
            lp.view(-1)[lo:hi].copy_(master.view(-1)[lo:hi].to(lp.dtype))


def moment_plane(n_pad: int, device) -> torch.Tensor:
    """A zeroed 8-bit moment plane (the zero state) of a padded bucket of ``n_pad`` elements: uint8,
    ``n_pad * 17 / 16`` bytes (``bfp_oracle.moment_plane_bytes``)."""
    return torch.zeros(O.moment_plane_bytes(n_pad), dtype=torch.uint8, device=device)


def moment_check(plane, ref: torch.Tensor, n_pad: int | None = None, what: str = "moment plane") -> int:
    """Validate one 8-bit moment plane against the tensor it updates (``ref``: its device) and, when given, the
    bucket's ``n_pad``; returns the plane's element count."""
    if not (isinstance(plane, torch.Tensor) and plane.dtype == torch.uint8):
        raise ValueError(f"moment_codec bfp8: the {what} is a uint8 tensor, got "
                         f"{getattr(plane, 'dtype', type(plane).__name__)}")
    if not plane.is_contiguous():
        raise ValueError(f"moment_codec bfp8: the {what} must be contiguous")
    if plane.device != ref.device:
        raise ValueError(f"moment_codec bfp8: the {what} lives on {plane.device}, the weights on {ref.device}")
    nb = plane.numel()
    if nb % (17 * 16) or (n_pad is not None and nb != O.moment_plane_bytes(n_pad)):
        want = "n_pad * 17 / 16" if n_pad is None else f"exactly n_pad * 17 / 16 = {O.moment_plane_bytes(n_pad)}"
        raise ValueError(f"moment_codec bfp8: the {what} has {nb} bytes, not {want}")
    if plane.data_ptr() % 16:
        raise ValueError(f"moment_codec bfp8: the {what} must be 16-byte aligned (a slice of a larger tensor may not be)")
    n = nb // 17 * 16
    O.moment_plane_bytes(n)  # (refuses 2^32 elements or more)
    return n


def moment_decode(plane: torch.Tensor) -> torch.Tensor:
    """The f32 values of a whole 8-bit moment plane (``bfp_oracle.moment_decode``), on the plane's device."""
    n = moment_check(plane, plane)
    out = torch.empty(n, dtype=torch.float32, device=plane.device)
    if n:
        unpack(plane, out, n, "bfp_rne")
    return out


def adamw_q(wire: torch.Tensor, shard_elems: int, n_shards: int, master: torch.Tensor, *, codec,
            mom_q: torch.Tensor, var_q: torch.Tensor, scalars: O.AdamWScalars, seed: int,
            lp: torch.Tensor | None = None, grad_scale: float = 1.0, n_valid: int | None = None,
            skip_shard: int = -1, skip_period: int = 0, shard_stride: int = 0, clip: torch.Tensor | None = None,
            elem_base: int = 0):
    """:func:`adamw` with both moments in 8-bit block floating point (``bfp_oracle.adamw_q`` defines the bits):
    ``mom_q`` / ``var_q`` are the bucket's whole planes (:func:`moment_plane`; the second holds sqrt(v)), ``seed`` the
    request's 64-bit seed of the state's stochastic rounding, ``elem_base`` (a multiple of 256) the bucket index of the
    wire region's element 0. ``codec`` is the *wire's*; the other arguments are :func:`adamw`'s."""
    c = codec_id(codec)
    if c not in O.CODEC_NAMES:
        raise ValueError(f"unknown wire codec {codec!r}")
    if not isinstance(scalars, O.AdamWScalars):
        raise TypeError(f"wire.adamw_q takes bfp_oracle.adamw_scalars, got {type(scalars).__name__}")
    seed = O.sr_seed_check(seed)
    n_pad = moment_check(mom_q, master, what="first-moment plane")
    moment_check(var_q, master, n_pad, what="second-moment plane")
    n_valid = master.numel() if n_valid is None else int(n_valid)
    n = shard_elems * n_shards
    elem_base = int(elem_base)
    if shard_elems <= 0 or shard_elems % 256 or n_shards <= 0 or not 0 <= n_valid <= n:
        raise ValueError(f"adamw_q: {n_shards} shards of {shard_elems} elements (a multiple of 256), n_valid {n_valid}")
    if elem_base < 0 or elem_base % 256 or elem_base + n_valid > n_pad:
        raise ValueError(f"adamw_q: elem_base {elem_base} must be a multiple of 256 with the region's {n_valid} valid "
                         f"elements inside the planes' {n_pad}")
    if master.is_cuda:
        _ext.require().wire_adamw_q(wire, int(shard_elems), int(n_shards), int(skip_shard), int(skip_period), master,
                                    lp, mom_q, var_q, scalars.kernel_args(), float(grad_scale), float(scalars.wd),
                                    seed, n_valid, c, int(shard_stride), clip, elem_base)
        return
    if clip is not None:
        grad_scale = O.clip_scale(grad_scale, _np_f32(clip))
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(wire)
    if shard_stride:
        raw = np.concatenate([raw[s * shard_stride: s * shard_stride + sb] for s in range(n_shards)])
    g = O.unpack(raw, n, shard_elems, c)
    w = master.view(-1).numpy()
    mq, vq = mom_q.view(-1).numpy(), var_q.view(-1).numpy()
    period = skip_period if skip_period >= 1 else (1 << 30)
    for s in range(n_shards):
        if skip_shard >= 0 and s % period == skip_shard:
            continue
        lo, hi = s * shard_elems, min((s + 1) * shard_elems, n_valid)
        if hi <= lo:
            continue
        top = lo + -(-(hi - lo) // 16) * 16          # whole groups: the oracle zeroes the tail of the last one
        wpad = np.zeros(top - lo, np.float32)
        wpad[:hi - lo] = w[lo:hi]
        w2, mq[:], vq[:] = O.adamw_q(wpad, g[lo:top], mq, vq, scalars, grad_scale, seed, hi - lo, elem_base + lo)
        w[lo:hi] = w2[:hi - lo]
        if lp is not None:
            lp.view(-1)[lo:hi].copy_(master.view(-1)[lo:hi].to(lp.dtype))


def _lamb_ranges(shard_elems, n_shards, n_valid, skip_shard, skip_period):
    """The flat [lo, hi) ranges one trust-ratio launch covers: every shard but the skipped ones, cut at n_valid."""
    period = skip_period if skip_period >= 1 else (1 << 30)
    out = []
    for s in range(n_shards):
        if skip_shard >= 0 and s % period == skip_shard:
            continue
        lo, hi = s * shard_elems, min((s + 1) * shard_elems, n_valid)
        if hi > lo:
            out.append((lo, hi))
    return out


def _sum64(x: np.ndarray) -> float:
    """Exactly rounded float64 sum (math.fsum); a non-finite term gives numpy's non-finite sum instead of an error."""
    if np.isfinite(x).all():
        return math.fsum(x)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(x))


def lamb_partials_for(master: torch.Tensor, shard_elems: int) -> int:
    """{S_w, S_r} pairs one :func:`lamb_moments` launch over shards of ``shard_elems`` writes (CPU: one)."""
    return int(_ext.require().lamb_partials_for(int(shard_elems))) if master.is_cuda else 1


def lamb_moments(wire: torch.Tensor, shard_elems: int, n_shards: int, master: torch.Tensor, *, codec,
                 mom: torch.Tensor, var: torch.Tensor, scalars: O.LambScalars, partials: torch.Tensor,
                 partials_base: int = 0, grad_scale: float = 1.0, n_valid: int | None = None,
                 n_adapt: int | None = None, skip_shard: int = -1, skip_period: int = 0, shard_stride: int = 0,
                 clip: torch.Tensor | None = None) -> int:
    """Pass 1 of the trust-ratio (LAMB) update (``bfp_oracle.lamb_moments``): decode the wire, store the new moments
    in ``mom`` / ``var``, leave ``master`` untouched, and write the launch's fp64 partial sums of w^2 and r^2 over the
    flat elements below ``n_adapt`` (default ``n_valid``) as {S_w, S_r} pairs from pair ``partials_base`` of
    ``partials`` (float64). Returns the pairs written (:func:`lamb_partials_for`); :func:`lamb_ratio` sums the pairs of
    every launch of a request. ``clip``: as :func:`sgd` (the moments take the clipped gradient)."""
    c = codec_id(codec)
    if mom is None or var is None:
        raise ValueError("the trust-ratio update needs both moment planes (mom, var)")
    n_valid = master.numel() if n_valid is None else int(n_valid)
    n_adapt = n_valid if n_adapt is None else int(n_adapt)
    if not 0 <= n_adapt <= n_valid:
        raise ValueError(f"n_adapt must lie in [0, n_valid = {n_valid}], got {n_adapt}")
    if master.is_cuda:
        return int(_ext.require().wire_lamb_moments(wire, int(shard_elems), int(n_shards), int(skip_shard),
                                                    int(skip_period), master, mom, var, scalars.kernel_args(),
                                                    float(grad_scale), n_valid, n_adapt, partials,
                                                    int(partials_base), c, int(shard_stride), clip))
    if clip is not None:
        grad_scale = O.clip_scale(grad_scale, _np_f32(clip))
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(wire)
    if shard_stride:
        raw = np.concatenate([raw[s * shard_stride: s * shard_stride + sb] for s in range(n_shards)])
    g = O.unpack(raw, shard_elems * n_shards, shard_elems, c)
    w, m, v = master.view(-1).numpy(), mom.view(-1).numpy(), var.view(-1).numpy()
    sw, sr = [], []
    for lo, hi in _lamb_ranges(shard_elems, n_shards, n_valid, skip_shard, skip_period):
        m[lo:hi], v[lo:hi], r = O.lamb_moments(w[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], scalars, grad_scale)
        k = max(0, min(n_adapt, hi) - lo)
        sw.append(w[lo:lo + k].astype(np.float64) ** 2)
        sr.append(r[:k].astype(np.float64) ** 2)
    tot = [_sum64(np.concatenate(x)) if x else 0.0 for x in (sw, sr)]
    partials.view(-1)[2 * partials_base: 2 * partials_base + 2] = torch.tensor(tot, dtype=torch.float64)
    return 1


def lamb_ratio(partials: torch.Tensor, n_pairs: int, lr: float, words: torch.Tensor):
    """Sum ``n_pairs`` {S_w, S_r} pairs in float64 and write the three f32 words {lr * phi, lr, phi}
    (``bfp_oracle.lamb_words``) into ``words``."""
    if partials.is_cuda:
        _ext.require().lamb_ratio(partials, int(n_pairs), float(lr), words)
        return
    p = partials.view(-1)[: 2 * n_pairs].numpy()
    sums = [_sum64(x) for x in (p[0::2], p[1::2])]
    words.view(-1)[:3] = torch.from_numpy(O.lamb_words(sums[0], sums[1], lr))


def lamb_apply(master: torch.Tensor, shard_elems: int, *, mom: torch.Tensor, var: torch.Tensor,
               scalars: O.LambScalars, words: torch.Tensor, lp: torch.Tensor | None = None,
               n_valid: int | None = None, n_adapt: int | None = None, skip_shard: int = -1, skip_period: int = 0):
    """Pass 2 (``bfp_oracle.lamb_apply``): master -= (i < n_adapt ? words[0] : words[1]) * r over [0, n_valid), r
    recomputed from the moments pass 1 stored; lp = bf16(master). Shards (of ``shard_elems``) that pass 1 skipped
    are skipped alike."""
    n_valid = master.numel() if n_valid is None else int(n_valid)
    n_adapt = n_valid if n_adapt is None else int(n_adapt)
    if not 0 <= n_adapt <= n_valid:
        raise ValueError(f"n_adapt must lie in [0, n_valid = {n_valid}], got {n_adapt}")
    if master.is_cuda:
        _ext.require().wire_lamb_apply(master, lp, mom, var, scalars.kernel_args(), words, int(shard_elems),
                                       int(skip_shard), int(skip_period), n_valid, n_adapt)
        return
    w, m, v = master.view(-1).numpy(), mom.view(-1).numpy(), var.view(-1).numpy()
    wd = words.view(-1)[:3].numpy()
    n_shards = -(-n_valid // shard_elems)
    for lo, hi in _lamb_ranges(shard_elems, n_shards, n_valid, skip_shard, skip_period):
        w[lo:hi] = O.lamb_apply(w[lo:hi], m[lo:hi], v[lo:hi], scalars, wd, max(0, min(n_adapt, hi) - lo))
        if lp is not None:
            lp.view(-1)[lo:hi].copy_(master.view(-1)[lo:hi].to(lp.dtype))


def sumsq_partials_for(ref: torch.Tensor, shard_elems: int) -> int:
    """fp64 partials one :func:`sumsq` launch over shards of ``shard_elems`` writes (CPU: one); ``ref``: any tensor
    on the device the launch runs on."""
    return int(_ext.require().sumsq_partials_for(int(shard_elems))) if ref.is_cuda else 1


def sumsq(wire: torch.Tensor, shard_elems: int, n_shards: int, *, codec, partials: torch.Tensor,
          partials_base: int = 0, n_valid: int | None = None, skip_shard: int = -1, skip_period: int = 0,
          shard_stride: int = 0) -> int:
    """The norm pass of a clip group over one gathered wire region (``bfp_oracle.clip_sumsq``): float64 partial sums
    of the squares of the decoded values over the flat elements [0, n_valid) (:func:`sgd`'s traversal: skipped shards,
    ``shard_stride``), written from ``partials[partials_base]``. Returns the partials written
    (:func:`sumsq_partials_for`); :func:`clip_coef` sums the segments of every request of the group."""
    c = codec_id(codec)
    n_valid = shard_elems * n_shards if n_valid is None else int(n_valid)
    if wire.is_cuda:
        return int(_ext.require().wire_sumsq(wire, int(shard_elems), int(n_shards), int(skip_shard),
                                             int(skip_period), n_valid, partials, int(partials_base), c,
                                             int(shard_stride)))
    sb = O.shard_bytes(c, shard_elems)
    raw = _np_u8(wire)
    if shard_stride:
        raw = np.concatenate([raw[s * shard_stride: s * shard_stride + sb] for s in range(n_shards)])
    g = O.unpack(raw, shard_elems * n_shards, shard_elems, c)
    parts = [g[lo:hi] for lo, hi in _lamb_ranges(shard_elems, n_shards, n_valid, skip_shard, skip_period)]
    partials.view(-1)[partials_base] = O.clip_sumsq(np.concatenate(parts)) if parts else 0.0
    return 1


def clip_coef(segments, max_norm: float, grad_scale: float, words: torch.Tensor):
    """The coefficient of a clip group: sum the ``segments`` — (partials, base, count) triples, one per request, at
    most 8, in order — in float64 and write the four f32 words {coef, f32(total), f32(max_norm), nonfinite}
    (``bfp_oracle.clip_words``) into ``words``."""
    segments = [(p, int(b), int(k)) for p, b, k in segments]
    max_norm = float(max_norm)
    if not (max_norm > 0 and math.isfinite(max_norm)):
        raise ValueError(f"max_norm must be finite and positive, got {max_norm}")
    if len(segments) > 8:
        raise ValueError(f"a clip group holds at most 8 partial segments, got {len(segments)}")
    if words.is_cuda:
        _ext.require().clip_coef([p for p, _, _ in segments], [b for _, b, _ in segments],
                                 [k for _, _, k in segments], max_norm, float(grad_scale), words)
        return
    terms = [p.view(-1)[b:b + k].numpy() for p, b, k in segments if k]
    S = _sum64(np.concatenate(terms)) if terms else 0.0
    words.view(-1)[:4] = torch.from_numpy(O.clip_words(S, grad_scale, max_norm))
