"""Bit-exact NumPy oracles for the BFP wire format (the ground truth every kernel is tested against).

Two numerics are modelled:

* ``trunc`` — the reference NIC, bit for bit (NX_MODE=0, MANT_SIZE=8, group 16):
  encode = hw/bf16_to_bfp_core.sv:97-126 + hw/bfp_adapter.sv:145-154 (shared exponent = max biased exponent,
  hidden bit forced to 1 even for zeros/denormals, right shift with shifts >= 32 clearing
  (hw/barrel_shifter.sv:44-51), 25-bit two's complement, keep bits [24:17] => floor);
  decode = hw/bfp_to_bf16_core.sv:55-117 (magnitude |q|<<16 with |-128| = 128, exponent field
  E + 1 - lzc24 wrapping mod 256, mantissa bit 0 forced to 0; so q = 0 decodes to 2^(E-150)).
* ``rne`` — this framework's default: q = clamp(rint(x * 2^(133-E)), -127, 127), decode q * 2^(E-133)
  (exact zero, symmetric range, half the error bound of truncation). E = 255 (Inf/NaN in the group)
  decodes to NaN so corrupted gradients fail loudly.

``bfp4_rne`` is the ``rne`` form at a 4-bit mantissa (the reference's MANT_SIZE knob; it ships no such configuration,
so there is no truncating form): q = clamp(rint(x * 2^(129-E)), -7, 7), decode q * 2^(E-129), E = 255 -> NaN.

Packed layout of a shard of n_s elements (n_s % 256 == 0): ``[int8 mant[n_s]][uint8 exp[n_s/16]]``;
``bfp4_rne``: ``[uint8 nib[n_s/2]][uint8 exp[n_s/16]]``, byte i of a group's 8 holding value 2i in bits [3:0] and
value 2i+1 in bits [7:4] (two's complement nibbles). Multi-shard buffers are shards back to back.
"""
from __future__ import annotations

import math

import numpy as np

GROUP = 16
CODECS = {"bfp_trunc": 0, "bfp_rne": 1, "raw_f32": 2, "raw_bf16": 3, "bfp4_rne": 4}
BFP_CODECS = (0, 1, 4)  # a shared exponent per group of 16; (0, 1) are the 8-bit ones the GEMM epilogues encode
CODEC_NAMES = {v: k for k, v in CODECS.items()}


def codec_id(codec) -> int:
    if isinstance(codec, str):
        return CODECS[codec]
    return int(codec)


def shard_bytes(codec, n_s: int) -> int:
    c = codec_id(codec)
    if c in (0, 1):
        return n_s + n_s // 16
    if c == 4:
        return n_s // 2 + n_s // 16
    return n_s * (4 if c == 2 else 2)


# --------------------------------------------------------------------------- bf16 helpers
def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """RNE fp32 -> bf16 (NaN preserving), returned as uint16."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = np.isnan(np.ascontiguousarray(x, dtype=np.float32))
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r = np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)
    return r.astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# --------------------------------------------------------------------------- group primitives
def _shared_exp(bits: np.ndarray) -> np.ndarray:
    """bits: uint32 [G, 16] -> E uint32 [G, 1] (max biased exponent of the group)."""
    return (((bits & 0x7FFFFFFF).max(axis=1, keepdims=True)) >> 23).astype(np.uint32)


def encode_groups(x: np.ndarray, rounding: str = "rne"):
    """x: float32 [..] (size % 16 == 0) -> (q int8 [n], E uint8 [n/16])."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, GROUP)
    bits = x.view(np.uint32)
    E = _shared_exp(bits)
    if rounding == "trunc":
        e = (bits >> 23) & 0xFF
        m = ((bits & 0x7FFFFF) | 0x800000).astype(np.int64)
        d = (E - e).astype(np.int64)  # 0..255 (E >= e)
        a = np.where(d >= 32, 0, m >> np.minimum(d, 31))
        t = np.where((bits >> 31) == 1, -a, a)
        q = (t >> 17).astype(np.int8)
    elif rounding in ("rne", "rne4"):
        top, lim = (133, 127.0) if rounding == "rne" else (129, 7.0)
        with np.errstate(over="ignore", invalid="ignore"):
            s = np.ldexp(x, (top - E.astype(np.int32)))
            s = np.rint(s)
            s = np.clip(np.nan_to_num(s, nan=-lim, posinf=lim, neginf=-lim), -lim, lim)
        q = s.astype(np.int8)
    else:
        raise ValueError(rounding)
    return q.reshape(-1), E.reshape(-1).astype(np.uint8)


def decode_groups(q: np.ndarray, E: np.ndarray, rounding: str = "rne") -> np.ndarray:
    q = np.asarray(q, dtype=np.int8).reshape(-1, GROUP).astype(np.int32)
    Eu = np.asarray(E, dtype=np.uint8).reshape(-1, 1).astype(np.uint32)
    if rounding == "trunc":
        sign = (q < 0).astype(np.uint32)
        M = (np.abs(q).astype(np.uint32)) << 16  # |-128| = 128 -> 2^23
        # 24-bit leading-zero count (24 for 0)
        zc = np.where(M == 0, 24, 23 - np.floor(np.log2(np.maximum(M, 1))).astype(np.int64)).astype(np.uint32)
        ex = (Eu + 1 - zc) & 0xFF
        frac = (M << zc) & 0x7FFFFE
        bits = (sign << 31) | (ex << 23) | frac
        return bits.astype(np.uint32).view(np.float32).reshape(-1)
    if rounding in ("rne", "rne4"):
        with np.errstate(over="ignore"):  # (E = 255 decodes to NaN below)
            v = np.ldexp(q.astype(np.float32), Eu.astype(np.int32) - (133 if rounding == "rne" else 129))
        v = np.where(Eu == 255, np.float32(np.nan), v)
        return v.reshape(-1).astype(np.float32)
    raise ValueError(rounding)


def _rounding_of(codec) -> str:
    c = codec_id(codec)
    return "trunc" if c == 0 else "rne4" if c == 4 else "rne"


def pack_nibbles(q: np.ndarray) -> np.ndarray:
    """int8 values in [-8, 7] (even count) -> uint8, value 2i in bits [3:0] of byte i and value 2i+1 in bits [7:4]."""
    u = np.asarray(q, dtype=np.int8).reshape(-1).view(np.uint8) & 0xF
    return (u[0::2] | (u[1::2] << 4)).astype(np.uint8)


def unpack_nibbles(b: np.ndarray) -> np.ndarray:
    """The inverse of :func:`pack_nibbles`: uint8 [n/2] -> sign-extended int8 [n]."""
    b = np.asarray(b, dtype=np.uint8).reshape(-1)
    u = np.stack([b & 0xF, b >> 4], 1).reshape(-1).astype(np.int16)
    return np.where(u >= 8, u - 16, u).astype(np.int8)


# --------------------------------------------------------------------------- packed buffers
def pack(x: np.ndarray, shard_elems: int, codec="bfp_rne") -> np.ndarray:
    """Dense f32 (or bf16 given as float32 values) -> packed uint8 buffer (per-shard layout)."""
    c = codec_id(codec)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    assert x.size % shard_elems == 0 and shard_elems % 256 == 0
    if c == 2:
        return x.view(np.uint8).copy()
    if c == 3:
        return f32_to_bf16_bits(x).view(np.uint8).copy()
    out = []
    for s in range(x.size // shard_elems):
        q, E = encode_groups(x[s * shard_elems:(s + 1) * shard_elems], _rounding_of(c))
        out.append(pack_nibbles(q) if c == 4 else q.view(np.uint8))
        out.append(E)
    return np.concatenate(out)


def unpack(buf: np.ndarray, n: int, shard_elems: int, codec="bfp_rne") -> np.ndarray:
    c = codec_id(codec)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    if c == 2:
        return buf[: 4 * n].view(np.float32).copy()
    if c == 3:
        return bf16_bits_to_f32(buf[: 2 * n].view(np.uint16))
    sb = shard_bytes(c, shard_elems)
    out = []
    for s in range(n // shard_elems):
        sh = buf[s * sb:(s + 1) * sb]
        nm = shard_elems // 2 if c == 4 else shard_elems
        q = unpack_nibbles(sh[:nm]) if c == 4 else sh[:nm].view(np.int8)
        out.append(decode_groups(q, sh[nm:], _rounding_of(c)))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def quantize(x: np.ndarray, codec="bfp_rne") -> np.ndarray:
    """decode(encode(x)) for a dense vector (size % 16 == 0)."""
    c = codec_id(codec)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if c == 2:
        return x.copy()
    if c == 3:
        return bf16_bits_to_f32(f32_to_bf16_bits(x))
    q, E = encode_groups(x, _rounding_of(c))
    return decode_groups(q, E, _rounding_of(c))


def reduce_slots(slots, local=None, self_pos: int = -1, codec="bfp_rne", shard_elems: int | None = None):
    """Sum decoded slots (packed single-shard buffers) in slot order, with the dense ``local`` operand
    standing in for slot ``self_pos``. Returns the float32 sum (the caller re-encodes)."""
    c = codec_id(codec)
    n = shard_elems
    acc = np.zeros(n, np.float32)
    nslots = len(slots)
    for r in range(nslots):
        if local is not None and r == self_pos:
            v = np.asarray(local, np.float32).reshape(-1)[:n]
        else:
            v = unpack(slots[r], n, n, c)
        acc = (acc + v).astype(np.float32)
    return acc


# --------------------------------------------------------------------------- error feedback
def _ef_codec(codec) -> int:
    c = codec_id(codec)
    if c not in BFP_CODECS:
        raise ValueError(f"error feedback: BFP codecs only, got {CODEC_NAMES.get(c, c)!r} (a raw codec drops nothing)")
    return c


def ef_pack(g: np.ndarray, e: np.ndarray, shard_elems: int, codec="bfp_rne", self_shard: int = -1):
    """Sender stage of the error-fed mesh all-reduce over a bucket of shards of ``shard_elems`` elements: every shard
    but ``self_shard`` is encoded from ``x = f32(g) + e`` (one f32 add, the group exponent taken from x) and keeps
    ``e' = x - dec(enc(x))`` (one f32 subtract, ``dec`` the decoder's real output); shard ``self_shard`` (-1: none) is
    encoded from g alone and its slice of e is left as it is. Returns (wire uint8, e' float32); e is not modified."""
    c = _ef_codec(codec)
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    e2 = np.array(e, dtype=np.float32).reshape(-1)
    assert g.size % shard_elems == 0 and shard_elems % 256 == 0 and e2.size >= g.size
    out = []
    for q in range(g.size // shard_elems):
        sl = slice(q * shard_elems, (q + 1) * shard_elems)
        if q == self_shard:
            out.append(pack(g[sl], shard_elems, c))
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            x = (g[sl] + e2[sl]).astype(np.float32)
            out.append(pack(x, shard_elems, c))
            e2[sl] = (x - quantize(x, c)).astype(np.float32)
    return np.concatenate(out), e2


def ef_reduce(slots, local, self_pos: int, e_shard: np.ndarray, codec="bfp_rne", shard_elems: int | None = None):
    """Owner stage: ``acc`` = :func:`reduce_slots` (slot order, slot ``self_pos`` from the dense ``local``), then
    ``y = acc + e_shard`` (one f32 add after the slot sum), the output wire ``enc(y)`` and
    ``e_shard' = y - dec(enc(y))``. Returns (wire uint8, e_shard' float32)."""
    c = _ef_codec(codec)
    n = shard_elems
    acc = reduce_slots(slots, local, self_pos, c, n)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (acc + np.asarray(e_shard, np.float32).reshape(-1)[:n]).astype(np.float32)
        return pack(y, n, c), (y - quantize(y, c)).astype(np.float32)


# --------------------------------------------------------------------------- stochastic rounding
# The rne codecs' encoders with an unbiased rounding: q = floor(t) + (frac(t) > u), u a counter-based random threshold.
# One 32-bit hash word serves the 4 consecutive elements 4w..4w+3 of the padded bucket (a byte each), keyed by the
# request's seed, the encoding rank and the stage, so the bits depend on nothing but (seed, rank, stage, element).
SR_CODECS = (1, 4)          # bfp_rne, bfp4_rne (the trunc codec is the reference's floor: nothing to randomise)
SR_MAX_ELEMS = 1 << 32      # element indices are 32-bit
_M32 = 0xFFFFFFFF
_M64 = (1 << 64) - 1


def sr_codec(codec) -> int:
    c = codec_id(codec)
    if c not in SR_CODECS:
        raise ValueError(f"stochastic rounding: bfp_rne and bfp4_rne only, got {CODEC_NAMES.get(c, c)!r}")
    return c


def sr_seed_check(seed) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"stochastic rounding: the seed is an int in [0, 2^64), got {seed!r}")
    seed = int(seed)
    if not 0 <= seed <= _M64:
        raise ValueError(f"stochastic rounding: the seed is an int in [0, 2^64), got {seed}")
    return seed


def _sr_mix(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def sr_hash(k0: int, k1: int, w) -> np.ndarray:
    """h(k0, k1, w) = mix(mix(w ^ k0) + k1) on uint32 with wraparound (w: word indices, any shape)."""
    w = np.asarray(w, dtype=np.uint32)
    with np.errstate(over="ignore"):
        return _sr_mix(_sr_mix(w ^ np.uint32(k0 & _M32)) + np.uint32(k1 & _M32))


def sr_key(seed: int, rank: int, stage: int) -> tuple[int, int]:
    """The two key words of (request seed, encoding rank, stage: 0 the sender's pack, 1 the owner's re-encode)."""
    seed = sr_seed_check(seed)
    return seed & _M32, (seed >> 32) ^ (((2 * int(rank) + int(stage) + 1) * 0x9E3779B9) & _M32)


def sr_step_seed(base: int, step: int, bucket: int) -> int:
    """The trainer's seed of one request: update ``step`` of bucket (layer) ``bucket`` under the run's ``base``."""
    return sr_seed_check(base) ^ ((int(step) * 0x9E3779B97F4A7C15 + int(bucket) * 0xD1B54A32D192ED03) & _M64)


def sr_bytes(key, base: int, n: int) -> np.ndarray:
    """The random bytes of elements base..base+n-1 (base % 4 == 0): byte i & 3 of h(key, i >> 2)."""
    if base % 4 or n % 4 or base < 0 or base + n > SR_MAX_ELEMS:
        raise ValueError(f"stochastic rounding: elements [{base}, {base + n}) must lie below 2^32 on multiples of 4")
    h = sr_hash(key[0], key[1], np.arange(base >> 2, (base + n) >> 2, dtype=np.uint64).astype(np.uint32))
    return ((h[:, None] >> (np.arange(4, dtype=np.uint32) * np.uint32(8))) & np.uint32(0xFF)).reshape(-1)


def sr_encode_groups(x: np.ndarray, codec, key, base: int = 0):
    """x: float32 (size % 16 == 0), element 0 at index ``base`` of the padded bucket -> (q int8 [n], E uint8 [n/16]).
    Per group of shared exponent E (the rne encoder's own): E == 255 takes the rne encoder; otherwise, in f32,
    t = ldexp(x, k - E), f = floor(t), d = t - f, u = (b + 0.5) / 256, q = clamp(f + (d > u), -qmax, qmax)."""
    c = sr_codec(codec)
    top, lim = (133, 127.0) if c == 1 else (129, 7.0)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, GROUP)
    E = _shared_exp(x.view(np.uint32))
    q_rne, _ = encode_groups(x, _rounding_of(c))
    u = ((sr_bytes(key, base, x.size).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 256)).reshape(-1, GROUP)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.ldexp(x, top - E.astype(np.int32)).astype(np.float32)
        f = np.floor(t)
        d = (t - f).astype(np.float32)
        s = np.clip(f + (d > u).astype(np.float32), -lim, lim)
        q = np.where(E == 255, q_rne.reshape(-1, GROUP), np.nan_to_num(s).astype(np.int8))
    return q.reshape(-1).astype(np.int8), E.reshape(-1).astype(np.uint8)


def sr_quantize(x: np.ndarray, codec, key, base: int = 0) -> np.ndarray:
    """decode(stochastic encode(x)): what every rank decodes (the decoder is the codec's own)."""
    c = sr_codec(codec)
    q, E = sr_encode_groups(x, c, key, base)
    return decode_groups(q, E, _rounding_of(c))


def _sr_pack_shard(x, c, key, base):
    q, E = sr_encode_groups(x, c, key, base)
    return np.concatenate([pack_nibbles(q) if c == 4 else q.view(np.uint8), E])


def sr_pack(g: np.ndarray, shard_elems: int, codec, seed: int, rank: int, self_shard: int = -1, base: int = 0):
    """Sender stage of the stochastically rounded mesh all-reduce: every shard of ``g`` but ``self_shard`` (-1: none;
    that one takes plain rne) is encoded with key (seed, rank, 0); element j of g is element ``base + j`` of the padded
    bucket. Returns the wire (shards back to back)."""
    c = sr_codec(codec)
    key = sr_key(seed, rank, 0)
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    assert g.size % shard_elems == 0 and shard_elems % 256 == 0
    out = []
    for q in range(g.size // shard_elems):
        sl = slice(q * shard_elems, (q + 1) * shard_elems)
        out.append(pack(g[sl], shard_elems, c) if q == self_shard
                   else _sr_pack_shard(g[sl], c, key, base + q * shard_elems))
    return np.concatenate(out)


def sr_reduce(slots, local, self_pos: int, codec, shard_elems: int, seed: int, rank: int, base: int = 0):
    """Owner stage: :func:`reduce_slots` (slot order, slot ``self_pos`` from the dense ``local``), the sum encoded
    stochastically with key (seed, rank, 1); ``base`` is the owner shard's first element in the padded bucket. Returns
    the wire shard."""
    c = sr_codec(codec)
    acc = reduce_slots(slots, local, self_pos, c, shard_elems)
    return _sr_pack_shard(acc, c, sr_key(seed, rank, 1), base)


def sgd(w: np.ndarray, g: np.ndarray, lr: float, grad_scale: float = 1.0, weight_decay: float = 0.0,
        momentum: float = 0.0, mom: np.ndarray | None = None, nesterov: bool = False):
    """fp32 SGD with the kernel's operation order (fma emulated in float64, then rounded)."""
    w = np.asarray(w, np.float32)
    g = (np.asarray(g, np.float32) * np.float32(grad_scale)).astype(np.float32)
    if weight_decay:
        g = (np.float64(np.float32(weight_decay)) * w.astype(np.float64) + g).astype(np.float32)
    new_mom = None
    if momentum:
        m = (np.float64(np.float32(momentum)) * mom.astype(np.float64) + g).astype(np.float32)
        new_mom = m
        g = (np.float64(np.float32(momentum)) * m.astype(np.float64) + g).astype(np.float32) if nesterov else m
    w = (np.float64(-np.float32(lr)) * g.astype(np.float64) + w.astype(np.float64)).astype(np.float32)
    return w, new_mom


def clip_sumsq(g: np.ndarray) -> float:
    """S of a clip group's norm: the exactly rounded float64 sum (``math.fsum``) of the exact float64 squares of the
    f32 values ``g``; a non-finite value gives numpy's non-finite sum."""
    g64 = np.asarray(g, np.float32).reshape(-1).astype(np.float64)
    if np.isfinite(g64).all():
        return math.fsum(g64 * g64)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(g64 * g64))


def clip_words(S: float, grad_scale: float, max_norm: float) -> np.ndarray:
    """The four f32 words {coef, f32(total), f32(max_norm), nonfinite} of a clip group from S = sum g^2 over all its
    requests: total = sqrt(S) * |f32(grad_scale)| (the scale the update kernels apply), coef = min(1, max_norm /
    (total + 1e-6)) (``torch.nn.utils.clip_grad_norm_``), all float64, rounded once to f32. A non-finite S gives a NaN
    coef (it propagates through the update, as torch's with ``error_if_nonfinite=False``) and sets the flag."""
    max_norm = float(max_norm)
    if not (max_norm > 0 and math.isfinite(max_norm)):
        raise ValueError(f"max_norm must be finite and positive, got {max_norm}")
    S = float(S)
    finite = math.isfinite(S)
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.sqrt(np.float64(S)) * abs(np.float64(np.float32(grad_scale)))
        coef = min(1.0, max_norm / (float(total) + 1e-6)) if finite else math.nan
        return np.array([coef, total, max_norm, 0.0 if finite else 1.0], np.float64).astype(np.float32)


def clip_scale(grad_scale: float, words) -> float:
    """The grad_scale a clipped update uses: the one f32 product f32(grad_scale) * words[0]."""
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.float32(grad_scale) * np.float32(np.asarray(words, np.float32).reshape(-1)[0]))


class AdamWScalars(tuple):
    """The per-step AdamW scalars, each already rounded to f32 (``adamw_scalars``); ``wd`` rides along because the
    update tests it against 0."""
    FIELDS = ("beta1", "omb1", "beta2", "omb2", "step_size", "rsbc2", "eps", "decay", "wd")

    def __new__(cls, *vals):
        assert len(vals) == len(cls.FIELDS)
        return super().__new__(cls, (np.float32(x) for x in vals))

    def __getattr__(self, name):
        try:
            return self[self.FIELDS.index(name)]
        except ValueError:
            raise AttributeError(name) from None

    def kernel_args(self):
        """The eight scalars the native launchers take (all but wd), as Python floats holding the f32 values."""
        return [float(x) for x in self[:8]]


def adamw_scalars(lr: float, wd: float, beta1: float, beta2: float, eps: float, step: int) -> AdamWScalars:
    """The scalars of update ``step`` (1-based), computed in float64 and rounded once to f32; the kernels, the C++
    engine and ``adamw`` below all receive these values, so every path sees the same bits."""
    if not eps > 0:
        raise ValueError(f"AdamW: eps must be positive, got {eps}")
    if int(step) != step or step < 1:
        raise ValueError(f"AdamW: step is the 1-based update count, got {step}")
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError(f"AdamW: betas must lie in [0, 1), got {(beta1, beta2)}")
    lr, wd, b1, b2, t = float(lr), float(wd), float(beta1), float(beta2), int(step)
    return AdamWScalars(b1, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t), float(eps),
                        1.0 - lr * wd, wd)


def adamw(w: np.ndarray, g: np.ndarray, m: np.ndarray, v: np.ndarray, scalars: AdamWScalars,
          grad_scale: float = 1.0):
    """fp32 AdamW with the kernel's operation order (csrc/bfp/bfp_format.h adamw_update): fma emulated in float64
    and rounded, sqrt and division in float64 and rounded (exact double rounding for both). Returns (w', m', v')."""
    s = scalars
    f64 = np.float64
    w = np.asarray(w, np.float32)
    m = np.asarray(m, np.float32)
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        g = (np.asarray(g, np.float32) * np.float32(grad_scale)).astype(np.float32)
        t1 = (s.omb1 * g).astype(np.float32)
        m2 = (f64(s.beta1) * m.astype(f64) + t1.astype(f64)).astype(np.float32)
        t2 = ((s.omb2 * g).astype(np.float32) * g).astype(np.float32)
        v2 = (f64(s.beta2) * v.astype(f64) + t2.astype(f64)).astype(np.float32)
        r = np.sqrt(v2.astype(f64)).astype(np.float32)
        d = (r.astype(f64) * f64(s.rsbc2) + f64(s.eps)).astype(np.float32)
        q = (m2.astype(f64) / d.astype(f64)).astype(np.float32)
        base = (w * s.decay).astype(np.float32) if s.wd != 0 else w
        w2 = (f64(-s.step_size) * q.astype(f64) + base.astype(f64)).astype(np.float32)
    return w2, m2, v2


class LionScalars(tuple):
    """Lion's scalars, each already rounded to f32 (``lion_scalars``); ``wd`` rides along because the update tests it
    against 0, as ``AdamWScalars`` does. No eps and no step: Lion has no bias correction."""
    FIELDS = ("beta1", "omb1", "beta2", "omb2", "lr", "decay", "wd")

    def __new__(cls, *vals):
        assert len(vals) == len(cls.FIELDS)
        return super().__new__(cls, (np.float32(x) for x in vals))

    def __getattr__(self, name):
        try:
            return self[self.FIELDS.index(name)]
        except ValueError:
            raise AttributeError(name) from None

    def kernel_args(self):
        """The seven scalars the native launchers take, as Python floats holding the f32 values."""
        return [float(x) for x in self]


def lion_scalars(lr: float, wd: float, beta1: float, beta2: float) -> LionScalars:
    """Lion's scalars of a request, computed in float64 and rounded once to f32; the kernels, the C++ engine and
    ``lion`` below all receive these values, so every path sees the same bits."""
    lr, wd, b1, b2 = float(lr), float(wd), float(beta1), float(beta2)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"Lion: betas must lie in [0, 1), got {(beta1, beta2)}")
    if not (math.isfinite(lr) and math.isfinite(wd)):
        raise ValueError(f"Lion: lr and weight_decay must be finite, got {(lr, wd)}")
    return LionScalars(b1, 1.0 - b1, b2, 1.0 - b2, lr, 1.0 - lr * wd, wd)


def lion(w: np.ndarray, g: np.ndarray, m: np.ndarray, scalars: LionScalars, grad_scale: float = 1.0):
    """fp32 Lion with the kernel's operation order (csrc/bfp/bfp_format.h lion_update): each fma emulated in float64
    and rounded. The float64 sum of an f32 product and an f32 has the exact fma's sign (a product of two f32 values is
    exact in float64, and a float64 sum is zero only when the exact sum is), so the sign decision compares bit for
    bit. Returns (w', m')."""
    s = scalars
    f64 = np.float64
    w = np.asarray(w, np.float32)
    m = np.asarray(m, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        g = (np.asarray(g, np.float32) * np.float32(grad_scale)).astype(np.float32)
        t1 = (s.omb1 * g).astype(np.float32)
        c = (f64(s.beta1) * m.astype(f64) + t1.astype(f64)).astype(np.float32)
        sg = np.where(c > 0, np.float32(1), np.where(c < 0, np.float32(-1), c)).astype(np.float32)
        base = (w * s.decay).astype(np.float32) if s.wd != 0 else w
        w2 = (f64(-s.lr) * sg.astype(f64) + base.astype(f64)).astype(np.float32)
        t2 = (s.omb2 * g).astype(np.float32)
        m2 = (f64(s.beta2) * m.astype(f64) + t2.astype(f64)).astype(np.float32)
    return w2, m2


# --------------------------------------------------------------------------- 8-bit AdamW state (moment_codec="bfp8")
# Both moments of a bucket of n_pad elements live in one uint8 plane each, exactly ``pack(x, n_pad, "bfp_rne")`` of one
# shard of n_pad elements: bytes [0, n_pad) the int8 mantissas (element-indexed), bytes [n_pad, n_pad + n_pad/16) the
# groups' biased exponents. The layout is flat (no schedule, shard geometry or wire codec in it), a zeroed plane is the
# zero state, decoding is the bfp_rne decoder. The first plane holds m, the second r = sqrt(v): with beta2 = 0.999 the
# second moment moves 0.1 % a step, below an 8-bit mantissa's resolution, so both are stored with stochastic rounding
# (rank slot 16 of ``sr_key``: the wire's stochastic rounding uses ranks 0..15), and a positive r is never stored as 0
# (``m / (0 + eps)`` explodes; one quantum at least only makes that element's step smaller).
MOMENT_CODECS = ("f32", "bfp8")
MOMENT_RANK = 16            # the sr_key rank slot of the state's random bytes; stage 0: m, stage 1: r


def moment_codec_check(name) -> str:
    if name not in MOMENT_CODECS:
        raise ValueError(f"moment_codec: one of {MOMENT_CODECS}, got {name!r}")
    return name


def moment_plane_bytes(n_pad: int) -> int:
    """Bytes of one moment plane of a padded bucket of ``n_pad`` elements (a multiple of 256, below 2^32)."""
    n_pad = int(n_pad)
    if n_pad < 0 or n_pad % 256:
        raise ValueError(f"moment plane: the padded bucket is a multiple of 256 elements, got {n_pad}")
    if n_pad >= SR_MAX_ELEMS:
        raise ValueError(f"moment plane: a padded bucket of 2^32 or more elements ({n_pad}; element indices are 32-bit)")
    return n_pad + n_pad // 16


def moment_encode(x: np.ndarray, key, base: int = 0, floor1: bool = False):
    """The stochastic group encoder of the state: ``sr_encode_groups(x, bfp_rne, key, base)``; with ``floor1`` then
    q = max(q, 1) wherever x > 0 in a finite group (E != 255). Returns (q int8 [n], E uint8 [n/16])."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    q, E = sr_encode_groups(x, 1, key, base)
    if floor1:
        lift = (x > 0) & (np.repeat(E, GROUP) != 255)
        q = np.where(lift, np.maximum(q, 1), q).astype(np.int8)
    return q, E


def moment_decode(plane: np.ndarray) -> np.ndarray:
    """f32 values of a whole moment plane (the bfp_rne decoder, q * 2^(E-133); E = 255 -> NaN)."""
    plane = np.ascontiguousarray(plane, dtype=np.uint8).reshape(-1)
    if plane.size % 17:
        raise ValueError(f"moment plane: {plane.size} bytes is not n_pad * 17 / 16")
    n = plane.size // 17 * 16
    return decode_groups(plane[:n].view(np.int8), plane[n:], "rne")


def adamw_q(w: np.ndarray, g: np.ndarray, mom_q: np.ndarray, var_q: np.ndarray, scalars: AdamWScalars,
            grad_scale: float = 1.0, seed: int = 0, n_valid: int | None = None, base: int = 0):
    """AdamW over a region of a bucket whose moments are 8-bit planes. ``w`` / ``g``: the region's weights and decoded
    gradient (size % 16 == 0), element j being element ``base + j`` (base % 16 == 0) of the padded bucket; ``mom_q`` /
    ``var_q``: the bucket's whole planes. Per element below ``n_valid`` (default all), in f32: m_old = dec, r_old = dec,
    v_old = r_old * r_old (one multiply), ``adamw`` unchanged, then m' and r' = sqrt(v') (the value ``adamw`` uses in
    its denominator) are encoded per group with keys sr_key(seed, 16, 0) and sr_key(seed, 16, 1), the latter with the
    floor. In a group that straddles n_valid the elements at or past it enter the encode as 0 and keep their weights;
    groups entirely at or past it are not touched. Returns (w', mom_q', var_q'); the inputs are not modified."""
    w2 = np.array(w, dtype=np.float32).reshape(-1)
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    mq = np.array(mom_q, dtype=np.uint8).reshape(-1)
    vq = np.array(var_q, dtype=np.uint8).reshape(-1)
    n = w2.size
    n_valid = n if n_valid is None else int(n_valid)
    base = int(base)
    n_pad = mq.size // 17 * 16
    if mq.size != moment_plane_bytes(n_pad) or vq.size != mq.size:
        raise ValueError("adamw_q: both planes are n_pad * 17 / 16 bytes of one padded bucket")
    if n % GROUP or g.size < n or base % GROUP or base < 0 or base + n > n_pad or not 0 <= n_valid <= n:
        raise ValueError(f"adamw_q: region [{base}, {base + n}) with n_valid {n_valid} in a bucket of {n_pad}")
    seed = sr_seed_check(seed)
    k = -(-n_valid // GROUP) * GROUP     # the groups the update touches: [0, k)
    if k == 0:
        return w2, mq, vq
    ms, es = slice(base, base + k), slice(n_pad + base // GROUP, n_pad + (base + k) // GROUP)
    m_old = decode_groups(mq[ms].view(np.int8), mq[es], "rne")
    r_old = decode_groups(vq[ms].view(np.int8), vq[es], "rne")
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        v_old = (r_old * r_old).astype(np.float32)
        wn, m2, v2 = adamw(w2[:k], g[:k], m_old, v_old, scalars, grad_scale)
        r2 = np.sqrt(v2.astype(np.float64)).astype(np.float32)
    m2 = np.array(m2, np.float32)
    m2[n_valid:] = 0
    r2[n_valid:] = 0
    w2[:n_valid] = wn[:n_valid]
    for plane, x, stage in ((mq, m2, 0), (vq, r2, 1)):
        q, E = moment_encode(x, sr_key(seed, MOMENT_RANK, stage), base, floor1=stage == 1)
        plane[ms] = q.view(np.uint8)
        plane[es] = E
    return w2, mq, vq


class LambScalars(tuple):
    """The per-step scalars of AdamW with the layer-wise trust ratio (``lamb_scalars``), each already rounded to f32:
    AdamW's moment scalars, ``rbc1 = 1 / (1 - beta1^t)``, and ``wd`` / ``lr`` themselves (the step size is multiplied
    by the trust ratio, so it is not folded into one scalar). A class of its own beside ``AdamWScalars``, not one of
    them: it has no ``step_size`` or ``decay``, so the AdamW update fails on it instead of taking wrong scalars."""
    FIELDS = ("beta1", "omb1", "beta2", "omb2", "rsbc2", "eps", "rbc1", "wd", "lr")

    def __new__(cls, *vals):
        assert len(vals) == len(cls.FIELDS)
        return super().__new__(cls, (np.float32(x) for x in vals))

    def __getattr__(self, name):
        try:
            return self[self.FIELDS.index(name)]
        except ValueError:
            raise AttributeError(name) from None

    def kernel_args(self):
        """The nine scalars the native launchers take, as Python floats holding the f32 values."""
        return [float(x) for x in self]


def lamb_scalars(lr: float, wd: float, beta1: float, beta2: float, eps: float, step: int) -> LambScalars:
    """The trust-ratio update's scalars of update ``step`` (1-based): float64, rounded once to f32; beta1 .. eps are
    exactly ``adamw_scalars``' values."""
    a = adamw_scalars(lr, wd, beta1, beta2, eps, step)
    return LambScalars(a.beta1, a.omb1, a.beta2, a.omb2, a.rsbc2, a.eps, 1.0 / (1.0 - float(beta1) ** int(step)),
                       float(wd), float(lr))


def _lamb_direction(w, m2, v2, s: LambScalars):
    """r of csrc/bfp/bfp_format.h lamb_direction from the new moments and the old weights (all f32 arrays)."""
    f64 = np.float64
    r = np.sqrt(v2.astype(f64)).astype(np.float32)
    d = (r.astype(f64) * f64(s.rsbc2) + f64(s.eps)).astype(np.float32)
    u = (m2.astype(f64) / d.astype(f64)).astype(np.float32)
    ub = (u * s.rbc1).astype(np.float32)
    if s.wd != 0:
        return (f64(s.wd) * w.astype(f64) + ub.astype(f64)).astype(np.float32)
    return ub


def lamb_moments(w: np.ndarray, g: np.ndarray, m: np.ndarray, v: np.ndarray, scalars: LambScalars,
                 grad_scale: float = 1.0):
    """Pass 1 of the trust-ratio update in the kernel's operation order (lamb_moments / lamb_direction of
    csrc/bfp/bfp_format.h; fma, sqrt and division emulated in float64 and rounded, as ``adamw``): the new moments —
    ``adamw``'s statements, the same bits — and the direction r. Returns (m', v', r); w is not changed."""
    s = scalars
    f64 = np.float64
    w = np.asarray(w, np.float32)
    m = np.asarray(m, np.float32)
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        g = (np.asarray(g, np.float32) * np.float32(grad_scale)).astype(np.float32)
        t1 = (s.omb1 * g).astype(np.float32)
        m2 = (f64(s.beta1) * m.astype(f64) + t1.astype(f64)).astype(np.float32)
        t2 = ((s.omb2 * g).astype(np.float32) * g).astype(np.float32)
        v2 = (f64(s.beta2) * v.astype(f64) + t2.astype(f64)).astype(np.float32)
        r = _lamb_direction(w, m2, v2, s)
    return m2, v2, r


def lamb_ratio(w: np.ndarray, r: np.ndarray, n_adapt: int, lr: float) -> np.ndarray:
    """The three f32 scale words {lr * phi, lr, phi}: phi = f32(sqrt(S_w / S_r)) over the first ``n_adapt`` elements,
    the sums of the (exact) float64 squares taken with ``math.fsum``; 1 unless both sums are positive and finite."""
    w64 = np.asarray(w, np.float32)[:n_adapt].astype(np.float64)
    r64 = np.asarray(r, np.float32)[:n_adapt].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sw, sr = math.fsum(w64 * w64) if np.isfinite(w64).all() else math.inf, \
            math.fsum(r64 * r64) if np.isfinite(r64).all() else math.inf
    return lamb_words(sw, sr, lr)


def lamb_words(sw: float, sr: float, lr: float) -> np.ndarray:
    """{lr * phi, lr, phi} in f32 from the two float64 sums (``lamb_ratio``); lr * phi is one f32 product."""
    ok = sw > 0 and sr > 0 and math.isfinite(sw) and math.isfinite(sr)
    phi = np.float32(math.sqrt(sw / sr)) if ok else np.float32(1.0)
    lr32 = np.float32(lr)
    return np.array([lr32 * phi, lr32, phi], np.float32)


def lamb_apply(w: np.ndarray, m2: np.ndarray, v2: np.ndarray, scalars: LambScalars, words: np.ndarray,
               n_adapt: int) -> np.ndarray:
    """Pass 2: r recomputed from the stored moments and the untouched weights (pass 1's statements),
    w' = fma(-(i < n_adapt ? words[0] : words[1]), r, w). Returns w'."""
    w = np.asarray(w, np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        r = _lamb_direction(w, np.asarray(m2, np.float32), np.asarray(v2, np.float32), scalars)
        scale = np.where(np.arange(w.size) < n_adapt, np.float32(words[0]), np.float32(words[1])).astype(np.float32)
        return (-scale.astype(np.float64) * r.astype(np.float64) + w.astype(np.float64)).astype(np.float32)
