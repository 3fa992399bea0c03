// Block-floating-point (BFP) wire format and the other wire codecs of the all-reduce engine.
//
// Behavioural spec (derived from the reference RTL):
//   encode  hw/bf16_to_bfp_core.sv:97-126 (shared exp = max, right barrel shift of the 24-bit
//           mantissa with forced hidden 1, 25-bit two's complement, keep [24:1]),
//           hw/bfp_adapter.sv:145-154 (truncate to the top MANT_SIZE=8 bits -> floor),
//           hw/barrel_shifter.sv:44-51 (shift >= 32 clears).
//   decode  hw/bfp_to_bf16_core.sv:55-117 (|q| << 16, exp = E + 1 - lzc, normalise, bit0 = 0).
//
// CDNA4 mapping: one group of 16 values is handled by a PAIR of lanes (8 values each, 16-byte
// loads of bf16 / 2x16-byte of f32); the shared exponent is one v_max_u32 tree per lane plus a
// single DPP/swizzle exchange (__shfl_xor 1). No LDS round trip, no cross-wave traffic.
//
// Packed layout of one shard of n_s elements (n_s % 256 == 0): [int8 mant[n_s]][uint8 exp[n_s/16]]
// (the SoA analogue of the reference's 16 mantissa flits + 1 exponent flit per 32 groups,
// hw/bfp_adapter.sv:279-379). A multi-shard buffer is shards back to back.
//
// The reference's MANTISSA_SIZE / MANT_SIZE is a parameter of its encoder, decoder and adapter; kBfp4Rne is the
// framework's rne form at 4 bits: [u8 nib[n_s/2]][u8 exp[n_s/16]], 9 bytes per 16 values, byte i of a group's 8
// holding value 2i in bits [3:0] and value 2i+1 in bits [7:4] (two's complement). Exponent plane and shard starts
// stay 16-B aligned (n_s % 256 == 0). The reference ships no 4-bit configuration, so there is no truncating form.
#pragma once
#include "common/hip_common.h"

namespace fan {

enum Codec : int {
  kBfpTrunc = 0,  // bit-exact reference numerics (floor truncation, reference decode quirks)
  kBfpRne = 1,    // framework default: round-to-nearest-even, exact decode q * 2^(E-133)
  kRawF32 = 2,    // uncompressed fp32 on the wire
  kRawBf16 = 3,   // uncompressed bf16 on the wire
  kBfp4Rne = 4,   // 4-bit mantissas (two per byte), round-to-nearest-even, exact decode q * 2^(E-129)
};

// Codecs whose groups of 16 values share an exponent byte (every BFP width), and the 8-bit ones among them: the only
// ones the GEMM wire epilogues encode (prepack, the fused update) and the 4-values-per-lane layout (Lanes4) handles.
__host__ __device__ constexpr bool codec_shared_exp(int c) { return c == kBfpTrunc || c == kBfpRne || c == kBfp4Rne; }
__host__ __device__ constexpr bool codec_bfp8(int c) { return c == kBfpTrunc || c == kBfpRne; }

enum DType : int { kF32 = 0, kBF16 = 1 };

struct SgdParams {
  float lr;
  float grad_scale;
  float weight_decay;
  float momentum;
  int nesterov;
};

// One element's SGD step (weight decay, momentum, Nesterov), all f32. Every update path calls it (wire_sgd_kernel,
// the merged reduce-and-update kernel, the GEMMs' fused-update epilogues), so their weights are bit-identical.
__device__ __forceinline__ void sgd_update(const SgdParams& p, float g, float& w, float& m, bool has_mom) {
  float gj = g * p.grad_scale;
  if (p.weight_decay != 0.0f) gj = fmaf(p.weight_decay, w, gj);
  if (has_mom) {
    m = fmaf(p.momentum, m, gj);
    gj = p.nesterov ? fmaf(p.momentum, m, gj) : m;
  }
  w = fmaf(-p.lr, gj, w);
}

// AdamW (decoupled decay, bias correction) of the update kernels. The per-step scalars are computed on the host in
// float64 and rounded once to f32 (ops/bfp_oracle.py adamw_scalars): omb1 = 1 - beta1, omb2 = 1 - beta2,
// step_size = lr / (1 - beta1^t), rsbc2 = 1 / sqrt(1 - beta2^t), decay = 1 - lr * wd. `var` is the second-moment
// plane (the first moment travels in the launchers' `mom`), at the same flat indices as master. A struct of its own:
// SgdParams is embedded in the GEMM kernels' argument block and stays as it is.
struct AdamWParams {
  float grad_scale;
  float beta1, omb1;
  float beta2, omb2;
  float step_size;
  float rsbc2;
  float eps;
  float weight_decay;  // only tested against 0: the decay itself is `decay`
  float decay;
  float* var;
};

// One element's AdamW step, all f32, in the order bfp_oracle.adamw emulates (change both together):
//   g = g * grad_scale; m' = fma(beta1, m, omb1 * g); v' = fma(beta2, v, (omb2 * g) * g)
//   d = fma(sqrt(v'), rsbc2, eps); w' = fma(-step_size, m' / d, wd != 0 ? w * decay : w)
// `/` and sqrtf are the correctly rounded forms (v_div_scale / v_div_fmas / v_div_fixup; v_sqrt_f32 + refinement).
__device__ __forceinline__ void adamw_update(const AdamWParams& p, float g, float& w, float& m, float& v) {
  g = g * p.grad_scale;
  m = fmaf(p.beta1, m, p.omb1 * g);
  v = fmaf(p.beta2, v, (p.omb2 * g) * g);
  const float d = fmaf(sqrtf(v), p.rsbc2, p.eps);
  w = fmaf(-p.step_size, m / d, p.weight_decay != 0.0f ? w * p.decay : w);
}

// Lion (Chen et al. 2023: sign of the interpolated momentum, decoupled decay) of the update kernels. One moment plane,
// the launchers' `mom`, so it reads and writes exactly SGD-momentum's planes; no divide, no square root, no step
// counter. The scalars are computed on the host in float64 and rounded once to f32 (ops/bfp_oracle.py lion_scalars):
// omb1 = 1 - beta1, omb2 = 1 - beta2, decay = 1 - lr * wd.
struct LionParams {
  float grad_scale;
  float beta1, omb1;
  float beta2, omb2;
  float lr;
  float weight_decay;  // only tested against 0: the decay itself is `decay`
  float decay;
};

// One element's Lion step, all f32, in the order bfp_oracle.lion emulates (change both together):
//   g = g * grad_scale; c = fma(beta1, m, omb1 * g); s = c > 0 ? 1 : c < 0 ? -1 : c
//   w' = fma(-lr, s, wd != 0 ? w * decay : w); m' = fma(beta2, m, omb2 * g)
// c == +-0 leaves the weight on w * decay (and -lr * +-0 adds nothing); a NaN c propagates into w'.
__device__ __forceinline__ void lion_update(const LionParams& p, float g, float& w, float& m) {
  g = g * p.grad_scale;
  const float c = fmaf(p.beta1, m, p.omb1 * g);
  const float s = c > 0.0f ? 1.0f : c < 0.0f ? -1.0f : c;
  w = fmaf(-p.lr, s, p.weight_decay != 0.0f ? w * p.decay : w);
  m = fmaf(p.beta2, m, p.omb2 * g);
}

// AdamW with a layer-wise trust ratio (LAMB), the two-pass update of the all-reduce epilogues. The host scalars are
// ops/bfp_oracle.py lamb_scalars (float64, rounded once to f32): AdamW's beta1, omb1, beta2, omb2, rsbc2, eps, plus
// rbc1 = 1 / (1 - beta1^t), the decay coefficient and lr themselves (the step size is not folded into a scalar: it is
// multiplied by the trust ratio on the device). `var` as AdamWParams::var.
struct LambParams {
  float grad_scale;
  float beta1, omb1;
  float beta2, omb2;
  float rsbc2;
  float eps;
  float rbc1;
  float weight_decay;
  float lr;
  float* var;
};

// Pass 1's moments of one element: adamw_update's first three statements, so the same bits.
__device__ __forceinline__ void lamb_moments(const LambParams& p, float g, float& m, float& v) {
  g = g * p.grad_scale;
  m = fmaf(p.beta1, m, p.omb1 * g);
  v = fmaf(p.beta2, v, (p.omb2 * g) * g);
}

// The update direction of one element from the NEW moments and the OLD weight, all f32, in the order
// bfp_oracle.lamb_moments emulates (change both together):
//   d = fma(sqrt(v'), rsbc2, eps); u = m' / d; r = wd != 0 ? fma(wd, w, u * rbc1) : u * rbc1
// Pass 1 (for the norm) and pass 2 (for the step) both call it on the same values, so no `r` plane is kept.
__device__ __forceinline__ float lamb_direction(const LambParams& p, float w, float m, float v) {
  const float d = fmaf(sqrtf(v), p.rsbc2, p.eps);
  const float u = m / d;
  const float ub = u * p.rbc1;
  return p.weight_decay != 0.0f ? fmaf(p.weight_decay, w, ub) : ub;
}

__host__ __device__ inline size_t wire_shard_bytes(int codec, size_t n_s) {
  switch (codec) {
    case kBfpTrunc:
    case kBfpRne: return n_s + n_s / 16;
    case kBfp4Rne: return n_s / 2 + n_s / 16;
    case kRawF32: return n_s * 4;
    default: return n_s * 2;
  }
}

// ---------------------------------------------------------------- scalar BFP primitives
// Reference (trunc) encode of one value given the group's shared exponent E.
__device__ __forceinline__ int32_t bfp_encode_trunc(uint32_t bits, uint32_t E) {
  const uint32_t e = (bits >> 23) & 0xFFu;
  const uint32_t m = (bits & 0x7FFFFFu) | 0x800000u;  // hidden 1 forced, even for 0/denormals
  const uint32_t d = E - e;
  const uint32_t a = d >= 32u ? 0u : (m >> d);         // VALU shifts are mod 32: clear explicitly
  const int32_t t = (bits >> 31) ? -(int32_t)a : (int32_t)a;
  return t >> 17;  // keep t[24:17] of the 25-bit two's complement: floor
}

// Reference decode (bit-level: q==0 -> 2^(E-150), |-128| = 128, exponent field wraps mod 256).
__device__ __forceinline__ float bfp_decode_trunc(int32_t q, uint32_t E) {
  const uint32_t sign = q < 0 ? 1u : 0u;
  const uint32_t M = (uint32_t)(q < 0 ? -q : q) << 16;  // 24-bit magnitude
  const uint32_t zc = __clz(M) - 8u;                     // 24-bit leading-zero count (24 for 0)
  const uint32_t ex = (E + 1u - zc) & 0xFFu;
  const uint32_t frac = (M << zc) & 0x7FFFFEu;           // bit 0 forced to 0
  return __uint_as_float((sign << 31) | (ex << 23) | frac);
}

// Framework encode: q = clamp(rne(x * 2^(133-E)), -127, 127).
__device__ __forceinline__ int32_t bfp_encode_rne(float x, uint32_t E) {
  float s = rintf(ldexpf(x, 133 - (int)E));
  s = fminf(fmaxf(s, -127.0f), 127.0f);
  return (int32_t)s;
}

__device__ __forceinline__ float bfp_decode_rne(int32_t q, uint32_t E) {
  return E == 255u ? __uint_as_float(0x7FC00000u) : ldexpf((float)q, (int)E - 133);
}

// The 4-bit form: q = clamp(rne(x * 2^(129-E)), -7, 7), a two's-complement nibble; decode q * 2^(E-129).
__device__ __forceinline__ int32_t bfp4_encode_rne(float x, uint32_t E) {
  float s = rintf(ldexpf(x, 129 - (int)E));
  s = fminf(fmaxf(s, -7.0f), 7.0f);
  return (int32_t)s;
}

__device__ __forceinline__ float bfp4_decode_rne(int32_t q, uint32_t E) {
  return E == 255u ? __uint_as_float(0x7FC00000u) : ldexpf((float)q, (int)E - 129);
}

// Nibble j (0..7) of a dword of mantissas, sign-extended (a shift pair).
__device__ __forceinline__ int32_t bfp4_nibble(uint32_t w, int j) { return (int32_t)(w << (28 - 4 * j)) >> 28; }

// Encode / decode of one value by codec (the 8-bit forms take and return the byte's value, the 4-bit form the nibble's).
template <int C>
__device__ __forceinline__ int32_t bfp_encode(float x, uint32_t E) {
  static_assert(codec_shared_exp(C), "BFP codecs");
  if constexpr (C == kBfpTrunc) return bfp_encode_trunc(__float_as_uint(x), E);
  else if constexpr (C == kBfpRne) return bfp_encode_rne(x, E);
  else return bfp4_encode_rne(x, E);
}
template <int C>
__device__ __forceinline__ float bfp_decode(int32_t q, uint32_t E) {
  static_assert(codec_shared_exp(C), "BFP codecs");
  if constexpr (C == kBfpTrunc) return bfp_decode_trunc(q, E);
  else if constexpr (C == kBfpRne) return bfp_decode_rne(q, E);
  else return bfp4_decode_rne(q, E);
}

// ---------------------------------------------------------------- 8-value lane codecs
template <int C>
struct WireLane;

template <int C>
struct BfpLane {
  __device__ static __forceinline__ void load8(const uint8_t* shard, size_t n_s, size_t le, float v[8]) {
    const uint2 m = *reinterpret_cast<const uint2*>(shard + le);
    const uint32_t E = shard[n_s + (le >> 4)];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t w = j < 4 ? m.x : m.y;
      const int32_t q = (int32_t)(int8_t)(uint8_t)(w >> (8 * (j & 3)));
      v[j] = bfp_decode<C>(q, E);
    }
  }
  // Both lanes of the pair (lane, lane^1) must be active: they hold the two halves of a group.
  __device__ static __forceinline__ void store8(uint8_t* shard, size_t n_s, size_t le, const float v[8]) {
    uint32_t mx = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = max(mx, __float_as_uint(v[j]) & 0x7FFFFFFFu);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 1));
    const uint32_t E = mx >> 23;
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int32_t q = bfp_encode<C>(v[j], E);
      w[j >> 2] |= ((uint32_t)q & 0xFFu) << (8 * (j & 3));
    }
    *reinterpret_cast<uint2*>(shard + le) = make_uint2(w[0], w[1]);
    if ((le & 15) == 0) shard[n_s + (le >> 4)] = (uint8_t)E;
  }
};

template <>
struct WireLane<kBfpTrunc> : BfpLane<kBfpTrunc> {};
template <>
struct WireLane<kBfpRne> : BfpLane<kBfpRne> {};

// 4-bit mantissas, shard layout [u8 nib[n_s/2]][u8 exp[n_s/16]]: a lane's 8 values are ONE dword of nibbles (value 2i
// in bits [3:0] of byte i, value 2i+1 in bits [7:4], i.e. value j in bits [4j+3:4j] of the dword), the exponent
// exchange of the pair is BfpLane's.
template <>
struct WireLane<kBfp4Rne> {
  __device__ static __forceinline__ void load8(const uint8_t* shard, size_t n_s, size_t le, float v[8]) {
    const uint32_t m = *reinterpret_cast<const uint32_t*>(shard + (le >> 1));
    const uint32_t E = shard[(n_s >> 1) + (le >> 4)];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bfp4_decode_rne(bfp4_nibble(m, j), E);
  }
  // Both lanes of the pair (lane, lane^1) must be active: they hold the two halves of a group.
  __device__ static __forceinline__ void store8(uint8_t* shard, size_t n_s, size_t le, const float v[8]) {
    uint32_t mx = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = max(mx, __float_as_uint(v[j]) & 0x7FFFFFFFu);
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, 1));
    const uint32_t E = mx >> 23;
    uint32_t w = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) w |= ((uint32_t)bfp4_encode_rne(v[j], E) & 0xFu) << (4 * j);
    *reinterpret_cast<uint32_t*>(shard + (le >> 1)) = w;
    if ((le & 15) == 0) shard[(n_s >> 1) + (le >> 4)] = (uint8_t)E;
  }
};

template <>
struct WireLane<kRawF32> {
  __device__ static __forceinline__ void load8(const uint8_t* shard, size_t, size_t le, float v[8]) {
    const float4* p = reinterpret_cast<const float4*>(shard) + (le >> 2);
    const float4 a = p[0], b = p[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  __device__ static __forceinline__ void store8(uint8_t* shard, size_t, size_t le, const float v[8]) {
    float4* p = reinterpret_cast<float4*>(shard) + (le >> 2);
    p[0] = make_float4(v[0], v[1], v[2], v[3]);
    p[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
};

template <>
struct WireLane<kRawBf16> {
  __device__ static __forceinline__ void load8(const uint8_t* shard, size_t, size_t le, float v[8]) {
    const uint4 u = *(reinterpret_cast<const uint4*>(shard) + (le >> 3));
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = __uint_as_float(w[j] << 16);
      v[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
    }
  }
  __device__ static __forceinline__ void store8(uint8_t* shard, size_t, size_t le, const float v[8]) {
    uint4 u;
    u.x = pack_bf16x2(v[0], v[1]);
    u.y = pack_bf16x2(v[2], v[3]);
    u.z = pack_bf16x2(v[4], v[5]);
    u.w = pack_bf16x2(v[6], v[7]);
    *(reinterpret_cast<uint4*>(shard) + (le >> 3)) = u;
  }
};

// ---------------------------------------------------------------- 16-value lane codecs (one BFP group per lane)
// The streaming kernels give each lane a whole 16-value group: the shared exponent needs no cross-lane exchange,
// the mantissas leave as ONE 16-B store, and the 16 exponents of 16 consecutive lanes are gathered into ONE 16-B
// store by the group's first lane (the NIC ships the 32 exponents of a frame as one 256-bit flit,
// hw/bfp_adapter.sv:279-379). Every store of a wire shard is then a full 16-B vector store, which is what a store
// into a peer's uncached receive arena over xGMI needs (a byte store there is one fabric write per byte).
// Requirements: the 16 lanes 16k..16k+15 of a wave handle 16 consecutive groups starting at a multiple of 16
// (grid-stride loops over group indices with block and stride multiples of 16; n_s % 256 == 0, so a 16-lane
// segment is either entirely inside the shard or entirely past its end), and they are all active at the store.
template <int C>
struct WireLane16 {
  __device__ static __forceinline__ void load16(const uint8_t* shard, size_t n_s, size_t le, float v[16]) {
    WireLane<C>::load8(shard, n_s, le, v);
    WireLane<C>::load8(shard, n_s, le + 8, v + 8);
  }
  __device__ static __forceinline__ void store16(uint8_t* shard, size_t n_s, size_t le, const float v[16]) {
    WireLane<C>::store8(shard, n_s, le, v);
    WireLane<C>::store8(shard, n_s, le + 8, v + 8);
  }
};

// The shared exponent of a 16-value group one lane holds whole: the largest magnitude's exponent field.
__device__ __forceinline__ uint32_t bfp_group_exponent(const float* v) {
  uint32_t mx = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) mx = max(mx, __float_as_uint(v[j]) & 0x7FFFFFFFu);
  return mx >> 23;
}

// The exponent bytes E of 16 consecutive lanes as the 16 B lane 16k stores: 4 lanes -> one dword, 4 dwords -> one
// uint4 (valid in lane 16k; all 16 lanes must be active).
__device__ __forceinline__ uint4 bfp_gather_exponents(uint32_t E) {
  uint32_t e4 = E | ((uint32_t)__shfl_down((int)E, 1) << 8) | ((uint32_t)__shfl_down((int)E, 2) << 16) |
                ((uint32_t)__shfl_down((int)E, 3) << 24);
  const uint32_t e4b = (uint32_t)__shfl_down((int)e4, 4), e4c = (uint32_t)__shfl_down((int)e4, 8),
                 e4d = (uint32_t)__shfl_down((int)e4, 12);
  return make_uint4(e4, e4b, e4c, e4d);
}

template <int C>
struct BfpLane16 {
  __device__ static __forceinline__ void load16(const uint8_t* shard, size_t n_s, size_t le, float v[16]) {
    const uint4 m = *reinterpret_cast<const uint4*>(shard + le);
    const uint32_t E = shard[n_s + (le >> 4)];
    const uint32_t w[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int32_t q = (int32_t)(int8_t)(uint8_t)(w[j >> 2] >> (8 * (j & 3)));
      v[j] = bfp_decode<C>(q, E);
    }
  }
  __device__ static __forceinline__ void store16(uint8_t* shard, size_t n_s, size_t le, const float v[16]) {
    const uint32_t E = bfp_group_exponent(v);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int32_t q = bfp_encode<C>(v[j], E);
      w[j >> 2] |= ((uint32_t)q & 0xFFu) << (8 * (j & 3));
    }
    *reinterpret_cast<uint4*>(shard + le) = make_uint4(w[0], w[1], w[2], w[3]);
    const uint4 e16 = bfp_gather_exponents(E);  // the exponent plane: one 16-B store by lane 16k
    if ((threadIdx.x & 15) == 0) *reinterpret_cast<uint4*>(shard + n_s + (le >> 4)) = e16;
  }
};

template <>
struct WireLane16<kBfpTrunc> : BfpLane16<kBfpTrunc> {};
template <>
struct WireLane16<kBfpRne> : BfpLane16<kBfpRne> {};

// The 4-bit group per lane: ONE 8-B load or store of nibbles per lane (adjacent lanes cover contiguous bytes), the
// exponent plane gathered into one 16-B store by lane 16k as above.
template <>
struct WireLane16<kBfp4Rne> {
  __device__ static __forceinline__ void load16(const uint8_t* shard, size_t n_s, size_t le, float v[16]) {
    const uint2 m = *reinterpret_cast<const uint2*>(shard + (le >> 1));
    const uint32_t E = shard[(n_s >> 1) + (le >> 4)];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = bfp4_decode_rne(bfp4_nibble(j < 8 ? m.x : m.y, j & 7), E);
  }
  __device__ static __forceinline__ void store16(uint8_t* shard, size_t n_s, size_t le, const float v[16]) {
    const uint32_t E = bfp_group_exponent(v);
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 3] |= ((uint32_t)bfp4_encode_rne(v[j], E) & 0xFu) << (4 * (j & 7));
    *reinterpret_cast<uint2*>(shard + (le >> 1)) = make_uint2(w[0], w[1]);
    const uint4 e16 = bfp_gather_exponents(E);
    if ((threadIdx.x & 15) == 0) *reinterpret_cast<uint4*>(shard + (n_s >> 1) + (le >> 4)) = e16;
  }
};

// Dense (local) operand loads: f32 or bf16 arrays.
template <typename T>
struct DenseLane;
template <>
struct DenseLane<float> {
  __device__ static __forceinline__ void load8(const float* p, size_t e, float v[8]) {
    WireLane<kRawF32>::load8(reinterpret_cast<const uint8_t*>(p), 0, e, v);
  }
  __device__ static __forceinline__ void store8(float* p, size_t e, const float v[8]) {
    WireLane<kRawF32>::store8(reinterpret_cast<uint8_t*>(p), 0, e, v);
  }
};
template <>
struct DenseLane<bf16_t> {
  __device__ static __forceinline__ void load8(const bf16_t* p, size_t e, float v[8]) {
    WireLane<kRawBf16>::load8(reinterpret_cast<const uint8_t*>(p), 0, e, v);
  }
  __device__ static __forceinline__ void store8(bf16_t* p, size_t e, const float v[8]) {
    WireLane<kRawBf16>::store8(reinterpret_cast<uint8_t*>(p), 0, e, v);
  }
};
template <typename T>
struct DenseLane16 {
  __device__ static __forceinline__ void load16(const T* p, size_t e, float v[16]) {
    DenseLane<T>::load8(p, e, v);
    DenseLane<T>::load8(p, e + 8, v + 8);
  }
  __device__ static __forceinline__ void store16(T* p, size_t e, const float v[16]) {
    DenseLane<T>::store8(p, e, v);
    DenseLane<T>::store8(p, e + 8, v + 8);
  }
};

// ---------------------------------------------------------------- lane layouts of the reduce kernels
// What a lane of wire_reduce / wire_reduce_to / wire_reduce_sgd (bfp_kernels.hip) holds per trip: a whole group
// (Lanes16, every codec) or 4 values of one (Lanes4, BFP codecs). Same members, same operations per value, so a kernel
// body written against them gives the same bits in either layout. `roundtrip` turns the lane's values into what every
// rank decodes after the owner re-encodes them with codec C.

// The value every rank decodes after `x` is encoded in a group of shared exponent E.
template <int C>
__device__ __forceinline__ float bfp_roundtrip(float x, uint32_t E) {
  const int32_t q = bfp_encode<C>(x, E);
  // the stored byte (nibble), as the decoder reads it
  const int32_t qs = C == kBfp4Rne ? bfp4_nibble((uint32_t)q & 0xFu, 0) : (int32_t)(int8_t)(uint8_t)((uint32_t)q & 0xFFu);
  return bfp_decode<C>(qs, E);
}

template <int C>
struct Lanes16 {
  static constexpr int kVals = 16;
  __device__ static __forceinline__ void load_wire(const uint8_t* shard, size_t n_s, size_t le, float v[16]) {
    WireLane16<C>::load16(shard, n_s, le, v);
  }
  template <typename T>
  __device__ static __forceinline__ void load_dense(const T* p, size_t e, float v[16]) {
    DenseLane16<T>::load16(p, e, v);
  }
  __device__ static __forceinline__ void store_wire(uint8_t* shard, size_t n_s, size_t le, const float v[16]) {
    WireLane16<C>::store16(shard, n_s, le, v);
  }
  __device__ static __forceinline__ void store_f32(float* p, size_t e, const float v[16]) {
    DenseLane16<float>::store16(p, e, v);
  }
  __device__ static __forceinline__ void store_bf16(bf16_t* p, size_t e, const float v[16]) {
    DenseLane16<bf16_t>::store16(p, e, v);
  }
  __device__ static __forceinline__ void roundtrip(float v[16]) {
    if constexpr (codec_shared_exp(C)) {
      const uint32_t E = bfp_group_exponent(v);
#pragma unroll
      for (int j = 0; j < 16; ++j) v[j] = bfp_roundtrip<C>(v[j], E);
    } else if constexpr (C == kRawBf16) {
#pragma unroll
      for (int j = 0; j < 16; j += 2) {
        const uint32_t u = pack_bf16x2(v[j], v[j + 1]);
        v[j] = __uint_as_float(u << 16);
        v[j + 1] = __uint_as_float(u & 0xFFFF0000u);
      }
    }
  }
};

// The shared exponent of the group whose 16 values a quad of lanes 4k..4k+3 holds 4 each (two xor shuffles: exact).
// All four lanes must be active.
__device__ __forceinline__ uint32_t bfp_quad_exponent(const float v[4]) {
  uint32_t mx = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) mx = max(mx, __float_as_uint(v[j]) & 0x7FFFFFFFu);
  mx = max(mx, (uint32_t)__shfl_xor((int)mx, 1));
  mx = max(mx, (uint32_t)__shfl_xor((int)mx, 2));
  return mx >> 23;
}

// The lane-contiguous form: a lane holds 4 consecutive values and a quad of lanes one group, so every load and store of
// a wave covers contiguous bytes instead of striding a group per lane; a lane's mantissas are one dword, and the
// group's exponent byte is read by all four lanes and stored by the first.
// Requirements: n_s % 16 == 0 and a thread count that is a multiple of 4, so a quad's lanes are always all in or all
// out of range, and they are all active at store_wire and roundtrip (bfp_quad_exponent).
template <int C>
struct Lanes4 {
  static_assert(codec_bfp8(C), "8-bit BFP codecs");
  static constexpr int kVals = 4;
  __device__ static __forceinline__ void load_wire(const uint8_t* shard, size_t n_s, size_t le, float v[4]) {
    const uint32_t m = *reinterpret_cast<const uint32_t*>(shard + le);
    const uint32_t E = shard[n_s + (le >> 4)];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int32_t q = (int32_t)(int8_t)(uint8_t)(m >> (8 * j));
      v[j] = bfp_decode<C>(q, E);
    }
  }
  __device__ static __forceinline__ void load_dense(const float* p, size_t e, float v[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p + e);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  }
  __device__ static __forceinline__ void load_dense(const bf16_t* p, size_t e, float v[4]) {
    const uint2 a = *reinterpret_cast<const uint2*>(p + e);
    v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xFFFF0000u);
    v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xFFFF0000u);
  }
  __device__ static __forceinline__ void store_wire(uint8_t* shard, size_t n_s, size_t le, const float v[4]) {
    const uint32_t E = bfp_quad_exponent(v);
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int32_t q = bfp_encode<C>(v[j], E);
      w |= ((uint32_t)q & 0xFFu) << (8 * j);
    }
    *reinterpret_cast<uint32_t*>(shard + le) = w;
    if ((le & 15) == 0) shard[n_s + (le >> 4)] = (uint8_t)E;
  }
  __device__ static __forceinline__ void store_f32(float* p, size_t e, const float v[4]) {
    *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __device__ static __forceinline__ void store_bf16(bf16_t* p, size_t e, const float v[4]) {
    *reinterpret_cast<uint2*>(p + e) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  }
  __device__ static __forceinline__ void roundtrip(float v[4]) {
    const uint32_t E = bfp_quad_exponent(v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = bfp_roundtrip<C>(v[j], E);
  }
};

// ---------------------------------------------------------------- stochastic rounding (ops/bfp_oracle.py sr_*)
// The rne codecs' encoders with an unbiased rounding, q = floor(t) + (frac(t) > u): the wire format and the decoders
// stay as they are. The random byte of element i of the padded bucket (i < 2^32) is byte i & 3 of the hash word
// h(k0, k1, i >> 2), so a lane's 4 consecutive values cost one hash and the bits depend on nothing but the key and the
// element. The key is computed on the host from the request's 64-bit seed, the encoding rank and the stage.
__host__ __device__ constexpr bool codec_sr(int c) { return c == kBfpRne || c == kBfp4Rne; }

struct SrKey {
  uint32_t k0, k1;
};

// stage: 0 the sender's pack, 1 the owner's re-encode.
inline SrKey sr_key(uint64_t seed, int rank, int stage) {
  return {(uint32_t)seed, (uint32_t)(seed >> 32) ^ ((uint32_t)(2 * rank + stage + 1) * 0x9E3779B9u)};
}

__host__ __device__ __forceinline__ uint32_t sr_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint32_t sr_hash(SrKey k, uint32_t w) { return sr_mix(sr_mix(w ^ k.k0) + k.k1); }

// One value of a finite group (E != 255; the caller sends an E == 255 group through bfp_encode<C>), all f32:
// t = x * 2^(k-E), f = floor(t), d = t - f, u = (b + 0.5) / 256 (exact), q = clamp(f + (d > u), -qmax, qmax). A value
// the codec represents exactly has d == 0 and keeps its q whatever b is.
template <int C>
__device__ __forceinline__ int32_t bfp_encode_sr(float x, uint32_t E, uint32_t b) {
  static_assert(codec_sr(C), "rne codecs");
  constexpr int kTop = C == kBfp4Rne ? 129 : 133;
  constexpr float kMax = C == kBfp4Rne ? 7.0f : 127.0f;
  const float t = ldexpf(x, kTop - (int)E);
  const float f = floorf(t);
  const float d = t - f;
  const float u = ((float)b + 0.5f) * (1.0f / 256.0f);
  const float s = f + (d > u ? 1.0f : 0.0f);
  return (int32_t)fminf(fmaxf(s, -kMax), kMax);
}

// The mantissas of kVals (4 or 16) consecutive values of a group of shared exponent E, first element i of the padded
// bucket (i % 4 == 0), packed as the wire holds them: 8-bit codec value j in byte j, 4-bit value j in nibble j.
// kFloor1 (the 8-bit optimizer state's r = sqrt(v) plane, ops/bfp_oracle.py moment_encode): a positive value of a
// finite group is never stored as 0, q = max(q, 1); the unflagged instantiation is the wire's encoder, unchanged.
template <int C, int kVals, bool kFloor1 = false>
__device__ __forceinline__ void sr_encode_vals(const float (&v)[kVals], uint32_t E, SrKey key, uint32_t i,
                                               uint32_t (&w)[(kVals * (C == kBfp4Rne ? 4 : 8) + 31) / 32]) {
  constexpr int kBits = C == kBfp4Rne ? 4 : 8;
  constexpr uint32_t kMask = (1u << kBits) - 1u;
#pragma unroll
  for (int j = 0; j < (kVals * kBits + 31) / 32; ++j) w[j] = 0u;
  if (E != 255u) {
#pragma unroll
    for (int g = 0; g < kVals / 4; ++g) {
      const uint32_t h = sr_hash(key, (i >> 2) + g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = 4 * g + j;
        int32_t q = bfp_encode_sr<C>(v[e], E, (h >> (8 * j)) & 0xFFu);
        if constexpr (kFloor1) q = v[e] > 0.0f ? max(q, 1) : q;
        w[(e * kBits) >> 5] |= ((uint32_t)q & kMask) << ((e * kBits) & 31);
      }
    }
  } else {  // a non-finite group: the rne encoder's bytes
#pragma unroll
    for (int e = 0; e < kVals; ++e)
      w[(e * kBits) >> 5] |= ((uint32_t)bfp_encode<C>(v[e], E) & kMask) << ((e * kBits) & 31);
  }
}

// Value e of the words sr_encode_vals packed, as the decoder reads it.
template <int C>
__device__ __forceinline__ float sr_decode_val(const uint32_t* w, int e, uint32_t E) {
  if constexpr (C == kBfp4Rne) return bfp4_decode_rne(bfp4_nibble(w[e >> 3], e & 7), E);
  else return bfp_decode_rne((int32_t)(int8_t)(uint8_t)(w[e >> 2] >> (8 * (e & 3))), E);
}

// The stochastic forms of a lane layout's store_wire and roundtrip (Lanes16<C> / Lanes4<C> above, same requirements on
// the active lanes): `to` is a destination table, every non-null entry below n_dst receives the same bytes from one
// encode; `i` is the bucket index of the lane's first value.
template <typename L>
struct SrLanes;

template <int C>
struct SrLanes<Lanes16<C>> {
  static constexpr int kWords = C == kBfp4Rne ? 2 : 4;
  __device__ static __forceinline__ void store_wire(uint8_t* const* to, int n_dst, size_t n_s, size_t le,
                                                    const float (&v)[16], SrKey key, uint32_t i) {
    const uint32_t E = bfp_group_exponent(v);
    uint32_t w[kWords];
    sr_encode_vals<C, 16>(v, E, key, i, w);
    const uint4 e16 = bfp_gather_exponents(E);  // the exponent plane: one 16-B store by lane 16k (WireLane16)
    const size_t mant = C == kBfp4Rne ? n_s >> 1 : n_s;  // bytes of the mantissa plane
    for (int k = 0; k < n_dst; ++k) {                    // (wave-uniform condition)
      uint8_t* shard = to[k];
      if (shard == nullptr) continue;
      if constexpr (C == kBfp4Rne) *reinterpret_cast<uint2*>(shard + (le >> 1)) = make_uint2(w[0], w[1]);
      else *reinterpret_cast<uint4*>(shard + le) = make_uint4(w[0], w[1], w[2], w[3]);
      if ((threadIdx.x & 15) == 0) *reinterpret_cast<uint4*>(shard + mant + (le >> 4)) = e16;
    }
  }
  __device__ static __forceinline__ void roundtrip(float (&v)[16], SrKey key, uint32_t i) {
    const uint32_t E = bfp_group_exponent(v);
    uint32_t w[kWords];
    sr_encode_vals<C, 16>(v, E, key, i, w);
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = sr_decode_val<C>(w, j, E);
  }
};

template <int C>
struct SrLanes<Lanes4<C>> {
  __device__ static __forceinline__ void store_wire(uint8_t* const* to, int n_dst, size_t n_s, size_t le,
                                                    const float (&v)[4], SrKey key, uint32_t i) {
    const uint32_t E = bfp_quad_exponent(v);
    uint32_t w[1];
    sr_encode_vals<C, 4>(v, E, key, i, w);
    for (int k = 0; k < n_dst; ++k) {
      uint8_t* shard = to[k];
      if (shard == nullptr) continue;
      *reinterpret_cast<uint32_t*>(shard + le) = w[0];
      if ((le & 15) == 0) shard[n_s + (le >> 4)] = (uint8_t)E;
    }
  }
  __device__ static __forceinline__ void roundtrip(float (&v)[4], SrKey key, uint32_t i) {
    const uint32_t E = bfp_quad_exponent(v);
    uint32_t w[1];
    sr_encode_vals<C, 4>(v, E, key, i, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sr_decode_val<C>(w, j, E);
  }
};

// ---------------------------------------------------------------- release of stores into peer memory
// A kernel that stores into peers' receive arenas (direct P2P transport) must have every store performed before the
// stream-ordered flag write that tells the peer to read them (p2p_comm.h, memory ordering). Modes (FAN_P2P_RELEASE,
// settable at run time for A/B: p2p_release_mode()):
//   3 cp (default): nothing in the kernel; the transport records a system-scope release event
//     (hipEventReleaseToSystem) on the stream right before it writes the flags: ONE command-processor release
//     per round, ordered after every kernel of the round (2-rank flagship 2.25 vs 2.59 ms/step with "block",
//     profiles/r3_p2p_release_ab.txt);
//   1 block: every wave drains its own stores (s_waitcnt vmcnt(0)), the workgroup meets at a barrier,
//     then ONE lane issues the system-scope release (the valid form of MI355X_MICROARCH.md §Workgroup dispatch);
//   2 thread: every wave issues __threadfence_system() (the round-2 form: one system fence per wave, 4.9 ms/step);
//   0 none: rely on the end-of-kernel release alone (diagnostic only).
int p2p_release_mode();
void set_p2p_release_mode(int mode);
int p2p_grid_cap();  // workgroup cap of the peer-storing kernels (FAN_P2P_GRID)
void set_p2p_grid_cap(int blocks);

__device__ __forceinline__ void p2p_release(int mode) {
  if (mode == 2) {
    __threadfence_system();
  } else if (mode == 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // keep the wait after the write-back (compiler hazard)
    }
  }
}

// ---------------------------------------------------------------- host launchers
// Destination table of a kernel that stores its output straight into several buffers (the direct peer-to-peer
// transport: one entry per rank, each an IPC-mapped slot of that peer's receive arena; nullptr entries skipped).
constexpr int kMaxPeers = 16;
struct WirePtrs {
  uint8_t* p[kMaxPeers];
};

void launch_wire_pack(int codec, int in_dtype, const void* in, void* out, size_t n_s, int n_shards,
                      hipStream_t stream);
void launch_wire_unpack(int codec, int out_dtype, const void* in, void* out, size_t n_s, int n_shards,
                        hipStream_t stream);
// Pack flat elements [begin, end) (multiples of 16) into the shard layout (shards of n_s elements).
void launch_wire_pack_range(int codec, int in_dtype, const void* in, void* out, size_t n_s, size_t begin,
                            size_t end, hipStream_t stream);
// out = sum over slots (slot self_pos replaced by the dense local operand when given).
void launch_wire_reduce(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                        int self_pos, const void* local, void* out_wire, float* out_f32, size_t n_s,
                        hipStream_t stream);
// Fused all-gather epilogue: decode + SGD in place (master f32, optional bf16 copy, optional momentum).
// Shards s with (s % skip_period) == skip_shard are left untouched (skip_shard < 0: none).
// shard_stride: bytes between consecutive shards of `wire` (0: packed, wire_shard_bytes(codec, n_s)) — a gathered
// wire read in place from a receive arena has its shards one arena slot pair apart.
void launch_wire_sgd(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                     float* master, bf16_t* lp, float* mom, SgdParams p, size_t n_valid, hipStream_t stream,
                     size_t shard_stride = 0, const float* clip = nullptr);
// launch_wire_sgd with the AdamW step: `mom` is the first moment, p.var the second, both required.
void launch_wire_adamw(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                       float* master, bf16_t* lp, float* mom, AdamWParams p, size_t n_valid, hipStream_t stream,
                       size_t shard_stride = 0, const float* clip = nullptr);
// launch_wire_sgd with the Lion step: `mom` is its one moment plane, required.
void launch_wire_lion(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                      float* master, bf16_t* lp, float* mom, LionParams p, size_t n_valid, hipStream_t stream,
                      size_t shard_stride = 0, const float* clip = nullptr);
// Global-norm gradient clipping of a clip group (the update requests of one optimizer step), three kinds of launch
// on one stream. The update launchers above and launch_wire_lamb_moments take `clip`, the group's four f32 device
// words {coef, f32(total), f32(max_norm), nonfinite ? 1 : 0}: non-null, the kernel uses grad_scale * clip[0] (one f32
// product, computed once per kernel from a uniform load) in place of grad_scale and changes nothing else, so a
// coefficient of 1.0f gives the unclipped update's bits; nullptr is the unclipped code path itself (another kernel
// instantiation that never reads the pointer). SgdParams is not grown: it is part of the GEMM kernels' argument block.
// 1. launch_wire_sumsq, once per gathered wire region: a read-only pass with launch_wire_sgd's traversal (codecs,
//    shard_stride, skipped shards, the n_valid tail inside a group; values at or past n_valid enter as 0) that sums
//    the exact fp64 squares of the decoded values in a fixed order per lane, wave and block; block b stores its sum at
//    partials[b]. sumsq_partials_for(n_s) blocks — a function of n_s and the grid cap alone. An empty region is refused.
// 2. launch_clip_coef, once per group: one block sums up to kClipSegments segments of partials in segment order and
//    index order (a segment of count 0 contributes nothing) into S and writes the four words:
//    total = sqrt(S) * |grad_scale|, coef = min(1, max_norm / (total + 1e-6)) in fp64, rounded once to f32; S not
//    finite: coef = NaN and words[3] = 1.
// 3. the group's update launches with clip = words.
constexpr int kClipSegments = 8;  // = the engine's request slots: a clip group holds at most that many requests
struct ClipSegments {
  const double* p[kClipSegments];
  int n[kClipSegments];
};
int sumsq_partials_for(size_t n_s);
void launch_wire_sumsq(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                       size_t n_valid, double* partials, hipStream_t stream, size_t shard_stride = 0);
void launch_clip_coef(const ClipSegments& seg, int n_seg, double max_norm, float grad_scale, float* words,
                      hipStream_t stream);
// The trust-ratio (LAMB) epilogue: three launches on one stream.
// Pass 1, launch_wire_lamb_moments: decode the wire as launch_wire_adamw does (codecs, shard_stride, skipped shards,
// n_valid tail), store the new moments (`mom`, p.var) and leave `master` untouched; over the flat elements below
// adapt_end (any value, clamped to n_valid; it may fall inside a 16-value group) accumulate S_w = sum w^2 and
// S_r = sum r^2 in fp64, reduced in a fixed order per lane, wave and block: block b stores {S_w, S_r} at
// partials[2b], partials[2b + 1]. The launch has lamb_partials_for(n_s) blocks — a function of n_s and the grid cap
// alone, so every rank that runs the same launch on the same wire produces the same bits.
int lamb_partials_for(size_t n_s);
void launch_wire_lamb_moments(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                              const float* master, float* mom, LambParams p, size_t n_valid, size_t adapt_end,
                              double* partials, hipStream_t stream, size_t shard_stride = 0,
                              const float* clip = nullptr);
// One block: sums the n_pairs {S_w, S_r} pairs of every pass-1 launch of a request (each lane takes pairs
// t, t + 256, ... in ascending order, the lanes' sums then combine in a fixed tree, all fp64) and writes the three f32
// words {lr * phi, lr, phi}, phi = (float)sqrt(S_w / S_r) when both sums are positive and finite, else 1.
void launch_lamb_ratio(const double* partials, int n_pairs, float lr, float* words, hipStream_t stream);
// Pass 2, launch_wire_lamb_apply: a dense pass over elements [0, n_valid) of master / mom / p.var (the planes pass 1
// left): w' = fma(-(i < adapt_end ? words[0] : words[1]), r, w), lp = bf16(w') when given. Elements of shards s
// (of n_s elements) with (s % skip_period) == skip_shard are left untouched, as in pass 1.
void launch_wire_lamb_apply(float* master, bf16_t* lp, const float* mom, LambParams p, const float* words, size_t n_s,
                            int skip_shard, int skip_period, size_t n_valid, size_t adapt_end, hipStream_t stream);
// Decode to f32/bf16 from a strided wire (as launch_wire_sgd's shard_stride).
void launch_wire_unpack_strided(int codec, int out_dtype, const void* in, size_t shard_stride, void* out, size_t n_s,
                                int n_shards, hipStream_t stream);
// The encoder of the mesh schedule's two stages (the sender's pack, the owner's re-encode), one record for both
// launchers below. plain: the codec's own rounding. feedback (BFP codecs only): residual compensation; `residual` is
// this rank's f32 plane of the elements the launch covers (16-B aligned, zeroed by the caller before the bucket's first
// request), updated in place; ops/bfp_oracle.py ef_pack / ef_reduce define the bits. stochastic (kBfpRne and kBfp4Rne
// only): stateless unbiased rounding under `key` = sr_key(seed, rank, stage); `base` is the bucket index of the
// launch's first element and the launch's last index must be below 2^32; the wire format is unchanged and the bits
// (ops/bfp_oracle.py sr_pack / sr_reduce) do not depend on the grid or the lane layout.
struct WireEncoder {
  enum Kind : int { kPlain, kFeedback, kStochastic };
  Kind kind = kPlain;
  float* residual = nullptr;
  SrKey key{};
  size_t base = 0;
  static WireEncoder feedback(float* residual) { return {kFeedback, residual, {}, 0}; }
  static WireEncoder stochastic(SrKey key, size_t base) { return {kStochastic, nullptr, key, base}; }
};
// Sender stage: pack shards 0..n_shards-1 of `in`, shard s stored at dst.p[s]; a null destination skips its shard
// entirely (neither encoded nor fed back). plain: every shard alike. feedback: x = f32(in) + residual (one f32 add; the
// group exponent comes from x), residual' = x - dec(enc(x)) (one f32 subtract; dec is the decoder's real output).
// feedback and stochastic: shard self_shard (-1: none) takes the plain encoder, from `in` alone, and its residual is
// left alone. peers: the destinations are peers' receive slots — the P2P grid cap, and a system-scope release at the
// end so a peer may read the stores once the (stream-ordered) ready flag is set; otherwise a local buffer, the
// ordinary grid and no release.
void launch_wire_pack_to(int codec, int in_dtype, const void* in, const WirePtrs& dst, size_t n_s, int n_shards,
                         int self_shard, const WireEncoder& enc, bool peers, hipStream_t stream);
// Owner stage: launch_wire_reduce (local operand required) whose encoded output is stored to every non-null dst.p[i]
// (i < n_dst; `peers` as above: the owner's reduced shard goes straight into every peer's receive slot). feedback:
// y = (the slots' sum) + residual, the add after the slot sum, residual' = y - dec(enc(y)); `residual` is the owner
// shard's n_s elements of the plane. stochastic: the sum is encoded once, every destination receives the same words;
// `base` is the owner shard's first element in the bucket. Both lane layouts (set_wire_reduce4), the same bits.
void launch_wire_reduce_to(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots, int self_pos,
                           const void* local, const WirePtrs& dst, int n_dst, size_t n_s, const WireEncoder& enc,
                           bool peers, hipStream_t stream);
// Sharded update of the owner's shard (engine shard_update mode, ZeRO-1 style): sum the N received wire shards
// (slot self_pos replaced by the dense local operand), take the sum through the wire codec's round trip in registers
// (exactly the values every rank would decode from the re-encoded owner shard in the unsharded schedule), apply SGD to
// `master` / `mom` (this shard's planes; elements at or past n_valid keep their values) and write the updated
// weights in bf16 to every non-null dst.p[i] (i < n_dst: this rank's own copy and, on the direct P2P transport,
// every peer's receive slot), ending with the P2P release of `rel` (-1: none, a local output). Same arithmetic in
// the same order as wire_reduce (re-encode) + wire_sgd, so the weights are bit-identical to the unsharded schedule.
void launch_wire_reduce_sgd(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                            int self_pos, const void* local, float* master, float* mom, SgdParams p, size_t n_valid,
                            const WirePtrs& dst, int n_dst, size_t n_s, bool peers, hipStream_t stream);
// launch_wire_reduce_sgd with the AdamW step (`mom` / p.var: this shard's moment planes, both required):
// bit-identical to wire_reduce (re-encode) + wire_adamw.
void launch_wire_reduce_adamw(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                              int self_pos, const void* local, float* master, float* mom, AdamWParams p,
                              size_t n_valid, const WirePtrs& dst, int n_dst, size_t n_s, bool peers,
                              hipStream_t stream);
// launch_wire_reduce_sgd with the Lion step (`mom`: this shard's moment plane, required): bit-identical to
// wire_reduce (re-encode) + wire_lion.
void launch_wire_reduce_lion(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                             int self_pos, const void* local, float* master, float* mom, LionParams p,
                             size_t n_valid, const WirePtrs& dst, int n_dst, size_t n_s, bool peers,
                             hipStream_t stream);
// AdamW with both moments in 8-bit block floating point (moment_codec "bfp8"; ops/bfp_oracle.py adamw_q defines the
// bits). mom_q / var_q: the bucket's WHOLE planes, each [int8 mant[plane_elems]][u8 exp[plane_elems/16]] (the kBfpRne
// shard layout of one shard of plane_elems elements, 16-B aligned, plane_elems % 256 == 0 and below 2^32), the first
// holding m, the second r = sqrt(v). The wire region (launch_wire_adamw's traversal: every wire codec, shards, skipped
// shards, shard_stride, the n_valid tail, the clip words' one product) starts at element elem_base (% 256 == 0) of the
// bucket: region element e reads and writes mant[elem_base + e] and exp[(elem_base + e) / 16], and master / lp at e.
// Per element: m_old, r_old decoded, v_old = r_old * r_old, adamw_update unchanged, m' and r' = sqrtf(v') encoded per
// group with the stochastic encoder under sr_key(seed, 16, 0) / sr_key(seed, 16, 1), r' with the floor (kFloor1). In a
// group that straddles n_valid the values at or past it enter the encode as 0; groups entirely past it keep their
// bytes. The bits do not depend on the grid.
constexpr int kMomentRank = 16;  // sr_key's rank slot of the state's random bytes (the wire uses ranks 0..15)
void launch_wire_adamw_q(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                         float* master, bf16_t* lp, uint8_t* mom_q, uint8_t* var_q, size_t plane_elems,
                         size_t elem_base, AdamWParams p, uint64_t seed, size_t n_valid, hipStream_t stream,
                         size_t shard_stride = 0, const float* clip = nullptr);
// Workgroup cap of launch_wire_adamw_q below the wire kernels' own (0, the default: none), settable at run time like
// set_p2p_grid_cap: the bits do not depend on the grid, which is what a one-block launch shows.
int moment_grid_cap();
void set_moment_grid_cap(int blocks);
// BFP codecs: the lane-contiguous form of that kernel, 4 values per lane (1, default) or one 16-value group per lane
// (0) (FAN_WIRE_REDUCE4); bit-identical either way
void set_wire_reduce4(int on);
int wire_reduce4();

}  // namespace fan
