// Wire-codec kernels of the compressed all-reduce engine (gfx950).
//
// All kernels are HBM-streaming: each lane owns one 16-element BFP group (32-B loads of bf16, 64-B of f32; one
// 16-B mantissa store, and the group exponents of 16 consecutive lanes leave as one 16-B store, bfp_format.h
// WireLane16) — except wire_pack_range (the short bias / padding tails at any 16-element offset), where a lane
// PAIR owns a group. Grids are capped at 2048 blocks and grid-stride over every shard, so each lane runs the same
// number of iterations per shard and 16-lane segments never split (group counts are multiples of 16). The three
// reduce kernels (wire_reduce, wire_reduce_to, wire_reduce_sgd) are one body each over a lane layout (bfp_format.h
// Lanes16 / Lanes4): for the BFP codecs at up to two slots a lane owns 4 values and 4 lanes a group (with_lanes).
//
// Reference parity:
//   wire_pack    = bfp_adapter TX (hw/bfp_adapter.sv:100-154, 279-379)
//   wire_unpack  = bfp_adapter RX (hw/bfp_adapter.sv:489-699)
//   wire_reduce  = the ring engine's 8-lane fadd stage + re-encode (hw/all_reduce.sv:1090-1183)
//   wire_sgd     = weight_update FFMA w' = fma(-lr, g, w) (hw/weight_update.sv:433-452), fused
//                  into the all-gather epilogue so weights never take an extra HBM round trip.
//   AdamW        = no counterpart in the reference (its update unit is one FFMA): the update kernels (wire_sgd,
//                  wire_reduce_sgd in both lane layouts) instantiated with AdamWParams run adamw_update
//                  (bfp_format.h) per value, with a second moment plane.
//   trust ratio  = AdamW scaled per bucket by ||w|| / ||update|| (LAMB): no element may move before two norms over
//                  the whole bucket exist, so three launches — wire_lamb_moments (pass 1), lamb_ratio,
//                  wire_lamb_apply (pass 2) — with a deterministic fp64 reduction in between (no atomics).
//   wire_pack_to, wire_reduce_to = the mesh schedule's two encoders, each one kernel (traversal, destination table,
//                  release) over an encoder policy: EncPlain, the codec as it is, and two forms without a counterpart
//                  in the reference —
//   error feedback = EncFeedback (what the reference's adapter drops is gone): a per-rank f32 residual plane beside the
//                  unchanged wire;
//   stochastic rounding = EncStochastic: rounding up with probability equal to the dropped fraction (a counter-based
//                  hash per 4 values, no state).
#include "bfp/bfp_format.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <type_traits>

namespace fan {

static int wire_max_blocks();

// The lane-contiguous (4 values per lane) BFP reduce kernels pay off where the dense f32 operands dominate the bytes
// (the local gradient, the master / momentum planes) and cost where the 1-byte wire slots do — one group per lane
// already reads a slot's mantissas 1 KiB per wave instruction, 4 values per lane 256 B: C.wire_reduce of 8 slots
// measured 38.1 vs 33.6 us, of 2 slots 17.0 vs 17.1 (tools/probes/wire_reduce4_probe.py). So they run for at most two
// slots (world 1 through the multi-rank path, 2 ranks); FAN_WIRE_REDUCE4=0 turns them off.
static bool wire_reduce4_for(int n_slots) { return n_slots <= 2 && wire_reduce4() != 0; }

static std::atomic<int>& release_mode_flag() {
  static std::atomic<int> m{[] {
    const char* e = getenv("FAN_P2P_RELEASE");
    if (!e) return 3;
    if (!strcmp(e, "thread")) return 2;
    if (!strcmp(e, "none")) return 0;
    if (!strcmp(e, "block")) return 1;
    return 3;
  }()};
  return m;
}
int p2p_release_mode() { return release_mode_flag().load(std::memory_order_relaxed); }
void set_p2p_release_mode(int mode) { release_mode_flag().store(mode < 0 ? 0 : mode > 3 ? 3 : mode); }

// Grid cap of the kernels that store into peers' receive arenas (FAN_P2P_GRID; 0 = auto): with the in-kernel
// release forms every workgroup ends with one system-scope release, so fewer, longer-lived workgroups pay fewer of
// them — "block" (the cross-device default) 128: 2 ranks, 2.27 ms/step at 64-128 workgroups vs 2.36 at 256, 2.49 at
// 512, 2.63 at 1024, 2.83 at 2048, i.e. the whole cost of the in-kernel release over "cp" (2.27)
// (profiles/r4_p2p_block_grid_sweep.jsonl); "thread" 512; with the command-processor release nothing is paid per
// workgroup and the cap is the ordinary one (profiles/r3_wire_store_bw.jsonl: 18.95 us at 512 vs 17.39 at 2048).
static std::atomic<int>& p2p_grid_flag() {
  static std::atomic<int> g{[] {
    const char* e = getenv("FAN_P2P_GRID");
    return e ? atoi(e) : 0;
  }()};
  return g;
}
int p2p_grid_cap() {
  const int g = p2p_grid_flag().load(std::memory_order_relaxed);
  if (g > 0) return g;
  const int m = p2p_release_mode();
  return m == 1 ? 128 : m == 2 ? 512 : wire_max_blocks();
}
void set_p2p_grid_cap(int blocks) { p2p_grid_flag().store(blocks > 0 ? blocks : 0); }

// Upper bound on the workgroups of one wire kernel (env FAN_WIRE_MAX_BLOCKS, default 2048): these memory-bound
// kernels run on the comm stream beside the GEMMs at world > 1, and every CU they occupy cannot host a GEMM
// workgroup (profiles/r1_gemm_cu_contention_probe.txt), so the footprint is a tunable. Measured at world 1 through
// the multi-rank path: capping it at 512 / 128 / 64 made the step 0.4 / 4 / 11 % slower
// (profiles/r1_wire_grid_cap_ab.txt) — the kernels are on the critical path more than they crowd the GEMMs.
static int wire_max_blocks() {
  static const int v = [] {
    const char* e = getenv("FAN_WIRE_MAX_BLOCKS");
    const int x = e ? atoi(e) : 0;
    return x > 0 ? x : 2048;
  }();
  return v;
}

namespace {

constexpr int kBlock = 256;

template <typename TIN, int C>
__global__ void __launch_bounds__(kBlock) wire_pack_kernel(const TIN* __restrict__ in, uint8_t* __restrict__ out,
                                                          size_t n_s, int n_shards) {
  const size_t tasks = n_s >> 4;  // one 16-value group per lane (WireLane16)
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t sb = wire_shard_bytes(C, n_s);
  for (int s = 0; s < n_shards; ++s) {
    const TIN* src = in + (size_t)s * n_s;
    uint8_t* dst = out + (size_t)s * sb;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      float v[16];
      DenseLane16<TIN>::load16(src, t << 4, v);
      WireLane16<C>::store16(dst, n_s, t << 4, v);
    }
  }
}

// Pack flat elements [begin, end) (multiples of 16) of a bucket into its shard layout (shards of n_s elements):
// the part of a bucket the producing GEMM did not encode itself (bias gradient + padding).
template <typename TIN, int C>
__global__ void __launch_bounds__(kBlock) wire_pack_range_kernel(const TIN* __restrict__ in, uint8_t* __restrict__ out,
                                                                size_t n_s, size_t begin, size_t end) {
  const size_t tasks = (end - begin) >> 3;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t sb = wire_shard_bytes(C, n_s);
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
    const size_t f = begin + (t << 3);
    const size_t sh = f / n_s;
    float v[8];
    DenseLane<TIN>::load8(in, f, v);
    WireLane<C>::store8(out + sh * sb, n_s, f - sh * n_s, v);
  }
}

template <typename TOUT, int C>
__global__ void __launch_bounds__(kBlock) wire_unpack_kernel(const uint8_t* __restrict__ in, TOUT* __restrict__ out,
                                                            size_t n_s, int n_shards) {
  const size_t tasks = n_s >> 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t sb = wire_shard_bytes(C, n_s);
  for (int s = 0; s < n_shards; ++s) {
    const uint8_t* src = in + (size_t)s * sb;
    TOUT* dst = out + (size_t)s * n_s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      float v[16];
      WireLane16<C>::load16(src, n_s, t << 4, v);
      DenseLane16<TOUT>::store16(dst, t << 4, v);
    }
  }
}

// The three reduce kernels below are written once against a lane layout L (bfp_format.h: Lanes16<C>, a group per lane,
// or Lanes4<C>, 4 values per lane and 4 lanes a group, BFP codecs): a lane's trip covers L::kVals values at element le.

// acc = the sum of the n_slots slots' values at le, in slot order; slot self_pos comes from the dense local operand.
template <typename L, typename TL, bool HAS_LOCAL = true>
__device__ __forceinline__ void sum_slots(const uint8_t* __restrict__ slots, size_t slot_stride, int n_slots,
                                          int self_pos, const TL* __restrict__ local, size_t n_s, size_t le,
                                          float (&acc)[L::kVals]) {
#pragma unroll
  for (int j = 0; j < L::kVals; ++j) acc[j] = 0.0f;
  for (int r = 0; r < n_slots; ++r) {
    float v[L::kVals];
    if (HAS_LOCAL && r == self_pos) L::load_dense(local, le, v);
    else L::load_wire(slots + (size_t)r * slot_stride, n_s, le, v);
#pragma unroll
    for (int j = 0; j < L::kVals; ++j) acc[j] += v[j];
  }
}

template <typename L, typename TL, bool HAS_LOCAL, bool OUT_WIRE, bool OUT_F32>
__global__ void __launch_bounds__(kBlock)
    wire_reduce_kernel(const uint8_t* __restrict__ slots, size_t slot_stride, int n_slots, int self_pos,
                       const TL* __restrict__ local, uint8_t* __restrict__ out_wire, float* __restrict__ out_f32,
                       size_t n_s) {
  const size_t tasks = n_s / L::kVals;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
    const size_t le = t * L::kVals;
    float acc[L::kVals];
    sum_slots<L, TL, HAS_LOCAL>(slots, slot_stride, n_slots, self_pos, local, n_s, le, acc);
    if (OUT_F32) L::store_f32(out_f32, le, acc);
    if (OUT_WIRE) L::store_wire(out_wire, n_s, le, acc);
  }
}

// ---------------------------------------------------------------- the mesh schedule's two encoders
// Pack and reduce with the encoded output stored into a table of destinations (the copying transports' buffers, or
// peers' receive slots over xGMI), then the release before the kernel retires. Each kernel holds its traversal once and
// is instantiated over an encoder policy Enc, the device side of bfp_format.h WireEncoder: the form's arguments by
// value, and what happens between "the lane's values are in registers" and the end of the loop trip, chosen at compile
// time (`if constexpr` in the kernel bodies: as device functions of the policy structs the same statements cost the
// feedback kernels registers and one of them a wave, profiles/wire_encoder_fold_resources.txt). No form uses atomics
// or LDS; the arithmetic and the store order of each are its own and are NOT shared.
enum EncForm { kEncPlain, kEncFeedback, kEncStochastic };

struct EncPlain {  // the codec as it is
  static constexpr EncForm kForm = kEncPlain;
  template <int C>
  static constexpr bool kHas = true;
};

// Error feedback (bfp_oracle.ef_pack / ef_reduce): both encoders keep what they drop. The f32 residual plane enters the
// encoder's input with one f32 add, and x - dec(enc(x)) (one f32 subtract; dec is the decoder's real output,
// Lanes*::roundtrip) is stored back at the same elements. A lane reads and writes only its own elements of the plane,
// and the two stages cover disjoint shards of it. resid: the sender's whole plane / the owner shard's part of it.
struct EncFeedback {
  static constexpr EncForm kForm = kEncFeedback;
  template <int C>
  static constexpr bool kHas = codec_shared_exp(C);  // (a raw codec drops nothing)
  float* resid;
};

// Stochastic rounding (bfp_oracle.sr_pack / sr_reduce): the unbiased rounding of bfp_format.h SrLanes, no state; the
// element index that selects the random byte is base + (offset in the launch), whatever the grid.
struct EncStochastic {
  static constexpr EncForm kForm = kEncStochastic;
  template <int C>
  static constexpr bool kHas = codec_sr(C);
  SrKey key;
  uint32_t base;
};

// Sender stage: a group per lane; a null destination skips its shard entirely. Plain: every shard alike, and the
// release is unconditional (p2p_release of a negative mode does nothing). The other two: shard self_shard takes the
// plain encoder (a grid-uniform branch) from `in` alone, its residual neither read nor written; rel < 0 (a local
// output) skips the release.
template <typename TIN, int C, typename Enc>
__global__ void __launch_bounds__(kBlock)
    wire_pack_to_kernel(const TIN* __restrict__ in, WirePtrs dst, size_t n_s, int n_shards, int rel, int self_shard,
                        Enc enc) {
  static_assert(Enc::template kHas<C>, "not a form of this codec");
  const size_t tasks = n_s >> 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (int s = 0; s < n_shards; ++s) {
    uint8_t* d = dst.p[s];
    if (d == nullptr) continue;
    const size_t se = (size_t)s * n_s;  // the shard's first element
    const TIN* src = in + se;
    const bool self = s == self_shard;  // (uniform over the grid)
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      float v[16];
      DenseLane16<TIN>::load16(src, t << 4, v);
      if constexpr (Enc::kForm == kEncFeedback) {
        float* e = enc.resid + se;
        if (!self) {
          float r[16];
          DenseLane16<float>::load16(e, t << 4, r);
#pragma unroll
          for (int j = 0; j < 16; ++j) v[j] = v[j] + r[j];
        }
        WireLane16<C>::store16(d, n_s, t << 4, v);
        if (!self) {
          float q[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) q[j] = v[j];
          Lanes16<C>::roundtrip(q);
#pragma unroll
          for (int j = 0; j < 16; ++j) q[j] = v[j] - q[j];
          DenseLane16<float>::store16(e, t << 4, q);
        }
      } else if constexpr (Enc::kForm == kEncStochastic) {
        const uint32_t i = enc.base + (uint32_t)se + (uint32_t)(t << 4);  // the group's first element in the bucket
        if (self) WireLane16<C>::store16(d, n_s, t << 4, v);
        else SrLanes<Lanes16<C>>::store_wire(&d, 1, n_s, t << 4, v, enc.key, i);
      } else {
        WireLane16<C>::store16(d, n_s, t << 4, v);
      }
    }
  }
  if (Enc::kForm == kEncPlain || rel >= 0) p2p_release(rel);
}

// Owner stage, in either lane layout (same operations per value, so the same bits): the slots' sum to every non-null
// destination (a wave-uniform condition: every lane of a group's segment stores). Plain: one encode per destination.
// Feedback: y = sum + residual to the destinations, then y - roundtrip(y) stored back. Stochastic: the sum is encoded
// once and the same words go to every destination. The release as in the sender.
template <typename L, typename TL, typename Enc>
__global__ void __launch_bounds__(kBlock)
    wire_reduce_to_kernel(const uint8_t* __restrict__ slots, size_t slot_stride, int n_slots, int self_pos,
                          const TL* __restrict__ local, WirePtrs dst, int n_dst, size_t n_s, int rel, Enc enc) {
  const size_t tasks = n_s / L::kVals;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
    const size_t le = t * L::kVals;
    float acc[L::kVals];
    sum_slots<L>(slots, slot_stride, n_slots, self_pos, local, n_s, le, acc);
    if constexpr (Enc::kForm == kEncStochastic) {
      SrLanes<L>::store_wire(dst.p, n_dst, n_s, le, acc, enc.key, enc.base + (uint32_t)le);
    } else {
      float e[L::kVals];
      if constexpr (Enc::kForm == kEncFeedback) {
        L::load_dense(enc.resid, le, e);
#pragma unroll
        for (int j = 0; j < L::kVals; ++j) acc[j] = acc[j] + e[j];
      }
      for (int i = 0; i < n_dst; ++i)
        if (dst.p[i] != nullptr) L::store_wire(dst.p[i], n_s, le, acc);
      if constexpr (Enc::kForm == kEncFeedback) {
#pragma unroll
        for (int j = 0; j < L::kVals; ++j) e[j] = acc[j];
        L::roundtrip(e);
#pragma unroll
        for (int j = 0; j < L::kVals; ++j) e[j] = acc[j] - e[j];
        L::store_f32(enc.resid, le, e);
      }
    }
  }
  if (Enc::kForm == kEncPlain || rel >= 0) p2p_release(rel);
}

// The merged reduce-and-update of the owner's shard: the slots' sum through the codec's round trip, then the update
// per value (the same operations as wire_reduce's re-encode + wire_sgd_kernel, so the same bits), the new weights in
// bf16 to every destination. P: SgdParams, AdamWParams (HAS_MOM: mom is the first moment, p.var the second), or
// LionParams (HAS_MOM: mom is its one moment plane).
template <typename L, typename TL, bool HAS_MOM, typename P = SgdParams>
__global__ void __launch_bounds__(kBlock)
    wire_reduce_sgd_kernel(const uint8_t* __restrict__ slots, size_t slot_stride, int n_slots, int self_pos,
                           const TL* __restrict__ local, float* __restrict__ master, float* __restrict__ mom,
                           P p, size_t n_valid, WirePtrs dst, int n_dst, size_t n_s, int rel) {
  constexpr bool kAdam = std::is_same<P, AdamWParams>::value;
  constexpr bool kLion = std::is_same<P, LionParams>::value;
  static_assert(!kAdam || HAS_MOM, "AdamW needs both moment planes");
  static_assert(!kLion || HAS_MOM, "Lion needs its moment plane");
  const size_t tasks = n_s / L::kVals;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
    const size_t le = t * L::kVals;
    float acc[L::kVals];
    sum_slots<L>(slots, slot_stride, n_slots, self_pos, local, n_s, le, acc);
    L::roundtrip(acc);
    float w[L::kVals], m[L::kVals];
    L::load_dense(master, le, w);
    if (HAS_MOM) L::load_dense(mom, le, m);
    if constexpr (kAdam) {
      float v2[L::kVals];
      L::load_dense(p.var, le, v2);
#pragma unroll
      for (int j = 0; j < L::kVals; ++j)
        if (le + j < n_valid) adamw_update(p, acc[j], w[j], m[j], v2[j]);
      if (le < n_valid) L::store_f32(p.var, le, v2);
    } else if constexpr (kLion) {
#pragma unroll
      for (int j = 0; j < L::kVals; ++j)
        if (le + j < n_valid) lion_update(p, acc[j], w[j], m[j]);
    } else {
#pragma unroll
      for (int j = 0; j < L::kVals; ++j)
        if (le + j < n_valid) sgd_update(p, acc[j], w[j], m[j], HAS_MOM);
    }
    if (le < n_valid) {
      L::store_f32(master, le, w);
      if (HAS_MOM) L::store_f32(mom, le, m);
    }
    for (int i = 0; i < n_dst; ++i)
      if (dst.p[i] != nullptr) L::store_bf16(reinterpret_cast<bf16_t*>(dst.p[i]), le, w);
  }
  if (rel >= 0) p2p_release(rel);
}

template <typename TOUT, int C>
__global__ void __launch_bounds__(kBlock) wire_unpack_strided_kernel(const uint8_t* __restrict__ in,
                                                                    size_t shard_stride, TOUT* __restrict__ out,
                                                                    size_t n_s, int n_shards) {
  const size_t tasks = n_s >> 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (int s = 0; s < n_shards; ++s) {
    const uint8_t* src = in + (size_t)s * shard_stride;
    TOUT* dst = out + (size_t)s * n_s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      float v[16];
      WireLane16<C>::load16(src, n_s, t << 4, v);
      DenseLane16<TOUT>::store16(dst, t << 4, v);
    }
  }
}

// CLIP: the request belongs to a clip group — grad_scale is multiplied by the group's coefficient clip[0] (four f32
// words clip_coef_kernel wrote earlier on the stream), one f32 product per kernel from a uniform load; nothing else in
// the update changes, and a coefficient of 1.0f leaves grad_scale's bits. !CLIP: `clip` is not read.
template <int C, bool HAS_LP, bool HAS_MOM, typename P = SgdParams, bool CLIP = false>
__global__ void __launch_bounds__(kBlock)
    wire_sgd_kernel(const uint8_t* __restrict__ wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                    float* __restrict__ master, bf16_t* __restrict__ lp, float* __restrict__ mom, P p,
                    size_t n_valid, size_t sb, const float* __restrict__ clip) {
  constexpr bool kAdam = std::is_same<P, AdamWParams>::value;
  constexpr bool kLion = std::is_same<P, LionParams>::value;
  static_assert(!kAdam || HAS_MOM, "AdamW needs both moment planes");
  static_assert(!kLion || HAS_MOM, "Lion needs its moment plane");
  if constexpr (CLIP) p.grad_scale = p.grad_scale * clip[0];
  // 8 elements per lane here (a read-only wire: the 16-per-lane store layout buys nothing, and the smaller
  // register footprint streams master / lp faster: 33.5 vs 42.5 us on a 16.8 M bucket in the flagship step)
  const size_t tasks = n_s >> 3;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (int s = 0; s < n_shards; ++s) {
    if (skip_shard >= 0 && (s % skip_period) == skip_shard) continue;
    const uint8_t* src = wire + (size_t)s * sb;
    const size_t base = (size_t)s * n_s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      const size_t e = base + (t << 3);
      if (e >= n_valid) continue;
      float g[8], w[8];
      WireLane<C>::load8(src, n_s, t << 3, g);
      DenseLane<float>::load8(master, e, w);
      float m[8];
      if (HAS_MOM) DenseLane<float>::load8(mom, e, m);
      const bool full = e + 8 <= n_valid;
      if constexpr (kAdam) {
        // the second-moment plane: read whole (the planes are padded to the wire's shards), stored as master is
        float v2[8];
        DenseLane<float>::load8(p.var, e, v2);
#pragma unroll
        for (int j = 0; j < 8; ++j) adamw_update(p, g[j], w[j], m[j], v2[j]);
        if (full) {
          DenseLane<float>::store8(p.var, e, v2);
        } else {
          for (int j = 0; j < 8 && e + j < n_valid; ++j) p.var[e + j] = v2[j];
        }
      } else if constexpr (kLion) {
#pragma unroll
        for (int j = 0; j < 8; ++j) lion_update(p, g[j], w[j], m[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) sgd_update(p, g[j], w[j], m[j], HAS_MOM);
      }
      if (full) {
        DenseLane<float>::store8(master, e, w);
        if (HAS_MOM) DenseLane<float>::store8(mom, e, m);
        if (HAS_LP) DenseLane<bf16_t>::store8(lp, e, w);
      } else {
        for (int j = 0; j < 8 && e + j < n_valid; ++j) {
          master[e + j] = w[j];
          if (HAS_MOM) mom[e + j] = m[j];
          if (HAS_LP) lp[e + j] = f32_to_bf16(w[j]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- AdamW with 8-bit moment planes (moment_codec bfp8)
// wire_sgd_kernel's traversal (shards, skipped shards, shard stride, the n_valid tail, the clip words' one product)
// with both moments read from and written to the bucket's 8-bit planes (bfp_format.h launch_wire_adamw_q). A lane owns
// a whole 16-value group per trip: the planes' shared exponents then need no cross-lane exchange (the 8-per-lane body's
// `continue` on e >= n_valid would leave lanes out of a shuffle), a plane's mantissas are ONE 16-B load and ONE 16-B
// store, and the exponent bytes go as WireLane16's: a byte load per lane, and the 16 bytes of 16 consecutive lanes
// leave as one 16-B store by lane 16k. A 16-lane segment covers 256 consecutive elements from a multiple of 256 (grid
// and stride are multiples of 256 lanes, n_s, elem_base and plane_elems multiples of 256), so it is entirely inside the
// `t` loop or outside it, and entirely inside the planes when its first group is below n_valid; its lanes past n_valid
// carry their group's OLD exponent byte through the gather, so groups the update does not touch keep their bytes.
// No atomics, no LDS, no scratch (every array index is a compile-time constant).
template <int C, bool HAS_LP, bool CLIP>
__global__ void __launch_bounds__(kBlock)
    wire_adamw_q_kernel(const uint8_t* __restrict__ wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                        float* __restrict__ master, bf16_t* __restrict__ lp, uint8_t* mom_q, uint8_t* var_q,
                        size_t plane_elems, size_t elem_base, AdamWParams p, SrKey key_m, SrKey key_r, size_t n_valid,
                        size_t sb, const float* __restrict__ clip) {
  if constexpr (CLIP) p.grad_scale = p.grad_scale * clip[0];  // (as wire_sgd_kernel)
  const size_t tasks = n_s >> 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  uint8_t* const mom_e = mom_q + plane_elems;
  uint8_t* const var_e = var_q + plane_elems;
  const size_t seg_lane = (size_t)(threadIdx.x & 15) << 4;  // elements between the segment's first group and this one
  for (int s = 0; s < n_shards; ++s) {
    if (skip_shard >= 0 && (s % skip_period) == skip_shard) continue;
    const uint8_t* src = wire + (size_t)s * sb;
    const size_t base = (size_t)s * n_s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      const size_t e = base + (t << 4);
      if (e - seg_lane >= n_valid) continue;  // the whole 16-lane segment is past n_valid: all its lanes leave
      const size_t i = elem_base + e;          // the group's first element in the padded bucket
      const bool act = e < n_valid;
      uint32_t Em = mom_e[i >> 4], Er = var_e[i >> 4];
      if (act) {
        float g[16], w[16], m[16], r[16];
        WireLane16<C>::load16(src, n_s, t << 4, g);
        DenseLane16<float>::load16(master, e, w);
        const uint4 qm = *reinterpret_cast<const uint4*>(mom_q + i);
        const uint4 qr = *reinterpret_cast<const uint4*>(var_q + i);
        const uint32_t qmw[4] = {qm.x, qm.y, qm.z, qm.w}, qrw[4] = {qr.x, qr.y, qr.z, qr.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          m[j] = bfp_decode_rne((int32_t)(int8_t)(uint8_t)(qmw[j >> 2] >> (8 * (j & 3))), Em);
          const float ro = bfp_decode_rne((int32_t)(int8_t)(uint8_t)(qrw[j >> 2] >> (8 * (j & 3))), Er);
          float v = ro * ro;
          adamw_update(p, g[j], w[j], m[j], v);
          r[j] = sqrtf(v);  // the value adamw_update's denominator used
        }
        if (e + 16 <= n_valid) {
          DenseLane16<float>::store16(master, e, w);
          if (HAS_LP) DenseLane16<bf16_t>::store16(lp, e, w);
        } else {
          // the group straddles n_valid: values at or past it keep their weights and enter the encode as 0
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            if (e + j < n_valid) {
              master[e + j] = w[j];
              if (HAS_LP) lp[e + j] = f32_to_bf16(w[j]);
            } else {
              m[j] = 0.0f;
              r[j] = 0.0f;
            }
          }
        }
        Em = bfp_group_exponent(m);
        Er = bfp_group_exponent(r);
        uint32_t wm[4], wr[4];
        sr_encode_vals<kBfpRne, 16>(m, Em, key_m, (uint32_t)i, wm);
        sr_encode_vals<kBfpRne, 16, true>(r, Er, key_r, (uint32_t)i, wr);
        *reinterpret_cast<uint4*>(mom_q + i) = make_uint4(wm[0], wm[1], wm[2], wm[3]);
        *reinterpret_cast<uint4*>(var_q + i) = make_uint4(wr[0], wr[1], wr[2], wr[3]);
      }
      // exponent planes: one 16-B store each by lane 16k (WireLane16); every lane of the segment is here
      const uint4 em16 = bfp_gather_exponents(Em), er16 = bfp_gather_exponents(Er);
      if ((threadIdx.x & 15) == 0) {
        *reinterpret_cast<uint4*>(mom_e + (i >> 4)) = em16;
        *reinterpret_cast<uint4*>(var_e + (i >> 4)) = er16;
      }
    }
  }
}

// ---------------------------------------------------------------- trust-ratio (LAMB) epilogue
// Fixed-order fp64 sums of kN values over the workgroup: the wave's lanes by shuffles (32, 16, ... 1), then the waves'
// sums in wave order by thread 0 through LDS (an array per instantiation). Every thread of the block must call it; the
// results are valid in thread 0.
template <int kN>
__device__ __forceinline__ void block_sum(double (&a)[kN]) {
  __shared__ double red[kN][kBlock / 64];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kN; ++k) a[k] += __shfl_down(a[k], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kN; ++k) red[k][threadIdx.x >> 6] = a[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kN; ++k) a[k] = red[k][0];
#pragma unroll
    for (int i = 1; i < kBlock / 64; ++i) {
#pragma unroll
      for (int k = 0; k < kN; ++k) a[k] += red[k][i];
    }
  }
}

// Pass 1: wire_sgd_kernel's traversal (8 values per lane, shards, skipped shards, the n_valid tail); stores the new
// moments, reads master only. The lane's fp64 sums grow in its own iteration order, which the grid alone decides.
template <int C, bool CLIP = false>
__global__ void __launch_bounds__(kBlock)
    wire_lamb_moments_kernel(const uint8_t* __restrict__ wire, size_t n_s, int n_shards, int skip_shard,
                             int skip_period, const float* __restrict__ master, float* __restrict__ mom, LambParams p,
                             size_t n_valid, size_t adapt_end, size_t sb, double* __restrict__ partials,
                             const float* __restrict__ clip) {
  if constexpr (CLIP) p.grad_scale = p.grad_scale * clip[0];  // (as wire_sgd_kernel)
  const size_t tasks = n_s >> 3;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  double sw = 0.0, sr = 0.0;
  for (int s = 0; s < n_shards; ++s) {
    if (skip_shard >= 0 && (s % skip_period) == skip_shard) continue;
    const uint8_t* src = wire + (size_t)s * sb;
    const size_t base = (size_t)s * n_s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      const size_t e = base + (t << 3);
      if (e >= n_valid) continue;
      float g[8], w[8], m[8], v2[8];
      WireLane<C>::load8(src, n_s, t << 3, g);
      DenseLane<float>::load8(master, e, w);
      DenseLane<float>::load8(mom, e, m);
      DenseLane<float>::load8(p.var, e, v2);
#pragma unroll
      for (int j = 0; j < 8; ++j) lamb_moments(p, g[j], m[j], v2[j]);
      if (e < adapt_end) {  // (adapt_end <= n_valid: the launcher clamps it)
        // branch-free per value: a value at or past adapt_end enters as 0, and s + 0.0 is s bit for bit
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool in = e + j < adapt_end;
          const float r = lamb_direction(p, w[j], m[j], v2[j]);
          const double wa = in ? (double)w[j] : 0.0, ra = in ? (double)r : 0.0;
          sw = fma(wa, wa, sw);
          sr = fma(ra, ra, sr);
        }
      }
      if (e + 8 <= n_valid) {
        DenseLane<float>::store8(mom, e, m);
        DenseLane<float>::store8(p.var, e, v2);
      } else {
        for (int j = 0; j < 8 && e + j < n_valid; ++j) {
          mom[e + j] = m[j];
          p.var[e + j] = v2[j];
        }
      }
    }
  }
  double sums[2] = {sw, sr};
  block_sum(sums);
  if (threadIdx.x == 0) {
    partials[2 * (size_t)blockIdx.x] = sums[0];
    partials[2 * (size_t)blockIdx.x + 1] = sums[1];
  }
}

__global__ void __launch_bounds__(kBlock)
    lamb_ratio_kernel(const double* __restrict__ partials, int n_pairs, float lr, float* __restrict__ words) {
  double sums[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < n_pairs; i += kBlock) {
    sums[0] += partials[2 * (size_t)i];
    sums[1] += partials[2 * (size_t)i + 1];
  }
  block_sum(sums);
  if (threadIdx.x == 0) {
    const double sw = sums[0], sr = sums[1];
    const bool ok = sw > 0.0 && sr > 0.0 && sw < __builtin_huge_val() && sr < __builtin_huge_val();
    const float phi = ok ? (float)sqrt(sw / sr) : 1.0f;
    words[0] = lr * phi;
    words[1] = lr;
    words[2] = phi;
  }
}

// Pass 2: dense, 4 values per lane (16-B loads of the three planes, one 16-B store of master, 8 B of bf16).
template <bool HAS_LP>
__global__ void __launch_bounds__(kBlock)
    wire_lamb_apply_kernel(float* __restrict__ master, bf16_t* __restrict__ lp, const float* __restrict__ mom,
                           LambParams p, const float* __restrict__ words, size_t n_s, int skip_shard, int skip_period,
                           size_t n_valid, size_t adapt_end) {
  const float s_adapt = words[0], s_tail = words[1];
  const size_t tasks = (n_valid + 3) >> 2;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
    const size_t e = t << 2;
    // (n_s is a multiple of 256: a lane's 4 values lie in one shard)
    if (skip_shard >= 0 && (int)((e / n_s) % (size_t)skip_period) == skip_shard) continue;
    const float4 wv = *reinterpret_cast<const float4*>(master + e);
    const float4 mv = *reinterpret_cast<const float4*>(mom + e);
    const float4 vv = *reinterpret_cast<const float4*>(p.var + e);
    float w[4] = {wv.x, wv.y, wv.z, wv.w};
    const float m[4] = {mv.x, mv.y, mv.z, mv.w}, v2[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float r = lamb_direction(p, w[j], m[j], v2[j]);
      w[j] = fmaf(-(e + j < adapt_end ? s_adapt : s_tail), r, w[j]);
    }
    if (e + 4 <= n_valid) {
      *reinterpret_cast<float4*>(master + e) = make_float4(w[0], w[1], w[2], w[3]);
      if (HAS_LP)
        *reinterpret_cast<uint2*>(lp + e) = make_uint2(pack_bf16x2(w[0], w[1]), pack_bf16x2(w[2], w[3]));
    } else {
      for (int j = 0; j < 4 && e + j < n_valid; ++j) {
        master[e + j] = w[j];
        if (HAS_LP) lp[e + j] = f32_to_bf16(w[j]);
      }
    }
  }
}

// ---------------------------------------------------------------- global-norm clipping
// The norm pass of a clip group over one gathered wire region: wire_sgd_kernel's traversal (shards, shard stride,
// skipped shards, the n_valid tail inside a group), read-only. A lane owns a whole 16-value group per trip — the BFP
// codecs' 17 bytes per 16 values arrive as ONE 16-B mantissa load plus the exponent byte, half the load instructions
// of the update kernels' 8 values per lane, and there are no dense planes whose register footprint made 8 the better
// choice there (this kernel holds 16 decoded values and one fp64 sum). g^2 is exact in fp64, the lane's sum grows in
// its own iteration order (the grid alone decides it), then the block sum: one double per block, no atomics.
template <int C>
__global__ void __launch_bounds__(kBlock)
    wire_sumsq_kernel(const uint8_t* __restrict__ wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                      size_t n_valid, size_t sb, double* __restrict__ partials) {
  const size_t tasks = n_s >> 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  double sum = 0.0;
  for (int s = 0; s < n_shards; ++s) {
    if (skip_shard >= 0 && (s % skip_period) == skip_shard) continue;
    const uint8_t* src = wire + (size_t)s * sb;
    const size_t base = (size_t)s * n_s;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < tasks; t += stride) {
      const size_t e = base + (t << 4);
      if (e >= n_valid) continue;
      float g[16];
      WireLane16<C>::load16(src, n_s, t << 4, g);
      // branch-free per value: a value at or past n_valid enters as 0, and s + 0.0 is s bit for bit
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double ga = e + j < n_valid ? (double)g[j] : 0.0;
        sum = fma(ga, ga, sum);
      }
    }
  }
  double sums[1] = {sum};
  block_sum(sums);
  if (threadIdx.x == 0) partials[blockIdx.x] = sums[0];
}

// One block: S = the sum of every segment's partials — each lane takes, segment by segment in the order given,
// indices t, t + 256, ... in ascending order; the lanes' sums then combine in the fixed tree — and the group's four
// words {coef, f32(total), f32(max_norm), nonfinite}: total = sqrt(S) * gs_abs, coef = min(1, max_norm / (total +
// 1e-6)), all fp64, rounded once to f32 (torch.nn.utils.clip_grad_norm_'s formula). A non-finite S (raw codecs only)
// gives a NaN coefficient, which the updates propagate.
__global__ void __launch_bounds__(kBlock)
    clip_coef_kernel(ClipSegments seg, int n_seg, double max_norm, double gs_abs, float* __restrict__ words) {
  double sum = 0.0;
  for (int k = 0; k < n_seg; ++k) {
    const double* __restrict__ p = seg.p[k];
    const int n = seg.n[k];
    for (int i = threadIdx.x; i < n; i += kBlock) sum += p[i];
  }
  double sums[1] = {sum};
  block_sum(sums);
  if (threadIdx.x == 0) {
    sum = sums[0];
    const bool finite = sum < __builtin_huge_val();  // (false for NaN too; the squares' sum is never negative)
    const double total = sqrt(sum) * gs_abs;
    const double coef = finite ? fmin(1.0, max_norm / (total + 1e-6)) : __builtin_nan("");
    words[0] = (float)coef;
    words[1] = (float)total;
    words[2] = (float)max_norm;
    words[3] = finite ? 0.0f : 1.0f;
  }
}

}  // namespace

#define FAN_CODEC_SWITCH(codec, ...)                         \
  switch (codec) {                                           \
    case kBfpTrunc: { constexpr int C = kBfpTrunc; __VA_ARGS__; break; } \
    case kBfpRne: { constexpr int C = kBfpRne; __VA_ARGS__; break; }     \
    case kRawF32: { constexpr int C = kRawF32; __VA_ARGS__; break; }     \
    case kRawBf16: { constexpr int C = kRawBf16; __VA_ARGS__; break; }   \
    case kBfp4Rne: { constexpr int C = kBfp4Rne; __VA_ARGS__; break; }   \
    default: FAN_CHECK(false, "unknown codec");              \
  }

static void check_ns(size_t n_s) {
  FAN_CHECK(n_s % 256 == 0, "shard element count must be a multiple of 256");
}

void launch_wire_pack(int codec, int in_dtype, const void* in, void* out, size_t n_s, int n_shards,
                      hipStream_t stream) {
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0) return;
  const int grid = stream_grid(n_s / 16, kBlock, wire_max_blocks());
  FAN_CODEC_SWITCH(codec, {
    if (in_dtype == kF32)
      hipLaunchKernelGGL((wire_pack_kernel<float, C>), grid, kBlock, 0, stream, (const float*)in, (uint8_t*)out,
                         n_s, n_shards);
    else
      hipLaunchKernelGGL((wire_pack_kernel<bf16_t, C>), grid, kBlock, 0, stream, (const bf16_t*)in,
                         (uint8_t*)out, n_s, n_shards);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_pack_range(int codec, int in_dtype, const void* in, void* out, size_t n_s, size_t begin,
                            size_t end, hipStream_t stream) {
  check_ns(n_s);
  FAN_CHECK(begin % 16 == 0 && end % 16 == 0 && begin <= end, "pack_range: bounds must be multiples of 16");
  if (end == begin) return;
  const int grid = stream_grid((end - begin) / 8, kBlock, wire_max_blocks());
  FAN_CODEC_SWITCH(codec, {
    if (in_dtype == kF32)
      hipLaunchKernelGGL((wire_pack_range_kernel<float, C>), grid, kBlock, 0, stream, (const float*)in,
                         (uint8_t*)out, n_s, begin, end);
    else
      hipLaunchKernelGGL((wire_pack_range_kernel<bf16_t, C>), grid, kBlock, 0, stream, (const bf16_t*)in,
                         (uint8_t*)out, n_s, begin, end);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_unpack(int codec, int out_dtype, const void* in, void* out, size_t n_s, int n_shards,
                        hipStream_t stream) {
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0) return;
  const int grid = stream_grid(n_s / 16, kBlock, wire_max_blocks());
  FAN_CODEC_SWITCH(codec, {
    if (out_dtype == kF32)
      hipLaunchKernelGGL((wire_unpack_kernel<float, C>), grid, kBlock, 0, stream, (const uint8_t*)in, (float*)out,
                         n_s, n_shards);
    else
      hipLaunchKernelGGL((wire_unpack_kernel<bf16_t, C>), grid, kBlock, 0, stream, (const uint8_t*)in,
                         (bf16_t*)out, n_s, n_shards);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

// The lane layout and the grid of a reduce kernel: launch(L{}, grid) with L = Lanes4<C> (4 values per lane) for an
// 8-bit BFP codec when wire_reduce4_for(n_slots), else Lanes16<C> (a group per lane; kBfp4Rne always: 4 of its values
// are two bytes, too narrow a store to be worth a layout of their own).
template <int C, typename F>
static void with_lanes(int n_slots, size_t n_s, int cap, F&& launch) {
  if constexpr (codec_bfp8(C)) {
    if (wire_reduce4_for(n_slots)) return launch(Lanes4<C>{}, stream_grid(n_s / 4, kBlock, cap));
  }
  launch(Lanes16<C>{}, stream_grid(n_s / 16, kBlock, cap));
}

template <typename TL, int C>
static void reduce_dispatch(const void* slots, size_t slot_stride, int n_slots, int self_pos, const void* local,
                            void* out_wire, float* out_f32, size_t n_s, hipStream_t stream) {
  const uint8_t* sl = (const uint8_t*)slots;
  const TL* lo = (const TL*)local;
  uint8_t* ow = (uint8_t*)out_wire;
  const bool hl = local != nullptr, w = out_wire != nullptr, f = out_f32 != nullptr;
  FAN_CHECK(w || f, "wire_reduce needs an output");
  with_lanes<C>(n_slots, n_s, wire_max_blocks(), [&](auto lanes, int grid) {
    using L = decltype(lanes);
#define FAN_RED(HL, OW, OF)                                                                                  \
  hipLaunchKernelGGL((wire_reduce_kernel<L, TL, HL, OW, OF>), grid, kBlock, 0, stream, sl, slot_stride, n_slots, \
                     self_pos, lo, ow, out_f32, n_s)
    if (hl) {
      if (w && f) FAN_RED(true, true, true);
      else if (w) FAN_RED(true, true, false);
      else FAN_RED(true, false, true);
    } else {
      if (w && f) FAN_RED(false, true, true);
      else if (w) FAN_RED(false, true, false);
      else FAN_RED(false, false, true);
    }
#undef FAN_RED
  });
}

void launch_wire_reduce(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                        int self_pos, const void* local, void* out_wire, float* out_f32, size_t n_s,
                        hipStream_t stream) {
  check_ns(n_s);
  if (n_s == 0) return;
  FAN_CODEC_SWITCH(codec, {
    if (local_dtype == kF32)
      reduce_dispatch<float, C>(slots, slot_stride, n_slots, self_pos, local, out_wire, out_f32, n_s, stream);
    else
      reduce_dispatch<bf16_t, C>(slots, slot_stride, n_slots, self_pos, local, out_wire, out_f32, n_s, stream);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_sgd(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                     float* master, bf16_t* lp, float* mom, SgdParams p, size_t n_valid, hipStream_t stream,
                     size_t shard_stride, const float* clip) {
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0) return;
  const int grid = stream_grid(n_s / 8, kBlock, wire_max_blocks());
  const uint8_t* w = (const uint8_t*)wire;
#define FAN_SGD(LP, MOM)                                                                                          \
  do {                                                                                                            \
    if (clip)                                                                                                     \
      hipLaunchKernelGGL((wire_sgd_kernel<C, LP, MOM, SgdParams, true>), grid, kBlock, 0, stream, w, n_s, n_shards, \
                         skip_shard, skip_period, master, lp, mom, p, n_valid, sb, clip);                         \
    else                                                                                                          \
      hipLaunchKernelGGL((wire_sgd_kernel<C, LP, MOM>), grid, kBlock, 0, stream, w, n_s, n_shards, skip_shard,    \
                         skip_period, master, lp, mom, p, n_valid, sb, clip);                                     \
  } while (0)
  FAN_CODEC_SWITCH(codec, {
    const size_t sb = shard_stride ? shard_stride : wire_shard_bytes(C, n_s);
    if (lp && mom) FAN_SGD(true, true);
    else if (lp) FAN_SGD(true, false);
    else if (mom) FAN_SGD(false, true);
    else FAN_SGD(false, false);
  });
#undef FAN_SGD
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_adamw(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                       float* master, bf16_t* lp, float* mom, AdamWParams p, size_t n_valid, hipStream_t stream,
                       size_t shard_stride, const float* clip) {
  FAN_CHECK(master != nullptr && mom != nullptr && p.var != nullptr, "wire_adamw: master and both moment planes");
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0) return;
  const int grid = stream_grid(n_s / 8, kBlock, wire_max_blocks());
  const uint8_t* w = (const uint8_t*)wire;
#define FAN_ADAMW(LP, CLIP)                                                                                      \
  hipLaunchKernelGGL((wire_sgd_kernel<C, LP, true, AdamWParams, CLIP>), grid, kBlock, 0, stream, w, n_s, n_shards, \
                     skip_shard, skip_period, master, lp, mom, p, n_valid, sb, clip)
  FAN_CODEC_SWITCH(codec, {
    const size_t sb = shard_stride ? shard_stride : wire_shard_bytes(C, n_s);
    if (lp && clip) FAN_ADAMW(true, true);
    else if (lp) FAN_ADAMW(true, false);
    else if (clip) FAN_ADAMW(false, true);
    else FAN_ADAMW(false, false);
  });
#undef FAN_ADAMW
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_lion(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                      float* master, bf16_t* lp, float* mom, LionParams p, size_t n_valid, hipStream_t stream,
                      size_t shard_stride, const float* clip) {
  FAN_CHECK(master != nullptr && mom != nullptr, "wire_lion: master and the moment plane");
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0) return;
  const int grid = stream_grid(n_s / 8, kBlock, wire_max_blocks());
  const uint8_t* w = (const uint8_t*)wire;
#define FAN_LION(LP, CLIP)                                                                                      \
  hipLaunchKernelGGL((wire_sgd_kernel<C, LP, true, LionParams, CLIP>), grid, kBlock, 0, stream, w, n_s, n_shards, \
                     skip_shard, skip_period, master, lp, mom, p, n_valid, sb, clip)
  FAN_CODEC_SWITCH(codec, {
    const size_t sb = shard_stride ? shard_stride : wire_shard_bytes(C, n_s);
    if (lp && clip) FAN_LION(true, true);
    else if (lp) FAN_LION(true, false);
    else if (clip) FAN_LION(false, true);
    else FAN_LION(false, false);
  });
#undef FAN_LION
  FAN_HIP_CHECK(hipGetLastError());
}

static std::atomic<int>& moment_grid_flag() {
  static std::atomic<int> g{0};
  return g;
}
int moment_grid_cap() { return moment_grid_flag().load(std::memory_order_relaxed); }
void set_moment_grid_cap(int blocks) { moment_grid_flag().store(blocks > 0 ? blocks : 0); }

void launch_wire_adamw_q(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                         float* master, bf16_t* lp, uint8_t* mom_q, uint8_t* var_q, size_t plane_elems,
                         size_t elem_base, AdamWParams p, uint64_t seed, size_t n_valid, hipStream_t stream,
                         size_t shard_stride, const float* clip) {
  FAN_CHECK(master != nullptr && mom_q != nullptr && var_q != nullptr, "wire_adamw_q: master and both moment planes");
  FAN_CHECK(plane_elems % 256 == 0 && elem_base % 256 == 0, "wire_adamw_q: plane_elems and elem_base are multiples of 256");
  FAN_CHECK((uint64_t)plane_elems < ((uint64_t)1 << 32),
            "wire_adamw_q: a padded bucket of 2^32 or more elements (element indices are 32-bit)");
  FAN_CHECK(((uintptr_t)mom_q | (uintptr_t)var_q) % 16 == 0, "wire_adamw_q: the planes are 16-byte aligned");
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0 || n_valid == 0) return;
  FAN_CHECK(n_valid <= n_s * (size_t)n_shards, "wire_adamw_q: n_valid beyond the wire region");
  FAN_CHECK(elem_base <= plane_elems && n_valid <= plane_elems - elem_base,
            "wire_adamw_q: the region's valid elements must lie inside the planes");
  const int cap = moment_grid_cap();
  const int grid = stream_grid(n_s / 16, kBlock, cap > 0 ? std::min(cap, wire_max_blocks()) : wire_max_blocks());
  const uint8_t* w = (const uint8_t*)wire;
  const SrKey km = sr_key(seed, kMomentRank, 0), kr = sr_key(seed, kMomentRank, 1);
#define FAN_ADAMW_Q(LP, CLIP)                                                                                    \
  hipLaunchKernelGGL((wire_adamw_q_kernel<C, LP, CLIP>), grid, kBlock, 0, stream, w, n_s, n_shards, skip_shard,  \
                     skip_period, master, lp, mom_q, var_q, plane_elems, elem_base, p, km, kr, n_valid, sb, clip)
  FAN_CODEC_SWITCH(codec, {
    const size_t sb = shard_stride ? shard_stride : wire_shard_bytes(C, n_s);
    if (lp && clip) FAN_ADAMW_Q(true, true);
    else if (lp) FAN_ADAMW_Q(true, false);
    else if (clip) FAN_ADAMW_Q(false, true);
    else FAN_ADAMW_Q(false, false);
  });
#undef FAN_ADAMW_Q
  FAN_HIP_CHECK(hipGetLastError());
}

int lamb_partials_for(size_t n_s) { return stream_grid(n_s / 8, kBlock, wire_max_blocks()); }

void launch_wire_lamb_moments(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                              const float* master, float* mom, LambParams p, size_t n_valid, size_t adapt_end,
                              double* partials, hipStream_t stream, size_t shard_stride, const float* clip) {
  FAN_CHECK(master != nullptr && mom != nullptr && p.var != nullptr && partials != nullptr,
            "wire_lamb_moments: master, both moment planes and the partials buffer");
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  // (an empty launch would leave its partials unwritten for launch_lamb_ratio to read)
  FAN_CHECK(n_s > 0 && n_shards > 0, "wire_lamb_moments: empty wire");
  if (adapt_end > n_valid) adapt_end = n_valid;
  const int grid = lamb_partials_for(n_s);
  const uint8_t* w = (const uint8_t*)wire;
  FAN_CODEC_SWITCH(codec, {
    const size_t sb = shard_stride ? shard_stride : wire_shard_bytes(C, n_s);
    if (clip)
      hipLaunchKernelGGL((wire_lamb_moments_kernel<C, true>), grid, kBlock, 0, stream, w, n_s, n_shards, skip_shard,
                         skip_period, master, mom, p, n_valid, adapt_end, sb, partials, clip);
    else
      hipLaunchKernelGGL((wire_lamb_moments_kernel<C>), grid, kBlock, 0, stream, w, n_s, n_shards, skip_shard,
                         skip_period, master, mom, p, n_valid, adapt_end, sb, partials, clip);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

int sumsq_partials_for(size_t n_s) { return stream_grid(n_s / 16, kBlock, wire_max_blocks()); }

void launch_wire_sumsq(int codec, const void* wire, size_t n_s, int n_shards, int skip_shard, int skip_period,
                       size_t n_valid, double* partials, hipStream_t stream, size_t shard_stride) {
  FAN_CHECK(wire != nullptr && partials != nullptr, "wire_sumsq: the wire and the partials buffer");
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  // (an empty launch would leave its partials unwritten for launch_clip_coef to read)
  FAN_CHECK(n_s > 0 && n_shards > 0, "wire_sumsq: empty wire");
  const int grid = sumsq_partials_for(n_s);
  const uint8_t* w = (const uint8_t*)wire;
  FAN_CODEC_SWITCH(codec, {
    const size_t sb = shard_stride ? shard_stride : wire_shard_bytes(C, n_s);
    hipLaunchKernelGGL((wire_sumsq_kernel<C>), grid, kBlock, 0, stream, w, n_s, n_shards, skip_shard, skip_period,
                       n_valid, sb, partials);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_clip_coef(const ClipSegments& seg, int n_seg, double max_norm, float grad_scale, float* words,
                      hipStream_t stream) {
  FAN_CHECK(words != nullptr && n_seg >= 0 && n_seg <= kClipSegments, "clip_coef: the four output words and at most "
                                                                      "8 partial segments");
  FAN_CHECK(max_norm > 0.0 && max_norm < __builtin_huge_val(), "clip_coef: max_norm must be finite and positive");
  for (int k = 0; k < n_seg; ++k)
    FAN_CHECK(seg.n[k] >= 0 && (seg.n[k] == 0 || seg.p[k] != nullptr), "clip_coef: a segment without its partials");
  hipLaunchKernelGGL(clip_coef_kernel, 1, kBlock, 0, stream, seg, n_seg, max_norm, fabs((double)grad_scale), words);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_lamb_ratio(const double* partials, int n_pairs, float lr, float* words, hipStream_t stream) {
  FAN_CHECK(partials != nullptr && words != nullptr && n_pairs >= 0, "lamb_ratio: partials and the three output words");
  hipLaunchKernelGGL(lamb_ratio_kernel, 1, kBlock, 0, stream, partials, n_pairs, lr, words);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_lamb_apply(float* master, bf16_t* lp, const float* mom, LambParams p, const float* words, size_t n_s,
                            int skip_shard, int skip_period, size_t n_valid, size_t adapt_end, hipStream_t stream) {
  FAN_CHECK(master != nullptr && mom != nullptr && p.var != nullptr && words != nullptr,
            "wire_lamb_apply: master, both moment planes and the scale words");
  if (skip_period < 1) skip_period = 1 << 30;
  check_ns(n_s);
  FAN_CHECK(n_s > 0 || skip_shard < 0, "wire_lamb_apply: skipped shards need the shard size");
  if (n_valid == 0) return;
  if (adapt_end > n_valid) adapt_end = n_valid;
  const int grid = stream_grid((n_valid + 3) / 4, kBlock, wire_max_blocks());
  if (lp)
    hipLaunchKernelGGL((wire_lamb_apply_kernel<true>), grid, kBlock, 0, stream, master, lp, mom, p, words, n_s,
                       skip_shard, skip_period, n_valid, adapt_end);
  else
    hipLaunchKernelGGL((wire_lamb_apply_kernel<false>), grid, kBlock, 0, stream, master, lp, mom, p, words, n_s,
                       skip_shard, skip_period, n_valid, adapt_end);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_unpack_strided(int codec, int out_dtype, const void* in, size_t shard_stride, void* out, size_t n_s,
                                int n_shards, hipStream_t stream) {
  check_ns(n_s);
  if (n_s == 0 || n_shards == 0) return;
  const int grid = stream_grid(n_s / 16, kBlock, wire_max_blocks());
  FAN_CODEC_SWITCH(codec, {
    if (out_dtype == kF32)
      hipLaunchKernelGGL((wire_unpack_strided_kernel<float, C>), grid, kBlock, 0, stream, (const uint8_t*)in,
                         shard_stride, (float*)out, n_s, n_shards);
    else
      hipLaunchKernelGGL((wire_unpack_strided_kernel<bf16_t, C>), grid, kBlock, 0, stream, (const uint8_t*)in,
                         shard_stride, (bf16_t*)out, n_s, n_shards);
  });
  FAN_HIP_CHECK(hipGetLastError());
}

// Grid cap and release mode of a kernel whose destinations are peers' receive slots, or a local buffer's (no release).
struct PeerLaunch {
  int cap, rel;
};
static PeerLaunch peer_launch(bool peers) {
  if (!peers) return {wire_max_blocks(), -1};
  return {std::min(wire_max_blocks(), p2p_grid_cap()), p2p_release_mode()};
}

static void check_ef(int codec, const float* residual) {
  FAN_CHECK(codec_shared_exp(codec), "error feedback: BFP codecs only (a raw codec drops nothing)");
  FAN_CHECK(residual != nullptr && (reinterpret_cast<uintptr_t>(residual) & 15) == 0,
            "error feedback: a 16-B aligned f32 residual plane");
}

static void check_sr(int codec, size_t base, size_t n) {
  FAN_CHECK(codec_sr(codec), "stochastic rounding: bfp_rne and bfp4_rne only");
  FAN_CHECK(base % 16 == 0 && base <= ((size_t)1 << 32) && n <= ((size_t)1 << 32) - base,
            "stochastic rounding: element indices must stay below 2^32");
}

static const char* enc_suffix(const WireEncoder& enc) {
  return enc.kind == WireEncoder::kFeedback ? "ef" : enc.kind == WireEncoder::kStochastic ? "sr" : "to";
}

// launch(e) with e the device policy of `enc`; only the forms codec C has are instantiated (check_ef / check_sr have
// refused the others).
template <int C, typename F>
static void with_encoder(const WireEncoder& enc, F&& launch) {
  if (enc.kind == WireEncoder::kPlain) return launch(EncPlain{});
  if constexpr (EncFeedback::kHas<C>) {
    if (enc.kind == WireEncoder::kFeedback) return launch(EncFeedback{enc.residual});
  }
  if constexpr (EncStochastic::kHas<C>) {
    if (enc.kind == WireEncoder::kStochastic) return launch(EncStochastic{enc.key, (uint32_t)enc.base});
  }
  FAN_CHECK(false, "wire encoder: not a form of this codec");
}

void launch_wire_pack_to(int codec, int in_dtype, const void* in, const WirePtrs& dst, size_t n_s, int n_shards,
                         int self_shard, const WireEncoder& enc, bool peers, hipStream_t stream) {
  const bool sr = enc.kind == WireEncoder::kStochastic;
  check_ns(n_s);
  if (enc.kind == WireEncoder::kFeedback) check_ef(codec, enc.residual);
  FAN_CHECK((!sr || n_shards >= 0) && n_shards <= kMaxPeers,
            std::string("pack_") + enc_suffix(enc) + ": at most 16 destinations");
  if (sr) check_sr(codec, enc.base, n_s * (size_t)n_shards);
  if (n_s == 0 || n_shards == 0) return;
  const PeerLaunch pl = peer_launch(peers);
  const int grid = stream_grid(n_s / 16, kBlock, pl.cap);
  FAN_CODEC_SWITCH(codec, with_encoder<C>(enc, [&](auto e) {
    using Enc = decltype(e);
    if (in_dtype == kF32)
      hipLaunchKernelGGL((wire_pack_to_kernel<float, C, Enc>), grid, kBlock, 0, stream, (const float*)in, dst, n_s,
                         n_shards, pl.rel, self_shard, e);
    else
      hipLaunchKernelGGL((wire_pack_to_kernel<bf16_t, C, Enc>), grid, kBlock, 0, stream, (const bf16_t*)in, dst, n_s,
                         n_shards, pl.rel, self_shard, e);
  }));
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_reduce_to(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots, int self_pos,
                           const void* local, const WirePtrs& dst, int n_dst, size_t n_s, const WireEncoder& enc,
                           bool peers, hipStream_t stream) {
  check_ns(n_s);
  if (enc.kind == WireEncoder::kPlain) {
    FAN_CHECK(n_dst <= kMaxPeers && local != nullptr, "reduce_to: local operand and at most 16 destinations");
  } else {
    const std::string name = std::string("reduce_") + enc_suffix(enc);
    if (enc.kind == WireEncoder::kFeedback) check_ef(codec, enc.residual);
    else check_sr(codec, enc.base, n_s);
    FAN_CHECK(n_dst >= 1 && n_dst <= kMaxPeers && local != nullptr,
              name + ": local operand and 1 to 16 destinations");
    FAN_CHECK(self_pos >= 0 && self_pos < n_slots, name + ": self_pos names the slot the local operand stands for");
  }
  if (n_s == 0) return;
  const uint8_t* sl = (const uint8_t*)slots;
  const PeerLaunch pl = peer_launch(peers);
  FAN_CODEC_SWITCH(codec, with_encoder<C>(enc, [&](auto e) {
    using Enc = decltype(e);
    with_lanes<C>(n_slots, n_s, pl.cap, [&](auto lanes, int grid) {
      using L = decltype(lanes);
      if (local_dtype == kF32)
        hipLaunchKernelGGL((wire_reduce_to_kernel<L, float, Enc>), grid, kBlock, 0, stream, sl, slot_stride, n_slots,
                           self_pos, (const float*)local, dst, n_dst, n_s, pl.rel, e);
      else
        hipLaunchKernelGGL((wire_reduce_to_kernel<L, bf16_t, Enc>), grid, kBlock, 0, stream, sl, slot_stride, n_slots,
                           self_pos, (const bf16_t*)local, dst, n_dst, n_s, pl.rel, e);
    });
  }));
  FAN_HIP_CHECK(hipGetLastError());
}

static std::atomic<int>& reduce4_flag() {
  static std::atomic<int> f{[] {
    const char* e = getenv("FAN_WIRE_REDUCE4");
    return e && e[0] == '0' ? 0 : 1;
  }()};
  return f;
}
void set_wire_reduce4(int on) { reduce4_flag().store(on); }
int wire_reduce4() { return reduce4_flag().load(std::memory_order_relaxed); }

template <typename P>
static void launch_reduce_update(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                                 int self_pos, const void* local, float* master, float* mom, P p, size_t n_valid,
                                 const WirePtrs& dst, int n_dst, size_t n_s, bool peers, hipStream_t stream) {
  // AdamW: both moment planes, always; Lion: its one plane, always
  constexpr bool kMomAlways = std::is_same<P, AdamWParams>::value || std::is_same<P, LionParams>::value;
  check_ns(n_s);
  FAN_CHECK(n_dst <= kMaxPeers && local != nullptr && master != nullptr,
            "reduce_sgd: local operand, master shard and at most 16 destinations");
  if (n_s == 0) return;
  const uint8_t* sl = (const uint8_t*)slots;
  const PeerLaunch pl = peer_launch(peers);
#define FAN_RSGD(TL, MOM)                                                                                         \
  hipLaunchKernelGGL((wire_reduce_sgd_kernel<L, TL, MOM, P>), grid, kBlock, 0, stream, sl, slot_stride, n_slots, \
                     self_pos, (const TL*)local, master, mom, p, n_valid, dst, n_dst, n_s, pl.rel)
  FAN_CODEC_SWITCH(codec, with_lanes<C>(n_slots, n_s, pl.cap, [&](auto lanes, int grid) {
    using L = decltype(lanes);
    if (local_dtype == kF32) {
      if (kMomAlways || mom) FAN_RSGD(float, true);
      else if constexpr (!kMomAlways) FAN_RSGD(float, false);
    } else {
      if (kMomAlways || mom) FAN_RSGD(bf16_t, true);
      else if constexpr (!kMomAlways) FAN_RSGD(bf16_t, false);
    }
  }));
#undef FAN_RSGD
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_wire_reduce_sgd(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                            int self_pos, const void* local, float* master, float* mom, SgdParams p, size_t n_valid,
                            const WirePtrs& dst, int n_dst, size_t n_s, bool peers, hipStream_t stream) {
  launch_reduce_update(codec, local_dtype, slots, slot_stride, n_slots, self_pos, local, master, mom, p, n_valid, dst,
                       n_dst, n_s, peers, stream);
}

void launch_wire_reduce_adamw(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                              int self_pos, const void* local, float* master, float* mom, AdamWParams p,
                              size_t n_valid, const WirePtrs& dst, int n_dst, size_t n_s, bool peers,
                              hipStream_t stream) {
  FAN_CHECK(mom != nullptr && p.var != nullptr, "reduce_adamw: both moment shards");
  launch_reduce_update(codec, local_dtype, slots, slot_stride, n_slots, self_pos, local, master, mom, p, n_valid, dst,
                       n_dst, n_s, peers, stream);
}

void launch_wire_reduce_lion(int codec, int local_dtype, const void* slots, size_t slot_stride, int n_slots,
                             int self_pos, const void* local, float* master, float* mom, LionParams p,
                             size_t n_valid, const WirePtrs& dst, int n_dst, size_t n_s, bool peers,
                             hipStream_t stream) {
  FAN_CHECK(mom != nullptr, "reduce_lion: the moment shard");
  launch_reduce_update(codec, local_dtype, slots, slot_stride, n_slots, self_pos, local, master, mom, p, n_valid, dst,
                       n_dst, n_s, peers, stream);
}

}  // namespace fan
