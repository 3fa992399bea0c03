// Randomised Hadamard rotation and the one-bit quantiser behind it, for gfx950 (rht.h; ops/rht_oracle.py is the
// definition).
//
// One workgroup of 4 waves transforms one block of 4096 values, 16 per lane, viewed as X[a][b][c] at 256 a + 16 b + c.
// H_4096 = H16 (x) H16 (x) H16 acts on one axis at a time, each a 16 x 16 product with the +-1 matrix
// H16[i][j] = (-1)^popcount(i & j) on v_mfma_f32_16x16x4_f32 (D[16][16] += A[16][4] B[4][16]: lane l supplies
// A[l % 16][l / 16] and B[l / 16][l % 16] and holds D[4 * (l / 16) + v][l % 16] in accumulator register v). With
// r = l % 16 and q = l / 16, the four numbers h[j] = H16[4 q + j][r] a lane derives from its own id are its share of H16
// as the B operand of the first round and, H16 being symmetric, as the A operand of the other two.
//
//   axis c  wave w owns a = 4 w .. 4 w + 3; the lane loads the 16-B vector X[a][r][4 q .. 4 q + 3], which is the A operand
//           as it stands once k-slot q of instruction j means c = 4 q + j: T = X_a H16, four instructions.
//   axis b  the accumulator holds T[4 q + i][r] in register i: a valid B operand once k-slot q of instruction i means
//           b = 4 q + i. U = H16 T, register to register.
//   axis a  crosses waves: U goes through a 16 KB LDS tile, wave w takes b = 4 w .. 4 w + 3 and multiplies by H16 from
//           the left again. The tile keeps c in the low four bits of the bank and swizzles the next two with
//           (b & 3) ^ (b >> 2) ^ (a >> 2), which differs between the four q of a wave both when it writes (b = 4 q + v)
//           and when it reads (a = 4 q + i): neither side conflicts and the tile needs no padding.
//
// The lane ends with element (a = 4 q + v, b = 4 w + bi, c = r) in y[bi][v]: a wave store covers four 64-B segments.
// The sign bits of such a store are a wave ballot, whose four 16-bit fields are two sign bytes each; lanes 0 .. 15
// collect the fields of their (v, q) over bi into one 8-B store, so the sign plane takes no second trip through LDS.
// Nothing here uses an atomic or waits for another workgroup; persistent workgroups stride over the blocks, and every
// sum has a fixed order, so no result depends on the grid.
#include "rht/rht.h"

#include <initializer_list>

#include "bfp/bfp_format.h"

namespace fan {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;

#define FAN_MFMA_16x16x4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// The element-wise f32 statements of the definition, each rounded on its own.
__device__ __forceinline__ float rht_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float rht_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float rht_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
// x with its sign flipped where bit 0 of h is set.
__device__ __forceinline__ float rht_flip(float x, uint32_t h) {
  return __uint_as_float(__float_as_uint(x) ^ ((h & 1u) << 31));
}

struct RhtLane {
  uint32_t r, q, w;
  float h[4];  // H16[4 q + j][r]
};
__device__ __forceinline__ RhtLane rht_lane() {
  RhtLane L;
  L.r = threadIdx.x & 15u;
  L.q = (threadIdx.x >> 4) & 3u;
  L.w = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) L.h[j] = (__popc((4 * L.q + j) & L.r) & 1) ? -1.0f : 1.0f;
  return L;
}
// Offset in the block of the lane's input vector ai (elements .. + 3) and of its output element (bi, v).
__device__ __forceinline__ uint32_t rht_in_at(const RhtLane& L, uint32_t ai) {
  return 256 * (4 * L.w + ai) + 16 * L.r + 4 * L.q;
}
__device__ __forceinline__ uint32_t rht_out_at(const RhtLane& L, uint32_t bi, uint32_t v) {
  return 256 * (4 * L.q + v) + 16 * (4 * L.w + bi) + L.r;
}
__device__ __forceinline__ uint32_t rht_tile_at(uint32_t a, uint32_t b, uint32_t c) {
  return 256 * a + 64 * (b >> 2) + ((((b & 3) ^ (b >> 2) ^ (a >> 2)) & 3) << 4) + c;
}

// y = (1/64) H_4096 x of the workgroup's block; a zero result is +0. tile: 4096 f32 of LDS. The barrier in front lets
// the caller loop over blocks.
__device__ __forceinline__ void rht_core(const v4f (&x)[4], float (&y)[4][4], float* tile, const RhtLane& L) {
  __syncthreads();
#pragma unroll
  for (uint32_t ai = 0; ai < 4; ++ai) {
    v4f t = 0.0f, u = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) t = FAN_MFMA_16x16x4(x[ai][j], L.h[j], t);
#pragma unroll
    for (int i = 0; i < 4; ++i) u = FAN_MFMA_16x16x4(L.h[i], t[i], u);
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) tile[rht_tile_at(4 * L.w + ai, 4 * L.q + v, L.r)] = u[v];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t bi = 0; bi < 4; ++bi) {
    v4f z = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) z = FAN_MFMA_16x16x4(L.h[i], tile[rht_tile_at(4 * L.q + i, 4 * L.w + bi, L.r)], z);
#pragma unroll
    for (int v = 0; v < 4; ++v) y[bi][v] = rht_add(rht_mul(z[v], 0.015625f), 0.0f);
  }
}

// D on the input vectors and on the output elements; base: the bucket index of the block's first element.
__device__ __forceinline__ void rht_flip_in(v4f (&x)[4], SrKey key, uint32_t base, const RhtLane& L) {
#pragma unroll
  for (uint32_t ai = 0; ai < 4; ++ai) {
    const uint32_t i = base + rht_in_at(L, ai);
    const uint32_t h = sr_hash(key, i >> 5) >> (i & 31);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[ai][j] = rht_flip(x[ai][j], h >> j);
  }
}
__device__ __forceinline__ void rht_flip_out(float (&y)[4][4], SrKey key, uint32_t base, const RhtLane& L) {
#pragma unroll
  for (uint32_t v = 0; v < 4; ++v) {
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {  // b = 4 w + 2 half and the next one share a hash word
      const uint32_t h = sr_hash(key, (base + rht_out_at(L, 2 * half, v)) >> 5) >> L.r;
      y[2 * half][v] = rht_flip(y[2 * half][v], h);
      y[2 * half + 1][v] = rht_flip(y[2 * half + 1][v], h >> 16);
    }
  }
}

// The 16-B vector at element i (i % 4 == 0); the elements at or past n are not read and come back as +0.
__device__ __forceinline__ v4f rht_load4(const float* __restrict__ p, uint32_t i, uint32_t n) {
  if (i + 4 <= n) return *reinterpret_cast<const v4f*>(p + i);
  v4f v = 0.0f;
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) {
    if (i + j < n) v[j] = p[i + j];
  }
  return v;
}

// ---------------------------------------------------------------- the bare transform, out of place
template <bool kInverse>
__global__ void __launch_bounds__(kThreads)
    rht_transform_kernel(const float* __restrict__ x, float* __restrict__ out, SrKey key, uint32_t n, uint32_t nb) {
  __shared__ float tile[kRhtBlock];
  const RhtLane L = rht_lane();
  for (uint32_t blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    const uint32_t base = blk * kRhtBlock;
    v4f in[4];
    float y[4][4];
#pragma unroll
    for (uint32_t ai = 0; ai < 4; ++ai) {
      const uint32_t i = base + rht_in_at(L, ai);
      in[ai] = kInverse ? *reinterpret_cast<const v4f*>(x + i) : rht_load4(x, i, n);
    }
    if (!kInverse) rht_flip_in(in, key, base, L);
    rht_core(in, y, tile, L);
    if (kInverse) rht_flip_out(y, key, base, L);
#pragma unroll
    for (uint32_t bi = 0; bi < 4; ++bi) {
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v) {
        const uint32_t i = base + rht_out_at(L, bi, v);
        if (!kInverse || i < n) out[i] = y[bi][v];
      }
    }
  }
}

// ---------------------------------------------------------------- y = rht(g) + e -> sign bits, scale, e'
__global__ void __launch_bounds__(kThreads)
    rht_encode_kernel(const float* __restrict__ g, float* __restrict__ e, uint8_t* __restrict__ sign,
                      float* __restrict__ scale, SrKey key, uint32_t n, uint32_t nb) {
  __shared__ float tile[kRhtBlock];
  __shared__ float wsum[4];
  const RhtLane L = rht_lane();
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    const uint32_t base = blk * kRhtBlock;
    v4f in[4];
    float y[4][4];
#pragma unroll
    for (uint32_t ai = 0; ai < 4; ++ai) in[ai] = rht_load4(g, base + rht_in_at(L, ai), n);
    rht_flip_in(in, key, base, L);
    rht_core(in, y, tile, L);
    float* __restrict__ eb = e + base;
    float sum = 0.0f;
    uint32_t neg = 0u, field[4] = {0u, 0u, 0u, 0u};  // the lane's own 16 bits; (lanes 0 .. 15) the bytes they store
#pragma unroll
    for (uint32_t bi = 0; bi < 4; ++bi) {
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v) {
        const float yv = rht_add(y[bi][v], eb[rht_out_at(L, bi, v)]);
        y[bi][v] = yv;
        sum = rht_add(sum, fabsf(yv));
        const bool b = yv < 0.0f;
        neg |= (uint32_t)b << (4 * bi + v);
        // bits 16 q' .. 16 q' + 15 of the ballot: elements (a = 4 q' + v, b = 4 w + bi, c = 0 .. 15), two sign bytes
        const uint32_t two = (uint32_t)(__ballot(b) >> (16 * (lane & 3u))) & 0xFFFFu;
        if ((lane >> 2) == v) field[bi] = two;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum = rht_add(sum, __shfl_xor(sum, off));
    if (lane == 0) wsum[L.w] = sum;
    __syncthreads();
    const float s = rht_mul(rht_add(rht_add(rht_add(wsum[0], wsum[1]), wsum[2]), wsum[3]), 1.0f / kRhtBlock);
#pragma unroll
    for (uint32_t bi = 0; bi < 4; ++bi) {
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v)
        eb[rht_out_at(L, bi, v)] = rht_sub(y[bi][v], rht_flip(s, neg >> (4 * bi + v)));
    }
    if (lane < 16)  // lane = 4 v + q': bytes 32 a + 2 b .. of a = 4 q' + v for b = 4 w .. 4 w + 3
      *reinterpret_cast<uint2*>(sign + (size_t)blk * kRhtSignBytes + 32 * (4 * (lane & 3u) + (lane >> 2)) + 8 * L.w) =
          make_uint2(field[0] | (field[1] << 16), field[2] | (field[3] << 16));
    if (threadIdx.x == 0) scale[blk] = s;
    if (blk == nb - 1 && threadIdx.x >= 1 && nb + threadIdx.x - 1 < (nb + 3) / 4 * 4) scale[nb + threadIdx.x - 1] = 0.0f;
  }
}

// ---------------------------------------------------------------- g = inverse(sum over the ranks) * inv_world
__global__ void __launch_bounds__(kThreads)
    rht_decode_kernel(const uint8_t* __restrict__ wires, size_t stride, uint32_t world, float* __restrict__ g, SrKey key,
                      uint32_t n, uint32_t nb, float inv_world) {
  __shared__ float tile[kRhtBlock];
  const RhtLane L = rht_lane();
  for (uint32_t blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    const uint32_t base = blk * kRhtBlock;
    v4f acc[4];
    float y[4][4];
#pragma unroll
    for (int ai = 0; ai < 4; ++ai) acc[ai] = 0.0f;
    for (uint32_t rank = 0; rank < world; ++rank) {
      const uint8_t* __restrict__ wr = wires + rank * stride;
      const float s = reinterpret_cast<const float*>(wr + (size_t)nb * kRhtSignBytes)[blk];
#pragma unroll
      for (uint32_t ai = 0; ai < 4; ++ai) {  // bytes 32 a + 2 r, + 1: c = 0 .. 15 of (a, b = r); the lane's c start at 4 q
        const uint32_t bits = *reinterpret_cast<const uint16_t*>(wr + (size_t)blk * kRhtSignBytes +
                                                                 (rht_in_at(L, ai) >> 4 << 1)) >> (4 * L.q);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[ai][j] = rht_add(acc[ai][j], rht_flip(s, bits >> j));
      }
    }
    rht_core(acc, y, tile, L);
    rht_flip_out(y, key, base, L);
#pragma unroll
    for (uint32_t bi = 0; bi < 4; ++bi) {
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v) {
        const uint32_t i = base + rht_out_at(L, bi, v);
        if (i < n) g[i] = rht_mul(y[bi][v], inv_world);
      }
    }
  }
}

void check_shape(int64_t n_pad, int64_t n, int max_blocks) {
  FAN_CHECK(n_pad > 0 && n_pad % 4 == 0 && n_pad < ((int64_t)1 << 31),
            "rht: n_pad must be a positive multiple of 4 below 2^31");
  FAN_CHECK(n >= 1 && n <= n_pad, "rht: 1 <= n <= n_pad");
  FAN_CHECK(max_blocks >= 0, "rht: max_blocks >= 0");
}

void check_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    FAN_CHECK(p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0, "rht: planes must be 16-byte aligned");
}

unsigned grid_for(int64_t blocks, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : kNumCU * 8;
  return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

void launch_rht_transform(const float* x, float* out, int64_t n_pad, int64_t n, uint64_t seed, bool inverse,
                          int max_blocks, hipStream_t s) {
  check_shape(n_pad, n, max_blocks);
  check_aligned({x, out});
  const RhtLayout lay = rht_layout(n);
  const unsigned grid = grid_for(lay.blocks, max_blocks);
  const SrKey key = sr_key(seed, 0, 2);
  if (inverse) rht_transform_kernel<true><<<grid, kThreads, 0, s>>>(x, out, key, (uint32_t)n, (uint32_t)lay.blocks);
  else rht_transform_kernel<false><<<grid, kThreads, 0, s>>>(x, out, key, (uint32_t)n, (uint32_t)lay.blocks);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_rht_encode(const float* g, float* e, void* wire, int64_t n_pad, int64_t n, uint64_t seed, int max_blocks,
                       hipStream_t s) {
  check_shape(n_pad, n, max_blocks);
  check_aligned({g, e, wire});
  const RhtLayout lay = rht_layout(n);
  uint8_t* sign = static_cast<uint8_t*>(wire);
  rht_encode_kernel<<<grid_for(lay.blocks, max_blocks), kThreads, 0, s>>>(
      g, e, sign, reinterpret_cast<float*>(sign + lay.blocks * kRhtSignBytes), sr_key(seed, 0, 2), (uint32_t)n,
      (uint32_t)lay.blocks);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_rht_decode(const void* wires, int world, float* g, int64_t n_pad, int64_t n, uint64_t seed,
                       float inv_world, int max_blocks, hipStream_t s) {
  check_shape(n_pad, n, max_blocks);
  FAN_CHECK(world >= 1 && world <= kRhtMaxWorld, "rht: 1 <= world <= 16");
  check_aligned({wires, g});
  const RhtLayout lay = rht_layout(n);
  rht_decode_kernel<<<grid_for(lay.blocks, max_blocks), kThreads, 0, s>>>(
      static_cast<const uint8_t*>(wires), (size_t)lay.wire_bytes, (uint32_t)world, g, sr_key(seed, 0, 2), (uint32_t)n,
      (uint32_t)lay.blocks, inv_world);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace fan
