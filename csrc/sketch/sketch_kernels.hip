// Count-sketch gradient compression kernels for gfx950 (sketch.h; ops/sketch_oracle.py is the definition).
//
// The vector to sketch exists only as gradient + residual: the accumulate and the estimate both load the two planes and
// add them in registers, one f32 add per element, so both see the same bits; the estimate stores the sum into the
// residual plane and the estimates into the gradient plane, and the keys-only radix select of topk/ and the fetch work
// on those.
//
// The bucket hash is a rotation per chunk of C elements by a multiple of 4 columns, so the accumulate is a gather: the
// workgroup that owns 1024 columns of one row reads, per chunk, one contiguous span of 1024 elements of each plane (it
// wraps at most once, between two 16-B vectors), one vector per lane, and keeps its four sums in registers in chunk
// order. The four elements of a lane share one 32-bit word of sign bits: one hash per lane and chunk. Strips of 16
// chunks go to different workgroups and land in slabs that sketch_combine_kernel adds in strip order. Nothing here uses
// an atomic or waits for another workgroup, and persistent workgroups stride over the work items, so no result depends
// on the grid.
#include "sketch/sketch.h"

#include <initializer_list>

#include "bfp/bfp_format.h"

namespace fan {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kUnroll = 4;  // chunks per batch: 8 16-B loads per lane in flight before the first add

// sr_key(seed, row, stage) of bfp_format.h from the seed's two words (stage 0: the offsets, 1: the signs).
__device__ __forceinline__ SrKey sketch_key(uint32_t lo, uint32_t hi, uint32_t row, uint32_t stage) {
  return {lo, hi ^ ((2 * row + stage + 1) * 0x9E3779B9u)};
}

__device__ __forceinline__ uint32_t sketch_off(SrKey koff, uint32_t q, uint32_t c4) { return 4 * (sr_hash(koff, q) % c4); }

// The element-wise f32 statements of the definition, each rounded on its own.
__device__ __forceinline__ float sk_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// v with the sign of component c flipped where bit c of h is set.
__device__ __forceinline__ v4f sk_flip(v4f v, uint32_t h) {
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = __uint_as_float(__float_as_uint(v[c]) ^ (((h >> c) & 1u) << 31));
  return v;
}

// The 16-B vector at element i (i % 4 == 0, i < n); the elements at or past n are not read and come back as +0.
__device__ __forceinline__ v4f load4(const float* __restrict__ p, uint32_t i, uint32_t n) {
  if (i + 4 <= n) return *reinterpret_cast<const v4f*>(p + i);
  v4f v = 0.0f;
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) {
    if (i + j < n) v[j] = p[i + j];
  }
  return v;
}
__device__ __forceinline__ void store4(float* __restrict__ p, uint32_t i, uint32_t n, v4f v) {
  if (i + 4 <= n) {
    *reinterpret_cast<v4f*>(p + i) = v;
    return;
  }
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) {
    if (i + j < n) p[i + j] = v[j];
  }
}

// ---------------------------------------------------------------- per strip: out[strip][row][b] = sum over its chunks
// A work item is (strip, row, tile of 1024 columns); a lane owns columns b .. b + 3. For chunk q the lane's source is
// the vector at i = q * C + ((b - off) mod C): off is uniform over the workgroup, a multiple of 4, so the four elements
// stay together and in one sign word. Chunks are taken four at a time: all eight loads first, then the adds in chunk
// order. An element at or past n adds nothing: the loads give +0 there, and no sum is ever -0, so adding a zero of
// either sign leaves the sum's bits alone.
__global__ void __launch_bounds__(kBlock)
    sketch_accumulate_kernel(const float* __restrict__ g, const float* __restrict__ e, float* __restrict__ out,
                             uint32_t seed_lo, uint32_t seed_hi, uint32_t n, uint32_t C, uint32_t Q, uint32_t rows,
                             uint32_t strips) {
  const uint32_t tiles = C / kSketchTile, c4 = C / 4;
  const uint32_t items = tiles * rows * strips;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t tile = item % tiles, row = (item / tiles) % rows, strip = item / (tiles * rows);
    const SrKey koff = sketch_key(seed_lo, seed_hi, row, 0), ksgn = sketch_key(seed_lo, seed_hi, row, 1);
    const uint32_t b = tile * kSketchTile + threadIdx.x * 4;
    const uint32_t q0 = strip * kSketchStrip, q1 = min(q0 + (uint32_t)kSketchStrip, Q);
    v4f acc = 0.0f;
    for (uint32_t q = q0; q < q1; q += kUnroll) {
      v4f gv[kUnroll], ev[kUnroll];
      uint32_t at[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        at[u] = n;  // (absent)
        gv[u] = 0.0f;
        ev[u] = 0.0f;
        if (q + u < q1) {  // (uniform)
          const uint32_t off = sketch_off(koff, q + u, c4);
          const uint32_t i = (q + u) * C + (b >= off ? b - off : b + (C - off));
          if (i < n) {
            at[u] = i;
            gv[u] = load4(g, i, n);
            ev[u] = load4(e, i, n);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (at[u] < n) {
          const uint32_t h = sr_hash(ksgn, at[u] >> 5) >> (at[u] & 31);
          v4f x;
#pragma unroll
          for (int c = 0; c < 4; ++c) x[c] = sk_add(gv[u][c], ev[u][c]);
          x = sk_flip(x, h);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = sk_add(acc[c], x[c]);
        }
      }
    }
    *reinterpret_cast<v4f*>(out + ((size_t)strip * rows + row) * C + b) = acc;
  }
}

// ---------------------------------------------------------------- S = part[0] + part[1] + ... in strip order
__global__ void __launch_bounds__(kBlock)
    sketch_combine_kernel(const v4f* __restrict__ part, uint32_t strips, v4f* __restrict__ S, uint32_t n4) {
  for (uint32_t t = blockIdx.x * kBlock + threadIdx.x; t < n4; t += gridDim.x * kBlock) {
    v4f a = part[t];
    for (uint32_t s = 1; s < strips; ++s) {
      const v4f p = part[(size_t)s * n4 + t];
#pragma unroll
      for (int c = 0; c < 4; ++c) a[c] = sk_add(a[c], p[c]);
    }
    S[t] = a;
  }
}

// ---------------------------------------------------------------- est = median over the rows; e = g + e; g = est
// Compare-exchange: the pair is swapped where b < a (so -0 and +0 keep their order, as in the oracle).
__device__ __forceinline__ void sk_cx(float& a, float& b) {
  const bool sw = b < a;
  const float lo = sw ? b : a, hi = sw ? a : b;
  a = lo;
  b = hi;
}

template <int R>
__device__ __forceinline__ float sk_median(const float (&v)[R]) {
  bool nan = false;
#pragma unroll
  for (int j = 0; j < R; ++j) nan = nan || v[j] != v[j];
  float m[3] = {v[0], 0.0f, 0.0f};
  if (R == 5) {  // drop the least of the first four and the greatest of them: the median of the other three
    float a = v[0], b = v[R > 1 ? 1 : 0], c = v[R > 2 ? 2 : 0], d = v[R > 3 ? 3 : 0];
    sk_cx(a, b);
    sk_cx(c, d);
    sk_cx(a, c);
    sk_cx(b, d);
    m[0] = b;
    m[1] = c;
    m[2] = v[R > 4 ? 4 : 0];
  } else if (R == 3) {
    m[1] = v[R > 1 ? 1 : 0];
    m[2] = v[R > 2 ? 2 : 0];
  }
  if (R >= 3) {
    sk_cx(m[0], m[1]);
    sk_cx(m[1], m[2]);
    sk_cx(m[0], m[1]);
    m[0] = m[1];
  }
  return nan ? __uint_as_float(0x7fc00000u) : m[0];
}

// Tiles of 1024 elements never straddle a chunk (C is a multiple of 1024): the chunk and the R offsets are uniform over
// the workgroup, a lane's four elements map to one 16-B vector of every sketch row and share one sign word per row.
template <int R>
__global__ void __launch_bounds__(kBlock)
    sketch_estimate_kernel(float* __restrict__ g, float* __restrict__ e, const float* __restrict__ S, uint32_t seed_lo,
                           uint32_t seed_hi, uint32_t n, uint32_t C) {
  const uint32_t tiles = (n + kSketchTile - 1) / kSketchTile, c4 = C / 4;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t i = tile * kSketchTile + threadIdx.x * 4;
    if (i >= n) continue;
    const uint32_t q = (tile * kSketchTile) / C, t = i - q * C;
    v4f v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint32_t off = sketch_off(sketch_key(seed_lo, seed_hi, j, 0), q, c4);
      const uint32_t col = t + off >= C ? t + off - C : t + off;
      const uint32_t h = sr_hash(sketch_key(seed_lo, seed_hi, j, 1), i >> 5) >> (i & 31);
      v[j] = sk_flip(*reinterpret_cast<const v4f*>(S + (size_t)j * C + col), h);
    }
    const v4f gv = load4(g, i, n), ev = load4(e, i, n);
    v4f x, est;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float col[R];
#pragma unroll
      for (int j = 0; j < R; ++j) col[j] = v[j][c];
      est[c] = sk_median<R>(col);
      x[c] = sk_add(gv[c], ev[c]);
    }
    store4(e, i, n, x);
    store4(g, i, n, est);
  }
}

// ---------------------------------------------------------------- val[j] = e[idx[j]]; e[idx[j]] = +0
// The indices of a wire are distinct: no two lanes meet.
__global__ void __launch_bounds__(kBlock)
    sketch_fetch_kernel(float* __restrict__ e, const uint32_t* __restrict__ idx, float* __restrict__ val, uint32_t n,
                        uint32_t k) {
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < k; j += gridDim.x * kBlock) {
    const uint32_t i = idx[j];
    if (i < n) {  // (always, on a wire selected from this plane)
      val[j] = e[i];
      e[i] = 0.0f;
    }
  }
}

void check_shape(int64_t n_pad, int64_t n, int rows, int64_t cols, int max_blocks) {
  FAN_CHECK(n_pad > 0 && n_pad % 4 == 0 && n_pad < ((int64_t)1 << 31),
            "sketch: n_pad must be a positive multiple of 4 below 2^31");
  FAN_CHECK(n >= 1 && n <= n_pad, "sketch: 1 <= n <= n_pad");
  FAN_CHECK(rows == 1 || rows == 3 || rows == 5, "sketch: rows must be 1, 3 or 5");
  FAN_CHECK(cols >= kSketchTile && cols <= kSketchMaxCols && cols % kSketchTile == 0,
            "sketch: cols must be a multiple of 1024 in 1024 .. 2^22");
  FAN_CHECK(max_blocks >= 0, "sketch: max_blocks >= 0");
}

void check_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    FAN_CHECK(p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0, "sketch: planes must be 16-byte aligned");
}

unsigned grid_for(int64_t items, int cap, int max_blocks) {
  if (max_blocks > 0) cap = max_blocks;
  return (unsigned)(items < cap ? items : cap);
}

}  // namespace

void launch_sketch(const float* g, const float* e, float* part, float* S, int64_t n_pad, int64_t n, int rows,
                   int64_t cols, uint64_t seed, int max_blocks, hipStream_t s, int stages) {
  check_shape(n_pad, n, rows, cols, max_blocks);
  check_aligned({g, e, part, S});
  const SketchLayout L = sketch_layout(n_pad, rows, cols);
  const int64_t items = cols / kSketchTile * rows * L.strips;
  float* out = L.strips == 1 ? S : part;
  if (stages & 1)
    sketch_accumulate_kernel<<<grid_for(items, kNumCU * 8, max_blocks), kBlock, 0, s>>>(
        g, e, out, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)n, (uint32_t)cols, (uint32_t)L.chunks,
        (uint32_t)rows, (uint32_t)L.strips);
  if ((stages & 2) && L.strips > 1) {
    const int64_t n4 = L.sketch_elems / 4;
    sketch_combine_kernel<<<grid_for((n4 + kBlock - 1) / kBlock, kNumCU * 8, max_blocks), kBlock, 0, s>>>(
        reinterpret_cast<const v4f*>(part), (uint32_t)L.strips, reinterpret_cast<v4f*>(S), (uint32_t)n4);
  }
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_sketch_estimate(float* g, float* e, const float* S, int64_t n_pad, int64_t n, int rows, int64_t cols,
                            uint64_t seed, int max_blocks, hipStream_t s) {
  check_shape(n_pad, n, rows, cols, max_blocks);
  check_aligned({g, e, S});
  const unsigned grid = grid_for((n + kSketchTile - 1) / kSketchTile, kNumCU * 8, max_blocks);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32), un = (uint32_t)n, uc = (uint32_t)cols;
  if (rows == 1) sketch_estimate_kernel<1><<<grid, kBlock, 0, s>>>(g, e, S, lo, hi, un, uc);
  if (rows == 3) sketch_estimate_kernel<3><<<grid, kBlock, 0, s>>>(g, e, S, lo, hi, un, uc);
  if (rows == 5) sketch_estimate_kernel<5><<<grid, kBlock, 0, s>>>(g, e, S, lo, hi, un, uc);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_sketch_fetch(float* e, void* wire, int64_t n_pad, int64_t n, int64_t k, int max_blocks, hipStream_t s) {
  check_shape(n_pad, n, 1, kSketchTile, max_blocks);
  FAN_CHECK(k >= 1 && k <= n, "sketch: 1 <= k <= n");
  check_aligned({e, wire});
  uint32_t* idx = static_cast<uint32_t*>(wire);
  float* val = reinterpret_cast<float*>(idx + (k + 3) / 4 * 4);
  sketch_fetch_kernel<<<grid_for((k + kBlock - 1) / kBlock, kNumCU * 4, max_blocks), kBlock, 0, s>>>(
      e, idx, val, (uint32_t)n, (uint32_t)k);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace fan
