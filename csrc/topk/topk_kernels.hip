// Top-k gradient sparsification kernels for gfx950 (topk.h; ops/topk_oracle.py is the definition).
//
// The vector to select from exists only as gradient + residual: the first histogram pass adds the two planes, stores
// the sum into the residual plane and every later kernel reads that one plane. The k-th largest key (the f32 bits
// without the sign) is found exactly by a three-digit radix select, 11 / 10 / 10 bits from the top: a histogram of the
// digit over the elements whose higher digits equal the prefix found so far, then one workgroup that walks the bins
// from the top. With the threshold key T and the number of ties to take in hand, a count per tile of 4096 elements, a
// one-workgroup scan over the tiles and an ordered compaction write the wire: everything above T and the first
// `ties` elements equal to T, ascending by index.
//
// Nothing here depends on the grid or on the order in which workgroups run: the only atomics are the integer adds of
// the histograms (addition of counts commutes), every tile's output position comes from the scan, and no kernel waits
// for another workgroup. The way back (topk_accumulate_kernel) owns a tile of the dense gradient per workgroup, adds
// the ranks' values in rank order in LDS and writes the gradient once.
#include "topk/topk.h"

#include <initializer_list>

namespace fan {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr uint32_t kAbsMask = 0x7fffffffu;

__device__ __forceinline__ uint32_t topk_key(float x) { return __float_as_uint(x) & kAbsMask; }

// Step 1 of the definition: one f32 add, rounded on its own.
__device__ __forceinline__ float topk_x(float g, float e) {
#pragma clang fp contract(off)
  return g + e;
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
// ... and its store: elements at or past n are not written.
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

// Exclusive prefix of v over the workgroup's 256 threads in thread order (and the total): the wave by shuffles, the
// four wave totals through LDS.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* red, uint32_t& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off);
    if (lane >= off) inc += t;
  }
  if (lane == kWave - 1) red[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t t = red[w];
    if (w < wave) before += t;
    total += t;
  }
  __syncthreads();  // (red is free again)
  return before + inc - v;
}

// ---------------------------------------------------------------- histogram of one radix digit
// Digit PASS of a key and whether the key takes part: pass 0 counts every element by bits 30..20, pass 1 the elements
// whose bits 30..20 equal the prefix by bits 19..10, pass 2 those whose bits 30..10 equal it by bits 9..0.
template <int PASS>
__device__ __forceinline__ bool topk_digit(uint32_t key, uint32_t prefix, uint32_t& d) {
  if (PASS == 0) {
    d = key >> 20;
    return true;
  }
  if (PASS == 1) {
    d = (key >> 10) & (kTopkBins - 1);
    return (key >> 20) == prefix;
  }
  d = key & (kTopkBins - 1);
  return (key >> 10) == prefix;
}

// Persistent workgroups stride over tiles of 1024 elements, 16 B per lane. Pass 0 reads g and e and stores e = g + e;
// the others read e alone. Every wave counts into its own copy of the histogram in LDS (gradients crowd into a few
// exponent bins: four copies quarter the same-address traffic, and a lane whose consecutive elements share a digit
// adds their count once); the copies are added and the non-zero bins flushed into the global histogram. KEYS (pass 0
// of the keys-only select): the keys are those of the plane e as it stands: g is not read and e is not written.
template <int PASS, bool KEYS = false>
__global__ void __launch_bounds__(kBlock)
    topk_hist_kernel(const float* __restrict__ g, float* __restrict__ e, const uint32_t* __restrict__ state,
                     uint32_t* __restrict__ hist, uint32_t n) {
  constexpr int kB = PASS == 0 ? kTopkBins0 : kTopkBins;
  __shared__ uint32_t lh[kWaves * kB];  // 32 KB (pass 0) or 16 KB
  for (int t = threadIdx.x; t < kWaves * kB; t += kBlock) lh[t] = 0;
  __syncthreads();
  uint32_t* mine = lh + (threadIdx.x / kWave) * kB;
  const uint32_t prefix = PASS == 0 ? 0u : state[0];
  const uint32_t tiles = (n + kTopkHistTile - 1) / kTopkHistTile;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t i = tile * kTopkHistTile + threadIdx.x * 4;
    if (i >= n) continue;
    v4f x = load4(e, i, n);
    if (PASS == 0 && !KEYS) {
      const v4f gv = load4(g, i, n);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = topk_x(gv[j], x[j]);
      store4(e, i, n, x);
    }
    const uint32_t nv = n - i < 4 ? n - i : 4;
    uint32_t run_d = 0, run_c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      uint32_t d;
      if (j < nv && topk_digit<PASS>(topk_key(x[j]), prefix, d)) {
        if (run_c != 0 && d != run_d) {
          atomicAdd(mine + run_d, run_c);
          run_c = 0;
        }
        run_d = d;
        ++run_c;
      }
    }
    if (run_c != 0) atomicAdd(mine + run_d, run_c);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kB; b += kBlock) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += lh[w * kB + b];
    if (s != 0) atomicAdd(hist + b, s);
  }
}

// ---------------------------------------------------------------- the bin that holds the k_rem-th largest
// One workgroup. Thread t owns kB / 256 bins, thread 0 the top ones, so the exclusive prefix over the threads is the
// count above a thread's bins. The one thread whose bins straddle k_rem walks them, appends the bin to the prefix and
// leaves the rank inside the bin in k_rem. Every bin is zeroed for the next pass (and the next select). After pass 2
// the words are the threshold key T and ties = k - #(key > T) >= 1.
template <int PASS>
__global__ void __launch_bounds__(kBlock) topk_pick_kernel(uint32_t* __restrict__ hist, uint32_t* __restrict__ state,
                                                           uint32_t k) {
  constexpr int kB = PASS == 0 ? kTopkBins0 : kTopkBins, kPer = kB / kBlock, kBits = PASS == 0 ? 11 : 10;
  __shared__ uint32_t red[kWaves];
  const uint32_t prefix = PASS == 0 ? 0u : state[0], k_rem = PASS == 0 ? k : state[1];
  const int top = kB - 1 - (int)threadIdx.x * kPer;
  uint32_t c[kPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    c[j] = hist[top - j];
    hist[top - j] = 0;
    sum += c[j];
  }
  uint32_t total;
  uint32_t above = block_scan(sum, red, total);  // (its barriers order the reads of state before the write below)
  if (above < k_rem && k_rem <= above + sum) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      if (above < k_rem && k_rem <= above + c[j]) {
        state[0] = (prefix << kBits) | (uint32_t)(top - j);
        state[1] = k_rem - above;
      }
      above += c[j];
    }
  }
}

// ---------------------------------------------------------------- per tile: #(key > T), #(key == T)
__global__ void __launch_bounds__(kBlock)
    topk_count_kernel(const float* __restrict__ e, const uint32_t* __restrict__ state, uint32_t* __restrict__ cnt_gt,
                      uint32_t* __restrict__ cnt_eq, uint32_t n, uint32_t tiles) {
  __shared__ uint32_t red[2][kWaves];
  const uint32_t T = state[0];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t wg = 0, wq = 0;  // the wave's counts (the same in every lane)
#pragma unroll
    for (int r = 0; r < kTopkTile / (kBlock * 4); ++r) {
      const uint32_t i = tile * kTopkTile + r * (kBlock * 4) + threadIdx.x * 4;
      const uint32_t nv = i >= n ? 0 : n - i < 4 ? n - i : 4;
      v4f x = 0.0f;
      if (nv != 0) x = load4(e, i, n);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t key = topk_key(x[j]);
        wg += __popcll(__ballot(j < nv && key > T));
        wq += __popcll(__ballot(j < nv && key == T));
      }
    }
    if (lane == 0) {
      red[0][wave] = wg;
      red[1][wave] = wq;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      uint32_t s = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) s += red[threadIdx.x][w];
      (threadIdx.x == 0 ? cnt_gt : cnt_eq)[tile] = s;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- exclusive scan over the tiles
// One workgroup; thread t owns a run of consecutive tiles. off = the selected elements of the earlier tiles, take =
// how many of this tile's ties are selected (the first `ties` in index order over the whole plane).
__global__ void __launch_bounds__(kBlock)
    topk_scan_kernel(const uint32_t* __restrict__ state, const uint32_t* __restrict__ cnt_gt,
                     const uint32_t* __restrict__ cnt_eq, uint32_t* __restrict__ off, uint32_t* __restrict__ take,
                     uint32_t tiles) {
  __shared__ uint32_t red[kWaves];
  const uint32_t ties = state[1];
  const uint32_t per = (tiles + kBlock - 1) / kBlock;
  const uint32_t lo = min(threadIdx.x * per, tiles), hi = min(lo + per, tiles);
  uint32_t sg = 0, sq = 0;
  for (uint32_t t = lo; t < hi; ++t) {
    sg += cnt_gt[t];
    sq += cnt_eq[t];
  }
  uint32_t total;
  uint32_t gt_before = block_scan(sg, red, total), eq_before = block_scan(sq, red, total);
  for (uint32_t t = lo; t < hi; ++t) {
    const uint32_t q = cnt_eq[t];
    off[t] = gt_before + min(eq_before, ties);
    take[t] = eq_before >= ties ? 0u : min(ties - eq_before, q);
    gt_before += cnt_gt[t];
    eq_before += q;
  }
}

// ---------------------------------------------------------------- ordered compaction of a tile into the wire
// A lane owns 4 consecutive elements, a wave 256, a round the workgroup's 1024, a tile 4 rounds: index order is round,
// wave, lane, element. Inside a wave the number of flagged elements in lower lanes is the sum over the four element
// slots of mbcnt(ballot); the 16 (round, wave) totals cross the workgroup through LDS. Two running prefixes, one for
// key > T and one for key == T: an element above T lands at off + (#above before it) + min(#ties before it, take), a
// tie whose rank q among the tile's ties is below take at off + (#above before it) + q. The selected elements are
// zeroed in the residual plane, and only the vectors that changed are stored back (KEYS: the plane is left alone).
template <bool KEYS>
__global__ void __launch_bounds__(kBlock)
    topk_compact_kernel(float* __restrict__ e, const uint32_t* __restrict__ state, const uint32_t* __restrict__ off,
                        const uint32_t* __restrict__ take, uint32_t* __restrict__ idx, float* __restrict__ val,
                        uint32_t n, uint32_t tiles, uint32_t k, uint32_t k_pad) {
  constexpr int kRounds = kTopkTile / (kBlock * 4);
  __shared__ uint32_t tot[2][kRounds * kWaves];
  const uint32_t T = state[0];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (blockIdx.x == 0 && threadIdx.x < k_pad - k) {  // the pad entries
    idx[k + threadIdx.x] = kTopkPadIdx;
    val[k + threadIdx.x] = 0.0f;
  }
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    v4f x[kRounds];
    uint32_t gm[kRounds], qm[kRounds], pg[kRounds], pq[kRounds];  // 4-bit flag masks; flagged elements in lower lanes
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      const uint32_t i = tile * kTopkTile + r * (kBlock * 4) + threadIdx.x * 4;
      const uint32_t nv = i >= n ? 0 : n - i < 4 ? n - i : 4;
      x[r] = 0.0f;
      if (nv != 0) x[r] = load4(e, i, n);
      gm[r] = qm[r] = pg[r] = pq[r] = 0;
      uint32_t wg = 0, wq = 0;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t key = topk_key(x[r][j]);
        const bool gt = j < nv && key > T, eq = j < nv && key == T;
        const uint64_t bg = __ballot(gt), bq = __ballot(eq);
        gm[r] |= (uint32_t)gt << j;
        qm[r] |= (uint32_t)eq << j;
        pg[r] += __builtin_amdgcn_mbcnt_hi((uint32_t)(bg >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bg, 0));
        pq[r] += __builtin_amdgcn_mbcnt_hi((uint32_t)(bq >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bq, 0));
        wg += __popcll(bg);
        wq += __popcll(bq);
      }
      if (lane == 0) {
        tot[0][r * kWaves + wave] = wg;
        tot[1][r * kWaves + wave] = wq;
      }
    }
    __syncthreads();
    const uint32_t o = off[tile], tk = take[tile];
    uint32_t gb = 0, qb = 0;  // flagged elements of the (round, wave) slots before the current one
    int s = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
      for (; s < r * kWaves + wave; ++s) {
        gb += tot[0][s];
        qb += tot[1][s];
      }
      if ((gm[r] | qm[r]) == 0) continue;
      const uint32_t i = tile * kTopkTile + r * (kBlock * 4) + threadIdx.x * 4;
      uint32_t g_run = gb + pg[r], q_run = qb + pq[r];
      bool changed = false;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const bool gt = (gm[r] >> j) & 1, eq = (qm[r] >> j) & 1;
        if (gt || (eq && q_run < tk)) {
          const uint32_t pos = o + g_run + (gt ? min(q_run, tk) : q_run);
          if (pos < k) {  // (always, with counts of this plane: keeps a stale scratch inside the wire)
            idx[pos] = i + j;
            val[pos] = x[r][j];
            x[r][j] = 0.0f;
            changed = !KEYS;
          }
        }
        g_run += gt;
        q_run += eq;
      }
      if (changed) store4(e, i, n, x[r]);
    }
    __syncthreads();  // (tot is free again)
  }
}

// ---------------------------------------------------------------- gathered wires -> the dense gradient
// First position of idx[0 .. len) that is >= key (idx ascending; the pad entries, 0xffffffff, sort last).
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ idx, uint32_t len, uint32_t key) {
  uint32_t lo = 0, hi = len;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (idx[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup per tile of 4096 output elements, held as f32 in LDS and zero-filled. Rank by rank: the tile's segment
// of the rank's ascending indices by two binary searches, then the lanes stride over it with a plain LDS read-add-write
// (indices are unique within a rank: no two lanes meet), then a barrier. Every element so sees +0 + val_0 + val_1 ...
// in rank order. The tile times inv is written once with 16-B stores.
__global__ void __launch_bounds__(kBlock)
    topk_accumulate_kernel(const uint8_t* __restrict__ wires, int world, float* __restrict__ g, uint32_t n,
                           uint32_t tiles, uint32_t k_pad, float inv) {
  __shared__ v4f acc4[kTopkTile / 4];  // 16 KB
  float* acc = reinterpret_cast<float*>(acc4);
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t base = tile * kTopkTile;
#pragma unroll
    for (int r = 0; r < kTopkTile / (kBlock * 4); ++r) acc4[r * kBlock + threadIdx.x] = 0.0f;
    __syncthreads();
    for (int rank = 0; rank < world; ++rank) {
      const uint32_t* idx = reinterpret_cast<const uint32_t*>(wires + (size_t)rank * 8 * k_pad);
      const float* val = reinterpret_cast<const float*>(idx + k_pad);
      const uint32_t lo = lower_bound(idx, k_pad, base), hi = lower_bound(idx, k_pad, base + kTopkTile);
      for (uint32_t p = lo + threadIdx.x; p < hi; p += kBlock) {
        const uint32_t d = idx[p] - base;
        if (d < (uint32_t)kTopkTile) acc[d] = acc[d] + val[p];  // (always, on an ascending wire)
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < kTopkTile / (kBlock * 4); ++r) {
      const uint32_t i = base + (r * kBlock + threadIdx.x) * 4;
      if (i < n) store4(g, i, n, acc4[r * kBlock + threadIdx.x] * inv);
    }
    __syncthreads();  // (the next tile's zero fill)
  }
}

void check_plane(int64_t n_pad, int64_t n, int64_t k) {
  FAN_CHECK(n_pad > 0 && n_pad % 4 == 0 && n_pad < ((int64_t)1 << 31),
            "topk: n_pad must be a positive multiple of 4 below 2^31");
  FAN_CHECK(n >= 1 && n <= n_pad && k >= 1 && k <= n, "topk: 1 <= k <= n <= n_pad");
}

void check_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    FAN_CHECK(p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0, "topk: planes must be 16-byte aligned");
}

unsigned grid_for(int64_t tiles, int cap, int max_blocks) {
  if (max_blocks > 0) cap = max_blocks;
  return (unsigned)(tiles < cap ? tiles : cap);
}

template <bool KEYS>
void select_launches(const float* g, float* e, void* wire, uint32_t* scratch, int64_t n_pad, int64_t n, int64_t k,
                     int max_blocks, hipStream_t s, int stages) {
  check_plane(n_pad, n, k);
  check_aligned({g, e, wire, scratch});
  FAN_CHECK(max_blocks >= 0, "topk: max_blocks >= 0");
  const uint32_t un = (uint32_t)n, uk = (uint32_t)k, kp = (uint32_t)topk_k_pad(k);
  const uint32_t tiles = (uint32_t)((n + kTopkTile - 1) / kTopkTile);
  const int64_t all_tiles = topk_layout(n_pad, k).tiles;  // the arrays' stride (>= tiles)
  uint32_t* hist = scratch;
  uint32_t* state = scratch + kTopkBins0;
  uint32_t* cnt_gt = state + 4;
  uint32_t* cnt_eq = cnt_gt + all_tiles;
  uint32_t* off = cnt_eq + all_tiles;
  uint32_t* take = off + all_tiles;
  uint32_t* idx = static_cast<uint32_t*>(wire);
  float* val = reinterpret_cast<float*>(idx + kp);
  const unsigned hgrid = grid_for((n + kTopkHistTile - 1) / kTopkHistTile, kNumCU * 4, max_blocks);
  const unsigned tgrid = grid_for(tiles, kNumCU * 8, max_blocks);
  if (stages & 1) topk_hist_kernel<0, KEYS><<<hgrid, kBlock, 0, s>>>(g, e, state, hist, un);
  if (stages & 2) topk_pick_kernel<0><<<1, kBlock, 0, s>>>(hist, state, uk);
  if (stages & 4) topk_hist_kernel<1><<<hgrid, kBlock, 0, s>>>(g, e, state, hist, un);
  if (stages & 8) topk_pick_kernel<1><<<1, kBlock, 0, s>>>(hist, state, uk);
  if (stages & 16) topk_hist_kernel<2><<<hgrid, kBlock, 0, s>>>(g, e, state, hist, un);
  if (stages & 32) topk_pick_kernel<2><<<1, kBlock, 0, s>>>(hist, state, uk);
  if (stages & 64) topk_count_kernel<<<tgrid, kBlock, 0, s>>>(e, state, cnt_gt, cnt_eq, un, tiles);
  if (stages & 128) topk_scan_kernel<<<1, kBlock, 0, s>>>(state, cnt_gt, cnt_eq, off, take, tiles);
  if (stages & 256) topk_compact_kernel<KEYS><<<tgrid, kBlock, 0, s>>>(e, state, off, take, idx, val, un, tiles, uk, kp);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace

void launch_topk_select(const float* g, float* e, void* wire, uint32_t* scratch, int64_t n_pad, int64_t n, int64_t k,
                        int max_blocks, hipStream_t s, int stages) {
  select_launches<false>(g, e, wire, scratch, n_pad, n, k, max_blocks, s, stages);
}

void launch_topk_select_keys(const float* plane, void* wire, uint32_t* scratch, int64_t n_pad, int64_t n, int64_t k,
                             int max_blocks, hipStream_t s, int stages) {
  select_launches<true>(plane, const_cast<float*>(plane), wire, scratch, n_pad, n, k, max_blocks, s, stages);
}

void launch_topk_accumulate(const void* wires, int world, float* g, int64_t n_pad, int64_t n, int64_t k, float inv,
                            int max_blocks, hipStream_t s) {
  check_plane(n_pad, n, k);
  check_aligned({wires, g});
  FAN_CHECK(world >= 1 && world <= kTopkMaxWorld, "topk: 1..16 ranks");
  FAN_CHECK(max_blocks >= 0, "topk: max_blocks >= 0");
  const uint32_t tiles = (uint32_t)((n + kTopkTile - 1) / kTopkTile);
  topk_accumulate_kernel<<<grid_for(tiles, kNumCU * 8, max_blocks), kBlock, 0, s>>>(
      static_cast<const uint8_t*>(wires), world, g, (uint32_t)n, tiles, (uint32_t)topk_k_pad(k), inv);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace fan
