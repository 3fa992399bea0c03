// bf16x3 split-precision GEMM for gfx950: f32 operands in memory, three v_mfma_f32_16x16x32_bf16 per product.
//
// The step between the exact f32 GEMM (gemm_f32.hip, v_mfma_f32_16x16x4_f32, about 1/16 of the bf16 matrix rate; CDNA4
// has no xf32) and bf16 storage. Per operand element x (f32), in registers:
//   h = bf16_rne(x),  l = bf16_rne(x - f32(h))    (the subtraction is exact in f32)
// and the kernel accumulates  h_a*l_b + l_a*h_b + h_a*h_b  in the f32 MFMA accumulators; l_a*l_b is dropped. Within one
// 16x16 output tile and one K step the two correction MFMAs are issued BEFORE the hi*hi one (the small terms enter
// the accumulator chain first). Every kept product of two bf16 values is exact in f32, so what remains is
//   |x - h - l| <= 2^-16 |x| per operand  ->  3 * 2^-16 * (1 + 2^-7) |a||b| per product,
// plus the f32 accumulation of 3K terms. Range: non-finite inputs give non-finite outputs (a NaN where f32 would
// give +-Inf is allowed: x - f32(h) is Inf - Inf); |x| >= 2^127 may overflow h to Inf; pieces below bf16's normal
// range (|l| < 2^-126, that is |x| below about 2^-118) are lost.
//
// Design. Block tile 128x128x32, 4 waves (2x2), each wave 64x64 = 4x4 MFMA tiles of 16x16 (64 accumulator
// registers). Both operands are staged AS F32 with global_load_lds_dwordx4 (glds.h; no VGPR round trip), two LDS stages
// of 32 KiB, one barrier per K tile, with gemm_f32.hip's LDS images and source-address swizzles:
//   * K-contiguous operand: [outer][k], 128-B rows of 32 f32, 16-B chunk c of row r at c ^ ((r>>1)&7);
//   * MN-contiguous operand: [k][outer], 512-B rows of 128 f32, 16-float block b of row k at b ^ ((k>>2)&3).
// One 16x16x32 bf16 fragment is 8 K values per lane. Lane group g = lane >> 4 takes k = 4g..4g+3 and 16+4g..16+4g+3 of
// the K tile, the same permutation of K for A and for B (the MFMA's k index 8g+i meets the same element of both):
//   * K-contiguous: two ds_read_b128, chunks g and g+4 of the lane's row. Each is exactly the read gemm_f32.hip
//     issues for its k chunk 0 resp. 1: over a lane group's 16 rows swz takes each of the 8 chunk positions twice and
//     the four lane groups sit on four different positions of a row, so each 16-B bank group is hit by exactly 8 of
//     the 64 lanes: the 1024 B of the read spread evenly, the minimum of 8 passes over the 32 banks;
//   * MN-contiguous: eight ds_read_b32, rows 4g+u and 16+4g+u at column (o + lane&15) ^ (g << 4): ((k>>2)&3) == g for
//     all eight rows, so the four lane groups read four disjoint 16-bank quarters of one 512-B row each.
// Each wave splits its 4 A and 4 B fragments once per K tile (v_cvt_pk_bf16_f32, a shift / mask back to f32, one
// subtract, a second packed convert: 64 values per lane) and reuses the 8 (hi, lo) pairs over its 16 output tiles:
// 48 MFMAs per wave and K tile against the 128 16x16x4 f32 MFMAs of gemm_f32.hip for the same depth. LDS bytes per MFMA
// are 2/3 of the bf16 kernels'. The next tile's staging is in flight under the splits and MFMAs of the current one; two
// workgroups per CU (64 KiB LDS each) let one workgroup's splits run under the other's MFMAs. Measured
// (profiles/gemm_f32x3.txt): 1.4x to 1.9x the f32 kernel, NOT MFMA-bound; fragment reads and splits are not software-
// pipelined under the MFMAs here. 149-156 VGPRs, 0 AGPRs, 0 scratch, 2 waves/SIMD (LDS-limited) in every instantiation.
//
// Any M, N, K that are multiples of 8: tiles are ceil-divided; a workgroup whose tile crosses an operand edge stages
// its out-of-range 16-B chunks from a zero page and stores only in-range elements (edge code is compiled into a
// branch only edge workgroups take). Split-K: ragged ranges of K tiles per workgroup, raw f32 partial tiles to slabs
// ws[split][M][N], summed in split order by this file's own reduce with the epilogue (deterministic).
#include "gemm/gemm.h"
#include "gemm/glds.h"

namespace fan {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 32, NT = 256;
constexpr int TILE_BYTES = 128 * BK * 4;  // 16 KiB
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int LDS_BYTES = 2 * STAGE_BYTES;

__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

static __device__ __attribute__((aligned(256))) uint4 g_f32x3_zero16[16];  // zero page for edge-tile chunks

// EDGE: 16-B chunks at outer >= o_lim or k >= k_lim (multiples of 4 floats) load the zero page instead.
template <bool KCONTIG, bool EDGE>
__device__ __forceinline__ void stage(const float* __restrict__ g, int64_t ld, int o0, int k0, char* tile, int wave,
                                      int lane, int o_lim, int k_lim) {
  const int t = wave * 64 + lane;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* src;
    bool out = false;
    if (KCONTIG) {
      const int row = i * 32 + (t >> 3);
      const int c = (t & 7) ^ swz(row);
      src = g + (int64_t)(o0 + row) * ld + k0 + c * 4;
      if (EDGE) out = o0 + row >= o_lim || k0 + c * 4 >= k_lim;
    } else {
      const int krow = i * 8 + (t >> 5);
      const int col = ((t & 31) * 4) ^ (((krow >> 2) & 3) << 4);
      src = g + (int64_t)(k0 + krow) * ld + o0 + col;
      if (EDGE) out = k0 + krow >= k_lim || o0 + col >= o_lim;
    }
    if (EDGE && out) src = reinterpret_cast<const float*>(g_f32x3_zero16);
    glds16((const void*)src, __builtin_amdgcn_readfirstlane(lds_addr_of(tile + i * 4096 + wave * 1024)));
  }
}

// The lane's 8 K values of the 16-wide outer block at o: v[0] = k 4g..4g+3, v[1] = k 16+4g..16+4g+3 (g = lane >> 4).
template <bool KCONTIG>
__device__ __forceinline__ void frag(const char* tile, int o, int lane, f32x4 (&v)[2]) {
  const int g = lane >> 4;
  if (KCONTIG) {
    const int row = o + (lane & 15);
    const char* p = tile + row * 128;
    v[0] = *reinterpret_cast<const f32x4*>(p + ((g ^ swz(row)) << 4));
    v[1] = *reinterpret_cast<const f32x4*>(p + (((g + 4) ^ swz(row)) << 4));
  } else {
    const int col = (o + (lane & 15)) ^ (g << 4);  // (k >> 2) & 3 == g for all eight rows
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[h][u] = *reinterpret_cast<const float*>(tile + (h * 16 + 4 * g + u) * 512 + col * 4);
  }
}

// x -> (hi, lo) bf16 pieces, 8 values per lane, packed in k order (pack_bf16x2: v_cvt_pk_bf16_f32, RNE).
__device__ __forceinline__ void split(const f32x4 (&v)[2], bf16x8& hi, bf16x8& lo) {
  u32x4 ph, pl;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = v[p >> 1][(p & 1) * 2], x1 = v[p >> 1][(p & 1) * 2 + 1];
    const uint32_t h = pack_bf16x2(x0, x1);
    ph[p] = h;
    pl[p] = pack_bf16x2(x0 - __uint_as_float(h << 16), x1 - __uint_as_float(h & 0xffff0000u));
  }
  hi = __builtin_bit_cast(bf16x8, ph);
  lo = __builtin_bit_cast(bf16x8, pl);
}

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int xcd = bid % kNumXCD;
  const int q = nwg / kNumXCD, r = nwg % kNumXCD;
  const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + bid / kNumXCD;
}

template <bool AK, bool BKC, int EPI, bool ACCUM, bool SPLIT>
__global__ void __launch_bounds__(NT, 2)
    gemm_f32x3_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
                      float* __restrict__ C, int64_t ldc, const float* __restrict__ bias,
                      const float* __restrict__ aux, int64_t ldaux, int M, int N, int K, int split_k,
                      float* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tiles_n = (N + BN - 1) / BN;
  const int tiles = ((M + BM - 1) / BM) * tiles_n;
  const int wg = xcd_remap(blockIdx.x, tiles * split_k);
  const int tile = wg % tiles, ksplit = wg / tiles;
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nkt = (K + BK - 1) / BK;
  const int kt_per = (nkt + split_k - 1) / split_k;
  const int kt0 = ksplit * kt_per;
  const int nk = max(0, min(nkt, kt0 + kt_per) - kt0);
  const int kbeg = kt0 * BK;
  const bool mn_edge = m0 + BM > M || n0 + BN > N;
  const bool edge = mn_edge || (kt0 + nk) * BK > K;  // uniform: predicated staging for this workgroup
  auto stage_ab = [&](int k0, char* dst) {
    if (edge) {
      stage<AK, true>(A, lda, m0, k0, dst, wave, lane, M, K);
      stage<BKC, true>(B, ldb, n0, k0, dst + TILE_BYTES, wave, lane, N, K);
    } else {
      stage<AK, false>(A, lda, m0, k0, dst, wave, lane, 0, 0);
      stage<BKC, false>(B, ldb, n0, k0, dst + TILE_BYTES, wave, lane, 0, 0);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nk > 0) stage_ab(kbeg, smem);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const char* sa = smem + cur * STAGE_BYTES;
    const char* sb = sa + TILE_BYTES;
    if (kt + 1 < nk) stage_ab(kbeg + (kt + 1) * BK, smem + (cur ^ 1) * STAGE_BYTES);
    bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v[2];
      frag<AK>(sa, wm * 64 + i * 16, lane, v);
      split(v, ah[i], al[i]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v[2];
      frag<BKC>(sb, wn * 64 + j * 16, lane, v);
      split(v, bh[j], bl[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 c = acc[i][j];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], c, 0, 0, 0);  // corrections first
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], c, 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], c, 0, 0, 0);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  const int col_l = lane & 15, row_l = (lane >> 4) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + wn * 64 + j * 16 + col_l;
    if (mn_edge && col >= N) continue;
    const float bv = (!SPLIT && (EPI == kEpiBias || EPI == kEpiBiasRelu)) ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 64 + i * 16 + row_l + r;
        if (mn_edge && row >= M) continue;
        if (SPLIT) {
          ws[((int64_t)ksplit * M + row) * N + col] = acc[i][j][r];
          continue;
        }
        float v = acc[i][j][r] + bv;
        if (EPI == kEpiBiasRelu) v = fmaxf(v, 0.f);
        if (EPI == kEpiReluMask) v = aux[(int64_t)row * ldaux + col] > 0.f ? v : 0.f;
        float* p = C + (int64_t)row * ldc + col;
        if (ACCUM) v += *p;
        *p = v;
      }
  }
}

// Ordered split-K reduction (slabs summed in split order) + the epilogue.
template <int EPI, bool ACCUM>
__global__ void __launch_bounds__(256)
    f32x3_splitk_reduce_kernel(const float* __restrict__ ws, int split_k, float* __restrict__ C, int64_t ldc,
                               const float* __restrict__ bias, const float* __restrict__ aux, int64_t ldaux, int M,
                               int N) {
  const int64_t total = (int64_t)M * N;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / N), col = (int)(e % N);
    float v = ws[e];
    for (int k = 1; k < split_k; ++k) v += ws[(int64_t)k * total + e];
    if (EPI == kEpiBias || EPI == kEpiBiasRelu) v += bias[col];
    if (EPI == kEpiBiasRelu) v = fmaxf(v, 0.f);
    if (EPI == kEpiReluMask) v = aux[(int64_t)row * ldaux + col] > 0.f ? v : 0.f;
    float* p = C + (int64_t)row * ldc + col;
    if (ACCUM) v += *p;
    *p = v;
  }
}

template <bool AK, bool BKC, int EPI, bool ACCUM>
void launch_typed(const GemmArgs& a, int sk, hipStream_t s) {
  const int grid = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * sk;
  if (sk > 1) {
    hipLaunchKernelGGL((gemm_f32x3_kernel<AK, BKC, EPI, ACCUM, true>), grid, NT, LDS_BYTES, s, (const float*)a.A,
                       a.lda, (const float*)a.B, a.ldb, (float*)a.C, a.ldc, (const float*)a.bias, (const float*)a.aux,
                       a.ldaux, a.M, a.N, a.K, sk, (float*)a.workspace);
    hipLaunchKernelGGL((f32x3_splitk_reduce_kernel<EPI, ACCUM>), stream_grid((size_t)a.M * a.N), 256, 0, s,
                       (const float*)a.workspace, sk, (float*)a.C, a.ldc, (const float*)a.bias, (const float*)a.aux,
                       a.ldaux, a.M, a.N);
  } else {
    hipLaunchKernelGGL((gemm_f32x3_kernel<AK, BKC, EPI, ACCUM, false>), grid, NT, LDS_BYTES, s, (const float*)a.A,
                       a.lda, (const float*)a.B, a.ldb, (float*)a.C, a.ldc, (const float*)a.bias, (const float*)a.aux,
                       a.ldaux, a.M, a.N, a.K, 1, nullptr);
  }
}

template <bool AK, bool BKC>
void launch_layout(const GemmArgs& a, hipStream_t s) {
  const int sk = gemm_f32_split(a.M, a.N, a.K, a.split_k);
#define FAN_F32X3_CASE(E)                                       \
  case E:                                                       \
    if (a.accumulate) launch_typed<AK, BKC, E, true>(a, sk, s); \
    else launch_typed<AK, BKC, E, false>(a, sk, s);             \
    break;
  switch (a.epilogue) {
    FAN_F32X3_CASE(kEpiNone)
    FAN_F32X3_CASE(kEpiBias)
    FAN_F32X3_CASE(kEpiBiasRelu)
    FAN_F32X3_CASE(kEpiReluMask)
    default: FAN_CHECK(false, "bad epilogue");
  }
#undef FAN_F32X3_CASE
}

}  // namespace

bool gemm_f32x3_supported(const GemmArgs& a) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return false;
  if (a.M % 8 || a.N % 8 || a.K % 8) return false;
  if (a.lda % 4 || a.ldb % 4) return false;
  if (((uintptr_t)a.A | (uintptr_t)a.B) & 15) return false;
  if (a.c_bf16 || a.colsum || a.defer_reduce) return false;
  if (a.epilogue < kEpiNone || a.epilogue > kEpiReluMask) return false;  // (no wire epilogues)
  if ((a.epilogue == kEpiBias || a.epilogue == kEpiBiasRelu) && a.bias == nullptr) return false;
  if (a.epilogue == kEpiReluMask && a.aux == nullptr) return false;
  if (gemm_f32_split(a.M, a.N, a.K, a.split_k) > 1 && a.workspace == nullptr) return false;
  return true;
}

void launch_gemm_f32x3(const GemmArgs& a, hipStream_t s) {
  FAN_CHECK(gemm_f32x3_supported(a), "gemm_f32x3: unsupported shape / layout / epilogue (need M, N, K % 8 == 0)");
  if (a.a_kcontig && a.b_kcontig) launch_layout<true, true>(a, s);
  else if (a.a_kcontig) launch_layout<true, false>(a, s);
  else if (a.b_kcontig) launch_layout<false, true>(a, s);
  else launch_layout<false, false>(a, s);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace fan
