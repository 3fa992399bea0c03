// PowerSGD low-rank compression kernels for gfx950 (lowrank.h; ops/lowrank_oracle.py is the definition).
//
// The matrix X = G + E exists only as its two planes: every kernel here loads both and adds them in registers, one f32
// add per element, so all of them see the same bits. The two products are tall-skinny (N = 16, K in the thousands)
// and memory-bound: they run on v_mfma_f32_16x16x4_f32 with X straight from global memory in the instruction's A
// layout (no LDS for X) and the small dense operand staged in LDS once per workgroup. No atomics, no last-block
// fences: split-K partials land in slabs and lowrank_combine_kernel adds them in slab order, so every result is
// independent of the grid and of the order in which workgroups run. The orthogonalisation between the two products is
// either modified Gram-Schmidt in one workgroup (lowrank_orth_kernel) or CholeskyQR2 over 256-row strips in three
// launches (lowrank_gram_kernel, lowrank_cholqr_apply_kernel), whose 16 x 16 Gram matrices follow the same slab rule.
//
// v_mfma_f32_16x16x4_f32, D[16][16] += A[16][4] B[4][16]: lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16] and
// holds D[4 * (l / 16) + v][l % 16] in accumulator register v.
#include "lowrank/lowrank.h"

#include <initializer_list>

namespace fan {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kOrthBlock = 1024;
constexpr int kUnroll = 4;  // k-steps per batch; the next batch's loads are issued before this batch's MFMAs

// The three element-wise f32 statements of the definition, each rounded on its own (no contraction with a neighbour).
__device__ __forceinline__ v4f lr_x(v4f g, v4f e) {
#pragma clang fp contract(off)
  return g + e;
}
__device__ __forceinline__ v4f lr_sub(v4f x, v4f gh) {
#pragma clang fp contract(off)
  return x - gh;
}
__device__ __forceinline__ v4f lr_scale(v4f q, float inv) {
#pragma clang fp contract(off)
  return q * inv;
}

#define FAN_MFMA_16x16x4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ---------------------------------------------------------------- P partials: part[strip][rows][16] = X[:, strip] Q[strip]
// Workgroup (panel, strip): 4 waves x 16 rows by 512 columns. A k-step is 16 columns: lane l loads the float4 of G and
// of E at row l % 16, columns k0 + 4 * (l / 16) .. + 3, and MFMA j takes element j of it as A[l % 16][l / 16] — the K
// index of MFMA j's slot kk is column k0 + 4 * kk + j, a permutation of the 16 columns, legal because the K sum is
// order-free as long as B uses the same one: B[kk][n] = Q[k0 + 4 * kk + j][n]. The strip of Q lives in LDS as
// qs[k / 4][n] = the float4 {Q[k][n], k % 4 = 0..3}, so a lane's four B values are one 16-B read at qs[k0 / 4 + kk][n]
// = qs[(k0 / 16) * 64 + l]: consecutive lanes read consecutive 16 B, free of bank conflicts.
__global__ void __launch_bounds__(kBlock)
    lowrank_project_kernel(const float* __restrict__ g, const float* __restrict__ e, const float* __restrict__ q,
                           float* __restrict__ part, int rows, int cols) {
  __shared__ v4f qs[kLrProjStrip / 4 * kLrRank];  // 32 KB
  const int strip = blockIdx.y, c0 = strip * kLrProjStrip;
  const int len = min(kLrProjStrip, cols - c0);  // a multiple of 16
  for (int t = threadIdx.x; t < kLrProjStrip / 4 * kLrRank; t += kBlock) {
    const int kg = t >> 4, n = t & 15;
    v4f v = 0.0f;
    if (4 * kg < len) {  // (rows of Q past the strip's end stay zero)
      const float* src = q + (size_t)(c0 + 4 * kg) * kLrRank + n;
      v = (v4f){src[0], src[kLrRank], src[2 * kLrRank], src[3 * kLrRank]};
    }
    qs[t] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * kLrProjPanel + wave * 16;
  if (row0 >= rows) return;  // (rows % 16 == 0: a wave's 16 rows are all there or all missing)
  const int n = lane & 15, kk = lane >> 4;
  const size_t off = (size_t)(row0 + n) * cols + c0 + 4 * kk;
  const v4f* gp = reinterpret_cast<const v4f*>(g + off);  // k-step s: gp[4 * s]
  const v4f* ep = reinterpret_cast<const v4f*>(e + off);
  const int steps = len >> 4;
  v4f acc = 0.0f;
  v4f gc[kUnroll], ec[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    gc[u] = u < steps ? gp[4 * u] : (v4f)0.0f;
    ec[u] = u < steps ? ep[4 * u] : (v4f)0.0f;
  }
  for (int s0 = 0; s0 < steps; s0 += kUnroll) {
    v4f gn[kUnroll], en[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int s = s0 + kUnroll + u;
      gn[u] = s < steps ? gp[4 * s] : (v4f)0.0f;
      en[u] = s < steps ? ep[4 * s] : (v4f)0.0f;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (s0 + u < steps) {
        const v4f x = lr_x(gc[u], ec[u]);
        const v4f b = qs[(s0 + u) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = FAN_MFMA_16x16x4(x[j], b[j], acc);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      gc[u] = gn[u];
      ec[u] = en[u];
    }
  }
  float* out = part + ((size_t)strip * rows + row0 + 4 * kk) * kLrRank + n;
#pragma unroll
  for (int v = 0; v < 4; ++v) out[v * kLrRank] = acc[v];
}

// ---------------------------------------------------------------- Qn partials: part[strip][cols][16] = X[strip, :]^T P^[strip]
// The transposed product over the same planes: M is the column, K the row. Workgroup (tile, strip): 4 waves x 64
// columns by 512 rows. A k-step is 4 rows: lane l loads the float4 at row k0 + l / 16, columns c0 + 4 * (l % 16) .. + 3
// (sixteen lanes read 256 contiguous bytes of a row), and MFMA j takes element j as A[l % 16][l / 16]: its M index i
// is column c0 + 4 * i + j, so the four MFMAs of a k-step share one B, B[kk][n] = P^[k0 + kk][n] = ps[(k0 / 4) * 64 +
// l], and fill four accumulators; the store undoes the permutation.
__global__ void __launch_bounds__(kBlock)
    lowrank_backproject_kernel(const float* __restrict__ g, const float* __restrict__ e, const float* __restrict__ ph,
                               float* __restrict__ part, int rows, int cols) {
  __shared__ v4f ps4[kLrBackStrip * kLrRank / 4];  // 32 KB
  const int strip = blockIdx.y, r0 = strip * kLrBackStrip;
  const int len = min(kLrBackStrip, rows - r0);  // a multiple of 16
  const v4f* src = reinterpret_cast<const v4f*>(ph + (size_t)r0 * kLrRank);
  for (int t = threadIdx.x; t < kLrBackStrip * kLrRank / 4; t += kBlock) ps4[t] = t < len * 4 ? src[t] : (v4f)0.0f;
  __syncthreads();
  const float* ps = reinterpret_cast<const float*>(ps4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cw = blockIdx.x * kLrBackTile + wave * 64;
  if (cw >= cols) return;
  const int n = lane & 15, kk = lane >> 4;
  const int c = cw + 4 * n;
  const bool ok = c < cols;  // (cols % 4 == 0: a lane's four columns are all there or all missing)
  const size_t off = (size_t)(r0 + kk) * cols + c, step = (size_t)4 * cols;  // k-step s: + s * step
  const int steps = len >> 2;
  v4f acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  v4f gc[kUnroll], ec[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const bool ld = ok && u < steps;
    gc[u] = ld ? *reinterpret_cast<const v4f*>(g + off + u * step) : (v4f)0.0f;
    ec[u] = ld ? *reinterpret_cast<const v4f*>(e + off + u * step) : (v4f)0.0f;
  }
  for (int s0 = 0; s0 < steps; s0 += kUnroll) {
    v4f gn[kUnroll], en[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int s = s0 + kUnroll + u;
      const bool ld = ok && s < steps;
      gn[u] = ld ? *reinterpret_cast<const v4f*>(g + off + s * step) : (v4f)0.0f;
      en[u] = ld ? *reinterpret_cast<const v4f*>(e + off + s * step) : (v4f)0.0f;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (s0 + u < steps) {
        const v4f x = lr_x(gc[u], ec[u]);
        const float b = ps[(s0 + u) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = FAN_MFMA_16x16x4(x[j], b, acc[j]);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      gc[u] = gn[u];
      ec[u] = en[u];
    }
  }
  // acc[j][v] = Qn[cw + 4 * (4 * kk + v) + j][n]
  float* out = part + (size_t)strip * cols * kLrRank + n;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = cw + 4 * (4 * kk + v) + j;
      if (col < cols) out[(size_t)col * kLrRank] = acc[j][v];
    }
  }
}

// ---------------------------------------------------------------- out = part[0] + part[1] + ... in slab order
__global__ void __launch_bounds__(kBlock)
    lowrank_combine_kernel(const v4f* __restrict__ part, int slabs, v4f* __restrict__ out, size_t n4) {
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n4) return;
  v4f a = part[t];
  for (int s = 1; s < slabs; ++s) a = a + part[(size_t)s * n4 + t];
  out[t] = a;
}

// ---------------------------------------------------------------- P^ = orth(P): one workgroup, in place
// Sums of kN doubles over the workgroup in a fixed order — the lane's own partial, the wave's lanes by shuffles
// (32 .. 1), the waves in wave order — with the result in EVERY thread (all of them add the same 16 numbers in the same
// order).
template <int kN>
__device__ __forceinline__ void orth_block_sum(double (&a)[kN], double (*red)[kLrRank]) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int k = 0; k < kN; ++k) a[k] += __shfl_down(a[k], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kN; ++k) red[threadIdx.x >> 6][k] = a[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kN; ++k) a[k] = red[0][k];
#pragma unroll 1
  for (int w = 1; w < kOrthBlock / 64; ++w) {
#pragma unroll
    for (int k = 0; k < kN; ++k) a[k] += red[w][k];
  }
  __syncthreads();  // (red is free again)
}

// Modified Gram-Schmidt in powerSGD_hook's order. A thread owns rows t, t + 1024, ... for the whole kernel, so it only
// ever reads back what it wrote itself; the columns' fp64 dot products cross the workgroup through orth_block_sum.
// Per column j: (1) ||col_j|| -> inv = 1 / (norm + 1e-8); (2) col_j <- f32(col_j * inv) and the dots d_k = <col_j,
// col_k> for every later k at once (they are independent given j); (3) col_k <- f32(col_k - d_k * col_j), and while
// col_{j+1} is in hand, its squared norm for the next round's (1).
__global__ void __launch_bounds__(kOrthBlock) lowrank_orth_kernel(float* p, int rows, int rank) {
  __shared__ double red[kOrthBlock / 64][kLrRank];
  double nrm[1] = {0.0};
  for (int row = threadIdx.x; row < rows; row += kOrthBlock) {
    float* pr = p + (size_t)row * kLrRank;
#pragma unroll
    for (int k = 1; k < kLrRank; ++k) {
      if (k >= rank) pr[k] = 0.0f;
    }
    const double c = (double)pr[0];
    nrm[0] += c * c;
  }
  for (int j = 0; j < rank; ++j) {
    orth_block_sum<1>(nrm, red);
    const double inv = 1.0 / (sqrt(nrm[0]) + 1e-8);
    double d[kLrRank];
#pragma unroll
    for (int k = 0; k < kLrRank; ++k) d[k] = 0.0;
    for (int row = threadIdx.x; row < rows; row += kOrthBlock) {
      float* pr = p + (size_t)row * kLrRank;
      const float cj = (float)((double)pr[j] * inv);
      pr[j] = cj;
#pragma unroll
      for (int k = 1; k < kLrRank; ++k) {
        if (k > j && k < rank) d[k] += (double)cj * (double)pr[k];
      }
    }
    if (j + 1 == rank) break;
    orth_block_sum<kLrRank>(d, red);
    nrm[0] = 0.0;
    for (int row = threadIdx.x; row < rows; row += kOrthBlock) {
      float* pr = p + (size_t)row * kLrRank;
      const double cj = (double)pr[j];
#pragma unroll
      for (int k = 1; k < kLrRank; ++k) {
        if (k > j && k < rank) {
          const float v = (float)((double)pr[k] - d[k] * cj);
          pr[k] = v;
          if (k == j + 1) nrm[0] += (double)v * (double)v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- P^ = orth_cholqr2(P): three launches, in place
// CholeskyQR2 (the oracle's orth_cholqr2): per pass W = A^T A in fp64, Rinv from the Jacobi-scaled Cholesky factor of
// W, A <- A Rinv. The only dependency across rows is W, so every launch spreads over 256-row strips: the strips' Gram
// matrices land in part[strip][16][16] and every workgroup of the next launch adds them in strip order and redoes the
// few thousand flops of the factor for itself — the same bits everywhere, nobody waits for another workgroup.
//
// v_mfma_f64_16x16x4_f64, D[16][16] += A[16][4] B[4][16]: lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16], one
// double each, and holds D[4 * v + l / 16][l % 16] in accumulator register v. For W = X^T X over 4 rows of X the two
// operands are the same number, X[l / 16][l % 16]: no LDS, no transposition.
typedef double v4d __attribute__((ext_vector_type(4)));

#define FAN_MFMA_F64_16x16x4(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

constexpr double kCholPivotMin = 0x1p-40;

// Lane `src`'s value of x, in every lane (src is the same in all of them: a scalar read, no LDS).
__device__ __forceinline__ double lane_get(double x, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src),
                          __builtin_amdgcn_readlane(__double2loint(x), src));
}

// The four waves' Gram accumulators, added in wave order, to out[16][16] (row-major); ws: 4 x 256 doubles of LDS.
__device__ __forceinline__ void gram_store(v4d acc, double* ws, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < 4; ++v) ws[wave * 256 + (4 * v + (lane >> 4)) * kLrRank + (lane & 15)] = acc[v];
  __syncthreads();
  const int t = threadIdx.x;
  out[t] = ((ws[t] + ws[256 + t]) + ws[512 + t]) + ws[768 + t];
}

// part[strip][16][16] = A[strip]^T A[strip]. Workgroup = strip of 256 rows, a wave 64 of them in 16 k-steps of 4 rows:
// lane l loads the single float A[k0 + l / 16][l % 16] (the wave: 256 contiguous bytes), all 16 loads ahead of the
// 16 dependent MFMAs. Rows past the end are not loaded (rows % 16 == 0 keeps k-steps whole).
__global__ void __launch_bounds__(kBlock)
    lowrank_gram_kernel(const float* __restrict__ a, double* __restrict__ part, int rows) {
  __shared__ double ws[4 * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row0 = blockIdx.x * kLrOrthStrip + wave * 64 + (lane >> 4);
  float x[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int r = row0 + 4 * s;
    x[s] = r < rows ? a[(size_t)r * kLrRank + (lane & 15)] : 0.0f;
  }
  v4d acc = 0.0;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const double d = (double)x[s];
    acc = FAN_MFMA_F64_16x16x4(d, d, acc);
  }
  gram_store(acc, ws, part + (size_t)blockIdx.x * 256);
}

// The factor step, by the whole workgroup: W = the strips' partials in strip order (thread t element t), then wave 0
// alone: lane i (and its copies i + 16, ...) holds row i of C = S W S in registers and overwrites it with row i of L,
// column by column — L_jk crosses the wave by scalar lane reads, 120 of them; then lane j builds column j of T =
// (L^T)^-1 by back substitution, k = 15 .. 0, and stores column j of Rinv = S T as f32 in the apply's B layout,
// rs[l] = {Rinv[4 * (l / 16) + m][l % 16], m = 0..3}. *live = the mask of the live columns. Every statement in the
// oracle's order with no contraction; the caller's __syncthreads publishes rs and live.
__device__ __forceinline__ void cholqr_factor(const double* __restrict__ part, int strips, int rank, double* ws,
                                              v4f* rs, unsigned* live) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  double w = part[t];
#pragma unroll 8
  for (int s = 1; s < strips; ++s) w += part[(size_t)s * 256 + t];
  ws[t] = w;
  __syncthreads();
  if (t >= 64) return;
  const int i = t & 15;
  double c[kLrRank];
#pragma unroll
  for (int k = 0; k < kLrRank; ++k) c[k] = ws[i * kLrRank + k];
  const double d = ws[i * (kLrRank + 1)];
  int alive = i < rank && d != 0.0 && __builtin_isfinite(d);
  const double s = alive ? 1.0 / sqrt(d) : 0.0;
#pragma unroll
  for (int k = 0; k < kLrRank; ++k) {
    const double sk = lane_get(s, k);
    c[k] = alive && __builtin_amdgcn_readlane(alive, k) ? (c[k] * s) * sk : 0.0;
  }
#pragma unroll
  for (int j = 0; j < kLrRank; ++j) {
    double acc = c[j];
#pragma unroll
    for (int k = 0; k < j; ++k) acc = acc - c[k] * lane_get(c[k], j);
    const double piv = lane_get(acc, j);
    if (__builtin_amdgcn_readlane(alive, j) && piv > kCholPivotMin) {
      const double ljj = sqrt(piv);
      c[j] = i > j ? acc / ljj : (i == j ? ljj : 0.0);
    } else {  // column j is dead: its row and column of L are zero
      c[j] = 0.0;
      if (i == j) {
        alive = 0;
#pragma unroll
        for (int k = 0; k < j; ++k) c[k] = 0.0;
      }
    }
  }
  double tc[kLrRank];  // tc[k] = T[k][i]
#pragma unroll
  for (int k = kLrRank - 1; k >= 0; --k) {
    double acc = 0.0;
#pragma unroll
    for (int m = k + 1; m < kLrRank; ++m) acc = acc + lane_get(c[k], m) * tc[m];
    const double lkk = lane_get(c[k], k);
    tc[k] = lkk != 0.0 && alive ? (i > k ? -acc / lkk : (i == k ? 1.0 / lkk : 0.0)) : 0.0;
  }
  v4f r[4];
#pragma unroll
  for (int k = 0; k < kLrRank; ++k) r[k >> 2][k & 3] = (float)(lane_get(s, k) * tc[k]);
  if (t < 16) {
#pragma unroll
    for (int kq = 0; kq < 4; ++kq) rs[kq * 16 + i] = r[kq];
  }
  const unsigned mask = (unsigned)__ballot(alive) & 0xffffu;
  if (t == 0) *live = mask;
}

// A <- A Rinv in place, Rinv from the partials `win`. Workgroup = strip of 256 rows, a wave 4 tiles of 16 rows. A
// tile is loaded in the project kernel's A layout (lane l: the float4 at row l % 16, columns 4 * (l / 16) .. + 3; MFMA
// m takes element m, so its K slot kk is column 4 * kk + m and its B is rs[l][m]) ahead of the factor, whose latency
// hides the loads; dead columns are masked so that a non-finite entry there cannot reach a live one. The f32 tile
// leaves the four MFMAs as out[4 * (l / 16) + v][l % 16] in register v — for the fp64 matrix instruction that is
// k-step v with K slot l / 16 = row 4 * (l / 16) + v, a permutation of the tile's rows, which a Gram sum does not see.
// So the first apply (SECOND = false) also accumulates the Gram matrix of what it stores, from registers, and leaves
// it in wout[strip]: the second pass needs no Gram launch.
template <bool SECOND>
__global__ void __launch_bounds__(kBlock)
    lowrank_cholqr_apply_kernel(float* p, const double* __restrict__ win, double* __restrict__ wout, int rows,
                                int strips, int rank) {
  __shared__ double ws[4 * 256];
  __shared__ v4f rs[64];
  __shared__ unsigned live_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, kk = lane >> 4;
  const int row0 = blockIdx.x * kLrOrthStrip + wave * 64;
  v4f a[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = row0 + 16 * t;  // (rows % 16 == 0: a tile is all there or all missing)
    a[t] = r < rows ? *reinterpret_cast<const v4f*>(p + (size_t)(r + n) * kLrRank + 4 * kk) : (v4f)0.0f;
  }
  cholqr_factor(win, strips, rank, ws, rs, &live_s);
  __syncthreads();
  const v4f b = rs[lane];
  const unsigned live = live_s >> (4 * kk);
  v4d g = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = row0 + 16 * t;
    if (r >= rows) break;
    v4f acc = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; ++m) acc = FAN_MFMA_16x16x4((live >> m) & 1 ? a[t][m] : 0.0f, b[m], acc);
    float* out = p + (size_t)(r + 4 * kk) * kLrRank + n;
#pragma unroll
    for (int v = 0; v < 4; ++v) out[v * kLrRank] = acc[v];
    if (!SECOND) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const double d = (double)acc[v];
        g = FAN_MFMA_F64_16x16x4(d, d, g);
      }
    }
  }
  if (!SECOND) gram_store(g, ws, wout + (size_t)blockIdx.x * 256);  // (ws is free: wave 0 read it before the barrier)
}

// ---------------------------------------------------------------- G <- P^ Qm^T, E <- X - G, Q <- Qm = Qn * inv
// K is only 16: plain VALU. Workgroup (column tile, row panel): lane t owns columns c .. c + 3 of 1024 and keeps their
// Qm values (4 x 16, scaled by inv as they are loaded) in registers down a panel of 64 rows, whose P^ rows every lane
// reads from LDS at the same address (a broadcast). Per row: one 16-B load of G and of E, 64 fmas (each column's chain
// starts from 0 and runs k = 0 .. 15 in order), one 16-B store of G^ and of E'. The panel-0 workgroups also write their
// columns of Q. Built without the packed f32 instructions, like the project's other exact-order kernels; the barrier is
// spelled with builtins because the HIP headers' inline __syncthreads would become a call under the target attribute.
__global__ __attribute__((target("no-packed-fp32-ops"))) void __launch_bounds__(kBlock)
    lowrank_reconstruct_kernel(float* __restrict__ g, float* __restrict__ e, const float* __restrict__ ph,
                               const float* __restrict__ qn, float* __restrict__ q_out, float inv, int rows, int cols) {
  __shared__ v4f ps[kLrReconPanel * kLrRank / 4];  // 4 KB: one float4 per thread
  const int r0 = blockIdx.y * kLrReconPanel;
  const int len = rows - r0 < kLrReconPanel ? rows - r0 : kLrReconPanel;
  static_assert(kLrReconPanel * kLrRank / 4 == kBlock, "one staged float4 per thread");
  ps[threadIdx.x] = (int)threadIdx.x < len * 4
                        ? reinterpret_cast<const v4f*>(ph + (size_t)r0 * kLrRank)[threadIdx.x] : (v4f)0.0f;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const int c = blockIdx.x * kLrReconCols + (int)threadIdx.x * 4;
  if (c >= cols) return;  // (cols % 4 == 0: a lane's four columns are all there or all missing)
  v4f qm[4][4];  // [column][k / 4]
  const v4f* qsrc = reinterpret_cast<const v4f*>(qn + (size_t)c * kLrRank);
#pragma unroll
  for (int i = 0; i < 16; ++i) qm[i >> 2][i & 3] = lr_scale(qsrc[i], inv);
  if (blockIdx.y == 0) {
    v4f* qdst = reinterpret_cast<v4f*>(q_out + (size_t)c * kLrRank);
#pragma unroll
    for (int i = 0; i < 16; ++i) qdst[i] = qm[i >> 2][i & 3];
  }
  v4f* gp = reinterpret_cast<v4f*>(g + (size_t)r0 * cols + c);
  v4f* ep = reinterpret_cast<v4f*>(e + (size_t)r0 * cols + c);
  const size_t ld4 = (size_t)cols / 4;
#pragma unroll 2
  for (int r = 0; r < len; ++r) {
    const v4f x = lr_x(gp[r * ld4], ep[r * ld4]);
    v4f pv[4];
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) pv[k4] = ps[4 * r + k4];
    v4f gh;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
      float a = 0.0f;
#pragma unroll
      for (int k = 0; k < kLrRank; ++k) a = __builtin_fmaf(pv[k >> 2][k & 3], qm[cc][k >> 2][k & 3], a);
      gh[cc] = a;
    }
    gp[r * ld4] = gh;
    ep[r * ld4] = lr_sub(x, gh);
  }
}

void check_shape(int64_t rows, int64_t cols) {
  FAN_CHECK(rows > 0 && cols > 0 && rows % 16 == 0 && cols % 16 == 0,
            "lowrank: rows and cols must be positive multiples of 16");
  FAN_CHECK(rows <= INT32_MAX && cols <= INT32_MAX, "lowrank: rows and cols must fit 31 bits");
  FAN_CHECK((rows + kLrReconPanel - 1) / kLrReconPanel <= 65535 && (cols + kLrProjStrip - 1) / kLrProjStrip <= 65535,
            "lowrank: too many row panels or column strips for one grid");
}

void check_aligned(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    FAN_CHECK(p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0, "lowrank: planes must be 16-byte aligned");
}

}  // namespace

void launch_lowrank_project(const float* g, const float* e, const float* q, float* part, int64_t rows, int64_t cols,
                            hipStream_t s) {
  check_shape(rows, cols);
  check_aligned({g, e, q, part});
  const dim3 grid((unsigned)((rows + kLrProjPanel - 1) / kLrProjPanel), (unsigned)lowrank_layout(rows, cols).proj_strips);
  lowrank_project_kernel<<<grid, kBlock, 0, s>>>(g, e, q, part, (int)rows, (int)cols);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_lowrank_backproject(const float* g, const float* e, const float* ph, float* part, int64_t rows,
                                int64_t cols, hipStream_t s) {
  check_shape(rows, cols);
  check_aligned({g, e, ph, part});
  const dim3 grid((unsigned)((cols + kLrBackTile - 1) / kLrBackTile), (unsigned)lowrank_layout(rows, cols).back_strips);
  lowrank_backproject_kernel<<<grid, kBlock, 0, s>>>(g, e, ph, part, (int)rows, (int)cols);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_lowrank_combine(const float* part, int64_t slabs, float* out, int64_t n, hipStream_t s) {
  FAN_CHECK(slabs >= 1 && slabs <= INT32_MAX && n > 0 && n % 4 == 0, "lowrank combine: slabs >= 1, n a multiple of 4");
  check_aligned({part, out});
  const size_t n4 = (size_t)n / 4;
  const size_t blocks = (n4 + kBlock - 1) / kBlock;
  FAN_CHECK(blocks <= INT32_MAX, "lowrank combine: too many elements for one grid");
  lowrank_combine_kernel<<<(unsigned)blocks, kBlock, 0, s>>>(reinterpret_cast<const v4f*>(part), (int)slabs,
                                                             reinterpret_cast<v4f*>(out), n4);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_lowrank_orth(float* p, int64_t rows, int rank, hipStream_t s) {
  FAN_CHECK(rank >= 1 && rank <= kLrRank, "lowrank: the rank must lie in 1..16");
  FAN_CHECK(rows > 0 && rows % 16 == 0 && rows <= INT32_MAX, "lowrank: rows must be a positive multiple of 16");
  check_aligned({p});
  lowrank_orth_kernel<<<1, kOrthBlock, 0, s>>>(p, (int)rows, rank);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_lowrank_orth_cholqr2(float* p, int64_t rows, int rank, double* part, hipStream_t s) {
  FAN_CHECK(rank >= 1 && rank <= kLrRank, "lowrank: the rank must lie in 1..16");
  FAN_CHECK(rows > 0 && rows % 16 == 0 && rows <= INT32_MAX, "lowrank: rows must be a positive multiple of 16");
  check_aligned({p, part});
  const int strips = (int)lowrank_orth_strips(rows);
  double* part2 = part + (size_t)strips * 256;
  lowrank_gram_kernel<<<strips, kBlock, 0, s>>>(p, part, (int)rows);
  FAN_HIP_CHECK(hipGetLastError());
  lowrank_cholqr_apply_kernel<false><<<strips, kBlock, 0, s>>>(p, part, part2, (int)rows, strips, rank);
  FAN_HIP_CHECK(hipGetLastError());
  lowrank_cholqr_apply_kernel<true><<<strips, kBlock, 0, s>>>(p, part2, nullptr, (int)rows, strips, rank);
  FAN_HIP_CHECK(hipGetLastError());
}

void launch_lowrank_reconstruct(float* g, float* e, const float* ph, const float* qn, float* q_out, float inv,
                                int64_t rows, int64_t cols, hipStream_t s) {
  check_shape(rows, cols);
  check_aligned({g, e, ph, qn, q_out});
  const dim3 grid((unsigned)((cols + kLrReconCols - 1) / kLrReconCols),
                  (unsigned)((rows + kLrReconPanel - 1) / kLrReconPanel));
  lowrank_reconstruct_kernel<<<grid, kBlock, 0, s>>>(g, e, ph, qn, q_out, inv, (int)rows, (int)cols);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace fan
