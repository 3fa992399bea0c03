// PowerSGD low-rank gradient compression (ops/lowrank_oracle.py is the definition): the two tall-skinny products
// P = (G + E) Q and Qn = (G + E)^T P^ on the f32 matrix instruction, the slab combine, the Gram-Schmidt pass (or the
// multi-workgroup CholeskyQR2 in its place) and the reconstruction G^ = P^ Qm^T, E' = (G + E) - G^.
#pragma once
#include "common/hip_common.h"

namespace fan {

constexpr int kLrRank = 16;         // columns of P and Q, whatever the rank
constexpr int kLrProjPanel = 64;    // rows of a project workgroup (4 waves x 16)
constexpr int kLrProjStrip = 512;   // columns of a project strip (the Q rows one workgroup stages)
constexpr int kLrBackTile = 256;    // columns of a backproject workgroup (4 waves x 64)
constexpr int kLrBackStrip = 512;   // rows of a backproject strip (the P^ rows one workgroup stages)
constexpr int kLrReconCols = 1024;  // columns of a reconstruct workgroup (256 lanes x 4)
constexpr int kLrReconPanel = 64;   // rows of a reconstruct workgroup
constexpr int kLrOrthStrip = 256;   // rows of a CholeskyQR2 Gram strip (a workgroup: 4 waves x 64)

// CholeskyQR2 keeps two Gram partials (16 x 16 doubles) per strip in the bucket's partial buffer.
inline int64_t lowrank_orth_strips(int64_t rows) { return (rows + kLrOrthStrip - 1) / kLrOrthStrip; }
inline int64_t lowrank_cholqr_part_elems(int64_t rows) { return 2 * lowrank_orth_strips(rows) * 256 * 2; }  // in f32

struct LowrankLayout {
  int64_t proj_strips, back_strips, part_elems;  // part_elems: f32 elements of a partial buffer serving both products
};
inline LowrankLayout lowrank_layout(int64_t rows, int64_t cols) {
  const int64_t sp = (cols + kLrProjStrip - 1) / kLrProjStrip, sb = (rows + kLrBackStrip - 1) / kLrBackStrip;
  const int64_t a = sp * rows, b = sb * cols;
  return {sp, sb, (a > b ? a : b) * kLrRank};
}

// Every launcher checks rows % 16 == 0, cols % 16 == 0 and the 16-B alignment of its planes; the callers check the
// buffers' lengths (g, e: rows * cols; q, qn: cols * 16; p, ph: rows * 16; part: lowrank_layout(...).part_elems).
// part[strip][rows][16] = (g + e)[:, strip] q[strip]
void launch_lowrank_project(const float* g, const float* e, const float* q, float* part, int64_t rows, int64_t cols,
                            hipStream_t s);
// part[strip][cols][16] = (g + e)[strip, :]^T ph[strip]
void launch_lowrank_backproject(const float* g, const float* e, const float* ph, float* part, int64_t rows,
                                int64_t cols, hipStream_t s);
// out[i] = part[0][i] + part[1][i] + ... + part[slabs - 1][i] in that order, i < n (n % 4 == 0)
void launch_lowrank_combine(const float* part, int64_t slabs, float* out, int64_t n, hipStream_t s);
// p[rows][16] -> its orthonormalised columns 0..rank-1 in place, columns >= rank zeroed
void launch_lowrank_orth(float* p, int64_t rows, int rank, hipStream_t s);
// the same by CholeskyQR2 (the oracle's orth_cholqr2) in three launches over 256-row strips: Gram, apply + Gram of
// the result, apply. part: 2 * lowrank_orth_strips(rows) * 256 doubles of scratch, 16-B aligned
void launch_lowrank_orth_cholqr2(float* p, int64_t rows, int rank, double* part, hipStream_t s);
// qm = qn * inv -> q_out; g <- ph qm^T (fma chain over k = 0..15); e <- (g + e) - that
void launch_lowrank_reconstruct(float* g, float* e, const float* ph, const float* qn, float* q_out, float inv,
                                int64_t rows, int64_t cols, hipStream_t s);

}  // namespace fan
