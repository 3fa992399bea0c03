// Count-sketch gradient compression (ops/sketch_oracle.py is the definition): R rows of C columns; a chunk of C
// consecutive elements is rotated as a whole into every row (by a hashed multiple of 4 columns) and every element takes
// a hashed sign, so a sketch column is a gather over the chunks in a fixed order: contiguous 16-B loads, no atomics and
// results that do not depend on the grid. The estimate is the median over the rows; the k largest estimates are found
// by the keys-only radix select of topk/topk.h, and the exact values at those indices are fetched from the residual.
#pragma once
#include "common/hip_common.h"

namespace fan {

constexpr int kSketchTile = 1024;      // columns (accumulate) or elements (estimate) of one workgroup: 256 lanes x 16 B
constexpr int kSketchStrip = 16;       // chunks one accumulate workgroup adds, in chunk order
constexpr int kSketchMaxRows = 5;      // rows: 1, 3 or 5
constexpr int64_t kSketchMaxCols = (int64_t)1 << 22;

struct SketchLayout {
  int64_t chunks, strips, part_elems, sketch_elems;
};
inline SketchLayout sketch_layout(int64_t n_pad, int rows, int64_t cols) {
  const int64_t chunks = (n_pad + cols - 1) / cols, strips = (chunks + kSketchStrip - 1) / kSketchStrip;
  return {chunks, strips, strips * rows * cols, rows * cols};
}

// S[j][b] = the strips' partial sums in strip order, each the strip's sgn(g + e) at column b in chunk order (i < n).
// Two launches on s (accumulate into part, combine into S); with one strip the accumulate writes S itself and part is
// not touched. g, e: n_pad f32 (n_pad % 4 == 0, 1 <= n <= n_pad < 2^31), read only; part: sketch_layout().part_elems
// f32; S: rows * cols f32; all 16-B aligned. rows: 1, 3 or 5; cols: a multiple of 1024 in 1024 .. 2^22. max_blocks > 0
// caps every grid (the results do not depend on it). stages: bit 0 the accumulate, bit 1 the combine.
void launch_sketch(const float* g, const float* e, float* part, float* S, int64_t n_pad, int64_t n, int rows,
                   int64_t cols, uint64_t seed, int max_blocks, hipStream_t s, int stages = 3);
// For i < n: e[i] = g[i] + e[i]; g[i] = the median over the rows of sgn(S[j][col_j(i)]), the canonical NaN if any of
// them is NaN.
void launch_sketch_estimate(float* g, float* e, const float* S, int64_t n_pad, int64_t n, int rows, int64_t cols,
                            uint64_t seed, int max_blocks, hipStream_t s);
// val[j] = e[idx[j]], e[idx[j]] = +0 for j < k, on the top-k wire [u32 idx[k_pad]][f32 val[k_pad]]; an index at or
// past n (a stale wire) is skipped.
void launch_sketch_fetch(float* e, void* wire, int64_t n_pad, int64_t n, int64_t k, int max_blocks, hipStream_t s);

}  // namespace fan
