// Rotated one-bit gradient compression (DRIVE; ops/rht_oracle.py is the definition): a bucket is cut into blocks of
// 4096 values, every block is rotated by a randomised Hadamard transform y = (1/64) H_4096 D x (D: hashed signs), and
// the rotated block is sent as one sign bit per value and one f32 scale, the mean |y|. The residual of that quantiser
// is kept in rotated coordinates, so the encoder needs one transform. H_4096 = H16 (x) H16 (x) H16 runs as three rounds
// of 16 x 16 products with a +-1 matrix on v_mfma_f32_16x16x4_f32.
#pragma once
#include "common/hip_common.h"

namespace fan {

constexpr int kRhtBlock = 4096;     // values of one transform block, one workgroup's work item
constexpr int kRhtSignBytes = 512;  // sign bytes of one block
constexpr int kRhtMaxWorld = 16;

struct RhtLayout {
  int64_t blocks, resid_elems, wire_bytes;
};
// One rank's wire: [u8 sign[512 * blocks]][f32 scale[blocks rounded up to 4]], both planes and the whole 16-B aligned.
inline RhtLayout rht_layout(int64_t n) {
  const int64_t nb = (n + kRhtBlock - 1) / kRhtBlock;
  return {nb, nb * kRhtBlock, nb * kRhtSignBytes + (nb + 3) / 4 * 4 * 4};
}

// Forward (inverse = false): out[blocks * 4096] = (1/64) H D x per block, x: n_pad f32 of which elements at or past n
// read as +0. Inverse: out[i] = (D (1/64) H x)[i] for i < n, x: blocks * 4096 f32, out: n_pad f32. n_pad % 4 == 0,
// 1 <= n <= n_pad < 2^31; planes 16-B aligned; max_blocks > 0 caps the grid (the results do not depend on it).
void launch_rht_transform(const float* x, float* out, int64_t n_pad, int64_t n, uint64_t seed, bool inverse,
                          int max_blocks, hipStream_t s);
// Per block: y = rht(g) + e; scale = sum|y| / 4096; sign bit i = y_i < 0; e = y - (bit ? -scale : scale). g: n_pad f32,
// read only; e: blocks * 4096 f32; wire: rht_layout(n).wire_bytes, every byte written.
void launch_rht_encode(const float* g, float* e, void* wire, int64_t n_pad, int64_t n, uint64_t seed, int max_blocks,
                       hipStream_t s);
// Per block: acc = the ranks' (bit ? -scale : scale) added in rank order from +0; g[i] = inverse(acc)[i] * inv_world for
// i < n. wires: world wires back to back, 1 <= world <= 16.
void launch_rht_decode(const void* wires, int world, float* g, int64_t n_pad, int64_t n, uint64_t seed,
                       float inv_world, int max_blocks, hipStream_t s);

}  // namespace fan
