// Top-k gradient sparsification with memory (ops/topk_oracle.py is the definition): an exact radix select of the k
// largest |g + e| over a bucket, an ordered compaction into the wire [u32 idx[k_pad]][f32 val[k_pad]], and the
// scatter-accumulate of the gathered wires of up to 16 ranks back into the dense gradient.
#pragma once
#include "common/hip_common.h"

namespace fan {

constexpr int kTopkTile = 4096;      // elements of a count / compact / accumulate tile
constexpr int kTopkHistTile = 1024;  // elements one histogram workgroup takes per iteration (256 lanes x 16 B)
constexpr int kTopkBins0 = 2048;     // bins of digit 0 (key bits 30..20)
constexpr int kTopkBins = 1024;      // bins of digits 1 and 2 (key bits 19..10, 9..0)
constexpr int kTopkMaxWorld = 16;    // wires one accumulate launch takes
constexpr uint32_t kTopkPadIdx = 0xffffffffu;

// The select's scratch, u32 words: hist[2048], state[4] = {prefix, k_rem, -, -} ({T, ties} after the last pick), then
// per tile cnt_gt, cnt_eq, off, take. The caller zeroes it once; every select leaves the histogram zeroed.
struct TopkLayout {
  int64_t tiles, scratch_words, wire_bytes;
};
inline int64_t topk_k_pad(int64_t k) { return (k + 3) / 4 * 4; }
inline TopkLayout topk_layout(int64_t n_pad, int64_t k) {
  const int64_t tiles = (n_pad + kTopkTile - 1) / kTopkTile;
  return {tiles, kTopkBins0 + 4 + 4 * tiles, 8 * topk_k_pad(k)};
}

// e[i] = g[i] + e[i] (i < n); wire = the k largest |e| (ties to the lowest index), ascending by index, padded to
// k_pad; e[i] = +0 where sent. Nine launches on s (hist and pick per digit, count, scan, compact), no host sync. g, e:
// n_pad f32 (n_pad % 4 == 0, 1 <= k <= n <= n_pad < 2^31), wire: topk_layout().wire_bytes, scratch:
// topk_layout().scratch_words u32; all 16-B aligned. max_blocks > 0 caps every grid (the results do not depend on
// it). stages: bit i enables launch i in the order above (a probe times one launch at a time).
constexpr int kTopkAllStages = 511;
void launch_topk_select(const float* g, float* e, void* wire, uint32_t* scratch, int64_t n_pad, int64_t n, int64_t k,
                        int max_blocks, hipStream_t s, int stages = kTopkAllStages);
// The keys-only form: the k largest |plane[i]| (i < n) by the same keys, tie rule, wire, scratch and launches; val holds
// the plane's values. The plane is read only: nothing is added to it and nothing in it is zeroed.
void launch_topk_select_keys(const float* plane, void* wire, uint32_t* scratch, int64_t n_pad, int64_t n, int64_t k,
                             int max_blocks, hipStream_t s, int stages = kTopkAllStages);
// g[i] = (+0 + val_0[i] + val_1[i] + ...) * inv over the ranks that sent i, in rank order (i < n). wires: world wires
// of 8 * k_pad bytes each, back to back.
void launch_topk_accumulate(const void* wires, int world, float* g, int64_t n_pad, int64_t n, int64_t k, float inv,
                            int max_blocks, hipStream_t s);

}  // namespace fan
