// Grouped GEMM launch: up to kGroupMax bwd-weight GEMMs of one configuration in one dispatch. See gemm_group.hip.
#pragma once
#include "gemm/gemm.h"

namespace fan {

// n <= kGroupMax bwd-weight GEMMs dW_i = X_i^T . dY_i (A and B MN-contiguous, f32 out, no accumulate), each with its
// fused bias gradient (colsum) and either the BFP wire epilogue (all of them) or none; 256x128 tiles, one per
// workgroup, no split-K: M_i % 256 == 0, N_i % 128 == 0, K_i % 64 == 0. a[i].workspace: f32 scratch of
// gemm_wgrad_group_ws(a[i]) elements (the bias-gradient partials, one slab per 256-row tile row).
constexpr int kGroupMax = 8;
bool gemm_wgrad_group_supported(const GemmArgs* a, int n);
int64_t gemm_wgrad_group_ws(const GemmArgs& a);
void launch_gemm_wgrad_group(const GemmArgs* a, int n, hipStream_t stream);

// n <= kGroupMax bwd-weight GEMMs with the BFP wire epilogue (or its fused local update: every problem or none) and
// the fused bias gradient, on 256x256 tiles at one common split-K count `split` (2 or 4), one (tile, split) unit per
// workgroup, then ONE reduce launch over every problem's slabs (it also runs the stream's queued bias-gradient
// reduces, GemmArgs::defer_colsum): M_i % 256 == 0, N_i % 256 == 0, K_i % (64 * split) == 0. a[i].workspace: f32
// scratch of gemm_wgrad_splitk_group_ws(a[i], split) elements, laid out as the single launch's (split slabs of M x N,
// then the split bias partial rows). Each problem's outputs are bit-identical to launch_gemm_bf16 with
// tile 256x256 and split_k = split.
bool gemm_wgrad_splitk_group_supported(const GemmArgs* a, int n, int split);
int64_t gemm_wgrad_splitk_group_ws(const GemmArgs& a, int split);
void launch_gemm_wgrad_splitk_group(const GemmArgs* a, int n, int split, hipStream_t stream);

}  // namespace fan
