// Shared helpers for the torch-facing binding translation units.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#define FAN_T_CUDA_CONTIG(t)                                                       \
  TORCH_CHECK((t).is_cuda(), #t " must be a GPU tensor");                         \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

inline hipStream_t fan_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#include <vector>

#include "bfp/bfp_format.h"

// AdamWParams from the Python side's scalars (bfp_oracle.adamw_scalars, already rounded to f32, in its order:
// beta1, omb1, beta2, omb2, step_size, rsbc2, eps, decay) and the second-moment plane.
// The scalars alone (var = nullptr): the update with 8-bit moment planes keeps no f32 second-moment plane.
inline fan::AdamWParams fan_adamw_scalars(const std::vector<double>& s, double grad_scale, double weight_decay) {
  TORCH_CHECK(s.size() == 8, "adamw: 8 scalars (beta1, omb1, beta2, omb2, step_size, rsbc2, eps, decay)");
  return fan::AdamWParams{(float)grad_scale, (float)s[0], (float)s[1], (float)s[2], (float)s[3], (float)s[4],
                          (float)s[5], (float)s[6], (float)weight_decay, (float)s[7], nullptr};
}
inline fan::AdamWParams fan_adamw_params(const std::vector<double>& s, double grad_scale, double weight_decay,
                                         const at::Tensor& var, int64_t n_valid) {
  fan::AdamWParams p = fan_adamw_scalars(s, grad_scale, weight_decay);
  FAN_T_CUDA_CONTIG(var);
  TORCH_CHECK(var.scalar_type() == at::kFloat && var.numel() >= n_valid, "var: f32[n_valid]");
  p.var = var.data_ptr<float>();
  return p;
}
// LionParams from bfp_oracle.lion_scalars (already rounded to f32, in its order: beta1, omb1, beta2, omb2, lr, decay,
// wd).
inline fan::LionParams fan_lion_params(const std::vector<double>& s, double grad_scale) {
  TORCH_CHECK(s.size() == 7, "lion: 7 scalars (beta1, omb1, beta2, omb2, lr, decay, wd)");
  return fan::LionParams{(float)grad_scale, (float)s[0], (float)s[1], (float)s[2], (float)s[3], (float)s[4],
                         (float)s[6], (float)s[5]};
}
// One 8-bit moment plane of a padded bucket of n_pad elements (bfp_format.h launch_wire_adamw_q): contiguous uint8,
// exactly n_pad * 17 / 16 bytes, 16-byte aligned (a sliced tensor may not be), on `ref`'s device.
inline uint8_t* fan_moment_plane(const at::Tensor& t, int64_t n_pad, const at::Tensor& ref) {
  const int64_t pb = n_pad + n_pad / 16;
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kByte && t.numel() == pb &&
                  t.device() == ref.device(),
              "moment_codec bfp8: a moment plane is a contiguous uint8 tensor of exactly n_pad * 17 / 16 = ", pb,
              " bytes on the gradient's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "moment_codec bfp8: a moment plane is 16-byte aligned");
  return t.data_ptr<uint8_t>();
}

// LambParams from bfp_oracle.lamb_scalars (already rounded to f32, in its order: beta1, omb1, beta2, omb2, rsbc2, eps,
// rbc1, wd, lr) and the second-moment plane.
inline fan::LambParams fan_lamb_params(const std::vector<double>& s, double grad_scale, const at::Tensor& var,
                                       int64_t n_valid) {
  TORCH_CHECK(s.size() == 9, "lamb: 9 scalars (beta1, omb1, beta2, omb2, rsbc2, eps, rbc1, wd, lr)");
  FAN_T_CUDA_CONTIG(var);
  TORCH_CHECK(var.scalar_type() == at::kFloat && var.numel() >= n_valid, "var: f32[n_valid]");
  return fan::LambParams{(float)grad_scale, (float)s[0], (float)s[1], (float)s[2], (float)s[3], (float)s[4],
                         (float)s[5], (float)s[6], (float)s[7], (float)s[8], var.data_ptr<float>()};
}
