// Python bindings of the fpga_ai_nic_amd native runtime (module fpga_ai_nic_amd._C).
//
// Only this translation unit includes torch headers; kernels live in their own .hip files and
// take raw pointers + a hipStream_t (the caller's current torch HIP stream).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include "bfp/bfp_format.h"
#include "bindings_common.h"

namespace fan {
void register_gemm(pybind11::module_& m);
void register_nn(pybind11::module_& m);
void register_planner(pybind11::module_& m);
void register_engine(pybind11::module_& m);
}  // namespace fan

namespace {

using fan::DType;

int dtype_code(const at::Tensor& t) {
  if (t.scalar_type() == at::kFloat) return fan::kF32;
  if (t.scalar_type() == at::kBFloat16) return fan::kBF16;
  TORCH_CHECK(false, "expected float32 or bfloat16 tensor, got ", t.scalar_type());
}

void wire_pack(const at::Tensor& x, at::Tensor& out, int64_t shard_elems, int64_t codec) {
  FAN_T_CUDA_CONTIG(x);
  FAN_T_CUDA_CONTIG(out);
  TORCH_CHECK(out.scalar_type() == at::kByte, "packed buffer must be uint8");
  TORCH_CHECK(x.numel() % shard_elems == 0, "numel must be a multiple of shard_elems");
  const int n_shards = (int)(x.numel() / shard_elems);
  TORCH_CHECK((size_t)out.numel() >= fan::wire_shard_bytes((int)codec, shard_elems) * n_shards, "packed buffer too small");
  fan::launch_wire_pack((int)codec, dtype_code(x), x.data_ptr(), out.data_ptr(), (size_t)shard_elems, n_shards,
                        fan_stream());
}

// shard s of x encoded straight into dsts[s] (each a uint8 view, e.g. a peer's receive-arena slot; a None entry is a
// null destination: its shard is skipped); ends with a system-scope release (the direct P2P transport's producer kernel)
void wire_pack_to(const at::Tensor& x, const std::vector<c10::optional<at::Tensor>>& dsts, int64_t shard_elems,
                  int64_t codec) {
  FAN_T_CUDA_CONTIG(x);
  TORCH_CHECK(x.numel() == shard_elems * (int64_t)dsts.size(), "one destination per shard");
  TORCH_CHECK(dsts.size() <= (size_t)fan::kMaxPeers, "at most 16 destinations");
  fan::WirePtrs to{};
  for (size_t i = 0; i < dsts.size(); ++i) {
    if (!dsts[i] || !dsts[i]->defined()) continue;
    const at::Tensor& d = *dsts[i];
    TORCH_CHECK(d.is_cuda() && d.scalar_type() == at::kByte &&
                    (size_t)d.numel() >= fan::wire_shard_bytes((int)codec, shard_elems) &&
                    ((uintptr_t)d.data_ptr() & 15) == 0,
                "destination ", i, ": 16-B aligned uint8 buffer of one wire shard");
    to.p[i] = d.data_ptr<uint8_t>();
  }
  fan::launch_wire_pack_to((int)codec, dtype_code(x), x.data_ptr(), to, (size_t)shard_elems, (int)dsts.size(), -1, {},
                           true, fan_stream());
}

void wire_pack_range(const at::Tensor& x, at::Tensor& out, int64_t shard_elems, int64_t begin, int64_t end,
                     int64_t codec) {
  FAN_T_CUDA_CONTIG(x);
  FAN_T_CUDA_CONTIG(out);
  TORCH_CHECK(out.scalar_type() == at::kByte, "packed buffer must be uint8");
  TORCH_CHECK(shard_elems > 0 && shard_elems % 256 == 0, "shard_elems must be a positive multiple of 256");
  TORCH_CHECK(0 <= begin && begin <= end && end <= x.numel() && begin % 16 == 0 && end % 16 == 0, "bad range");
  if (end == begin) return;
  const int64_t shards = (end - 1) / shard_elems + 1;
  TORCH_CHECK((int64_t)out.numel() >= (int64_t)fan::wire_shard_bytes((int)codec, shard_elems) * shards,
              "packed buffer too small");
  fan::launch_wire_pack_range((int)codec, dtype_code(x), x.data_ptr(), out.data_ptr(), (size_t)shard_elems,
                              (size_t)begin, (size_t)end, fan_stream());
}

void wire_unpack(const at::Tensor& packed, at::Tensor& out, int64_t shard_elems, int64_t codec) {
  FAN_T_CUDA_CONTIG(packed);
  FAN_T_CUDA_CONTIG(out);
  TORCH_CHECK(out.numel() % shard_elems == 0, "numel must be a multiple of shard_elems");
  const int n_shards = (int)(out.numel() / shard_elems);
  TORCH_CHECK((size_t)packed.numel() >= fan::wire_shard_bytes((int)codec, shard_elems) * n_shards, "packed buffer too small");
  fan::launch_wire_unpack((int)codec, dtype_code(out), packed.data_ptr(), out.data_ptr(), (size_t)shard_elems,
                          n_shards, fan_stream());
}

void wire_reduce(const at::Tensor& slots, int64_t n_slots, int64_t self_pos, const c10::optional<at::Tensor>& local,
                 const c10::optional<at::Tensor>& out_wire, const c10::optional<at::Tensor>& out_f32,
                 int64_t shard_elems, int64_t codec) {
  FAN_T_CUDA_CONTIG(slots);
  const size_t sb = fan::wire_shard_bytes((int)codec, shard_elems);
  // only slots other than self_pos are read (self_pos is replaced by the dense local operand)
  const int64_t last_read = (local && self_pos == n_slots - 1) ? n_slots - 2 : n_slots - 1;
  TORCH_CHECK((size_t)slots.numel() * slots.element_size() >= sb * (size_t)(last_read + 1), "slots buffer too small");
  const void* lp = nullptr;
  int ld = fan::kF32;
  if (local) {
    FAN_T_CUDA_CONTIG((*local));
    TORCH_CHECK(local->numel() >= shard_elems, "local operand too small");
    lp = local->data_ptr();
    ld = dtype_code(*local);
  }
  void* ow = nullptr;
  float* of = nullptr;
  if (out_wire) {
    FAN_T_CUDA_CONTIG((*out_wire));
    TORCH_CHECK((size_t)out_wire->numel() * out_wire->element_size() >= sb, "out_wire too small");
    ow = out_wire->data_ptr();
  }
  if (out_f32) {
    FAN_T_CUDA_CONTIG((*out_f32));
    TORCH_CHECK(out_f32->scalar_type() == at::kFloat && out_f32->numel() >= shard_elems, "bad out_f32");
    of = out_f32->data_ptr<float>();
  }
  fan::launch_wire_reduce((int)codec, ld, slots.data_ptr(), sb, (int)n_slots, (int)self_pos, lp, ow, of,
                          (size_t)shard_elems, fan_stream());
}

// the four f32 device words of a clip group (bfp_format.h launch_clip_coef), or nullptr
const float* clip_words_ptr(const c10::optional<at::Tensor>& clip) {
  if (!clip) return nullptr;
  FAN_T_CUDA_CONTIG((*clip));
  TORCH_CHECK(clip->scalar_type() == at::kFloat && clip->numel() >= 4, "clip: f32[4]");
  return clip->data_ptr<float>();
}

void wire_sgd(const at::Tensor& wire, int64_t shard_elems, int64_t n_shards, int64_t skip_shard, int64_t skip_period,
              at::Tensor& master,
              const c10::optional<at::Tensor>& lp, const c10::optional<at::Tensor>& mom, double lr, double grad_scale,
              double weight_decay, double momentum, bool nesterov, int64_t n_valid, int64_t codec,
              const c10::optional<at::Tensor>& clip) {
  FAN_T_CUDA_CONTIG(wire);
  FAN_T_CUDA_CONTIG(master);
  TORCH_CHECK(master.scalar_type() == at::kFloat, "master weights must be float32");
  TORCH_CHECK(master.numel() >= n_valid, "master too small");
  TORCH_CHECK((size_t)wire.numel() * wire.element_size() >= fan::wire_shard_bytes((int)codec, shard_elems) * n_shards,
              "wire buffer too small");
  fan::bf16_t* lpp = nullptr;
  float* mp = nullptr;
  if (lp) {
    FAN_T_CUDA_CONTIG((*lp));
    TORCH_CHECK(lp->scalar_type() == at::kBFloat16 && lp->numel() >= n_valid, "bad lp weights");
    lpp = reinterpret_cast<fan::bf16_t*>(lp->data_ptr());
  }
  if (mom) {
    FAN_T_CUDA_CONTIG((*mom));
    TORCH_CHECK(mom->scalar_type() == at::kFloat && mom->numel() >= n_valid, "bad momentum buffer");
    mp = mom->data_ptr<float>();
  }
  fan::SgdParams p{(float)lr, (float)grad_scale, (float)weight_decay, (float)momentum, nesterov ? 1 : 0};
  fan::launch_wire_sgd((int)codec, wire.data_ptr(), (size_t)shard_elems, (int)n_shards, (int)skip_shard, (int)skip_period,
                       master.data_ptr<float>(), lpp, mp, p, (size_t)n_valid, fan_stream(), 0, clip_words_ptr(clip));
}

void wire_adamw(const at::Tensor& wire, int64_t shard_elems, int64_t n_shards, int64_t skip_shard, int64_t skip_period,
                at::Tensor& master, const c10::optional<at::Tensor>& lp, at::Tensor& mom, at::Tensor& var,
                const std::vector<double>& scalars, double grad_scale, double weight_decay, int64_t n_valid,
                int64_t codec, int64_t shard_stride, const c10::optional<at::Tensor>& clip) {
  FAN_T_CUDA_CONTIG(wire);
  FAN_T_CUDA_CONTIG(master);
  FAN_T_CUDA_CONTIG(mom);
  TORCH_CHECK(master.scalar_type() == at::kFloat, "master weights must be float32");
  TORCH_CHECK(master.numel() >= n_valid, "master too small");
  TORCH_CHECK(mom.scalar_type() == at::kFloat && mom.numel() >= n_valid, "bad first-moment buffer");
  const size_t sb = fan::wire_shard_bytes((int)codec, shard_elems);
  TORCH_CHECK(shard_stride == 0 || (size_t)shard_stride >= sb, "shard_stride below the packed shard size");
  const size_t need = n_shards > 0 ? (shard_stride ? (size_t)shard_stride * (n_shards - 1) + sb : sb * n_shards) : 0;
  TORCH_CHECK((size_t)wire.numel() * wire.element_size() >= need, "wire buffer too small");
  TORCH_CHECK(shard_stride % 16 == 0, "shard_stride must keep 16-byte alignment");
  fan::bf16_t* lpp = nullptr;
  if (lp) {
    FAN_T_CUDA_CONTIG((*lp));
    TORCH_CHECK(lp->scalar_type() == at::kBFloat16 && lp->numel() >= n_valid, "bad lp weights");
    lpp = reinterpret_cast<fan::bf16_t*>(lp->data_ptr());
  }
  const fan::AdamWParams p = fan_adamw_params(scalars, grad_scale, weight_decay, var, n_valid);
  fan::launch_wire_adamw((int)codec, wire.data_ptr(), (size_t)shard_elems, (int)n_shards, (int)skip_shard,
                         (int)skip_period, master.data_ptr<float>(), lpp, mom.data_ptr<float>(), p, (size_t)n_valid,
                         fan_stream(), (size_t)shard_stride, clip_words_ptr(clip));
}

// the planes of the trust-ratio passes: f32, whole lanes readable (8 values in pass 1, 4 in pass 2)
static void lamb_check_planes(const at::Tensor& master, const at::Tensor& mom, const at::Tensor& var, int64_t n_valid) {
  FAN_T_CUDA_CONTIG(master);
  FAN_T_CUDA_CONTIG(mom);
  FAN_T_CUDA_CONTIG(var);
  const int64_t need = (n_valid + 7) / 8 * 8;
  TORCH_CHECK(master.scalar_type() == at::kFloat && mom.scalar_type() == at::kFloat && var.scalar_type() == at::kFloat,
              "master, mom and var must be float32");
  TORCH_CHECK(master.numel() >= need && mom.numel() >= need && var.numel() >= need,
              "master, mom and var must hold n_valid rounded up to 8 elements");
}

int64_t wire_lamb_moments(const at::Tensor& wire, int64_t shard_elems, int64_t n_shards, int64_t skip_shard,
                          int64_t skip_period, const at::Tensor& master, at::Tensor& mom, at::Tensor& var,
                          const std::vector<double>& scalars, double grad_scale, int64_t n_valid, int64_t n_adapt,
                          at::Tensor& partials, int64_t partials_base, int64_t codec, int64_t shard_stride,
                          const c10::optional<at::Tensor>& clip) {
  FAN_T_CUDA_CONTIG(wire);
  FAN_T_CUDA_CONTIG(partials);
  TORCH_CHECK(shard_elems > 0 && n_shards > 0 && n_valid >= 0 && n_valid <= shard_elems * n_shards, "bad shape");
  TORCH_CHECK(n_adapt >= 0 && n_adapt <= n_valid, "n_adapt must lie in [0, n_valid]");
  lamb_check_planes(master, mom, var, n_valid);
  const size_t sb = fan::wire_shard_bytes((int)codec, shard_elems);
  TORCH_CHECK(shard_stride == 0 || (size_t)shard_stride >= sb, "shard_stride below the packed shard size");
  TORCH_CHECK(shard_stride % 16 == 0, "shard_stride must keep 16-byte alignment");
  const size_t need = shard_stride ? (size_t)shard_stride * (n_shards - 1) + sb : sb * n_shards;
  TORCH_CHECK((size_t)wire.numel() * wire.element_size() >= need, "wire buffer too small");
  const int64_t pairs = fan::lamb_partials_for((size_t)shard_elems);
  TORCH_CHECK(partials.scalar_type() == at::kDouble && partials_base >= 0 &&
                  partials.numel() >= 2 * (partials_base + pairs),
              "partials: f64[2 * (partials_base + ", pairs, ")]");
  const fan::LambParams p = fan_lamb_params(scalars, grad_scale, var, n_valid);
  fan::launch_wire_lamb_moments((int)codec, wire.data_ptr(), (size_t)shard_elems, (int)n_shards, (int)skip_shard,
                                (int)skip_period, master.data_ptr<float>(), mom.data_ptr<float>(), p, (size_t)n_valid,
                                (size_t)n_adapt, partials.data_ptr<double>() + 2 * partials_base, fan_stream(),
                                (size_t)shard_stride, clip_words_ptr(clip));
  return pairs;
}

// the norm pass of a clip group over one gathered wire region; returns the partials written from partials_base
int64_t wire_sumsq(const at::Tensor& wire, int64_t shard_elems, int64_t n_shards, int64_t skip_shard,
                   int64_t skip_period, int64_t n_valid, at::Tensor& partials, int64_t partials_base, int64_t codec,
                   int64_t shard_stride) {
  FAN_T_CUDA_CONTIG(wire);
  FAN_T_CUDA_CONTIG(partials);
  TORCH_CHECK(shard_elems > 0 && n_shards > 0 && n_valid >= 0 && n_valid <= shard_elems * n_shards, "bad shape");
  const size_t sb = fan::wire_shard_bytes((int)codec, shard_elems);
  TORCH_CHECK(shard_stride == 0 || (size_t)shard_stride >= sb, "shard_stride below the packed shard size");
  TORCH_CHECK(shard_stride % 16 == 0, "shard_stride must keep 16-byte alignment");
  const size_t need = shard_stride ? (size_t)shard_stride * (n_shards - 1) + sb : sb * n_shards;
  TORCH_CHECK((size_t)wire.numel() * wire.element_size() >= need, "wire buffer too small");
  const int64_t blocks = fan::sumsq_partials_for((size_t)shard_elems);
  TORCH_CHECK(partials.scalar_type() == at::kDouble && partials_base >= 0 &&
                  partials.numel() >= partials_base + blocks,
              "partials: f64[partials_base + ", blocks, "]");
  fan::launch_wire_sumsq((int)codec, wire.data_ptr(), (size_t)shard_elems, (int)n_shards, (int)skip_shard,
                         (int)skip_period, (size_t)n_valid, partials.data_ptr<double>() + partials_base, fan_stream(),
                         (size_t)shard_stride);
  return blocks;
}

// the coefficient of a clip group from its members' partial segments (tensor, first partial, count), in order
void clip_coef(const std::vector<at::Tensor>& partials, const std::vector<int64_t>& bases,
               const std::vector<int64_t>& counts, double max_norm, double grad_scale, at::Tensor& words) {
  FAN_T_CUDA_CONTIG(words);
  TORCH_CHECK(words.scalar_type() == at::kFloat && words.numel() >= 4, "words: f32[4]");
  const size_t n = partials.size();
  TORCH_CHECK(n <= (size_t)fan::kClipSegments && bases.size() == n && counts.size() == n, "clip_coef: at most ",
              fan::kClipSegments, " segments, one (partials, base, count) each");
  fan::ClipSegments seg{};
  for (size_t k = 0; k < n; ++k) {
    FAN_T_CUDA_CONTIG(partials[k]);
    TORCH_CHECK(partials[k].scalar_type() == at::kDouble && bases[k] >= 0 && counts[k] >= 0 &&
                    counts[k] <= (int64_t)INT32_MAX && partials[k].numel() >= bases[k] + counts[k],
                "clip_coef: segment ", k, ": f64[base + count]");
    seg.p[k] = partials[k].data_ptr<double>() + bases[k];
    seg.n[k] = (int)counts[k];
  }
  fan::launch_clip_coef(seg, (int)n, max_norm, (float)grad_scale, words.data_ptr<float>(), fan_stream());
}

void lamb_ratio(const at::Tensor& partials, int64_t n_pairs, double lr, at::Tensor& words) {
  FAN_T_CUDA_CONTIG(partials);
  FAN_T_CUDA_CONTIG(words);
  TORCH_CHECK(partials.scalar_type() == at::kDouble && n_pairs >= 0 && partials.numel() >= 2 * n_pairs,
              "partials: f64[2 * n_pairs]");
  TORCH_CHECK(words.scalar_type() == at::kFloat && words.numel() >= 3, "words: f32[3]");
  fan::launch_lamb_ratio(partials.data_ptr<double>(), (int)n_pairs, (float)lr, words.data_ptr<float>(), fan_stream());
}

void wire_lamb_apply(at::Tensor& master, const c10::optional<at::Tensor>& lp, const at::Tensor& mom,
                     const at::Tensor& var, const std::vector<double>& scalars, const at::Tensor& words,
                     int64_t shard_elems, int64_t skip_shard, int64_t skip_period, int64_t n_valid, int64_t n_adapt) {
  FAN_T_CUDA_CONTIG(words);
  TORCH_CHECK(words.scalar_type() == at::kFloat && words.numel() >= 3, "words: f32[3]");
  TORCH_CHECK(n_valid >= 0 && n_adapt >= 0 && n_adapt <= n_valid, "n_adapt must lie in [0, n_valid]");
  TORCH_CHECK(shard_elems > 0, "shard_elems");
  lamb_check_planes(master, mom, var, n_valid);
  fan::bf16_t* lpp = nullptr;
  if (lp) {
    FAN_T_CUDA_CONTIG((*lp));
    TORCH_CHECK(lp->scalar_type() == at::kBFloat16 && lp->numel() >= n_valid, "bad lp weights");
    lpp = reinterpret_cast<fan::bf16_t*>(lp->data_ptr());
  }
  const fan::LambParams p = fan_lamb_params(scalars, 1.0, var, n_valid);
  fan::launch_wire_lamb_apply(master.data_ptr<float>(), lpp, mom.data_ptr<float>(), p, words.data_ptr<float>(),
                              (size_t)shard_elems, (int)skip_shard, (int)skip_period, (size_t)n_valid, (size_t)n_adapt,
                              fan_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "fpga_ai_nic_amd native runtime: CDNA4 HIP kernels, BFP codec, ring planner, RCCL engine";
  m.attr("offload_arch") = "gfx950";
  m.def("wire_shard_bytes", [](int64_t codec, int64_t n_s) { return (int64_t)fan::wire_shard_bytes((int)codec, n_s); });
  m.def("wire_pack", &wire_pack, "encode dense f32/bf16 into the wire format (per shard)");
  m.def("wire_unpack", &wire_unpack, "decode wire format into dense f32/bf16");
  m.def("wire_pack_range", &wire_pack_range, "encode flat elements [begin, end) into the shard layout");
  m.def("wire_pack_to", &wire_pack_to, "encode shard s straight into dsts[s] (e.g. peers' receive slots)");
  m.def("p2p_release_mode", &fan::p2p_release_mode, "release form of peer-storing kernels: 1 block, 2 thread, 0 none");
  m.def("set_p2p_release_mode", &fan::set_p2p_release_mode);
  m.def("p2p_grid_cap", &fan::p2p_grid_cap, "workgroup cap of the peer-storing kernels");
  m.def("set_p2p_grid_cap", &fan::set_p2p_grid_cap);
  m.def("moment_grid_cap", &fan::moment_grid_cap, "workgroup cap of wire_adamw_q below the wire kernels' (0: none)");
  m.def("set_moment_grid_cap", &fan::set_moment_grid_cap);
  m.def("wire_reduce4", &fan::wire_reduce4, "owner reduce + SGD kernel: 4 values per lane (1) or 16 (0)");
  m.def("set_wire_reduce4", &fan::set_wire_reduce4);
  m.def("wire_reduce", &wire_reduce, "sum wire slots (+ dense local) -> wire and/or f32", pybind11::arg("slots"),
        pybind11::arg("n_slots"), pybind11::arg("self_pos"), pybind11::arg("local"), pybind11::arg("out_wire"),
        pybind11::arg("out_f32"), pybind11::arg("shard_elems"), pybind11::arg("codec"));
  m.def("wire_sgd", &wire_sgd, "fused decode + SGD weight update in place", pybind11::arg("wire"),
        pybind11::arg("shard_elems"), pybind11::arg("n_shards"), pybind11::arg("skip_shard"),
        pybind11::arg("skip_period"), pybind11::arg("master"), pybind11::arg("lp"), pybind11::arg("mom"),
        pybind11::arg("lr"), pybind11::arg("grad_scale"), pybind11::arg("weight_decay"), pybind11::arg("momentum"),
        pybind11::arg("nesterov"), pybind11::arg("n_valid"), pybind11::arg("codec"),
        pybind11::arg("clip") = pybind11::none());
  m.def("wire_adamw", &wire_adamw, "fused decode + AdamW weight update in place", pybind11::arg("wire"),
        pybind11::arg("shard_elems"), pybind11::arg("n_shards"), pybind11::arg("skip_shard"),
        pybind11::arg("skip_period"), pybind11::arg("master"), pybind11::arg("lp"), pybind11::arg("mom"),
        pybind11::arg("var"), pybind11::arg("scalars"), pybind11::arg("grad_scale"), pybind11::arg("weight_decay"),
        pybind11::arg("n_valid"), pybind11::arg("codec"), pybind11::arg("shard_stride") = 0,
        pybind11::arg("clip") = pybind11::none());
  m.def("sumsq_partials_for", [](int64_t n_s) { return (int64_t)fan::sumsq_partials_for((size_t)n_s); },
        "fp64 partials one wire_sumsq launch over shards of n_s elements writes");
  m.def("wire_sumsq", &wire_sumsq, "clip group norm pass: fp64 partial sums of squares of a gathered wire region",
        pybind11::arg("wire"), pybind11::arg("shard_elems"), pybind11::arg("n_shards"), pybind11::arg("skip_shard"),
        pybind11::arg("skip_period"), pybind11::arg("n_valid"), pybind11::arg("partials"),
        pybind11::arg("partials_base"), pybind11::arg("codec"), pybind11::arg("shard_stride") = 0);
  m.def("clip_coef", &clip_coef, "clip group coefficient -> words {coef, total, max_norm, nonfinite}",
        pybind11::arg("partials"), pybind11::arg("bases"), pybind11::arg("counts"), pybind11::arg("max_norm"),
        pybind11::arg("grad_scale"), pybind11::arg("words"));
  m.def("lamb_partials_for", [](int64_t n_s) { return (int64_t)fan::lamb_partials_for((size_t)n_s); },
        "{S_w, S_r} pairs one wire_lamb_moments launch over shards of n_s elements writes");
  m.def("wire_lamb_moments", &wire_lamb_moments,
        "trust-ratio pass 1: decode + new moments + fp64 norm partials; returns the pairs written", pybind11::arg("wire"),
        pybind11::arg("shard_elems"), pybind11::arg("n_shards"), pybind11::arg("skip_shard"),
        pybind11::arg("skip_period"), pybind11::arg("master"), pybind11::arg("mom"), pybind11::arg("var"),
        pybind11::arg("scalars"), pybind11::arg("grad_scale"), pybind11::arg("n_valid"), pybind11::arg("n_adapt"),
        pybind11::arg("partials"), pybind11::arg("partials_base"), pybind11::arg("codec"),
        pybind11::arg("shard_stride") = 0, pybind11::arg("clip") = pybind11::none());
  m.def("lamb_ratio", &lamb_ratio, "trust ratio of n_pairs norm partials -> words {lr * phi, lr, phi}",
        pybind11::arg("partials"), pybind11::arg("n_pairs"), pybind11::arg("lr"), pybind11::arg("words"));
  m.def("wire_lamb_apply", &wire_lamb_apply, "trust-ratio pass 2: the weight step from the stored moments",
        pybind11::arg("master"), pybind11::arg("lp"), pybind11::arg("mom"), pybind11::arg("var"),
        pybind11::arg("scalars"), pybind11::arg("words"), pybind11::arg("shard_elems"), pybind11::arg("skip_shard"),
        pybind11::arg("skip_period"), pybind11::arg("n_valid"), pybind11::arg("n_adapt"));
  fan::register_gemm(m);
  fan::register_nn(m);
  fan::register_planner(m);
  fan::register_engine(m);
}
