// Grouped GEMM launches.
// * Up to kGroupMax bwd-weight GEMMs of one configuration in one dispatch (gemm_groupn_kernel): a transformer layer's
//   four projections (bench/bert_overlap.py), each too small to fill the CUs without split-K slabs and a reduce
//   pass, fill them once together.
// * Up to kGroupMax bwd-weight GEMMs on 256x256 tiles at ONE common split-K count in one dispatch, and ONE reduce over
//   every problem's slabs (launch_gemm_wgrad_splitk_group): the MLP's two narrow layers (1024x4096 and 4096x1024
//   outputs, 64 tiles each) need a 4-way split to fill the CUs alone and a 2-way split together — half the slab
//   bytes, one prologue / epilogue and one reduce launch instead of two.
#include "gemm/gemm_bf16_launch.h"
#include "gemm/gemm_group.h"

namespace fan {

using namespace gemm_detail;

namespace {

template <typename TC>
PlProblem<TC> problem_of(const GemmArgs& a, const WireOut& wo) {
  return PlProblem<TC>{(const bf16_t*)a.A, a.lda, (const bf16_t*)a.B, a.ldb, (TC*)a.C, a.ldc, (const bf16_t*)a.bias,
                       (const TC*)a.aux, a.ldaux, a.M, a.N, a.K, 1, (float*)a.workspace, a.colsum, wo};
}

// WireOut of one problem, as launch_typed builds it (the bias segment right after C in the flat bucket)
WireOut wire_of(const GemmArgs& a) {
  WireOut wo{};
  wo.prio = gemm_prio_flag().load(std::memory_order_relaxed);
  if (a.wire) {
    wo.p = a.wire;
    wo.shard = a.wire_shard;
    wo.own = a.wire_own;
    wo.period = a.wire_period;
    wo.codec = a.wire_codec;
    wo.inv_shard = a.wire_shard > 0 ? 1.0f / (float)a.wire_shard : 0.f;
    wo.bias_off = a.colsum ? (int)(a.wire_off + (int64_t)a.M * a.ldc) : 0;
    wo.off = (uint32_t)a.wire_off;
  }
  return wo;
}

template <int EPI>
void launch_wgrad_group(const GemmArgs* a, int n, hipStream_t s) {
  using P = PlCfg<false, false, EPI, float, false, false, true, 128, 256>;
  PlGroup<float> g{};
  ColsumGroup cg{};
  g.n = cg.n = n;
  int wg = 0, cb = 0;
  for (int i = 0; i < n; ++i) {
    const WireOut wo = wire_of(a[i]);
    g.p[i] = problem_of<float>(a[i], wo);
    g.first[i] = wg;
    const int tiles = (a[i].M / 256) * (a[i].N / 128);
    wg += (tiles + kNumXCD - 1) / kNumXCD * kNumXCD;
    cg.part[i] = (const float*)a[i].workspace;
    cg.parts[i] = a[i].M / 256;
    cg.colsum[i] = a[i].colsum;
    cg.wo[i] = wo;
    cg.N[i] = a[i].N;
    cg.first[i] = cb;
    cb += (a[i].N + 63) / 64;
  }
  g.first[n] = wg;
  cg.first[n] = cb;
  auto k = gemm_groupn_kernel<P>;
  FAN_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, P::kLds));
  hipLaunchKernelGGL(k, wg, 256, P::kLds, s, g);
  FAN_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL((colsum_reduce_group_kernel<is_wire_epi(EPI)>), cb, 256, 0, s, cg);
  FAN_HIP_CHECK(hipGetLastError());
}

// WireOut of one split-K problem, as launch_typed builds it (with the fused update's planes)
WireOut wire_upd_of(const GemmArgs& a) {
  WireOut wo = wire_of(a);
  wo.um = a.upd_master;
  wo.ulp = a.upd_lp;
  wo.umom = a.upd_mom;
  wo.up = a.upd;
  return wo;
}

// blocks of problem a's slab reduce (as the single launch's grid)
int slab_reduce_blocks(const GemmArgs& a) { return stream_grid((size_t)a.M * a.N / 4); }

template <int SK>
void launch_wgrad_splitk_group(const GemmArgs* a, int n, hipStream_t s) {
  // the single launch's main loop at a split plan (launch_main: gemm_pl4_kernel SPLIT + COLSUM; it only writes slabs)
  using P = PlCfg<false, false, kEpiWire, float, false, true, true, 256, 256>;
  PlGroup<float> g{};
  SlabGroup sg{};
  g.n = sg.n = n;
  int wg = 0, rb = 0;
  for (int i = 0; i < n; ++i) {
    const WireOut wo = wire_upd_of(a[i]);
    g.p[i] = problem_of<float>(a[i], wo);
    g.p[i].split_k = SK;
    g.first[i] = wg;
    const int units = (a[i].M / 256) * (a[i].N / 256) * SK;
    wg += (units + kNumXCD - 1) / kNumXCD * kNumXCD;
    sg.ws[i] = (const float*)a[i].workspace;
    sg.C[i] = (float*)a[i].C;
    sg.colsum[i] = a[i].colsum;
    sg.ldc[i] = a[i].ldc;
    sg.wo[i] = wo;
    sg.M[i] = a[i].M;
    sg.N[i] = a[i].N;
    sg.first[i] = rb;
    rb += slab_reduce_blocks(a[i]);
  }
  g.first[n] = wg;
  sg.first[n] = rb;
  auto k = gemm_groupn_kernel<P>;
  FAN_HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, P::kLds));
  hipLaunchKernelGGL(k, wg, 256, P::kLds, s, g);
  FAN_HIP_CHECK(hipGetLastError());
  // one reduce for every problem's slabs; the stream's queued bias-gradient reduces ride in its first blocks
  const bool upd = a[0].upd_master != nullptr;
  const ColsumGroup q = take_pending_colsum(s);
  const int qb = q.n > 0 ? q.first[q.n] : 0;
  auto reduce = [&](auto kr) { hipLaunchKernelGGL(kr, qb + rb, 256, 0, s, sg, q); };
  if (upd && q.n > 0) reduce(splitk_reduce_wire4_group_kernel<true, SK, true>);
  else if (upd) reduce(splitk_reduce_wire4_group_kernel<true, SK, false>);
  else if (q.n > 0) reduce(splitk_reduce_wire4_group_kernel<false, SK, true>);
  else reduce(splitk_reduce_wire4_group_kernel<false, SK, false>);
  FAN_HIP_CHECK(hipGetLastError());
}

}  // namespace

int64_t gemm_wgrad_splitk_group_ws(const GemmArgs& a, int split) { return (int64_t)split * ((int64_t)a.M * a.N + a.N); }

bool gemm_wgrad_splitk_group_supported(const GemmArgs* a, int n, int split) {
  if (n < 1 || n > kGroupMax || (split != 2 && split != 4)) return false;
  int64_t wg = 0;
  for (int i = 0; i < n; ++i) {
    const GemmArgs& g = a[i];
    if (g.a_kcontig || g.b_kcontig || g.c_bf16 || g.accumulate || !g.colsum || !g.workspace) return false;
    if (g.epilogue != kEpiWire || !g.wire || g.defer_colsum || g.defer_reduce) return false;
    if (g.M <= 0 || g.N <= 0 || g.M % 256 || g.N % 256 || g.K <= 0 || g.K % (64 * split) || g.ldc < g.N) return false;
    if (g.lda % 8 || g.ldb % 8 || g.ldc % 16) return false;
    if ((((uintptr_t)g.A | (uintptr_t)g.B | (uintptr_t)g.C | (uintptr_t)g.colsum | (uintptr_t)g.workspace) & 15))
      return false;
    if (g.wire_shard <= 0 || g.wire_shard % 256 || g.wire_off < 0 || g.wire_off % 16) return false;
    if (g.wire_codec != kBfpTrunc && g.wire_codec != kBfpRne) return false;
    if (g.wire_off + (int64_t)g.M * g.ldc + g.N >= (1ll << 31)) return false;
    // the fused update: every problem or none (one reduce kernel), rne codec, no owner shard (as the single launch)
    if ((g.upd_master != nullptr) != (a[0].upd_master != nullptr)) return false;
    if (g.upd_master && (g.wire_codec != kBfpRne || g.wire_own != -1)) return false;
    if (!g.upd_master && (g.upd_lp || g.upd_mom)) return false;
    wg += ((int64_t)(g.M / 256) * (g.N / 256) * split + kNumXCD - 1) / kNumXCD * kNumXCD;
  }
  return wg <= 64 * kNumCU;
}

void launch_gemm_wgrad_splitk_group(const GemmArgs* a, int n, int split, hipStream_t s) {
  FAN_CHECK(gemm_wgrad_splitk_group_supported(a, n, split),
            "gemm_wgrad_splitk_group: unsupported shapes / layouts / wire or update fields");
  if (split == 2) launch_wgrad_splitk_group<2>(a, n, s);
  else launch_wgrad_splitk_group<4>(a, n, s);
}

int64_t gemm_wgrad_group_ws(const GemmArgs& a) { return (int64_t)(a.M / 256) * a.N; }

bool gemm_wgrad_group_supported(const GemmArgs* a, int n) {
  static_assert(kGroupMax == kMaxGroup, "group capacity");
  if (n < 1 || n > kGroupMax) return false;
  int64_t wg = 0;
  for (int i = 0; i < n; ++i) {
    const GemmArgs& g = a[i];
    if (g.a_kcontig || g.b_kcontig || g.c_bf16 || g.accumulate || !g.colsum || !g.workspace) return false;
    if (g.epilogue != a[0].epilogue || (g.epilogue != kEpiNone && g.epilogue != kEpiWire)) return false;
    if (g.M <= 0 || g.N <= 0 || g.M % 256 || g.N % 128 || g.K <= 0 || g.K % 64 || g.ldc < g.N) return false;
    if (g.lda % 8 || g.ldb % 8 || g.ldc % 4 || ((uintptr_t)g.C & 15) || ((uintptr_t)g.colsum & 15)) return false;
    if (g.epilogue == kEpiWire) {
      if (!g.wire || g.wire_shard <= 0 || g.wire_shard % 256 || g.wire_off < 0 || g.wire_off % 16 || g.upd_master)
        return false;
      if (g.wire_off + (int64_t)g.M * g.ldc + g.N >= (1ll << 31)) return false;
    }
    wg += ((int64_t)(g.M / 256) * (g.N / 128) + kNumXCD - 1) / kNumXCD * kNumXCD;
  }
  return wg <= 64 * kNumCU;
}

void launch_gemm_wgrad_group(const GemmArgs* a, int n, hipStream_t s) {
  FAN_CHECK(gemm_wgrad_group_supported(a, n), "gemm_wgrad_group: unsupported shapes / layouts / epilogues");
  if (a[0].epilogue == kEpiWire) launch_wgrad_group<kEpiWire>(a, n, s);
  else launch_wgrad_group<kEpiNone>(a, n, s);
}

}  // namespace fan
