// Native compressed all-reduce engine. See engine.h.
#include "comm/engine.h"

#include <chrono>
#include <cstdlib>

#include "comm/p2p_comm.h"
#include "common/roctx.h"
#include "gemm/gemm.h"
#include <functional>
#include <sstream>
#include <thread>

namespace fan {

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int64_t round_up(int64_t a, int64_t b) { return cdiv(a, b) * b; }
static size_t esize(int dtype) { return dtype == kF32 ? 4 : 2; }
// elements of [off, off + len) that lie inside the bucket's n_valid
static int64_t valid_in(int64_t n_valid, int64_t off, int64_t len) {
  return std::max<int64_t>(0, std::min<int64_t>(n_valid - off, len));
}
// the gradient buffer already is the wire format: nothing to pack
static bool zero_copy(int codec, int gdt) {
  return (codec == kRawF32 && gdt == kF32) || (codec == kRawBf16 && gdt == kBF16);
}

AllReduceEngine::AllReduceEngine(Comm* comm, int rank, int world, EngineConfig cfg, int device)
    : comm_(comm), rank_(rank), world_(world), device_(device), cfg_(cfg) {
  FAN_CHECK(world >= 1 && rank >= 0 && rank < world, "bad rank/world");
  FAN_CHECK(world == 1 || comm != nullptr, "world > 1 needs a communicator");
  FAN_HIP_CHECK(hipSetDevice(device));
  orders_ = cfg.algo == 1 ? ring_orders(world, cfg.rings, cfg.links.empty() ? nullptr : &cfg.links)
                          : std::vector<std::vector<int>>{{}};
  if (cfg.algo != 1) {
    orders_[0].resize(world);
    for (int i = 0; i < world; ++i) orders_[0][i] = i;
  }
  inline_ = world == 1 && !cfg.force_comm;
  if (cfg_.shard_update < 0) {
    const char* su = std::getenv("FAN_SHARD_UPDATE");
    cfg_.shard_update = su && su[0] == '1' ? 1 : 0;
  }
  shard_upd_ = cfg_.shard_update > 0 && cfg.algo == 0 && !inline_ && !cfg.compat_owner_fp32;
  bool side_epi = false;
  if (inline_) {
    const char* se = std::getenv("FAN_SIDE_EPI");
    side_epi = cfg.side_epilogue >= 0 ? cfg.side_epilogue > 0 : (se && se[0] == '1');
    if (side_epi) FAN_HIP_CHECK(hipStreamCreateWithPriority(&epi_stream_, hipStreamNonBlocking, 0));
  }
  if (cfg_.ring_sub <= 0) {
    const char* rs = std::getenv("FAN_RING_SUB");
    cfg_.ring_sub = rs ? std::max(1, std::atoi(rs)) : 1;
  }
  if (cfg_.chunk_elems <= 0) {
    const char* ce = std::getenv("FAN_CHUNK_ELEMS");
    cfg_.chunk_elems = ce ? std::atoll(ce) : (int64_t(1) << 26);
  }
  FAN_CHECK(cfg_.chunk_elems >= 256, "chunk_elems must be >= 256");
  FAN_HIP_CHECK(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, cfg.stream_priority));
  FAN_HIP_CHECK(hipStreamCreateWithPriority(&aux_stream_, hipStreamNonBlocking, cfg.stream_priority));
  for (auto& row : cev_)
    for (auto& e : row) FAN_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  void* h = nullptr;
  FAN_HIP_CHECK(hipHostMalloc(&h, kSlots * 64, hipHostMallocMapped));
  std::memset(h, 0, kSlots * 64);
  flags_host_ = reinterpret_cast<volatile uint32_t*>(h);
  void* d = nullptr;
  FAN_HIP_CHECK(hipHostGetDevicePointer(&d, h, 0));
  flags_dev_ = reinterpret_cast<uint32_t*>(d);
  // Cross-stream events order kernels of this device's own streams, so a device-scope release (every XCD's L2
  // written back for the other streams' kernels) is enough; what leaves the device is released by its own path
  // (RCCL's kernels, the P2P transport's system-scope round event). Device scope measured 1 % faster on the forced
  // multi-rank path (1.151-1.153 vs 1.160-1.176 ms/step, same box, profiles/r3_event_fence_ab.txt).
  // FAN_EVENT_FENCE=system|default: system-scope release / HIP's default marker.
  unsigned evf = hipEventDisableTiming | hipEventReleaseToDevice;
  if (const char* f = std::getenv("FAN_EVENT_FENCE")) {
    if (!std::strcmp(f, "system")) evf = hipEventDisableTiming | hipEventReleaseToSystem;
    else if (!std::strcmp(f, "default")) evf = hipEventDisableTiming;
  }
  bool lazy_done = true;
  if (const char* ld = std::getenv("FAN_LAZY_DONE")) lazy_done = ld[0] != '0';
  bool elide_waits = true;  // FAN_ELIDE_WAITS=0: issue every cross-stream wait (A/B of the slot table's skip)
  if (const char* ew = std::getenv("FAN_ELIDE_WAITS")) elide_waits = ew[0] != '0';
  bool done_words = false;  // FAN_DONE_WORDS=1: comm-stream requests also write their host-mapped done word
  if (const char* dw = std::getenv("FAN_DONE_WORDS")) done_words = dw[0] != '0';
  const char* ve = std::getenv("FAN_VERIFY");
  verify_ = cfg.verify >= 0 ? cfg.verify > 0 : (ve && ve[0] == '1');
  if (verify_) {
    FAN_HIP_CHECK(hipMalloc(&tags_, (size_t)5 * kTagRows * 16));
    FAN_HIP_CHECK(hipMalloc(&verr_dev_, sizeof(VerifyError)));
    FAN_HIP_CHECK(hipMemset(verr_dev_, 0, sizeof(VerifyError)));
    FAN_HIP_CHECK(hipHostMalloc(&verr_host_, sizeof(VerifyError), hipHostMallocDefault));
    std::memset(verr_host_, 0, sizeof(VerifyError));
  }
  // request-slot state machine (slot_table.h): per slot the ready / update / comm_done / done events
  slot_events_.resize((size_t)kSlots * 4);
  for (auto& e : slot_events_) FAN_HIP_CHECK(hipEventCreateWithFlags(&e, evf));
  for (auto& x : extra_) {
    FAN_HIP_CHECK(hipEventCreate(&x.t0));
    FAN_HIP_CHECK(hipEventCreate(&x.t1));
  }
  dev_.host_words = flags_host_;
  dev_.dev_words = flags_dev_;
  SlotTable<HipSlotDevice>::Config tc;
  tc.inline_mode = inline_;
  tc.side_epi = side_epi;
  tc.lazy_done = lazy_done;
  tc.elide_waits = elide_waits;
  tc.done_words = done_words;
  tc.comm = stream_;
  tc.side = epi_stream_;
  table_ = std::make_unique<SlotTable<HipSlotDevice>>(dev_, tc, slot_events_);
  table_->on_forced_commit = [this](int) { counters_.forced_commits++; };
  table_->on_epilogue = [this](int slot, hipStream_t es) {  // the epilogue's end: timing / trace points
    const SlotExtra& x = extra_[slot];
    if (x.timed) FAN_HIP_CHECK(hipEventRecord(x.t1, es));
    if (x.trace >= 0) FAN_HIP_CHECK(hipEventRecord(trace_pool_[x.trace].ev[kTpEpiEnd], es));
  };
}

AllReduceEngine::~AllReduceEngine() {
  hipStreamSynchronize(stream_);
  hipStreamSynchronize(aux_stream_);
  for (auto& row : cev_)
    for (auto& e : row) hipEventDestroy(e);
  // epilogues may have run on a producer stream and still read the scratch
  table_->for_each_used([](int, const SlotTable<HipSlotDevice>::Slot& sl) { hipEventSynchronize(sl.done); });
  for (auto& e : slot_events_) hipEventDestroy(e);
  for (auto& x : extra_) {
    hipEventDestroy(x.t0);
    hipEventDestroy(x.t1);
  }
  for (auto& t : trace_pool_)
    for (auto& e : t.ev) hipEventDestroy(e);
  for (auto& e : hop_pool_) hipEventDestroy(e);
  for (auto& kv : scratch_) hipFree(kv.second.first);
  for (auto& kv : gall_)
    if (kv.second.free) hipEventDestroy(kv.second.free);
  if (flags_host_) hipHostFree((void*)flags_host_);
  if (tags_) hipFree(tags_);
  if (verr_dev_) hipFree(verr_dev_);
  if (verr_host_) hipHostFree(verr_host_);
  hipStreamDestroy(aux_stream_);
  if (epi_stream_) hipStreamDestroy(epi_stream_);
  hipStreamDestroy(stream_);
}

EngineLayout AllReduceEngine::layout(int64_t n, int64_t shard, int64_t chunks) const {
  EngineLayout L;
  L.n = n;
  L.algo = cfg_.algo;
  const int N = world_;
  if (shard > 0 || chunks > 0) {
    FAN_CHECK(cfg_.algo == 0, "explicit shard / chunk layouts are a mesh feature");
    FAN_CHECK(shard > 0 && shard % 256 == 0 && chunks >= 1, "explicit layout: shard % 256 == 0 and chunks >= 1");
    FAN_CHECK(shard * N * chunks >= n, "explicit layout smaller than the bucket");
    if (P2PComm* d = comm_ ? comm_->direct() : nullptr)
      FAN_CHECK(wire_shard_bytes(cfg_.codec, (size_t)shard) <= d->payload_bytes(), "explicit shard exceeds the p2p slot");
    L.shard = shard;
    L.chunks = chunks;
    L.n_pad = shard * N * chunks;
    return L;
  }
  if (cfg_.algo == 0) {
    // buckets above chunk_elems stream through the collectives in balanced chunks of N shards (multi-rank path
    // only: the inline world-1 engine has no collectives to pipeline)
    const bool local = N == 1 && !cfg_.force_comm;
    int64_t chunk = cfg_.chunk_elems;
    if (P2PComm* d = comm_ ? comm_->direct() : nullptr) {
      // a P2P message (one wire shard) must fit one arena slot: chunk the bucket so that it does
      // (sharded update: round 2 carries 2 B per element of bf16 weights)
      const size_t per256 = std::max<size_t>(wire_shard_bytes(cfg_.codec, 256), shard_upd_ ? 512 : 0);
      const int64_t max_shard = (int64_t)(d->payload_bytes() / per256) * 256;
      FAN_CHECK(max_shard >= 256, "p2p arena slot smaller than one 256-element wire shard");
      chunk = std::min<int64_t>(chunk, max_shard * N);
    }
    L.chunks = local ? 1 : std::max<int64_t>(1, cdiv(n, chunk));
    L.shard = round_up(std::max<int64_t>(cdiv(n, N * L.chunks), 1), 256);
    L.n_pad = L.shard * N * L.chunks;
    return L;
  }
  const int R = (int)orders_.size();
  const int64_t chunk = cdiv(std::max<int64_t>(n, 1), R);
  L.sub = ring_sub();
  int64_t max_slice = cfg_.max_slice_elems;
  if (P2PComm* d = comm_ ? comm_->direct() : nullptr) {
    // two (sub-)slice messages per peer and round must fit one arena slot (run_ring_direct): halve the slice cap
    // until they do (the arena slot is clamped by the IPC size cap, p2p_comm.h)
    const int64_t gran = 256 * (int64_t)L.sub;
    auto fits = [&](int64_t s) { return 2 * round_up((int64_t)wire_shard_bytes(cfg_.codec, s / L.sub), 256) <=
                                        (int64_t)d->payload_bytes(); };
    while (max_slice > gran && !fits(max_slice)) max_slice = std::max<int64_t>(gran, max_slice / 2 / gran * gran);
  }
  const RingGeometry g = ring_geometry(chunk, N, max_slice, 256 * (int64_t)L.sub);
  L.rings = R;
  L.slice = g.slice_elems;
  L.blocks = g.blocks;
  L.part = g.n_pad;
  L.n_pad = g.n_pad * R;
  return L;
}

int AllReduceEngine::ring_sub() const {
  P2PComm* d = comm_ ? comm_->direct() : nullptr;
  if (cfg_.algo != 1 || d == nullptr || world_ < 2 || cfg_.compat_owner_fp32) return 1;
  return std::max(1, std::min(cfg_.ring_sub, d->depth() - 1));
}

int64_t AllReduceEngine::wire_bytes(const EngineLayout& L) const {
  const int N = world_;
  if (N == 1) return 0;
  if (L.algo == 0) return 2 * (N - 1) * L.chunks * (int64_t)wire_shard_bytes(cfg_.codec, L.shard);
  return (int64_t)L.rings * L.blocks * 2 * (N - 1) * (int64_t)wire_shard_bytes(cfg_.codec, L.slice);
}

uint8_t* AllReduceEngine::scratch(const std::string& key, size_t bytes, hipStream_t st) {
  auto it = scratch_.find(key);
  if (it != scratch_.end() && it->second.second >= bytes) return it->second.first;
  if (it != scratch_.end()) {
    FAN_HIP_CHECK(hipDeviceSynchronize());  // rare (bucket grew): the old buffer may still be in flight
    hipFree(it->second.first);
  }
  void* p = nullptr;
  FAN_HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 256)));
  FAN_HIP_CHECK(hipMemsetAsync(p, 0, std::max<size_t>(bytes, 256), st));
  scratch_[key] = {reinterpret_cast<uint8_t*>(p), bytes};
  return reinterpret_cast<uint8_t*>(p);
}

uint8_t* AllReduceEngine::epi_scratch(const std::string& base, size_t bytes) {
  // one buffer per request slot; for ordinary buckets all kSlots are allocated on a key's first use, so the slot
  // rotation never allocates later (inside a timed loop); buckets above 64 MB allocate per slot on first use
  // (8 copies of a multi-GB gathered wire would be pure waste for a request stream that rarely defers them)
  const std::string key = base + "_s" + std::to_string(cur_.slot);
  if (scratch_.find(key) == scratch_.end() && bytes <= (size_t(64) << 20))
    for (int s = 0; s < kSlots; ++s) scratch(base + "_s" + std::to_string(s), bytes, cur_.run);
  return scratch(key, bytes, cur_.run);
}

// The decode + update launch of a request's optimizer over `nv` elements of its planes, `off` elements into the bucket.
static void update_at(const EngineRequest& req, int codec, const void* wire, size_t n_s, int n_shards, int skip_shard,
                      int skip_period, int64_t off, size_t nv, hipStream_t st, size_t shard_stride = 0) {
  bf16_t* lp = req.lp ? req.lp + off : nullptr;
  FAN_CHECK(!req.upd.trust, "a trust-ratio update is the two-pass epilogue (lamb_region), never a single launch");
  if (req.moment_q) {
    // the 8-bit planes are passed whole: the region's bucket offset addresses them (and keys the random bytes)
    launch_wire_adamw_q(codec, wire, n_s, n_shards, skip_shard, skip_period, req.master + off, lp, req.mom_q, req.var_q,
                        req.moment_elems, (size_t)off, req.upd.adamw, req.moment_seed, nv, st, shard_stride,
                        req.clip_words);
  } else if (req.upd.kind == kOptAdamW) {
    AdamWParams a = req.upd.adamw;
    a.var += off;
    launch_wire_adamw(codec, wire, n_s, n_shards, skip_shard, skip_period, req.master + off, lp, req.mom + off, a, nv,
                      st, shard_stride, req.clip_words);
  } else if (req.upd.kind == kOptLion) {
    launch_wire_lion(codec, wire, n_s, n_shards, skip_shard, skip_period, req.master + off, lp, req.mom + off,
                     req.upd.lion, nv, st, shard_stride, req.clip_words);
  } else {
    launch_wire_sgd(codec, wire, n_s, n_shards, skip_shard, skip_period, req.master + off, lp,
                    req.mom ? req.mom + off : nullptr, req.upd.sgd, nv, st, shard_stride, req.clip_words);
  }
}

// The sharded update's owner reduce + update of the shard that starts `off` elements into the bucket.
static void reduce_update_at(const EngineRequest& req, int codec, const void* slots, size_t slot_stride, int n_slots,
                             int self_pos, const void* local, int64_t off, size_t nv, const WirePtrs& dst, int n_dst,
                             size_t n_s, bool peers, hipStream_t st) {
  if (req.upd.kind == kOptAdamW) {
    AdamWParams a = req.upd.adamw;
    a.var += off;
    launch_wire_reduce_adamw(codec, req.grad_dtype, slots, slot_stride, n_slots, self_pos, local, req.master + off,
                             req.mom + off, a, nv, dst, n_dst, n_s, peers, st);
  } else if (req.upd.kind == kOptLion) {
    launch_wire_reduce_lion(codec, req.grad_dtype, slots, slot_stride, n_slots, self_pos, local, req.master + off,
                            req.mom + off, req.upd.lion, nv, dst, n_dst, n_s, peers, st);
  } else {
    launch_wire_reduce_sgd(codec, req.grad_dtype, slots, slot_stride, n_slots, self_pos, local, req.master + off,
                           req.mom ? req.mom + off : nullptr, req.upd.sgd, nv, dst, n_dst, n_s, peers, st);
  }
}

// Epilogue over a gathered wire region: fused decode + update (and/or decoded sum output).
static void epilogue(const EngineRequest& req, int codec, hipStream_t st, const uint8_t* G, int64_t shard, int n_shards,
                     int64_t off, int64_t len, int skip_shard = -1, int skip_period = 0) {
  const int64_t nv = valid_in(req.n_valid, off, len);
  if (req.update && nv > 0)
    update_at(req, codec, G, (size_t)shard, n_shards, skip_shard, skip_period, off, (size_t)nv, st);
  if (req.out_sum) launch_wire_unpack(codec, kF32, G, req.out_sum + off, (size_t)shard, n_shards, st);
}

// The request's LambParams with the second-moment plane `off` elements into the bucket.
static LambParams lamb_at(const EngineRequest& req, int64_t off) {
  LambParams p = req.upd.lamb;
  p.var = req.upd.adamw.var + off;
  return p;
}

EpiThunk AllReduceEngine::lamb_region(const EngineRequest& req, const uint8_t* wire, int64_t shard_elems, int n_shards,
                                      int64_t off, int64_t nv, int skip_shard, int skip_period, size_t shard_stride) {
  const int c = cfg_.codec;
  // flat offsets: the adapted tensor ends n_adapt - off elements into this region (clamped, as valid_in does n_valid)
  const int64_t n_adapt = req.n_adapt < 0 ? req.n_valid : req.n_adapt;
  const size_t adapt_end = (size_t)std::min(std::max<int64_t>(n_adapt - off, 0), nv);
  const int pairs = lamb_partials_for((size_t)shard_elems);
  FAN_CHECK(cur_.partials != nullptr && cur_.pairs + pairs <= cur_.pairs_cap,
            "trust ratio: more update regions than the request's partials buffer holds");
  double* part = cur_.partials + 2 * (size_t)cur_.pairs;
  cur_.pairs += pairs;
  const float* words = cur_.words;
  const LambParams p = lamb_at(req, off);
  float* master = req.master + off;
  float* mom = req.mom + off;
  bf16_t* lp = req.lp ? req.lp + off : nullptr;
  const float* clip = req.clip_words;  // pass 1 takes the clipped gradient; the ratio and pass 2 are as ever
  cur_.apply.push_back([=](hipStream_t es) {
    launch_wire_lamb_apply(master, lp, mom, p, words, (size_t)shard_elems, skip_shard, skip_period, (size_t)nv,
                           adapt_end, es);
  });
  return [=](hipStream_t es) {
    launch_wire_lamb_moments(c, wire, (size_t)shard_elems, n_shards, skip_shard, skip_period, master, mom, p,
                             (size_t)nv, adapt_end, part, es, shard_stride, clip);
  };
}

EpiThunk AllReduceEngine::make_epilogue(const EngineRequest& req, const uint8_t* wire, int64_t shard_elems,
                                        int n_shards, int64_t off, int64_t len, int skip_shard, int skip_period) {
  const int c = cfg_.codec;
  const int64_t nv = valid_in(req.n_valid, off, len);
  if (req.clip_words && nv > 0) {
    // the norm pass of this region, now: the gathered wire is complete in the order of cur_.run at every call site
    // (a clipped request is deferred, so the direct mesh has copied it out of the arena), and the launch runs beside
    // the backward's remaining GEMMs; only the group's coefficient launch waits for the end of the backward
    const int blocks = sumsq_partials_for((size_t)shard_elems);
    FAN_CHECK(cur_.clip_partials != nullptr && cur_.clip_count + blocks <= cur_.clip_cap,
              "clip: more update regions than the request's partials buffer holds");
    launch_wire_sumsq(c, wire, (size_t)shard_elems, n_shards, skip_shard, skip_period, (size_t)nv,
                      cur_.clip_partials + cur_.clip_count, cur_.run);
    cur_.clip_count += blocks;
  }
  if (trust(req) && nv > 0) {
    const EpiThunk pass1 = lamb_region(req, wire, shard_elems, n_shards, off, nv, skip_shard, skip_period);
    float* out_sum = req.out_sum;
    return [=](hipStream_t es) {
      pass1(es);
      if (out_sum) launch_wire_unpack(c, kF32, wire, out_sum + off, (size_t)shard_elems, n_shards, es);
    };
  }
  return [=](hipStream_t es) { epilogue(req, c, es, wire, shard_elems, n_shards, off, len, skip_shard, skip_period); };
}

std::array<int64_t, 3> AllReduceEngine::prepack_shape(int64_t n) const {
  if (cfg_.codec != kBfpTrunc && cfg_.codec != kBfpRne) return {0, 0, -1};
  const EngineLayout L = layout(n);
  const bool local = (world_ == 1 && !cfg_.force_comm) || comm_ == nullptr;
  if (cfg_.algo == 1)  // ring: one shard per slice (P sub-shards when the hops stream), ring-major; every local slice
                       // is also needed in f32 (each reduce hop adds the local contribution), except at world 1 where
                       // the encoding is the result
    return {L.slice / L.sub, (int64_t)L.rings * L.blocks * world_ * L.sub, world_ == 1 ? -1 : kWireOwnAll};
  // chunked buckets: the owner shard of chunk c is wire shard c*N + rank (owner = shard index mod N)
  return {L.shard, world_ * L.chunks, local ? -1 : rank_};
}

// The request's encoder (bfp_format.h WireEncoder) at stage 0, sender `rank`'s pack of the whole bucket, or stage 1,
// owner `rank`'s re-encode of its shard of `shard` elements: the stage's part of the residual plane, or the stochastic
// key (sr_seed, rank, stage) with the stage's first element index in the padded bucket.
static WireEncoder encoder_of(const EngineRequest& req, int rank, int stage, int64_t shard) {
  const size_t first = stage ? (size_t)rank * (size_t)shard : 0;
  if (req.residual) return WireEncoder::feedback(req.residual + first);
  if (req.sr) return WireEncoder::stochastic(sr_key(req.sr_seed, rank, stage), first);
  return {};
}

std::vector<EpiThunk> AllReduceEngine::run_mesh(const EngineLayout& L, const EngineRequest& req) {
  const int N = world_, r = rank_, c = cfg_.codec, gdt = req.grad_dtype;
  const int64_t s = L.shard;
  const size_t sb = wire_shard_bytes(c, s);
  const uint8_t* g = reinterpret_cast<const uint8_t*>(req.grad);
  hipStream_t st = cur_.run;
  // Error feedback: req.residual (submit(): mesh, a BFP codec, no prepacked input, one chunk, not sharded) is read and
  // written only by the kernels launched here and in run_mesh_direct, all on `st`, the stream of this request's
  // communication phase; the sender stage writes every shard of the plane but r, the owner stage shard r. Why step
  // t + 1's pack sees step t's owner-stage store: both run on the comm stream, in its order — or one of them on the
  // producer stream (an on_producer request, a backward's last), and SlotTable::begin orders the two streams in both
  // directions: a comm-stream request waits for `ready`, recorded on the producer stream after everything enqueued
  // there, the previous step's on-producer communication phase included; an on-producer request makes the producer
  // stream wait for everything on the comm stream so far. Inline engines run every request in the producer stream's
  // order. A caller that moves a bucket between producer streams orders them itself, as for the gradient buffer.
  // Stochastic rounding: req.sr (submit(): an rne BFP codec, mesh, no prepacked input, one chunk, not sharded, no
  // residual) swaps the same two encoders for their stateless stochastic forms (encoder_of). With neither, the copying
  // paths below keep the contiguous pack and the plain reduce.
  const bool enc = req.residual != nullptr || req.sr;
  if (req.prepacked) {  // encode what the producer did not (bias gradient + padding)
    launch_wire_pack_range(c, gdt, req.grad, const_cast<uint8_t*>(req.prepacked), (size_t)s,
                           (size_t)req.prepacked_elems, (size_t)L.n_pad, st);
  }
  if ((N == 1 && !cfg_.force_comm) || comm_ == nullptr) {
    // the producer's encoding IS the (single-rank) result: no reduce pass
    if (req.prepacked) return {make_epilogue(req, req.prepacked, s, 1, 0, s)};
    uint8_t* S = epi_scratch("mesh_S" + std::to_string(sb), sb);
    if (enc)  // one rank: the owner stage alone
      launch_wire_reduce_to(c, gdt, S, sb, 1, 0, g, WirePtrs{{S}}, 1, (size_t)s, encoder_of(req, 0, 1, s), false, st);
    else launch_wire_reduce(c, gdt, S, sb, 1, 0, g, S, nullptr, (size_t)s, st);
    return {make_epilogue(req, S, s, 1, 0, s)};
  }
  if (L.chunks > 1) return run_mesh_chunked(L, req);
  if (P2PComm* d = comm_->direct(); d && N <= kMaxPeers) return run_mesh_direct(d, L, req);
  uint8_t* S = scratch("mesh_S" + std::to_string(sb), sb, st);
  const uint8_t* P = req.prepacked ? req.prepacked : g;
  if (!zero_copy(c, gdt) && !req.prepacked) {
    RoctxRange rr("fan/mesh/pack");
    uint8_t* Pb = scratch("mesh_P" + std::to_string(sb * N), sb * N, st);
    if (enc) {
      // (shard r's row is the plain encoding of g, as without feedback or stochastic rounding: the owner reduce reads
      // g itself)
      WirePtrs to{};
      for (int q = 0; q < N; ++q) to.p[q] = Pb + (size_t)q * sb;
      launch_wire_pack_to(c, gdt, g, to, (size_t)s, N, r, encoder_of(req, r, 0, s), false, st);
    } else {
      launch_wire_pack(c, gdt, g, Pb, (size_t)s, N, st);
    }
    P = Pb;
  }
  mark(kTpPacked);
  // A 1-rank group (world 1 through the multi-rank path) moves nothing: its all-to-all is the identity and the
  // all-gather of the owner shard is the owner shard, so neither is issued (RCCL's 1-rank collectives are copies with
  // ~25-30 us of hand-off each around them, profiles/r5_forced_step_timeline.txt) — unless verify mode or a fault rule
  // wants to see the messages.
  const bool ident = N == 1 && !verify_ && !fault_.active();
  uint8_t* R = ident ? const_cast<uint8_t*>(P) : scratch("mesh_R" + std::to_string(sb * N), sb * N, st);
  if (!ident) {
    RoctxRange rr("fan/mesh/all_to_all");
    all_to_all_checked(P, R, sb, 0, st);
  }
  mark(kTpExchanged);
  if (sharded(req)) {
    // sharded update: the owner's reduce + round trip + SGD of shard r writes its new bf16 weights into lp's shard r,
    // then the weights are all-gathered in place (every rank's lp shard q comes from rank q)
    uint8_t* W = reinterpret_cast<uint8_t*>(req.lp);
    const size_t wb = (size_t)s * 2;
    {
      RoctxRange rr("fan/mesh/reduce_sgd");
      WirePtrs out{};
      out.p[0] = W + (size_t)r * wb;
      reduce_update_at(req, c, R, sb, N, r, g + (size_t)r * s * esize(gdt), (int64_t)r * s,
                       (size_t)valid_in(req.n_valid, (int64_t)r * s, s), out, 1, (size_t)s, false, st);
    }
    mark(kTpReduced);
    if (!ident) {
      RoctxRange rr("fan/mesh/all_gather_weights");
      // the weight shard goes through the same verify tags and fault hook as the unsharded path's gathered gradient
      all_gather_checked(W + (size_t)r * wb, W, wb, kSiteMeshWeightGather, 0, st);
    }
    counters_.sharded_updates++;
    return {};
  }
  uint8_t* G = epi_scratch("mesh_G" + std::to_string(sb * N), sb * N);
  {
    RoctxRange rr("fan/mesh/reduce");
    // (1-rank group: the reduced shard is the gathered bucket, so the reduce writes the epilogue's buffer directly)
    const uint8_t* own = g + (size_t)r * s * esize(gdt);
    if (enc)
      launch_wire_reduce_to(c, gdt, R, sb, N, r, own, WirePtrs{{ident ? G : S}}, 1, (size_t)s, encoder_of(req, r, 1, s),
                            false, st);
    else launch_wire_reduce(c, gdt, R, sb, N, r, own, ident ? G : S, nullptr, (size_t)s, st);
  }
  mark(kTpReduced);
  if (!ident) {
    RoctxRange rr("fan/mesh/all_gather");
    all_gather_checked(S, G, sb, kSiteMeshAllGather, 0, st);
  }
  return {make_epilogue(req, G, s, N, 0, L.n_pad)};
}

void AllReduceEngine::all_to_all_checked(const uint8_t* src, uint8_t* dst, size_t row_bytes, uint32_t row_base,
                                         hipStream_t st) {
  if (verify_) launch_msg_tags(src, row_bytes, row_bytes, world_, cur_.seq, tag_region(0), st);
  fault_.maybe_corrupt("mesh_pack", const_cast<uint8_t*>(src), row_bytes * world_, st);  // in flight: after the tags
  comm_->all_to_all(src, dst, row_bytes, st);
  count_peers(row_bytes);
  if (verify_) {
    comm_->all_to_all(tag_region(0), tag_region(1), 16, st);
    verify_rows(dst, row_bytes, world_, tag_region(1), kSiteMeshAllToAll, row_base, st);
  }
}

void AllReduceEngine::all_gather_checked(uint8_t* src, uint8_t* dst, size_t bytes, uint32_t verify_site,
                                         uint32_t row_base, hipStream_t st) {
  if (verify_) launch_msg_tags(src, bytes, bytes, 1, cur_.seq, tag_region(3), st);
  fault_.maybe_corrupt("mesh_reduce", src, bytes, st);
  comm_->all_gather(src, dst, bytes, st);
  count_peers(bytes);
  if (verify_) {
    comm_->all_gather(tag_region(3), tag_region(4), 16, st);
    verify_rows(dst, bytes, world_, tag_region(4), verify_site, row_base, st);
  }
}

// Mesh over the direct P2P transport: the encoder is the sender (the NIC streams its sums
// from send_fifo through the BFP TX framing onto the link, hw/all_reduce.sv:1155-1166, hw/bfp_adapter.sv:279-379).
//   round 1: the pack kernel stores shard p straight into peer p's receive slot (a prepacked bucket is copied
//            there); ready flags; the owner reduce reads the N-1 received shards IN PLACE from this rank's arena
//            (plus its own f32 shard) and stores the re-encoded owner shard straight into every peer's round-2
//            slot and its own; the round-1 slots are acknowledged;
//   round 2: ready flags; an immediate request decodes + applies SGD reading the gathered shards in place, then
//            acknowledges; a deferred one (epilogue at commit, after the producer's remaining GEMMs) first moves
//            them into per-slot scratch, since the slots are reused two rounds later.
// No staging buffer and no copy kernel on either side of a link. Verify mode tags every message where it landed
// (the slot trailer, P2PComm::dst_tag) and checks it on the consumer side after the ready flag, before the kernel
// that reads it (sites "mesh direct send" / "mesh direct gather", row = sender rank). Memory ordering: p2p_comm.h.
std::vector<EpiThunk> AllReduceEngine::run_mesh_direct(P2PComm* d, const EngineLayout& L, const EngineRequest& req) {
  const int N = world_, r = rank_, c = cfg_.codec, gdt = req.grad_dtype;
  const int64_t s = L.shard;
  const size_t sb = wire_shard_bytes(c, s);
  FAN_CHECK(sb <= d->payload_bytes(), "p2p: shard larger than the arena slot (raise slot_bytes)");
  const uint8_t* g = reinterpret_cast<const uint8_t*>(req.grad);
  hipStream_t st = cur_.run;
  const bool raw = zero_copy(c, gdt);
  // verify / fault hooks of one direct round: tag what this rank stored into each peer's slot (trailer tag 0), and
  // the receiver's check of every peer's message once its flag is up
  auto tag_sent = [&](const P2PComm::Round& rd, const char* fault_site, size_t bytes) {
    bool first = true;
    for (int q = 0; q < N; ++q) {
      if (q == r) continue;
      if (verify_) tag_direct(d->dst(rd, q), bytes, d->dst_tag(rd, q, 0), (uint32_t)rd.seq, st);
      if (first) fault_.maybe_corrupt(fault_site, d->dst(rd, q), bytes, st);  // in flight: after its tag
      first = false;
    }
  };
  auto check_received = [&](const P2PComm::Round& rd, uint32_t site, size_t bytes) {
    for (int q = 0; q < N; ++q) {
      if (q == r) continue;
      uint8_t* m = const_cast<uint8_t*>(d->src(rd, q));
      fault_.maybe_corrupt("p2p_recv", m, bytes, st);  // test hook: the slot changes after its flag was raised
      if (verify_) verify_direct(m, bytes, d->src_tag(rd, q, 0), (uint32_t)rd.seq, site, (uint32_t)q, st);
    }
  };
  P2PComm::Round r1 = d->begin(st);
  {
    RoctxRange rr("fan/mesh/direct_send");
    WirePtrs to{};
    std::vector<P2PCopy> segs;
    for (int q = 0; q < N; ++q) {
      if (q == r) continue;
      to.p[q] = d->dst(r1, q);
      if (req.prepacked) segs.push_back({req.prepacked + (size_t)q * sb, to.p[q], sb});
      else if (raw) segs.push_back({g + (size_t)q * s * esize(gdt), to.p[q], sb});
    }
    if (req.prepacked || raw) d->move(segs, st);
    // to.p[r] is null, so shard r is not encoded here — nor fed back (error feedback; ordering: run_mesh)
    else launch_wire_pack_to(c, gdt, g, to, (size_t)s, N, r, encoder_of(req, r, 0, s), true, st);
    tag_sent(r1, "mesh_pack", sb);
  }
  mark(kTpPacked);
  if (!fault_.maybe_drop("p2p_publish")) d->publish(r1, st);  // test hook: the round is never announced
  count_peers(sb, d);
  d->wait(r1, st);
  check_received(r1, kSiteMeshDirectSend, sb);
  mark(kTpExchanged);
  P2PComm::Round r2 = d->begin(st);
  if (sharded(req)) {
    // sharded update: the owner reduces the received shards in place, takes the sum through the codec round trip,
    // applies SGD to its master shard and stores its new bf16 weights straight into every peer's round-2 slot and
    // into its own lp shard; each rank then copies the peers' weight shards into lp (the layer's next weights)
    bf16_t* lp = req.lp;
    const size_t wb = (size_t)s * 2;
    {
      RoctxRange rr("fan/mesh/direct_reduce_sgd");
      WirePtrs out{};
      for (int q = 0; q < N; ++q) out.p[q] = q == r ? reinterpret_cast<uint8_t*>(lp + (size_t)r * s) : d->dst(r2, q);
      reduce_update_at(req, c, d->src_base(r1), d->src_stride(), N, r, g + (size_t)r * s * esize(gdt), (int64_t)r * s,
                       (size_t)valid_in(req.n_valid, (int64_t)r * s, s), out, N, (size_t)s, true, st);
      d->release(r1, st);
      tag_sent(r2, "mesh_reduce", wb);
    }
    mark(kTpReduced);
    if (!fault_.maybe_drop("p2p_publish")) d->publish(r2, st);
    count_peers(wb, d);
    d->wait(r2, st);
    check_received(r2, kSiteMeshDirectGather, wb);
    {
      RoctxRange rr("fan/mesh/direct_weights");
      std::vector<P2PCopy> segs;
      for (int q = 0; q < N; ++q)
        if (q != r) segs.push_back({d->src(r2, q), lp + (size_t)q * s, wb});
      d->move(segs, st);
    }
    d->release(r2, st);
    counters_.direct_rounds += 2;
    counters_.sharded_updates++;
    return {};
  }
  {
    RoctxRange rr("fan/mesh/direct_reduce");
    WirePtrs out{};
    for (int q = 0; q < N; ++q) out.p[q] = d->dst(r2, q);  // q == r: this rank's own copy (its own slot)
    const uint8_t* own = g + (size_t)r * s * esize(gdt);
    launch_wire_reduce_to(c, gdt, d->src_base(r1), d->src_stride(), N, r, own, out, N, (size_t)s,
                          encoder_of(req, r, 1, s), true, st);
    d->release(r1, st);
    tag_sent(r2, "mesh_reduce", sb);
  }
  mark(kTpReduced);
  if (!fault_.maybe_drop("p2p_publish")) d->publish(r2, st);
  count_peers(sb, d);
  d->wait(r2, st);
  check_received(r2, kSiteMeshDirectGather, sb);
  counters_.direct_rounds += 2;
  const uint8_t* Gv = d->src_base(r2);
  const size_t gstride = d->src_stride();
  if (req.defer) {
    uint8_t* G = epi_scratch("mesh_G" + std::to_string(sb * N), sb * N);
    std::vector<P2PCopy> segs;
    for (int q = 0; q < N; ++q) segs.push_back({Gv + (size_t)q * gstride, G + (size_t)q * sb, sb});
    d->move(segs, st);
    d->release(r2, st);
    return {make_epilogue(req, G, s, N, 0, L.n_pad)};
  }
  mark(kTpCommEnd);
  {
    RoctxRange rr("fan/mesh/direct_epilogue");
    const int64_t nv = valid_in(req.n_valid, 0, L.n_pad);
    // Trust ratio: pass 1 reads the arena in place, here on the comm stream before the slot is released; the ratio
    // and pass 2 (dense, no wire) follow as submit()'s thunks on the epilogue stream, which waits for comm_done,
    // recorded after this launch. kTpCommEnd is marked above, so a request trace counts all three launches in its
    // epilogue phase (kTpCommEnd -> kTpEpiEnd), although pass 1 runs on this stream, like the plain update of this
    // path, and the other two on the epilogue stream.
    if (trust(req) && nv > 0)
      lamb_region(req, Gv, s, N, 0, nv, -1, 0, gstride)(st);
    else if (req.update && nv > 0) update_at(req, c, Gv, (size_t)s, N, -1, 0, 0, (size_t)nv, st, gstride);
    if (req.out_sum) launch_wire_unpack_strided(c, kF32, Gv, gstride, req.out_sum, (size_t)s, N, st);
  }
  d->release(r2, st);
  return {};
}

// Chunked mesh (buckets above chunk_elems): the reference's block pipeline (hw/all_reduce.sv:330, 423-464,
// 1033-1061) re-expressed over two streams. Chunk c = N shards of L.shard elements (wire shards c*N .. c*N+N-1).
//   comm stream (every collective, in one order on every rank): pack(c), all_to_all(c), all_gather(c-1), ...
//   aux stream: owner reduce(c) [after all_to_all(c)], per-chunk decode+SGD epilogue(c-1) [after all_gather(c-1)]
// so chunk c's reduce / chunk c-1's epilogue run while the links carry chunk c's / c+1's exchange. Pack, receive
// and reduce buffers are double-buffered by chunk parity, so scratch is bounded by two chunks whatever the bucket
// size — except the gathered wire of a DEFERRED request, which its epilogue reads at commit (per slot, whole
// bucket: 17 B per 16 values). Buffer reuse is ordered by the stream order plus one wait each way:
//   P[c%2], R[c%2] rewritten by pack/all_to_all(c+2) after reduce(c) (comm waits reduce(c) before all_to_all(c+2))
//   S[c%2] rewritten by reduce(c+2) after all_gather(c): all_gather(c) precedes all_to_all(c+2) on the comm stream
//   G[c%2] rewritten by all_gather(c+2) after epilogue(c): reduce(c+2), which all_gather(c+2) waits for, follows
//   epilogue(c) on the aux stream.
std::vector<EpiThunk> AllReduceEngine::run_mesh_chunked(const EngineLayout& L, const EngineRequest& req) {
  const int N = world_, r = rank_, c = cfg_.codec, gdt = req.grad_dtype;
  const int64_t s = L.shard, C = L.chunks;
  const size_t sb = wire_shard_bytes(c, s), cb = sb * N;  // one shard / one chunk of wire
  const uint8_t* g = reinterpret_cast<const uint8_t*>(req.grad);
  const uint8_t* prepacked = req.prepacked;
  const bool defer = req.defer;
  hipStream_t A = cur_.run, B = aux_stream_;
  const bool raw = zero_copy(c, gdt);
  const std::string k = std::to_string(sb);
  uint8_t *Pb[2] = {nullptr, nullptr}, *R[2], *S[2], *Gc[2] = {nullptr, nullptr};
  for (int q = 0; q < 2; ++q) {
    if (!raw && !prepacked) Pb[q] = scratch("meshc_P" + std::to_string(q) + "_" + k, cb, A);
    R[q] = scratch("meshc_R" + std::to_string(q) + "_" + k, cb, A);
    S[q] = scratch("meshc_S" + std::to_string(q) + "_" + k, sb, A);
    if (!defer) Gc[q] = scratch("meshc_G" + std::to_string(q) + "_" + k, cb, A);
  }
  // A deferred request's epilogue reads the whole gathered bucket at commit. One such buffer per bucket size is
  // shared by every deferred chunked request (not one per slot: 17 B per 16 elements of a multi-GB bucket, 8 times
  // over): a new user first commits the previous one if it is still pending (ordered after its producer, as a
  // 9th deferred request does) and waits for that epilogue to finish reading before the all-gather overwrites it.
  uint8_t* Gall = nullptr;
  hipEvent_t gall_free = nullptr;
  if (defer) {
    GallBuf& gb = gall_[k + "_" + std::to_string(C)];
    if (gb.free == nullptr) FAN_HIP_CHECK(hipEventCreateWithFlags(&gb.free, hipEventDisableTiming));
    if (gb.seq != 0) {
      const auto& prev = table_->slot(gb.slot);
      if (prev.seq == gb.seq && prev.pending && gb.slot != cur_.slot) {
        counters_.forced_commits++;
        table_->commit(gb.slot, true, cur_.producer, gb.seq);
      }
      FAN_HIP_CHECK(hipStreamWaitEvent(A, gb.free, 0));  // recorded after that epilogue (no-op if it never ran)
    }
    gb.slot = cur_.slot;
    gb.seq = cur_.seq;
    Gall = scratch("meshc_Gall_" + k + "_" + std::to_string(C), cb * C, A);
    gall_free = gb.free;
  }
  auto gath = [&](int64_t ch) { return defer ? Gall + ch * cb : Gc[ch % 2]; };
  auto gather = [&](int64_t ch) {  // comm stream: all-gather of chunk ch's reduced owner shard
    RoctxRange rr("fan/mesh/all_gather");
    FAN_HIP_CHECK(hipStreamWaitEvent(A, cev_[1][ch % 2], 0));
    all_gather_checked(S[ch % 2], gath(ch), sb, kSiteMeshAllGather, (uint32_t)(ch * N), A);
    if (!defer) {  // per-chunk epilogue on the aux stream
      FAN_HIP_CHECK(hipEventRecord(cev_[2][ch % 2], A));
      FAN_HIP_CHECK(hipStreamWaitEvent(B, cev_[2][ch % 2], 0));
      RoctxRange re("fan/mesh/epilogue");
      epilogue(req, c, B, gath(ch), s, N, ch * N * s, N * s);
    }
  };
  for (int64_t ch = 0; ch < C; ++ch) {
    const uint8_t* P;
    if (prepacked) {
      P = prepacked + ch * cb;
    } else if (raw) {
      P = g + (size_t)ch * N * s * esize(gdt);
    } else {
      RoctxRange rr("fan/mesh/pack");
      launch_wire_pack(c, gdt, g + (size_t)ch * N * s * esize(gdt), Pb[ch % 2], (size_t)s, N, A);
      P = Pb[ch % 2];
    }
    {
      RoctxRange rr("fan/mesh/all_to_all");
      if (ch >= 2) FAN_HIP_CHECK(hipStreamWaitEvent(A, cev_[1][ch % 2], 0));  // reduce(ch-2) done with R, P
      all_to_all_checked(P, R[ch % 2], sb, (uint32_t)(ch * N), A);
      FAN_HIP_CHECK(hipEventRecord(cev_[0][ch % 2], A));
    }
    {
      RoctxRange rr("fan/mesh/reduce");
      FAN_HIP_CHECK(hipStreamWaitEvent(B, cev_[0][ch % 2], 0));
      launch_wire_reduce(c, gdt, R[ch % 2], sb, N, r, g + ((size_t)ch * N + r) * s * esize(gdt), S[ch % 2], nullptr,
                         (size_t)s, B);
      FAN_HIP_CHECK(hipEventRecord(cev_[1][ch % 2], B));
    }
    if (ch >= 1) gather(ch - 1);
  }
  gather(C - 1);
  // the request's completion on the comm stream covers the aux stream's last reduce / epilogue
  FAN_HIP_CHECK(hipEventRecord(cev_[3][1], B));
  FAN_HIP_CHECK(hipStreamWaitEvent(A, cev_[3][1], 0));
  if (!defer) return {};
  const EpiThunk epi = make_epilogue(req, Gall, s, (int)(C * N), 0, L.n_pad);
  return {[=](hipStream_t es) {
    epi(es);
    FAN_HIP_CHECK(hipEventRecord(gall_free, es));  // the shared gathered wire may be reused after this point
  }};
}

std::vector<AllReduceEngine::RingLane> AllReduceEngine::ring_lanes(const EngineLayout& L) const {
  const int N = world_;
  std::vector<RingLane> lanes;
  for (size_t i = 0; i < orders_.size(); ++i) {
    const auto& o = orders_[i];
    int pos = 0;
    for (int q = 0; q < N; ++q)
      if (o[q] == rank_) pos = q;
    lanes.push_back({(int64_t)i * L.part, pos, o[(pos - 1 + N) % N], o[(pos + 1) % N], ring_plan(N, pos, L.blocks)});
  }
  return lanes;
}

std::vector<EpiThunk> AllReduceEngine::run_ring(const EngineLayout& L, const EngineRequest& req) {
  const int N = world_, c = cfg_.codec, gdt = req.grad_dtype;
  const int64_t S = L.slice;
  const size_t sb = wire_shard_bytes(c, S);
  const int64_t nsl = L.blocks * N;
  const uint8_t* g = reinterpret_cast<const uint8_t*>(req.grad);
  const uint8_t* prepacked = req.prepacked;
  hipStream_t st = cur_.run;
  const bool compat = cfg_.compat_owner_fp32 && N > 1 && req.update;
  if (prepacked)  // encode what the producer did not (bias gradient + padding): slice-sized shards (sub-shards when
                  // the direct ring streams its hops), ring-major
    launch_wire_pack_range(c, gdt, req.grad, const_cast<uint8_t*>(prepacked), (size_t)(S / L.sub),
                           (size_t)req.prepacked_elems, (size_t)L.n_pad, st);
  if (P2PComm* d = comm_ ? comm_->direct() : nullptr; d && N > 1 && !compat) return run_ring_direct(d, L, req);
  struct RingState : RingLane {
    uint8_t *G, *send, *recv[2];
    const uint8_t* last_partial;
    float* fp32;
  };
  std::vector<RingState> rings;
  const std::string k = std::to_string(sb) + "_" + std::to_string(nsl);
  for (RingLane& lane : ring_lanes(L)) {
    const std::string i = std::to_string(rings.size());
    RingState rs{std::move(lane)};
    rs.G = epi_scratch("ring_G" + i + "_" + k, sb * nsl);
    rs.send = scratch("ring_send" + i + "_" + k, sb, st);
    rs.recv[0] = scratch("ring_recv0_" + i + "_" + k, sb, st);
    rs.recv[1] = scratch("ring_recv1_" + i + "_" + k, sb, st);
    rs.last_partial = nullptr;
    rs.fp32 = compat ? reinterpret_cast<float*>(epi_scratch("ring_fp32_" + i + "_" + k, 4 * S * L.blocks)) : nullptr;
    rings.push_back(std::move(rs));
  }
  auto local = [&](const RingState& rs, int64_t x) { return g + (size_t)(rs.off + x * S) * esize(gdt); };
  uint32_t round_id = 0;
  for (const auto& rnd : ring_rounds(rings[0].plan)) {
    RoctxRange rr("fan/ring/round");
    if (N > 1) {  // no credit phase on a copying transport: points 0 and 1 coincide; then kernels, exchange
      if (cur_.trace >= 0) trace_pool_[cur_.trace].hop_kernel_first = true;
      hop_mark(0);
      hop_mark(1);
    }
    std::vector<P2POp> sends, recvs;
    for (size_t j : rnd) {
      for (auto& rs : rings) {
        const RingRound& row = rs.plan[j];
        uint8_t* out = nullptr;
        if (row.send_src == kSendLocal) {
          if (prepacked) {  // the producer's encoding of this slice is the message
            const uint8_t* pk = prepacked + ((size_t)(&rs - rings.data()) * nsl + row.send_slice) * sb;
            if (row.owned >= 0) launch_multi_copy({{pk, rs.G + (size_t)row.send_slice * sb, sb}}, st);
            out = const_cast<uint8_t*>(pk);
          } else {
            out = row.owned >= 0 ? rs.G + (size_t)row.send_slice * sb : rs.send;
            launch_wire_pack(c, gdt, local(rs, row.send_slice), out, (size_t)S, 1, st);
          }
        } else if (row.send_src == kSendReduce) {
          out = row.owned >= 0 ? rs.G + (size_t)row.send_slice * sb : rs.send;
          float* f32 = nullptr;
          if (compat && row.owned >= 0) f32 = rs.fp32 + (size_t)(row.owned / N) * S;
          launch_wire_reduce(c, gdt, rs.last_partial, sb, 2, 1, local(rs, row.send_slice), out, f32, (size_t)S, st);
        } else if (row.send_src == kSendForward) {
          out = rs.G + (size_t)row.send_slice * sb;
        }
        if (out && N > 1) sends.push_back({out, sb, rs.down});
        if (row.recv_slice >= 0) {
          uint8_t* tgt;
          if (row.recv_full) {
            tgt = rs.G + (size_t)row.recv_slice * sb;
          } else {
            tgt = rs.recv[j % 2];
            rs.last_partial = tgt;
          }
          recvs.push_back({tgt, sb, rs.up});
        }
      }
    }
    if (N > 1) {
      const size_t nd = sends.size(), nr = recvs.size();
      if (verify_) {  // one tag per message, sent after all of the round's payloads (per-peer order is kept)
        FAN_CHECK(nd <= (size_t)kTagRows && nr <= (size_t)kTagRows, "verify: too many messages in a ring round");
        for (size_t q = 0; q < nd; ++q) {
          launch_msg_tags(static_cast<const uint8_t*>(sends[q].ptr), sb, sb, 1, cur_.seq, tag_region(0) + q * 4, st);
          sends.push_back({tag_region(0) + q * 4, 16, sends[q].peer});
        }
        for (size_t q = 0; q < nr; ++q) recvs.push_back({tag_region(1) + q * 4, 16, recvs[q].peer});
      }
      // (fault injection corrupts a message in flight: on a producer-encoded slice that is the producer's buffer)
      for (size_t q = 0; q < nd; ++q) fault_.maybe_corrupt("ring_send", static_cast<uint8_t*>(sends[q].ptr), sb, st);
      if (counters_.peer_bytes.size() != (size_t)world_) counters_.peer_bytes.assign(world_, 0);
      for (const P2POp& op : sends) counters_.peer_bytes[op.peer] += (int64_t)op.bytes;
      hop_mark(2);
      comm_->sendrecv(sends, recvs, st);
      hop_mark(3);
      if (verify_)
        for (size_t q = 0; q < nr; ++q)
          verify_rows(static_cast<const uint8_t*>(recvs[q].ptr), sb, 1, tag_region(1) + q * 4, kSiteRingRound,
                      round_id * kTagRows + (uint32_t)q, st);
    }
    ++round_id;
  }
  std::vector<EpiThunk> thunks;
  for (auto& rs : rings) {
    if (!compat) {
      thunks.push_back(make_epilogue(req, rs.G, S, (int)nsl, rs.off, L.part));
      continue;
    }
    // the owner of each slice updates it from the un-quantised f32 sum instead of the wire
    const int own = (rs.pos - 1 + N) % N;
    const EpiThunk rest = make_epilogue(req, rs.G, S, (int)nsl, rs.off, L.part, own, N);
    const int64_t off = rs.off, blocks = L.blocks;
    float* f32 = rs.fp32;
    thunks.push_back([=](hipStream_t es) {
      rest(es);
      for (int64_t b = 0; b < blocks; ++b) {
        const int64_t o2 = off + (b * N + own) * S;
        const int64_t nv = valid_in(req.n_valid, o2, S);
        if (nv > 0) update_at(req, kRawF32, f32 + b * S, (size_t)S, 1, -1, 0, o2, (size_t)nv, es);
      }
    });
  }
  return thunks;
}

// Ring over the direct P2P transport: the encoder is the sender. Every hop's fused decode + add + encode kernel
// (wire_reduce_to) reads the upstream partial IN PLACE from this rank's receive arena and stores its encoded output
// straight into the downstream neighbour's arena slot (the NIC pushes each reduced beat into send_fifo, through the
// BFP TX framing and onto the link, hw/all_reduce.sv:1155-1166, hw/bfp_adapter.sv:279-379); SEND_LOCAL encodes
// (or, for a producer-encoded bucket, copies) the local slice straight into that slot; a FORWARD hop copies the
// received full slice arena -> downstream arena, and every received full slice is copied once into the gathered
// wire the epilogue reads (pure copies: P2PComm::move, CU kernel or copy engines). The schedule, sums and summation
// order are those of run_ring's copying rounds (bit-identical; the compat owner-f32 mode uses that path).
//
// Streaming (L.sub = P > 1): every round's messages go out as P sub-slices (wire sub-shards of S/P elements), each
// its own P2P sub-round with its own ready flag. Sub-slice s of round t only needs sub-slice s of the upstream's
// round t-1, which landed P sub-rounds earlier, so the downstream starts reducing it while this rank still encodes
// the rest — the NIC forwards each reduced beat through send_fifo the same way instead of storing a whole slice
// (hw/all_reduce.sv:1155-1166, 1033-1061). A message is consumed P sub-rounds after it lands, so the arena keeps
// P + 1 or more slots per sender (P2PComm depth). P = 1 is the lock-step ring. Per sub-round j: credit wait for the
// downstream slots (begin_to), wait for the upstream messages of sub-round j - P (wait_from), the kernels / copies,
// ack of those upstream messages, ready flags downstream.
// Verify mode tags message k of a sub-round in its slot trailer (tag k) after the kernels and checks every message
// before the kernels that read it (site "ring direct hop", row = the sub-round it was sent in). Traced requests
// record four device timestamps per sub-round (hop_mark): start, credits granted, upstream data ready, kernels done.
std::vector<EpiThunk> AllReduceEngine::run_ring_direct(P2PComm* d, const EngineLayout& L, const EngineRequest& req) {
  const int N = world_, c = cfg_.codec, gdt = req.grad_dtype;
  const int P = L.sub;
  const int64_t S = L.slice, Sp = S / P;
  const size_t sb = wire_shard_bytes(c, Sp);  // one message: one sub-shard
  const size_t msg = (sb + 255) / 256 * 256;  // message stride inside an arena slot (<= 2 messages per peer/round)
  FAN_CHECK(S % (256 * (int64_t)P) == 0 && P <= d->depth() - 1, "p2p ring: bad sub-slice geometry");
  FAN_CHECK(2 * msg <= d->payload_bytes(), "p2p ring: two slices per round must fit an arena slot (lower max_slice_elems)");
  const int64_t nsl = L.blocks * N, nsh = nsl * P;  // slices / wire (sub-)shards per ring part
  const uint8_t* g = reinterpret_cast<const uint8_t*>(req.grad);
  const uint8_t* prepacked = req.prepacked;
  hipStream_t st = cur_.run;
  struct RS : RingLane {
    uint8_t* G;
  };
  struct Rx {
    int64_t slice;
    bool full;
    const uint8_t* ptr;
    const uint8_t* tag;
  };
  std::vector<RS> rings;
  std::vector<int> downs, ups;
  const std::string k = std::to_string(sb) + "_" + std::to_string(nsh);
  for (RingLane& lane : ring_lanes(L)) {
    RS rs{std::move(lane)};
    rs.G = epi_scratch("ring_G" + std::to_string(rings.size()) + "_" + k, sb * nsh);
    downs.push_back(rs.down);
    ups.push_back(rs.up);
    rings.push_back(std::move(rs));
  }
  const std::vector<std::vector<size_t>> rounds = ring_rounds(rings[0].plan);
  // local f32 / bf16 elements of sub-slice s of slice x
  auto local = [&](const RS& rs, int64_t x, int s) { return g + (size_t)(rs.off + x * S + (int64_t)s * Sp) * esize(gdt); };
  auto gsub = [&](const RS& rs, int64_t x, int s) { return rs.G + (size_t)(x * P + s) * sb; };  // G sub-shard
  std::vector<P2PComm::Round> sub_round(rounds.size() * P);  // P2P round of every sub-round (its sequence number)
  // the upstream messages of sub-round jj: ready wait, fault hook, verify
  auto arrive = [&](size_t jj, std::vector<std::vector<Rx>>& per_ring) {
    d->wait_from(sub_round[jj], ups, st);
    for (size_t i = 0; i < rings.size(); ++i)
      for (Rx& x : per_ring[i]) {
        fault_.maybe_corrupt("p2p_recv", const_cast<uint8_t*>(x.ptr), sb, st);  // test hook: changed after its flag
        if (verify_) verify_direct(x.ptr, sb, x.tag, (uint32_t)sub_round[jj].seq, kSiteRingDirect, (uint32_t)jj, st);
      }
  };
  if (counters_.peer_bytes.size() != (size_t)world_) counters_.peer_bytes.assign(world_, 0);
  if (cur_.trace >= 0) trace_pool_[cur_.trace].hop_kernel_first = false;  // points: credit, ready, kernels
  // got[s][ring]: the messages sub-round (t - 1, s) delivered, consumed by (t, s)
  std::vector<std::vector<std::vector<Rx>>> got(P, std::vector<std::vector<Rx>>(rings.size()));
  for (size_t t = 0; t < rounds.size(); ++t) {
    const auto& rnd = rounds[t];
    for (int s = 0; s < P; ++s) {
      RoctxRange rr_("fan/ring/direct_round");
      const size_t j = t * P + s;
      hop_mark(0);
      const P2PComm::Round rr = d->begin_to(downs, st);
      sub_round[j] = rr;
      hop_mark(1);
      std::vector<std::vector<Rx>>& prev = got[s];  // what sub-round (t - 1, s) delivered
      if (t > 0) arrive(j - P, prev);
      hop_mark(2);
      std::vector<P2PCopy> copies;  // forwards (arena -> downstream arena) and received full sub-slices -> G
      struct Sent {
        uint8_t* msg;
        uint8_t* tag;
      };
      std::vector<Sent> sent;  // this sub-round's messages, tagged after all of its kernels / copies
      for (size_t i = 0; i < rings.size(); ++i) {
        RS& rs = rings[i];
        size_t kmsg = 0;
        for (size_t jr : rnd) {
          const RingRound& row = rs.plan[jr];
          if (row.send_src == kSendNone) continue;
          uint8_t* to = d->dst(rr, rs.down) + kmsg * msg;
          sent.push_back({to, d->dst_tag(rr, rs.down, (int)kmsg)});
          ++kmsg;
          counters_.peer_bytes[rs.down] += (int64_t)sb;
          d->count_sent(rs.down, sb);
          if (row.send_src == kSendLocal) {
            if (prepacked) {
              copies.push_back({prepacked + ((size_t)i * nsh + (size_t)row.send_slice * P + s) * sb, to, sb});
            } else {
              WirePtrs w{};
              w.p[0] = to;
              launch_wire_pack_to(c, gdt, local(rs, row.send_slice, s), w, (size_t)Sp, 1, -1, {}, true, st);
            }
          } else if (row.send_src == kSendReduce) {
            const Rx* part = nullptr;
            for (const Rx& x : prev[i])
              if (!x.full) part = &x;
            FAN_CHECK(part != nullptr, "p2p ring: no upstream partial for a reduce hop");
            WirePtrs w{};
            w.p[0] = to;
            int nd = 1;
            if (row.owned >= 0) w.p[nd++] = gsub(rs, row.send_slice, s);  // this rank's fully reduced sub-slice
            launch_wire_reduce_to(c, gdt, part->ptr, 0, 2, 1, local(rs, row.send_slice, s), w, nd, (size_t)Sp, {}, true,
                                  st);
          } else {  // kSendForward: the full sub-slice received last round goes on downstream
            const Rx* full = nullptr;
            for (const Rx& x : prev[i])
              if (x.full && x.slice == row.send_slice) full = &x;
            FAN_CHECK(full != nullptr, "p2p ring: forwarded slice not received");
            copies.push_back({full->ptr, to, sb});
          }
        }
        for (const Rx& x : prev[i])  // every received full sub-slice lands once in the gathered wire
          if (x.full) copies.push_back({x.ptr, gsub(rs, x.slice, s), sb});
      }
      if (!copies.empty()) d->move(copies, st);
      for (const Sent& m : sent) {
        if (verify_) tag_direct(m.msg, sb, m.tag, (uint32_t)rr.seq, st);
        fault_.maybe_corrupt("ring_send", m.msg, sb, st);  // in flight: after its tag
      }
      hop_mark(3);
      if (t > 0) d->release_from(sub_round[j - P], ups, st);  // the messages of (t - 1, s) are consumed
      if (!fault_.maybe_drop("p2p_publish")) d->publish_to(rr, downs, st);
      // what this sub-round will deliver from upstream (read in (t + 1, s) or by the drain below)
      for (size_t i = 0; i < rings.size(); ++i) {
        prev[i].clear();
        size_t kmsg = 0;
        for (size_t jr : rnd) {
          const RingRound& row = rings[i].plan[jr];
          if (row.recv_slice < 0) continue;
          prev[i].push_back({row.recv_slice, row.recv_full != 0, d->src(rr, rings[i].up) + kmsg * msg,
                             d->src_tag(rr, rings[i].up, (int)kmsg)});
          ++kmsg;
        }
      }
      counters_.direct_rounds++;
    }
  }
  // drain: the last round's P sub-rounds of messages (full slices of the all-gather's end) -> G, then ack
  const size_t T = rounds.size();
  for (int s = 0; s < P; ++s) {
    const size_t jj = (T - 1) * P + s;
    arrive(jj, got[s]);
    std::vector<P2PCopy> tail;
    for (size_t i = 0; i < rings.size(); ++i)
      for (const Rx& x : got[s][i])
        if (x.full) tail.push_back({x.ptr, gsub(rings[i], x.slice, s), sb});
    if (!tail.empty()) d->move(tail, st);
    d->release_from(sub_round[jj], ups, st);
  }
  std::vector<EpiThunk> thunks;
  for (auto& rs : rings) thunks.push_back(make_epilogue(req, rs.G, Sp, (int)nsh, rs.off, L.part));
  return thunks;
}

void AllReduceEngine::gather_owned(float* plane, int64_t n) {
  if (!shard_upd_ || world_ == 1 || comm_ == nullptr) return;
  const EngineLayout L = layout(n);
  if (L.algo != 0 || L.chunks != 1) return;  // the sharded schedule runs on unchunked mesh buckets only
  FAN_HIP_CHECK(hipSetDevice(device_));
  const int N = world_, r = rank_;
  const int64_t s = L.shard;
  hipStream_t st = stream_;
  // every request that updated the plane has finished. Its owner SGD ran on this engine's comm / aux stream, or — the
  // backward's last request (on_producer) — on the caller's compute stream: the engine streams are synchronized and
  // every used slot's done event (recorded on whichever stream ran the request's epilogue) is waited for before the
  // all-gather reads the shard. Not a device-wide sync: virtual ranks in one process would wait on each other's
  // streams parked on this rank's coming flags.
  FAN_HIP_CHECK(hipStreamSynchronize(stream_));
  FAN_HIP_CHECK(hipStreamSynchronize(aux_stream_));
  table_->for_each_used([](int, const SlotTable<HipSlotDevice>::Slot& sl) {
    FAN_CHECK(!sl.pending, "gather_owned: a request is still deferred (commit or synchronize every request first)");
    FAN_HIP_CHECK(hipEventSynchronize(sl.done));
  });
  size_t max_bytes = (size_t)s * 4;
  if (P2PComm* d = comm_->direct()) max_bytes = std::min(max_bytes, d->payload_bytes() / 256 * 256);
  const int64_t piece = std::max<int64_t>(64, (int64_t)(max_bytes / 4) / 64 * 64);
  uint8_t* G = scratch("gather_owned", (size_t)N * piece * 4, st);
  for (int64_t off = 0; off < s; off += piece) {
    const int64_t k = std::min(piece, s - off);
    comm_->all_gather(plane + (size_t)r * s + off, G, (size_t)k * 4, st);
    std::vector<P2PCopy> segs;
    for (int q = 0; q < N; ++q)
      if (q != r) segs.push_back({G + (size_t)q * k * 4, plane + (size_t)q * s + off, (size_t)k * 4});
    launch_multi_copy(segs, st);
  }
  FAN_HIP_CHECK(hipStreamSynchronize(st));
}

void AllReduceEngine::tag_direct(const uint8_t* msg, size_t bytes, uint8_t* trailer, uint32_t seq, hipStream_t st) {
  uint32_t* t = tag_region(0);  // one local row: the tag kernels and this copy are stream-ordered
  launch_msg_tags(msg, bytes, bytes, 1, seq, t, st);
  launch_multi_copy({{t, trailer, 16}}, st);
}

void AllReduceEngine::verify_direct(const uint8_t* msg, size_t bytes, const uint8_t* trailer, uint32_t seq,
                                    uint32_t site, uint32_t row, hipStream_t st) {
  launch_msg_verify(msg, bytes, bytes, 1, reinterpret_cast<const uint32_t*>(trailer), seq, tag_region(2), verr_dev_,
                    site, row, st);
  counters_.verified_rows++;
}

void AllReduceEngine::hop_mark(int point) {
  if (cur_.trace < 0) return;
  if (hop_used_ == hop_pool_.size()) {
    hipEvent_t e;
    FAN_HIP_CHECK(hipEventCreate(&e));
    hop_pool_.push_back(e);
  }
  RequestTrace& t = trace_pool_[cur_.trace];
  if (t.hop_count == 0) t.hop_first = hop_used_;
  FAN_HIP_CHECK(hipEventRecord(hop_pool_[hop_used_++], cur_.run));
  t.hop_count++;
  (void)point;
}

int AllReduceEngine::submit(const EngineRequest& req, hipStream_t producer) {
  RoctxRange rr("fan/allreduce/submit");
  cur_ = Current{};
  FAN_CHECK(req.upd.kind != kOptAdamW || !req.update || req.moment_q ||
                (req.mom != nullptr && req.upd.adamw.var != nullptr),
            "AdamW needs both moment planes");
  FAN_CHECK(req.upd.kind == kOptSgd || req.upd.kind == kOptAdamW || req.upd.kind == kOptLion,
            "unknown optimizer kind (0 SGD, 1 AdamW, 2 Lion)");
  if (req.upd.kind == kOptLion) {
    // One f32 moment plane, where SGD's momentum travels (refused before the request takes a slot).
    FAN_CHECK(!req.update || req.mom != nullptr, "Lion needs its moment plane (mom)");
    FAN_CHECK(req.upd.adamw.var == nullptr, "Lion keeps one moment plane: no second-moment plane (var)");
    FAN_CHECK(!req.upd.trust, "trust ratio: a flag of AdamW update requests, not of Lion");
    FAN_CHECK(!req.moment_q, "moment_codec bfp8: AdamW update requests only (Lion's one moment plane stays f32)");
  }
  if (req.moment_q) {
    // The 8-bit state is read and written by update_at's one launch (refused before the request takes a slot).
    FAN_CHECK(req.upd.kind == kOptAdamW && req.update,
              "moment_codec bfp8: AdamW update requests only (SGD keeps no second moment; its momentum stays f32)");
    FAN_CHECK(!req.upd.trust, "moment_codec bfp8: not with the trust ratio (its pass 2 recomputes the direction from the "
                              "stored moments)");
    FAN_CHECK(!sharded(req), "moment_codec bfp8: not with the sharded update (shard_update), whose owner kernels keep "
                             "f32 moment shards");
    FAN_CHECK(req.mom_q != nullptr && req.var_q != nullptr, "moment_codec bfp8: both moment planes (uint8)");
    const EngineLayout ML = layout(req.n_valid, req.layout_shard, req.layout_chunks);
    FAN_CHECK((uint64_t)ML.n_pad < ((uint64_t)1 << 32),
              "moment_codec bfp8: a padded bucket of 2^32 or more elements (element indices are 32-bit)");
    FAN_CHECK(req.moment_elems == ML.n_pad, "moment_codec bfp8: the planes hold exactly the layout's n_pad = " +
                                                std::to_string(ML.n_pad) + " elements (n_pad * 17 / 16 bytes each)");
  }
  if (trust(req)) {
    // Every weight of the bucket waits for two norms over the whole bucket, so a schedule that updates part of it
    // before the rest is reduced cannot carry the request (refused before the request takes a slot).
    FAN_CHECK(!sharded(req), "trust ratio: not with the sharded update (shard_update), whose owners update their "
                             "shard before the bucket is reduced");
    FAN_CHECK(layout(req.n_valid, req.layout_shard, req.layout_chunks).chunks <= 1,
              "trust ratio: not with a chunked layout (layout_chunks > 1, or a bucket above chunk_elems)");
    FAN_CHECK(!(cfg_.compat_owner_fp32 && cfg_.algo == 1), "trust ratio: not with the ring's compat_owner_fp32");
    FAN_CHECK(req.n_adapt >= -1 && req.n_adapt <= req.n_valid, "trust ratio: n_adapt must lie in [0, n_valid]");
  }
  if (req.clip_words) {
    // No weight of any request of the group moves before the norm over all of them exists: the same refusals as the
    // trust ratio's, one level up (before the request takes a slot).
    FAN_CHECK(req.update, "clip: update requests only (a sum-only request has no gradient scale to clip)");
    FAN_CHECK(req.defer, "clip: a clipped request must be deferred (its update waits for the group's coefficient; the "
                         "direct mesh's immediate path updates inside the communication phase)");
    FAN_CHECK(!sharded(req), "clip: not with the sharded update (shard_update), whose owners update their shard before "
                             "the bucket is reduced");
    FAN_CHECK(layout(req.n_valid, req.layout_shard, req.layout_chunks).chunks <= 1,
              "clip: not with a chunked layout (layout_chunks > 1, or a bucket above chunk_elems)");
    FAN_CHECK(!(cfg_.compat_owner_fp32 && cfg_.algo == 1), "clip: not with the ring's compat_owner_fp32");
  }
  if (req.residual) {
    // Error feedback lives in the mesh schedule's two encoders (refused before the request takes a slot).
    FAN_CHECK(cfg_.codec != kRawF32, "error feedback: nothing to feed back with the raw codec (raw_f32 drops nothing)");
    FAN_CHECK(codec_shared_exp(cfg_.codec), "error feedback: raw_bf16 is not supported yet (BFP codecs only)");
    FAN_CHECK(req.prepacked == nullptr, "error feedback: not with prepacked input (the GEMM's encoding carries no "
                                        "residual)");
    FAN_CHECK(cfg_.algo == 0, "error feedback: mesh schedule only (the ring schedule is not supported yet)");
    FAN_CHECK(layout(req.n_valid, req.layout_shard, req.layout_chunks).chunks <= 1,
              "error feedback: not with a chunked layout (layout_chunks > 1, or a bucket above chunk_elems)");
    FAN_CHECK(!sharded(req), "error feedback: not with the sharded update (shard_update)");
    FAN_CHECK(world_ <= kMaxPeers, "error feedback: at most 16 ranks (one destination per shard)");
  }
  if (req.sr) {
    // Stochastic rounding lives in the same two encoders (refused before the request takes a slot).
    FAN_CHECK(cfg_.codec == kBfpRne || cfg_.codec == kBfp4Rne,
              "stochastic rounding: bfp_rne and bfp4_rne only (bfp_trunc is the reference's floor, a raw codec rounds "
              "nothing)");
    FAN_CHECK(req.residual == nullptr, "stochastic rounding: not together with error feedback (pick one)");
    FAN_CHECK(req.prepacked == nullptr, "stochastic rounding: not with prepacked input (the GEMM's encoding rounds to "
                                        "nearest)");
    FAN_CHECK(cfg_.algo == 0, "stochastic rounding: mesh schedule only (the ring schedule is not supported yet)");
    const EngineLayout SL = layout(req.n_valid, req.layout_shard, req.layout_chunks);
    FAN_CHECK(SL.chunks <= 1,
              "stochastic rounding: not with a chunked layout (layout_chunks > 1, or a bucket above chunk_elems)");
    FAN_CHECK(!sharded(req), "stochastic rounding: not with the sharded update (shard_update)");
    FAN_CHECK(world_ <= kMaxPeers, "stochastic rounding: at most 16 ranks (one destination per shard)");
    FAN_CHECK((uint64_t)SL.n_pad < ((uint64_t)1 << 32),
              "stochastic rounding: a padded bucket of 2^32 or more elements (element indices are 32-bit)");
  }
  {
    // the slot this request takes still holds a clipped request: its forced commit would update with a coefficient
    // that does not exist yet (refused before the slot table moves on)
    const int next = table_->next_slot();
    FAN_CHECK(!clip_pending(next, 0), "a clip group holds at most 8 deferred requests (slot " + std::to_string(next) +
                                          " still holds a clipped request: commit_group it first)");
  }
  FAN_HIP_CHECK(hipSetDevice(device_));
  // slot state machine (slot_table.h): the next slot (a still-deferred occupant is committed first, ordered after
  // the producer: the NIC's 8-deep command queue never drops a request), ordering after anything that may still
  // read the slot's buffers, and the stream this request's communication phase runs on
  const SlotTable<HipSlotDevice>::Begin b = table_->begin(producer, req.on_producer && !inline_);
  cur_.run = b.run;
  cur_.producer = producer;
  cur_.slot = b.slot;  // also keys the buffers a deferred epilogue reads (epi_scratch)
  cur_.seq = b.seq;    // the sequence number this request will get
  submitted_++;
  const EngineLayout L = layout(req.n_valid, req.layout_shard, req.layout_chunks);
  SlotExtra& x = extra_[b.slot];
  x.timed = timing_;
  x.counted = false;
  if (x.timed) FAN_HIP_CHECK(hipEventRecord(x.t0, cur_.run));
  const int64_t wb = wire_bytes(L);
  counters_.requests++;
  counters_.logical_bytes += req.n_valid * 4;
  counters_.wire_bytes += wb;
  x.trace = -1;
  if (tracing_) {
    if (trace_used_ < trace_pool_.size()) {
      x.trace = cur_.trace = (int)trace_used_++;
      trace_pool_[cur_.trace].hop_count = 0;
      trace_pool_[cur_.trace].logical_bytes = req.n_valid * 4;
      trace_pool_[cur_.trace].wire_bytes = wb;
      mark(kTpStart);
    } else {
      trace_dropped_++;
    }
  }
  if (req.prepacked) {
    FAN_CHECK(cfg_.codec == kBfpTrunc || cfg_.codec == kBfpRne, "prepacked input needs a BFP codec");
    FAN_CHECK(req.prepacked_elems % 16 == 0 && req.prepacked_elems <= L.n_pad, "bad prepacked_elems");
  }
  if (trust(req)) {
    // one partials segment per region a schedule may hand to make_epilogue: one (mesh), or one per ring
    const int cap = lamb_partials_for(~size_t(0) >> 1), regions = cfg_.algo == 1 ? std::max(1, L.rings) : 1;
    cur_.pairs_cap = cap * regions;
    cur_.partials = reinterpret_cast<double*>(epi_scratch("lamb_partials", (size_t)cur_.pairs_cap * 16));
    cur_.words = req.trust_out ? req.trust_out : reinterpret_cast<float*>(epi_scratch("lamb_words", 16));
  }
  x.clip_words = nullptr;
  if (req.clip_words) {
    const int cap = sumsq_partials_for(~size_t(0) >> 1), regions = cfg_.algo == 1 ? std::max(1, L.rings) : 1;
    cur_.clip_cap = cap * regions;
    cur_.clip_partials = reinterpret_cast<double*>(epi_scratch("clip_partials", (size_t)cur_.clip_cap * 8));
  }
  std::vector<EpiThunk> thunks = cfg_.algo == 0 ? run_mesh(L, req) : run_ring(L, req);
  if (req.clip_words) {
    x.clip_words = req.clip_words;
    x.clip_partials = cur_.clip_partials;
    x.clip_count = cur_.clip_count;  // (0: a request without a valid element contributes nothing)
  }
  if (trust(req)) {
    // the regions' pass-1 launches are enqueued (direct mesh) or in `thunks`; then one ratio over every region's
    // partials in region order, then the regions' pass 2 — all on the one stream the slot table runs a request's
    // thunks on, in this order. A request without a valid element (n_valid == 0) has no region: its ratio launch
    // sums nothing and writes {lr, lr, 1}, so the words are always this request's.
    const double* partials = cur_.partials;
    float* words = cur_.words;
    const int pairs = cur_.pairs;
    const float lr = req.upd.lamb.lr;
    thunks.push_back([=](hipStream_t es) { launch_lamb_ratio(partials, pairs, lr, words, es); });
    for (auto& t : cur_.apply) thunks.push_back(std::move(t));
    cur_.apply.clear();
  }
  FAN_HIP_CHECK(hipGetLastError());
  // phases this schedule does not have (ring hops, the world-1 local path) collapse onto the end of comm
  for (int tp = kTpPacked; tp <= kTpCommEnd; ++tp)
    if (!(cur_.marked & (1u << tp))) mark(tp);
  // verify mode: the device error block's host mirror, refreshed after every request's communication phase
  if (verify_) FAN_HIP_CHECK(hipMemcpyAsync(verr_host_, verr_dev_, sizeof(VerifyError), hipMemcpyDeviceToHost, cur_.run));
  x.t_issue = now_s();
  table_->set_keep_done(b.slot, x.timed || x.trace >= 0);  // timed / traced: a real done point, not a lazy one
  table_->end(b.slot, std::move(thunks), req.defer);  // comm_done, sequence number; an immediate request commits now
  return b.slot;
}

bool AllReduceEngine::clip_pending(int slot, uint32_t seq) const {
  const auto& sl = table_->slot(slot);
  return sl.pending && (seq == 0 || seq == sl.seq) && extra_.at(slot).clip_words != nullptr;
}

static const char* const kClipAlone =
    "a clipped request commits with its clip group only (commit_group): a clip group holds at most 8 deferred "
    "requests, and none updates before the group's coefficient exists";

void AllReduceEngine::commit(int slot, bool after_producer, hipStream_t producer, uint32_t seq) {
  RoctxRange rr("fan/allreduce/epilogue");
  FAN_CHECK(!clip_pending(slot, seq), kClipAlone);
  table_->commit(slot, after_producer, producer, seq);
}

void AllReduceEngine::commit_group(const std::vector<int>& slots, const std::vector<uint32_t>& seqs, double max_norm,
                                   float grad_scale, bool after_producer, hipStream_t producer) {
  RoctxRange rr("fan/allreduce/clip_group");
  const size_t n = slots.size();
  FAN_CHECK(n >= 1 && seqs.size() == n, "commit_group: one sequence number per slot, at least one request");
  FAN_CHECK(n <= (size_t)kSlots, "commit_group: a clip group holds at most 8 deferred requests");
  FAN_CHECK(max_norm > 0.0 && max_norm < __builtin_huge_val(), "commit_group: max_norm must be finite and positive");
  const float* words = nullptr;
  hipStream_t es = nullptr;
  ClipSegments seg{};
  for (size_t i = 0; i < n; ++i) {
    const int s = slots[i];
    FAN_CHECK(s >= 0 && s < kSlots, "commit_group: bad slot");
    for (size_t j = 0; j < i; ++j) FAN_CHECK(slots[j] != s, "commit_group: a slot named twice");
    const auto& sl = table_->slot(s);
    FAN_CHECK(sl.pending && seqs[i] != 0 && sl.seq == seqs[i],
              "commit_group: request " + std::to_string(i) + " (slot " + std::to_string(s) +
                  ") is not pending any more, or its slot holds another request");
    const SlotExtra& x = extra_[s];
    FAN_CHECK(x.clip_words != nullptr, "commit_group: request " + std::to_string(i) + " was not submitted with clip words");
    FAN_CHECK(i == 0 || x.clip_words == words, "commit_group: every request of a clip group names the same clip words");
    const hipStream_t e = table_->epilogue_stream(s, after_producer, producer);
    FAN_CHECK(i == 0 || e == es, "commit_group: the requests' epilogues would run on different streams (an on-producer "
                                 "request beside comm-stream epilogues): one coefficient launch cannot precede them all");
    words = x.clip_words;
    es = e;
    seg.p[i] = x.clip_partials;
    seg.n[i] = x.clip_count;
  }
  FAN_HIP_CHECK(hipSetDevice(device_));
  for (size_t i = 0; i < n; ++i) table_->wait_comm(slots[i], es, seqs[i]);
  launch_clip_coef(seg, (int)n, max_norm, grad_scale, const_cast<float*>(words), es);
  for (size_t i = 0; i < n; ++i) {
    extra_[slots[i]].clip_words = nullptr;  // (the update thunks hold the pointer)
    table_->commit(slots[i], after_producer, producer, seqs[i]);
  }
}

void AllReduceEngine::wait_stream(int slot, hipStream_t s, uint32_t seq) {
  FAN_CHECK(!clip_pending(slot, seq), kClipAlone);
  table_->wait_stream(slot, s, seq);
}

bool AllReduceEngine::query(int slot, uint32_t seq) { return table_->query(slot, seq); }

void AllReduceEngine::set_tracing(bool on, int capacity) {
  tracing_ = on;
  if (P2PComm* d = comm_ ? comm_->direct() : nullptr) d->set_timing(on);  // device stall time of the flag waits
  if (!on) return;
  // a new trace window: wait for the previous window's requests before their events are re-recorded
  for (size_t i = 0; i < trace_used_; ++i) hipEventSynchronize(trace_pool_[i].ev[kTpEpiEnd]);
  hop_used_ = 0;
  while ((int)trace_pool_.size() < capacity) {
    RequestTrace t;
    for (auto& e : t.ev) FAN_HIP_CHECK(hipEventCreate(&e));
    trace_pool_.push_back(t);
  }
  trace_used_ = 0;
  trace_dropped_ = 0;
}

TraceSummary AllReduceEngine::trace_summary() {
  TraceSummary r;
  r.dropped = trace_dropped_;
  for (int s = 0; s < kSlots; ++s)  // traced epilogues still deferred: their end point is not recorded yet
    if (table_->slot(s).pending && extra_[s].trace >= 0)
      throw std::runtime_error("trace_summary: a traced request's epilogue is not committed yet");
  for (size_t i = 0; i < trace_used_; ++i) {
    RequestTrace& t = trace_pool_[i];
    FAN_HIP_CHECK(hipEventSynchronize(t.ev[kTpEpiEnd]));
    float ms = 0.f;
    for (int p = 1; p < kTpCount; ++p) {
      FAN_HIP_CHECK(hipEventElapsedTime(&ms, t.ev[p - 1], t.ev[p]));
      r.ms[p] += ms;
    }
    FAN_HIP_CHECK(hipEventElapsedTime(&ms, t.ev[kTpStart], t.ev[kTpCommEnd]));
    r.comm_ms += ms;
    FAN_HIP_CHECK(hipEventElapsedTime(&ms, t.ev[kTpStart], t.ev[kTpEpiEnd]));
    r.total_ms += ms;
    r.requests++;
    r.logical_bytes += t.logical_bytes;
    r.wire_bytes += t.wire_bytes;
    for (size_t h = 0; h + 3 < t.hop_count; h += 4) {
      const hipEvent_t* e = &hop_pool_[t.hop_first + h];
      float a = 0.f, b = 0.f, c = 0.f;
      FAN_HIP_CHECK(hipEventElapsedTime(&a, e[0], e[1]));
      FAN_HIP_CHECK(hipEventElapsedTime(&b, e[1], e[2]));
      FAN_HIP_CHECK(hipEventElapsedTime(&c, e[2], e[3]));
      r.hop_rounds++;
      r.hop_credit_ms += a;
      r.hop_kernel_ms += t.hop_kernel_first ? b : c;
      r.hop_ready_ms += t.hop_kernel_first ? c : b;
      r.hop_max_ms = std::max<double>(r.hop_max_ms, (double)a + b + c);
    }
  }
  return r;
}

void AllReduceEngine::count_peers(size_t bytes, P2PComm* direct) {
  if (counters_.peer_bytes.size() != (size_t)world_) counters_.peer_bytes.assign(world_, 0);
  for (int p = 0; p < world_; ++p) {
    if (p == rank_) continue;
    counters_.peer_bytes[p] += (int64_t)bytes;
    if (direct) direct->count_sent(p, bytes);  // the P2P transport's own count (its copies count themselves)
  }
}

std::string AllReduceEngine::debug_status() {
  std::ostringstream os;
  os << "{\"rank\": " << rank_ << ", \"world\": " << world_ << ", \"algo\": \"" << (cfg_.algo ? "ring" : "mesh")
     << "\", \"codec\": " << cfg_.codec << ", \"inline\": " << (inline_ ? "true" : "false")
     << ", \"verify\": " << (verify_ ? "true" : "false") << ", \"requests\": " << submitted_
     << ", \"next_slot\": " << table_->next_slot() << ", \"slots\": [";
  for (int i = 0; i < kSlots; ++i) {
    const auto& sl = table_->slot(i);
    os << (i ? ", " : "") << "{\"slot\": " << i << ", \"seq\": " << sl.seq << ", \"pending\": "
       << (sl.pending ? "true" : "false") << ", \"done_word\": ";
    // host-mapped done words are written only with FAN_DONE_WORDS=1: otherwise report the done event's state
    if (table_->done_words()) os << flags_host_[i * 16];
    else os << "null";
    const int dn = table_->peek_done(i);
    os << ", \"done\": " << (dn < 0 ? "null" : dn ? "true" : "false")
       << ", \"epilogue_stream\": \""
       << (!sl.used || sl.pending ? "none"
           : sl.epi_stream == stream_ ? "comm"
           : (epi_stream_ && sl.epi_stream == epi_stream_) ? "side"
                                                             : "producer")
       << "\", \"age_s\": " << (sl.seq ? now_s() - extra_[i].t_issue : 0.0) << "}";
  }
  os << "], \"forced_commits\": " << counters_.forced_commits << ", \"direct_rounds\": " << counters_.direct_rounds
     << ", \"peer_bytes\": [";
  for (size_t p = 0; p < counters_.peer_bytes.size(); ++p) os << (p ? ", " : "") << counters_.peer_bytes[p];
  std::string err = comm_ ? comm_->async_error() : "";
  for (char& ch : err)
    if (ch == '"' || ch == '\\') ch = '\'';
  os << "], \"comm_error\": \"" << err << "\"";
  if (comm_) os << ", \"comm_kind\": \"" << comm_->kind() << "\", \"comm_ranks\": " << comm_->ranks_seen();
  if (verify_) os << ", \"verify_error\": " << (verr_host_->flag ? "true" : "false");
  if (P2PComm* d = comm_ ? comm_->direct() : nullptr) {
    // never blocks on the (possibly parked) streams: completed timed waits only, flag copy bounded by 2 s
    const P2PComm::Stats st = d->stats(false);
    os << ", \"p2p\": {\"sequence\": " << d->sequence() << ", \"ready_waits\": " << st.ready_waits
       << ", \"credit_waits\": " << st.credit_waits << ", \"timed_waits\": " << st.timed_waits
       << ", \"ready_stall_ms\": " << st.ready_stall_ms << ", \"credit_stall_ms\": " << st.credit_stall_ms
       << ", \"flags\": ";
    const std::vector<uint64_t> f = d->flags_snapshot(2.0);
    if (f.empty()) {
      os << "null, \"flags_error\": \"flag snapshot copy did not complete within 2 s\"";
    } else {
      os << "[";
      for (size_t i = 0; i < f.size(); ++i) os << (i ? ", " : "") << f[i];
      os << "]";
    }
    os << "}";
  }
  os << "}";
  return os.str();
}

std::string AllReduceEngine::diagnostics(int slot) const {
  const auto& sl = table_->slot(slot);
  std::ostringstream os;
  os << "rank=" << rank_ << " world=" << world_ << " algo=" << (cfg_.algo ? "ring" : "mesh") << " codec=" << cfg_.codec
     << " slot=" << slot << " seq=" << sl.seq
     << (table_->done_words() ? " done_word=" + std::to_string(flags_host_[slot * 16])
                              : std::string(" done_word=unwritten(FAN_DONE_WORDS=0)"))
     << " elapsed=" << (now_s() - extra_.at(slot).t_issue) << "s";
  if (comm_) os << " rccl_async_error='" << comm_->async_error() << "'";
  return os.str();
}

void AllReduceEngine::synchronize(int slot, double timeout_s, uint32_t seq) {
  FAN_CHECK(!clip_pending(slot, seq), kClipAlone);
  table_->commit_for_host_wait(slot, seq);
  const double t0 = now_s();
  const double tmo = timeout_s > 0 ? timeout_s : cfg_.timeout_s;
  int spins = 0;
  struct WaitAccount {  // host stall accounting on every exit path (including the timeout throw)
    EngineCounters& c;
    const double t0;
    const int& spins;
    ~WaitAccount() {
      if (spins > 0) {
        c.host_waits++;
        c.host_spins += (uint64_t)spins;
        c.host_wait_s += now_s() - t0;
      }
    }
  } account{counters_, t0, spins};
  while (!query(slot, seq)) {
    if (++spins > 64) {
      std::this_thread::sleep_for(std::chrono::microseconds(spins > 4096 ? 200 : 5));
      if (comm_ && (spins & 255) == 0) {
        const std::string e = comm_->async_error();
        if (!e.empty()) throw std::runtime_error("all-reduce failed: " + e + " [" + diagnostics(slot) + "]");
      }
      if (now_s() - t0 > tmo) {
        const std::string d = diagnostics(slot);
        if (comm_) comm_->abort();
        throw std::runtime_error("all-reduce timed out after " + std::to_string(tmo) + "s [" + d + "]");
      }
    }
  }
  check_verify();  // verify mode: surface a mismatch recorded while this request ran
}

void AllReduceEngine::verify_rows(const uint8_t* rows, size_t row_bytes, int nrows, const uint32_t* recv_tags,
                                  uint32_t site, uint32_t row_base, hipStream_t st) {
  launch_msg_verify(rows, row_bytes, row_bytes, nrows, recv_tags, cur_.seq, tag_region(2), verr_dev_, site, row_base,
                    st);
  counters_.verified_rows += (uint64_t)nrows;
}

void AllReduceEngine::check_verify() {
  if (!verify_ || verr_host_->flag == 0) return;
  static const char* sites[] = {"?", "mesh all_to_all", "mesh all_gather", "ring round", "mesh direct send",
                                "mesh direct gather", "ring direct hop", "mesh weight all_gather"};
  const VerifyError e = *verr_host_;
  std::ostringstream os;
  os << "verify: message " << (e.kind == 1 ? "corrupted" : "out of sequence (dropped or reordered)") << " in "
     << sites[e.site < sizeof(sites) / sizeof(*sites) ? e.site : 0] << " row " << e.row << " (checksum " << e.got_s1
     << " vs tag " << e.exp_s1 << ", request " << e.got_seq << " vs expected " << e.exp_seq << ") [rank=" << rank_ << " world=" << world_ << "]";
  throw std::runtime_error(os.str());
}

float AllReduceEngine::latency_ms(int slot) {
  SlotExtra& sl = extra_.at(slot);
  if (!sl.timed) return -1.f;
  synchronize(slot);
  float ms = 0.f;
  FAN_HIP_CHECK(hipEventElapsedTime(&ms, sl.t0, sl.t1));
  if (!sl.counted) {
    sl.counted = true;
    counters_.device_ms += ms;
    counters_.timed_requests++;
  }
  return ms;
}

}  // namespace fan
