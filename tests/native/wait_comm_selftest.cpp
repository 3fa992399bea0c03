// Host-only self-test of SlotTable::wait_comm / epilogue_stream (csrc/comm/slot_table.h), the two calls a clip
// group's commit adds to the request-slot state machine (AllReduceEngine::commit_group): built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_clip_native_selftest.py.
//
// The table runs against a simulated device (FIFO streams; a wait binds to the event's latest record when it is
// enqueued; the "GPU" executes the heads of random runnable streams in random order, as in slot_table_selftest.cpp).
// In every engine mode, groups of 1..8 deferred requests (from two producer streams, some on the producer stream
// itself) are committed the way commit_group does it: the members' common epilogue stream, wait_comm for each, one
// "coefficient" work item on that stream, then commit for each. Checked on every run:
//   G1 the coefficient runs after every member's communication phase;
//   G2 every member's epilogue runs after the coefficient, after its producer's work enqueued before the commit, once;
//   G3 epilogue_stream names the stream commit then uses; wait_comm does nothing for a committed or superseded handle;
//   G4 the device always drains, and the next requests on the same slots are not disturbed.
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "comm/slot_table.h"

using namespace fan;

static int failures = 0;
#define EXPECT(c, ...)                                            \
  do {                                                            \
    if (!(c)) {                                                   \
      if (failures < 30) {                                        \
        std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        std::fprintf(stderr, __VA_ARGS__);                        \
        std::fprintf(stderr, "\n");                               \
      }                                                           \
      ++failures;                                                 \
    }                                                             \
  } while (0)

struct Op {
  enum Kind { kRecord, kWait, kWrite, kWork } kind;
  int ev = -1;
  long inst = 0;
  int slot = -1;
  uint32_t seq = 0;
  long work = -1;
};

struct SimDevice {
  using Stream = int;
  using Event = int;
  std::vector<std::vector<Op>> q;
  std::vector<size_t> head;
  std::map<int, long> last_record;
  std::set<long> done_inst;
  long next_inst = 1, clock = 0, waits = 0;
  uint32_t words[8] = {};
  std::map<long, long> work_time;
  std::map<long, int> work_runs;
  explicit SimDevice(int ns) : q(ns), head(ns, 0) {}
  void record(Event e, Stream s) {
    Op o{Op::kRecord};
    o.ev = e;
    o.inst = next_inst++;
    last_record[e] = o.inst;
    q.at(s).push_back(o);
  }
  void wait(Stream s, Event e) {
    Op o{Op::kWait};
    o.ev = e;
    auto it = last_record.find(e);
    o.inst = it == last_record.end() ? 0 : it->second;
    q.at(s).push_back(o);
    ++waits;
  }
  bool query(Event e) {
    auto it = last_record.find(e);
    return it == last_record.end() || done_inst.count(it->second) > 0;
  }
  void write_done(Stream s, int slot, uint32_t seq) {
    Op o{Op::kWrite};
    o.slot = slot;
    o.seq = seq;
    q.at(s).push_back(o);
  }
  uint32_t read_done(int slot) { return words[slot]; }
  void work(Stream s, long id) {
    Op o{Op::kWork};
    o.work = id;
    q.at(s).push_back(o);
  }
  bool runnable(size_t s) const {
    if (head[s] >= q[s].size()) return false;
    const Op& o = q[s][head[s]];
    return o.kind != Op::kWait || o.inst == 0 || done_inst.count(o.inst) > 0;
  }
  bool step(std::mt19937& rng) {
    std::vector<size_t> r;
    for (size_t s = 0; s < q.size(); ++s)
      if (runnable(s)) r.push_back(s);
    if (r.empty()) return false;
    const size_t s = r[rng() % r.size()];
    const Op& o = q[s][head[s]++];
    ++clock;
    if (o.kind == Op::kRecord) done_inst.insert(o.inst);
    if (o.kind == Op::kWrite) words[o.slot] = o.seq;
    if (o.kind == Op::kWork) {
      work_time[o.work] = clock;
      work_runs[o.work]++;
    }
    return true;
  }
  bool drained() const {
    for (size_t s = 0; s < q.size(); ++s)
      if (head[s] < q[s].size()) return false;
    return true;
  }
};

static constexpr int P0 = 0, P1 = 1, COMM = 2, SIDE = 3;
using Table = SlotTable<SimDevice>;

struct Member {
  int slot;
  uint32_t seq;
  long comm, epi, before;  // work ids: communication phase, epilogue, producer work enqueued before the commit
};

// modes: 0 inline (lazy done), 1 inline (eager done), 2 inline + side epilogues, 3 multi-rank, epilogue on the comm
// stream, 4 multi-rank, epilogue on the producer (lazy done), 5 the same, eager done, 6 as 4 without wait elision
static void run_case(int mode, unsigned seed) {
  std::mt19937 rng(seed);
  SimDevice dev(4);
  Table::Config cfg;
  cfg.inline_mode = mode <= 2;
  cfg.lazy_done = mode != 1 && mode != 5;
  cfg.side_epi = mode == 2;
  cfg.epi_on_producer = mode >= 4;
  cfg.elide_waits = mode != 6;
  cfg.done_words = (seed & 1) != 0;
  cfg.comm = COMM;
  cfg.side = SIDE;
  std::vector<int> events(Table::kSlots * 4);
  for (size_t i = 0; i < events.size(); ++i) events[i] = (int)i;
  Table table(dev, cfg, events);
  if (seed % 3 == 0) table.set_seq(0xFFFFFFF0u);  // across the 32-bit wrap-around
  long next_work = 1;
  int forced = 0;
  table.on_forced_commit = [&](int) { ++forced; };
  for (int round = 0; round < 6; ++round) {
    const int k = 1 + (int)(rng() % Table::kSlots);
    // one producer per group in the modes whose epilogue stream is the request's own or its producer's: the members
    // of a group must resolve to one epilogue stream (commit_group refuses the rest)
    const int producer = (rng() & 1) ? P0 : P1;
    std::vector<Member> group;
    for (int i = 0; i < k; ++i) {
      // multi-rank, epilogue on the producer: some members run their communication phase on the producer itself
      const bool on_prod = mode >= 4 && rng() % 3 == 0;
      const Table::Begin b = table.begin(producer, on_prod);
      Member m{b.slot, b.seq, next_work++, next_work++, 0};
      dev.work(b.run, m.comm);
      const long epi = m.epi;
      const uint32_t seq = table.end(b.slot, {[&dev, epi](int st) { dev.work(st, epi); }}, true);
      EXPECT(seq == m.seq, "sequence number");
      group.push_back(m);
      for (int j = (int)(rng() % 3); j > 0; --j) dev.step(rng);
    }
    for (Member& m : group) {
      m.before = next_work++;
      dev.work(producer, m.before);
    }
    // the group commit
    const int es = table.epilogue_stream(group[0].slot, true, producer);
    for (const Member& m : group)
      EXPECT(table.epilogue_stream(m.slot, true, producer) == es, "mode %d: one epilogue stream", mode);
    const long waits0 = dev.waits;
    for (const Member& m : group) table.wait_comm(m.slot, es, m.seq);
    if (cfg.inline_mode && !cfg.side_epi) EXPECT(dev.waits == waits0, "inline: wait_comm enqueues nothing");
    const long coef = next_work++;
    dev.work(es, coef);
    for (const Member& m : group) {
      table.wait_comm(m.slot, es, m.seq + 1u == 0 ? 1u : m.seq + 1u);  // G3: another request's handle: nothing
      table.commit(m.slot, true, producer, m.seq);
      EXPECT(!table.slot(m.slot).pending, "committed");
      EXPECT(table.slot(m.slot).epi_stream == es, "mode %d: epilogue_stream named another stream", mode);
      const long w = dev.waits;
      table.wait_comm(m.slot, es, m.seq);  // G3: committed: nothing
      EXPECT(dev.waits == w, "wait_comm on a committed request");
    }
    for (int j = (int)(rng() % 40); j > 0; --j) dev.step(rng);
    // an ordinary immediate request in between (G4)
    const Table::Begin b = table.begin(producer);
    const long c2 = next_work++, e2 = next_work++;
    dev.work(b.run, c2);
    table.end(b.slot, {[&dev, e2](int st) { dev.work(st, e2); }}, false);
    while (dev.step(rng)) {
    }
    EXPECT(dev.drained(), "mode %d seed %u: device did not drain", mode, seed);
    for (const Member& m : group) {
      EXPECT(dev.work_time.count(coef) && dev.work_time[m.comm] < dev.work_time[coef],
             "mode %d seed %u: G1 coefficient before a member's communication phase", mode, seed);
      EXPECT(dev.work_runs[m.epi] == 1, "mode %d: G2 epilogue ran %d times", mode, dev.work_runs[m.epi]);
      EXPECT(dev.work_time[coef] < dev.work_time[m.epi], "mode %d seed %u: G2 epilogue before the coefficient", mode,
             seed);
      EXPECT(dev.work_time[m.before] < dev.work_time[m.epi], "mode %d seed %u: G2 epilogue before producer work", mode,
             seed);
      EXPECT(dev.work_time[m.comm] < dev.work_time[m.epi], "mode %d: epilogue before its communication phase", mode);
    }
    EXPECT(dev.work_runs[e2] == 1 && dev.work_time[c2] < dev.work_time[e2], "mode %d: the ordinary request", mode);
  }
  EXPECT(forced == 0, "a group of at most 8 never forces a commit");
}

int main() {
  for (int mode = 0; mode <= 6; ++mode)
    for (unsigned seed = 1; seed <= 60; ++seed) run_case(mode, seed * 7919u + (unsigned)mode);
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("wait_comm self-test OK\n");
  return 0;
}
