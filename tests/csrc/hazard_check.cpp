// hazard_check.cpp - qmps_amd/csrc/qmps_hazard.h on the host, as a stand-alone program (tests/test_launch_hazards_cpu.py builds it under
// the sanitizers and runs it):
//   1. hazard_conflict against brute force: every footprint over windows inside [0, 6) - with and without a warm start, with and
//      without stored environments, every accumulator position of a ring of three - as the sets of words it reads and writes; two
//      launches conflict when one writes a word the other reads or writes.
//   2. LaneTable, lanes_begin and lanes_join against a model of two in-order streams with events: random sequences of lane launches
//      and of other work on the context stream.  Whatever a launch conflicts with - any earlier launch, however far back - must have
//      completed before it by the streams' order and the waits issued; other work runs behind every launch, every launch behind all
//      earlier other work; and no wait may read an event that a later launch has taken over.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <bitset>
#include <random>
#include <vector>

#include "qmps_hazard.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                    \
  do {                                      \
    if (!(cond)) {                          \
      if (++failures <= 20) {               \
        printf("FAILED %s: ", #cond);       \
        printf(__VA_ARGS__);                \
        printf("\n");                       \
      }                                     \
    }                                       \
  } while (0)

constexpr int kEvals = 6, kRingPositions = 3;      // the enumeration;  the random sequences: kModelEvals evaluations
constexpr int kModelEvals = 80;

// a launch as the test states it: the footprint the library sees, and what it does with the window's environments
struct Launch {
  LaunchFootprint f;
  bool env_read = false, env_write = false;
};

// the words of a launch as bit sets, n evaluations in all: [0, n) tensors / parameter rows, [n, 2n) E / iters / status, [2n, 3n)
// environments, then the accumulator positions and the partial sums
struct Words {
  std::bitset<3 * kModelEvals + kRingPositions + 1> reads, writes;
};
Words words_of(const Launch& l, int n) {
  Words w;
  for (int64_t i = l.f.lo; i < l.f.hi; ++i) {
    w.reads.set(i);
    w.writes.set(n + i);
    if (l.env_read) w.reads.set(2 * n + i);
    if (l.env_write) w.writes.set(2 * n + i);
  }
  if (l.f.acc >= 0) w.writes.set(3 * n + l.f.acc);
  if (l.f.acc_zero >= 0) w.writes.set(3 * n + l.f.acc_zero);
  if (l.f.partials) w.writes.set(3 * n + kRingPositions);
  return w;
}
bool brute_conflict(const Words& x, const Words& y) { return (x.writes & (y.reads | y.writes)).any() || (y.writes & x.reads).any(); }
bool brute_conflict(const Launch& a, const Launch& b, int n) { return brute_conflict(words_of(a, n), words_of(b, n)); }

std::vector<Launch> every_launch() {
  std::vector<Launch> v;
  for (int lo = 0; lo <= kEvals; ++lo)
    for (int hi = lo; hi <= kEvals; ++hi)
      for (int env = 0; env < 4; ++env)
        for (int acc = -1; acc < kRingPositions; ++acc)
          for (int zero = -1; zero < kRingPositions; ++zero)
            for (int partials = 0; partials < 2; ++partials) {
              if (acc >= 0 && partials) continue;      // (the cost goes to the accumulator OR to the partial sums)
              if (acc < 0 && zero >= 0) continue;      // (only an accumulating launch clears a position)
              Launch l;
              l.f.lo = lo; l.f.hi = hi; l.f.acc = acc; l.f.acc_zero = zero; l.f.partials = partials != 0;
              l.env_read = (env & 1) != 0; l.env_write = (env & 2) != 0;
              v.push_back(l);
            }
  return v;
}

void conflicts_against_brute_force() {
  const std::vector<Launch> all = every_launch();
  long pairs = 0, conflicting = 0;
  for (const Launch& a : all)
    for (const Launch& b : all) {
      const bool want = brute_conflict(a, b, kEvals), got = hazard_conflict(a.f, b.f);
      ++pairs;
      conflicting += want;
      CHECK(got == want, "[%lld,%lld) acc %d zero %d partials %d env %d%d  against  [%lld,%lld) acc %d zero %d partials %d env %d%d: brute force %d",
            (long long)a.f.lo, (long long)a.f.hi, a.f.acc, a.f.acc_zero, a.f.partials, a.env_read, a.env_write, (long long)b.f.lo, (long long)b.f.hi,
            b.f.acc, b.f.acc_zero, b.f.partials, b.env_read, b.env_write, want);
      CHECK(hazard_conflict(b.f, a.f) == got, "not symmetric");
    }
  printf("hazard_conflict: %zu footprints, %ld pairs, %ld of them conflicting: %s\n", all.size(), pairs, conflicting,
         failures ? "DISAGREES with brute force" : "agrees with brute force");
}

// Two in-order streams with events.  done[s][l] = n: whatever stream s is given from now on starts after launch n of lane l (and all
// earlier ones) has completed; done[s][2] the same for the other work of the context stream.  An event carries the `done` of its
// stream at the time it was recorded.
struct Model {
  static constexpr int kMain = 2;
  int64_t done[2][3] = {};
  int64_t main_ops = 0;
  struct Event {
    int64_t seq = 0;
    int64_t done[3] = {};
  };
  Event ev[2][LaneTable::kDepth];
  LaneTable* t = nullptr;
  void absorb(int stream, const int64_t* d) {
    for (int k = 0; k < 3; ++k)
      if (d[k] > done[stream][k]) done[stream][k] = d[k];
  }
  int wait(int waiter, int lane, int64_t s) {
    const Event& e = ev[lane][LaneTable::slot_of(s)];
    CHECK(e.seq == s, "lane %d waits for launch %lld of lane %d, but the event holds launch %lld", waiter, (long long)s, lane, (long long)e.seq);
    absorb(waiter, e.done);
    return 0;
  }
  int fork() {      // lane 1 behind the context stream: lane 0's launches so far, the other work so far, and what that stream waited for
    int64_t d[3] = {t->issued[0], done[0][1], main_ops};
    absorb(1, d);
    return 0;
  }
  void record(int lane, int64_t s) {
    done[lane][lane] = s;
    if (lane == 0) done[0][kMain] = main_ops;      // (lane 0 IS the context stream)
    Event& e = ev[lane][LaneTable::slot_of(s)];
    e.seq = s;
    for (int k = 0; k < 3; ++k) e.done[k] = done[lane][k];
  }
};

void lanes_against_the_model(unsigned seed, int ops, bool alternate, long* launches, long* waits_needed) {
  std::mt19937 rng(seed);
  LaneTable t;
  Model m;
  m.t = &t;
  bool main_touched = false;
  int next_lane = 0;
  struct Past {
    Words w;
    int lane;
    int64_t seq;
  };
  std::vector<Past> past;
  // 1: the same window every step;  3, 9, 33: cycles - the longer ones meet no conflict while a lane's ring turns over, so launches leave
  // the ring unseen by the other lane;  40 windows drawn at random
  const int choices[5] = {1, 3, 9, 33, 40};
  const int n_windows = choices[rng() % 5];
  const bool cycle = n_windows != 40 && rng() % 2 != 0;
  const bool accumulate = rng() % 4 != 0;
  const int rates[3] = {0, 16, 64};
  const int other_every = rates[rng() % 3];      // other work on the context stream: never, or every 16th / 64th operation
  int step = 0;
  int64_t groups = rng() % 8;
  for (int op = 0; op < ops; ++op) {
    if (other_every > 0 && rng() % other_every == 0) {
      // other work on the context stream: behind every launch so far
      CHECK(lanes_join(t, m, main_touched) == 0, "join failed");
      m.done[0][0] = t.issued[0];
      CHECK(m.done[0][1] == t.issued[1], "other work starts with launch %lld of lane 1 complete, %lld issued", (long long)m.done[0][1], (long long)t.issued[1]);
      CHECK(main_touched, "main_touched not set");
      ++m.main_ops;
      continue;
    }
    Launch l;
    const int w = cycle ? step++ % n_windows : (int)(rng() % n_windows);
    l.f.lo = 2 * w; l.f.hi = 2 * w + 1 + (int)(rng() % 8 == 0 ? 2 : rng() % 2);      // (windows of two evaluations, some reaching into the next)
    if (l.f.hi > kModelEvals) l.f.hi = kModelEvals;
    if (accumulate && n_windows <= 3) {
      l.f.acc = (int)(groups % kRingPositions);
      l.f.acc_zero = (int)((groups + 2) % kRingPositions);
      groups += rng() % 2;
    } else if (n_windows <= 3) {
      l.f.partials = rng() % 2 != 0;
    }      // (the long cycles: windows alone, so that conflicts are rare)
    l.env_read = rng() % 2 != 0; l.env_write = rng() % 2 != 0;
    const int lane = alternate ? next_lane : (int)(rng() % 2);
    next_lane = 1 - lane;
    CHECK(lanes_begin(t, m, lane, l.f, main_touched) == 0, "begin failed");
    if (lane == 0) { m.done[0][0] = t.issued[0]; m.done[0][Model::kMain] = m.main_ops; }      // (its own stream's order)
    else m.done[1][1] = t.issued[1];
    const Words mine = words_of(l, kModelEvals);
    for (const Past& p : past)
      if (brute_conflict(p.w, mine)) {
        ++*waits_needed;
        CHECK(m.done[lane][p.lane] >= p.seq, "op %d: launch on lane %d conflicts with launch %lld of lane %d, of which %lld are complete", op, lane,
              (long long)p.seq, p.lane, (long long)m.done[lane][p.lane]);
      }
    CHECK(m.done[lane][Model::kMain] == m.main_ops, "op %d: launch on lane %d starts with %lld of %lld pieces of other work complete", op, lane,
          (long long)m.done[lane][Model::kMain], (long long)m.main_ops);
    // what the table believes must hold in the model
    CHECK(m.done[lane][1 - lane] >= t.ordered_after[lane], "ordered_after[%d] = %lld, the model has %lld", lane, (long long)t.ordered_after[lane],
          (long long)m.done[lane][1 - lane]);
    const int64_t s = t.record(lane, l.f);
    m.record(lane, s);
    past.push_back({mine, lane, s});
    ++*launches;
  }
}

}  // namespace

int main() {
  conflicts_against_brute_force();
  long launches = 0, needed = 0;
  const int sequences = 400, ops = 300;
  for (int k = 0; k < sequences; ++k) lanes_against_the_model(1000 + k, ops, k % 2 == 0, &launches, &needed);
  printf("LaneTable: %d sequences x %d operations, %ld launches, %ld conflicting pairs: %s\n", sequences, ops, launches, needed,
         failures ? "a launch could overtake what it conflicts with" : "every launch behind what it conflicts with");
  if (failures) printf("%d checks FAILED\n", failures);
  return failures ? 1 : 0;
}
