// qmps_hazard.h - which launches of the fused D = 4 energy kernel may run side by side on the two compute lanes of a context, stated
// in one place and free of HIP (a host compiler takes this header alone: tests/csrc/hazard_check.cpp runs it against brute force):
//   LaunchFootprint   what one launch reads and writes
//   hazard_conflict   two footprints that may not overlap in time (RAW, WAR or WAW on some word)
//   LaneTable         the recent launches of both lanes, and which of them the next launch has to wait for
// The context (qmps_ctx.h) keeps one LaneTable and an event per entry; it turns the table's answers into hipStreamWaitEvent.
#pragma once
#include <stdint.h>

// One launch of energy_direct_d4_kernel over the window [lo, hi) of the resident evaluations:
//   reads   the window's tensors or parameter rows, h, and - warm start - the window's environments
//   writes  the window's E, iteration counts and statuses (always), its environments (unless QMPS_FLAG_NO_ENV_OUT)
//   adds    to the cost accumulator of ring position `acc`, clears that of ring position `acc_zero` for a later step (-1: none)
//   writes  the context's one array of per-wave partial sums when the cost is not accumulated (partials)
// Every launch writes E / iters / status over its whole window, so two launches whose windows share an evaluation conflict whatever
// they do with the environments; what the window's environments add (a warm start behind a launch that stores them, two launches
// that store them) is a subset of that.  Tensors, parameter rows and h are written by setters only, which join both lanes.
struct LaunchFootprint {
  int64_t lo = 0, hi = 0;
  int acc = -1;
  int acc_zero = -1;
  bool partials = false;
};

inline bool hazard_conflict(const LaunchFootprint& a, const LaunchFootprint& b) {
  if (a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi) return true;
  if (a.partials && b.partials) return true;
  const int wa[2] = {a.acc, a.acc_zero}, wb[2] = {b.acc, b.acc_zero};      // (an add and a clear both write the position)
  for (int x : wa)
    for (int y : wb)
      if (x >= 0 && x == y) return true;
  return false;
}

// The launches of the two lanes.  A lane is a stream: its launches run in the order they were issued, and launch number s of a
// lane (s = 1, 2, ..) is followed by an event, kept while the lane's newest kDepth launches include s.  ordered_after[l] = n says
// lane l already waits for the other lane's launch n, and so for every earlier one.  The order of calls for a launch on `lane`:
//   s = must_wait(lane, f)    s > 0: the lane waits for the other lane's event s, then waited(lane, s)
//   s = evicts(lane)          s > 0: the OTHER lane waits for this lane's event s - about to be recorded anew -, then waited(other, s)
//   the kernel;  s = record(lane, f);  the event of (lane, s) is recorded
// join(l): lane l waits for all of the other lane (its newest event), for work that is no such launch.
struct LaneTable {
  static constexpr int kLanes = 2, kDepth = 16;
  LaunchFootprint ring[kLanes][kDepth];
  int64_t issued[kLanes] = {0, 0};
  int64_t ordered_after[kLanes] = {0, 0};

  static int slot_of(int64_t s) { return (int)(s % kDepth); }
  bool kept(int lane, int64_t s) const { return s >= 1 && s <= issued[lane] && issued[lane] - s < kDepth; }
  // the other lane's newest launch that conflicts with f and that `lane` does not follow yet (0: none).  Launches that have left
  // the ring are followed already: evicts() saw to that when they left.
  int64_t must_wait(int lane, const LaunchFootprint& f) const {
    const int other = 1 - lane;
    for (int64_t s = issued[other]; s > ordered_after[lane] && kept(other, s); --s)
      if (hazard_conflict(ring[other][slot_of(s)], f)) return s;
    return 0;
  }
  // the launch whose ring entry and event the next record(lane, ..) takes over, if the other lane does not follow it yet (0: none)
  int64_t evicts(int lane) const {
    const int64_t s = issued[lane] + 1 - kDepth;
    return s >= 1 && ordered_after[1 - lane] < s ? s : 0;
  }
  void waited(int lane, int64_t s) {
    if (s > ordered_after[lane]) ordered_after[lane] = s;
  }
  int64_t record(int lane, const LaunchFootprint& f) {
    const int64_t s = ++issued[lane];
    ring[lane][slot_of(s)] = f;
    return s;
  }
  // the other lane's newest launch, if `lane` does not follow it yet (0: nothing to wait for)
  int64_t join(int lane) const { return issued[1 - lane] > ordered_after[lane] ? issued[1 - lane] : 0; }
};

// The waits in front of a launch and in front of everything else, over whatever carries them out - the context with HIP streams and
// events (qmps_capi.hip), the host test with a model of them:
//   io.wait(waiter, lane, s)   lane `waiter` waits for the event of launch s of `lane`;  0, or an error code that is handed on
//   io.fork()                  lane 1 waits for the context stream (lane 0's stream: its launches and everything else) as it stands
// main_touched: the context stream carries work lane 1 does not follow yet.
template <class IO>
int lanes_begin(LaneTable& t, IO& io, int lane, const LaunchFootprint& f, bool& main_touched) {
  const int other = 1 - lane;
  if (lane == 1 && main_touched) {
    if (int rc = io.fork()) return rc;
    t.waited(1, t.issued[0]);
    main_touched = false;
  }
  if (const int64_t s = t.must_wait(lane, f)) {
    if (int rc = io.wait(lane, other, s)) return rc;
    t.waited(lane, s);
  }
  if (const int64_t s = t.evicts(lane)) {
    if (int rc = io.wait(other, lane, s)) return rc;
    t.waited(other, s);
  }
  return 0;
}

// everything that is no lane launch runs on the context stream behind this
template <class IO>
int lanes_join(LaneTable& t, IO& io, bool& main_touched) {
  if (const int64_t s = t.join(0)) {
    if (int rc = io.wait(0, 1, s)) return rc;
    t.waited(0, s);
  }
  main_touched = true;
  return 0;
}
