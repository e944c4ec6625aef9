// qmps_knobs.h - the ONLY place where libqmps_hip reads the environment.
//
// documented_switch: kernel-selection switches that are part of the library's documented behaviour (include/qmps_hip.h,
//   section "environment switches"): they select between two implementations of the SAME computation and exist so that the
//   test-suite can run both against the oracle.
// tuning_knob: thresholds and schedules that were swept while tuning (profiles/EXPERIMENTS.md).  They are compiled in only
//   with -DQMPS_DEBUG_KNOBS (make EXTRA=-DQMPS_DEBUG_KNOBS); the shipped library ignores them.
#pragma once
#include <stdlib.h>

namespace qmps {

inline const char* documented_switch(const char* name) { return getenv(name); }

inline const char* tuning_knob(const char* name) {
#ifdef QMPS_DEBUG_KNOBS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// QMPS_LAUNCH_LANES (documented switch, read when a context is created): compute streams that consecutive launches of the fused
// D = 4 energy kernel alternate between (qmps_hazard.h); 1 = every launch on the context stream.
constexpr int kLaunchLanes = 2;
inline int launch_lanes() {
  const char* e = documented_switch("QMPS_LAUNCH_LANES");
  const int n = e ? atoi(e) : kLaunchLanes;
  return n >= 2 ? 2 : 1;
}

}  // namespace qmps
