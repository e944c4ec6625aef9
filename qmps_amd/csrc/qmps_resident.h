// qmps_resident.h - what a context holds resident, stated in one place and free of HIP (a host compiler takes this header alone:
// tests/csrc/resident_check.cpp runs it under the sanitizers):
//   qmps_slots       which evaluations of a resident array hold what a launch or a setter left there
//   ResidentStates   what d_A / d_params hold: how many states, as tensors or as ansatz parameters, in whose parameter rows
// The context (qmps_ctx.h) has one ResidentStates, `states`, and a qmps_slots per kind of result.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

// Which evaluations of a resident array hold what a context-wide flag used to claim for all of them: a short list of disjoint
// half-open intervals [lo, hi), sorted.  Launches and read-backs are windowed (qmps_set_window), so the facts about d_r, d_E, d_iters
// and d_status are kept per slot: a launch adds its window, a call that overwrites or outdates slots removes them.
struct qmps_slots {
  std::vector<std::pair<int64_t, int64_t>> v;
  void clear() { v.clear(); }
  bool any() const { return !v.empty(); }
  bool touches(int64_t lo, int64_t hi) const {      // (an empty range touches nothing)
    if (hi <= lo) return false;
    for (const auto& s : v)
      if (s.second > lo && s.first < hi) return true;
    return false;
  }
  void remove(int64_t lo, int64_t hi) {
    if (hi <= lo || !touches(lo, hi)) return;      // (the common case on the hot path: nothing to do, nothing allocated)
    std::vector<std::pair<int64_t, int64_t>> out;
    for (const auto& s : v) {
      if (s.second <= lo || s.first >= hi) { out.push_back(s); continue; }
      if (s.first < lo) out.push_back({s.first, lo});
      if (s.second > hi) out.push_back({hi, s.second});
    }
    v.swap(out);
  }
  void add(int64_t lo, int64_t hi) {
    if (hi <= lo || covers(lo, hi)) return;        // (a step repeated over the same window: nothing to do, nothing allocated)
    for (const auto& s : v) {          // swallow what touches [lo, hi)
      if (s.second < lo || s.first > hi) continue;
      if (s.first < lo) lo = s.first;
      if (s.second > hi) hi = s.second;
    }
    remove(lo, hi);
    std::size_t at = 0;
    while (at < v.size() && v[at].first < lo) ++at;
    v.insert(v.begin() + at, {lo, hi});
  }
  // an empty range is covered as soon as anything is resident (B = 0 calls keep the answer of the old flag)
  bool covers(int64_t lo, int64_t hi) const {
    if (hi <= lo) return any();
    for (const auto& s : v)
      if (s.first <= lo && hi <= s.second) return true;
    return false;
  }
};

// The resident states: `count` of them, as tensors in d_A (has_tensors), as ansatz(kind, P) of parameter rows (ansatz), or both
// once ensure_tensors has built the tensors of the rows.  The rows are the context's own d_params, or - while a driver runs -
// rows borrowed from its work buffers: one row per state, or (shifts > 0, rotosolve) one row per restart, of which state
// shifts r + k is restart r with shift k on parameter *shift_index.  The D = 4 fused energy kernel reads rows and shift_index as
// device pointers, so the fields change together, through the transitions below and nowhere else (tests/test_csrc_layout.py).
struct ResidentStates {
  int64_t count = 0;
  bool has_tensors = true;             // d_A holds the tensors of the resident states
  bool ansatz = false;                 // the resident states ARE ansatz(kind, P) of the parameter rows
  int kind = 0, P = 0;
  const double* rows = nullptr;        // borrowed parameter rows (nullptr: the context's d_params)
  const int* shift_index = nullptr;    // device index of the parameter being shifted (shifts > 0)
  int shifts = 0;                      // shifts per restart (0: one parameter row per state)

  bool borrowed() const { return rows != nullptr; }
  // n tensors in d_A and nothing else: no ansatz, nothing borrowed (a fresh context holds 0 of them)
  void hold_tensors(int64_t n) {
    *this = ResidentStates();
    count = n;
  }
  // n states that are ansatz(kind, P) of the rows; d_A is not built (ensure_tensors builds it where shifts == 0)
  void hold_ansatz(int64_t n, int kind_, int P_, const double* rows_ = nullptr, const int* shift_index_ = nullptr, int shifts_ = 0) {
    count = n; has_tensors = false; ansatz = true; kind = kind_; P = P_;
    rows = rows_; shift_index = shift_index_; shifts = shifts_;
  }
  // no states, and d_A holds nothing a reader may ask for ("no resident states")
  void hold_nothing() {
    *this = ResidentStates();
    has_tensors = false;
  }
  void tensors_built() { has_tensors = true; }
};
