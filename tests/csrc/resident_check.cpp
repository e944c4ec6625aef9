// TEST INFRASTRUCTURE ONLY: a stand-alone check of qmps_amd/csrc/qmps_resident.h on the host, meant to be built with
// -fsanitize=address,undefined (tests/test_resident_cpu.py builds and runs it).
//   qmps_slots       against a bitmap model on [0, 64]: seeded random add / remove sequences, empty and inverted ranges among them
//   ResidentStates   every transition from every reachable state, the full field set afterwards
// Prints one line per part and returns 0, or the first disagreement and 1.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "qmps_resident.h"

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                  \
      printf("\n");                                         \
      if (++g_failures >= 10) return;                       \
    }                                                       \
  } while (0)

struct Rng {      // splitmix64: the same sequence with every standard library
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

// positions [lo, hi) of [0, 64) as bits; an empty or inverted range is no position
uint64_t mask(int64_t lo, int64_t hi) {
  if (hi <= lo) return 0;
  const uint64_t upto_hi = hi >= 64 ? ~0ull : ((1ull << hi) - 1), upto_lo = lo >= 64 ? ~0ull : ((1ull << lo) - 1);
  return upto_hi & ~upto_lo;
}

void check_invariant(const qmps_slots& s, uint64_t model, int seq, int op) {
  uint64_t all = 0;
  for (size_t i = 0; i < s.v.size(); ++i) {
    CHECK(s.v[i].first >= 0 && s.v[i].second <= 64 && s.v[i].first < s.v[i].second, "sequence %d op %d: interval %zu is [%lld, %lld)", seq, op, i,
          (long long)s.v[i].first, (long long)s.v[i].second);
    // sorted, disjoint and not adjacent: a gap of at least one position
    if (i > 0) CHECK(s.v[i - 1].second < s.v[i].first, "sequence %d op %d: intervals %zu and %zu touch", seq, op, i - 1, i);
    all |= mask(s.v[i].first, s.v[i].second);
  }
  CHECK(all == model, "sequence %d op %d: union %016llx, model %016llx", seq, op, (unsigned long long)all, (unsigned long long)model);
  CHECK(s.any() == (model != 0), "sequence %d op %d: any()", seq, op);
}

void check_slots() {
  constexpr int kSequences = 2000, kOps = 40;
  Rng rng{20240607};
  long proper = 0, degenerate = 0, touch_true = 0, cover_true = 0;
  for (int seq = 0; seq < kSequences; ++seq) {
    qmps_slots s;
    uint64_t model = 0;
    for (int op = 0; op < kOps; ++op) {
      // one range in four as drawn (half of those inverted, one in 65 empty), the others ordered
      int64_t lo = rng.below(65), hi = rng.below(65);
      if (rng.below(4) != 0 && hi < lo) { const int64_t t = lo; lo = hi; hi = t; }
      (hi <= lo ? degenerate : proper)++;
      if (rng.below(2)) { s.add(lo, hi); model |= mask(lo, hi); }
      else { s.remove(lo, hi); model &= ~mask(lo, hi); }
      check_invariant(s, model, seq, op);
      if (g_failures) return;
      // the queries: a proper range, and an empty or inverted one
      int64_t a = rng.below(64), b = a + 1 + rng.below(64 - (int)a);
      const uint64_t m = mask(a, b);
      const bool t = (model & m) != 0, c = (model & m) == m;
      touch_true += t; cover_true += c;
      CHECK(s.touches(a, b) == t, "sequence %d op %d: touches(%lld, %lld) is %d", seq, op, (long long)a, (long long)b, (int)s.touches(a, b));
      CHECK(s.covers(a, b) == c, "sequence %d op %d: covers(%lld, %lld) is %d", seq, op, (long long)a, (long long)b, (int)s.covers(a, b));
      const int64_t e_lo = rng.below(65), e_hi = rng.below((int)e_lo + 1);      // e_hi <= e_lo
      CHECK(s.covers(e_lo, e_hi) == s.any(), "sequence %d op %d: covers(%lld, %lld) on an empty range", seq, op, (long long)e_lo, (long long)e_hi);
      CHECK(!s.touches(e_lo, e_hi), "sequence %d op %d: touches(%lld, %lld) on an empty range is true", seq, op, (long long)e_lo, (long long)e_hi);
    }
    s.clear();
    check_invariant(s, 0, seq, kOps);
  }
  printf("qmps_slots: %d sequences x %d operations (%ld proper, %ld empty or inverted ranges), 4 queries each (touches true %ld, covers true %ld): agree with the model\n",
         kSequences, kOps, proper, degenerate, touch_true, cover_true);
}

struct Fields {
  int64_t count;
  bool has_tensors, ansatz;
  int kind, P;
  const double* rows;
  const int* shift_index;
  int shifts;
  bool operator==(const Fields& o) const {
    return count == o.count && has_tensors == o.has_tensors && ansatz == o.ansatz && kind == o.kind && P == o.P && rows == o.rows && shift_index == o.shift_index &&
           shifts == o.shifts;
  }
};
Fields fields(const ResidentStates& s) { return {s.count, s.has_tensors, s.ansatz, s.kind, s.P, s.rows, s.shift_index, s.shifts}; }

void check_states() {
  static const double rows_a[4] = {}, rows_b[4] = {};
  static const int idx[1] = {};
  const Fields fresh{0, true, false, 0, 0, nullptr, nullptr, 0};
  CHECK(fields(ResidentStates()) == fresh, "a default-constructed value");
  {
    ResidentStates s;
    s.hold_tensors(0);
    CHECK(fields(s) == fields(ResidentStates()), "hold_tensors(0) against a default-constructed value");
  }
  // the transitions with the arguments the library gives them: what each leaves depends on nothing that was there before
  // (tensors_built: on the validity flag alone)
  struct Transition {
    const char* name;
    void (*apply)(ResidentStates&);
    Fields leaves;      // (tensors_built: unused)
    bool borrowed;
  };
  const Transition transitions[] = {
      {"hold_tensors(0)", [](ResidentStates& s) { s.hold_tensors(0); }, {0, true, false, 0, 0, nullptr, nullptr, 0}, false},
      {"hold_tensors(5)", [](ResidentStates& s) { s.hold_tensors(5); }, {5, true, false, 0, 0, nullptr, nullptr, 0}, false},
      {"hold_ansatz(7, 2, 6)", [](ResidentStates& s) { s.hold_ansatz(7, 2, 6); }, {7, false, true, 2, 6, nullptr, nullptr, 0}, false},
      {"hold_ansatz(0, 1, 4)", [](ResidentStates& s) { s.hold_ansatz(0, 1, 4); }, {0, false, true, 1, 4, nullptr, nullptr, 0}, false},
      {"hold_ansatz(9, 0, 8, rows)", [](ResidentStates& s) { s.hold_ansatz(9, 0, 8, rows_a); }, {9, false, true, 0, 8, rows_a, nullptr, 0}, true},
      {"hold_ansatz(12, 3, 4, rows, index, 3)", [](ResidentStates& s) { s.hold_ansatz(12, 3, 4, rows_b, idx, 3); }, {12, false, true, 3, 4, rows_b, idx, 3}, true},
      {"hold_ansatz(4, 3, 4, rows, index, 0)", [](ResidentStates& s) { s.hold_ansatz(4, 3, 4, rows_b, idx, 0); }, {4, false, true, 3, 4, rows_b, idx, 0}, true},
      {"hold_nothing()", [](ResidentStates& s) { s.hold_nothing(); }, {0, false, false, 0, 0, nullptr, nullptr, 0}, false},
      {"tensors_built()", [](ResidentStates& s) { s.tensors_built(); }, {}, false},
  };
  const size_t n_tr = sizeof(transitions) / sizeof(transitions[0]);
  // the reachable states: the closure of the fresh value under the transitions
  std::vector<ResidentStates> reach{ResidentStates()};
  size_t pairs = 0;
  for (size_t at = 0; at < reach.size(); ++at) {
    for (size_t k = 0; k < n_tr; ++k) {
      const Transition& tr = transitions[k];
      ResidentStates s = reach[at];
      const Fields before = fields(s);
      tr.apply(s);
      ++pairs;
      Fields want = tr.leaves;
      bool want_borrowed = tr.borrowed;
      if (k == n_tr - 1) {      // tensors_built
        want = before;
        want.has_tensors = true;
        want_borrowed = before.rows != nullptr;
      }
      CHECK(fields(s) == want, "%s from state %zu", tr.name, at);
      CHECK(s.borrowed() == want_borrowed, "%s from state %zu: borrowed()", tr.name, at);
      bool seen = false;
      for (const ResidentStates& r : reach) seen = seen || fields(r) == fields(s);
      if (!seen) reach.push_back(s);
    }
  }
  CHECK(reach.size() < 64, "the closure did not close: %zu states", reach.size());
  {      // the cases by name: a tensor upload after a driver's borrowed rows; the BFGS drivers' "nothing resident"
    ResidentStates s;
    s.hold_ansatz(12, 3, 4, rows_b, idx, 3);
    CHECK(s.borrowed(), "borrowed rows");
    s.hold_tensors(4);
    CHECK(!s.borrowed() && s.shift_index == nullptr && s.shifts == 0 && !s.ansatz && s.has_tensors && s.count == 4, "hold_tensors after a borrowed hold_ansatz");
    s.hold_nothing();
    CHECK(!s.has_tensors && s.count == 0 && !s.ansatz && !s.borrowed(), "hold_nothing");
  }
  printf("ResidentStates: %zu transitions from each of %zu reachable states (%zu pairs): every field as stated\n", n_tr, reach.size(), pairs);
}

}  // namespace

int main() {
  check_slots();
  if (!g_failures) check_states();
  if (g_failures) printf("%d check(s) failed\n", g_failures);
  return g_failures ? 1 : 0;
}
