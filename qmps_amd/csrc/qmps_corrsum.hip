// qmps_corrsum.hip - correlator sums of the resident states (qmps_correlator_sums): for every evaluation b and every point z_j
//   G[j][a][c] = z_j tr(L_a (1 - z_j Tt)^(-1)(b_c)) / tau,   Tt(x) = T(x) - r tr(x) / tau,   b_c = E_{O_c}(r) - one[c] r,   tau = tr r,
//   E_O(x) = sum_{t,s} O[t][s] A_s x A_t^+,  T = E_1,  L_a = sum_{t,s} O_a[t][s] A_t^+ A_s,  one[a] = tr(E_{O_a}(r)) / tau,
//   site[a][c] = tr(E_{O_a O_c}(r)) / tau
// - the sum over n >= 1 of z^n times the connected two-point function, without truncation - in ONE launch.  A work item is one (b, j):
// a dense solve of order N = D^2 with n_ops right-hand sides.  Matrices are vectorised row-major (x[i][j] at i D + j), so the system
// matrix is  M[(i,j)][(k,l)] = delta - z (sum_s A_s[i][k] conj(A_s[j][l]) - delta_kl r[i][j] / tau);  it is built on the device.
//
// Four kernel shapes share one elimination and one matrix (qmps_corrsum_core.h); this file checks the arguments and chooses among them:
//   D = 2   one lane per item, everything in registers                                   (corrsum_lane_kernel, qmps_corrsum_small.hip)
//   D = 4   16 consecutive lanes per item, lane q owns row q                             (corrsum_rows_kernel, qmps_corrsum_small.hip)
//   D = 8   one workgroup of 256 threads per item, the matrix in LDS                     (corrsum_lds_kernel, qmps_corrsum_block.hip)
//   D = 16  one workgroup per item, the matrix in a global slab per workgroup            (corrsum_global_kernel, qmps_corrsum_block.hip)
// L_a, one and b_c are built once per item, not per right-hand side or step; their cost, O(D^3), is small next to the O(D^6) solve.
// Every loop has a trip count fixed by D, n_ops and the item count; there are no atomics, counters or waits between workgroups.
//
// What fills the right-hand sides and lv, the read-out scale and what the j = 0 item stores is the kernels' template argument: one-site
// operators as described above (OneSiteSource, qmps_corrsum_one_site.h), or two-site ones (qmps_correlator_sums_two_site; TwoSiteSource,
// formulas and builders in qmps_corrsum_two_site.h): b_c = E2_(O_c)(r) - one[c] r, L_a two-site, G scaled by z^2 / tau (the sum starts
// at n = 2), `site` receives near[a][c][0..2].  The matrix, the pivot search, the elimination and the read-out are the same code for both.
#include "qmps_corrsum_internal.h"

namespace qmps {

namespace {

template <class Src>
hipError_t launch_source(int D, const CorrSumArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.n_ops < 1 || a.n_ops > kMaxObservableOps || a.n_z < 1) return hipErrorInvalidValue;
  const int64_t items = a.B * a.n_z;
  switch (D) {
    case 2:
    case 4: launch_small<Src>(D, a, items, st); break;
    case 16:
      if (a.work == nullptr || a.n_slabs < 1 || a.n_slabs > kCorrSumMaxSlabs) return hipErrorInvalidValue;
      [[fallthrough]];
    case 8: launch_block<Src>(D, a, items, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_correlator_sums(int D, const CorrSumArgs& a, hipStream_t st) { return launch_source<OneSiteSource>(D, a, st); }
hipError_t launch_correlator_sums_two_site(int D, const CorrSumArgs& a, hipStream_t st) { return launch_source<TwoSiteSource>(D, a, st); }

}  // namespace qmps
