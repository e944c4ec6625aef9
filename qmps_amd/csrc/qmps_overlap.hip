// qmps_overlap.hip - time-evolution overlap objective at bond dimension D = 4, 8, 16: which kernel family solves a batch (gfx950 only).
//
// Reference: qmps/new_time_evolve.py:193-221, scripts/loschmidt.py:209-239 and qmps/time_evolve_tools.py:20-23 (`merge`,
// whose final reshape hard-codes D = 2 in the reference; the mathematics is bond-dimension agnostic):
//   T(x) = sum_{s=0..3} C_s x Bm_s^+ ,   C = WW . merge(A, A) ,   Bm = merge(B, B) ,   merge(A, A)[2 s1 + s2] = A_s1 A_s2
// eta = dominant eigenvalue of T (complex; T is not Hermitian).  The reference's circuit measures 2 |psi[0]| = |eta|
// and minimises -sqrt(|eta|), so the kernels are only the dominant-eigenvalue solve.
//
// Power method in operator form (never builds the D^2 x D^2 matrix): x <- T(x)/||T(x)||_F from a generic start (overlap_cold_start),
// eta = <x, T x> (Rayleigh quotient, ||x||_F = 1), stop when ||T x - eta x||_F < tol.  status 1 = no unique dominant
// eigenvalue within max_steps.  D = 2 and the D = 4 default square the matrix of the map instead.
//
//   qmps_overlap_square.hip   D = 2 (launch_overlap) and D = 4 on the matrix cores (launch_overlap_square_d4)
//   qmps_overlap_block.hip    the generic tile kernel: D = 8, the D = 4 and D = 16 fall-backs (launch_overlap_block, launch_overlap_pair_d8)
//   qmps_overlap_d16.hip      D = 16 on the matrix cores (launch_overlap_mfma_d16, launch_overlap_pair_d16)
//   qmps_overlap_krylov.hip   the Krylov fall-back behind the D = 8 and D = 16 power kernels
#include <hip/hip_runtime.h>

#include "qmps_kernels.h"

namespace qmps {

// the Krylov fall-back behind a power launch (both solves of a pair launch): candidates given up are finished, the others untouched
hipError_t launch_krylov_after(int D, const OverlapArgs& a, const OverlapArgs* second, hipStream_t st) {
  const bool first = a.krylov_after > 0 && a.kry_counter != nullptr;
  const bool both = first && second != nullptr && second->krylov_after > 0 && second->kry_counter != nullptr;
  if (both) return launch_overlap_krylov_pair(D, a, *second, st);
  if (first)
    if (hipError_t e = launch_overlap_krylov(D, a, a.kry_counter, st); e != hipSuccess) return e;
  if (second != nullptr && second->krylov_after > 0 && second->kry_counter != nullptr)
    if (hipError_t e = launch_overlap_krylov(D, *second, second->kry_counter, st); e != hipSuccess) return e;
  return hipSuccess;
}

hipError_t launch_overlap_d(int D, const OverlapArgs& a, bool mfma, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  hipError_t e;
  if (D == 4 && mfma) e = launch_overlap_square_d4(a, st);      // (hands out left fixed points itself: the largest row of the squared map)
  else if (D == 16 && mfma) e = launch_overlap_mfma_d16(a, st);
  else e = launch_overlap_block(D, a, st);
  if (e != hipSuccess) return e;
  if (D == 8 || (D == 16 && mfma && overlap_d16_four_waves(a))) return launch_krylov_after(D, a, nullptr, st);
  return hipSuccess;
}

}  // namespace qmps
