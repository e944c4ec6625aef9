// qmps_cell2.hip - kernel 1b (gfx950 only): two-site unit cell (qmps/ground_state.py:291-331, NonSparseFullTwoSiteEnergyOptimizer),
// one evaluation per lane.  Inputs are the two state UNITARIES U1, U2 [B][2D][2D]; the kernel applies
// unitary_to_tensor on load.  r12 = fixed point of r -> T_A1(T_A2(r)) (transfer map of
// merge(A1, A2), qmps/time_evolve_tools.py:20-23); r21 = T_A2(r12)/tr is the fixed point of the
// swapped cell, so ONE power iteration serves both energies:
//   E1 = sum h[s][t] tr(A1_t1 A2_t2 r12 A2_s2^+ A1_s1^+),  E2 = same with 1 <-> 2 and r21,  f = (E1+E2)/2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_lane_core.h"

namespace qmps {

template <int D>
__global__ __launch_bounds__(64) void cell2_lane_kernel(Cell2Args p) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B) return;
  double a1re[2][D][D], a1im[2][D][D], a2re[2][D][D], a2im[2][D][D];
  {
    const double2* u1 = (const double2*)p.U1 + b * (4 * D * D);
    const double2* u2 = (const double2*)p.U2 + b * (4 * D * D);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const double2 v1 = u1[(2 * i + s) * (2 * D) + j], v2 = u2[(2 * i + s) * (2 * D) + j];
          a1re[s][i][j] = v1.x; a1im[s][i][j] = v1.y;
          a2re[s][i][j] = v2.x; a2im[s][i][j] = v2.y;
        }
  }
  double rre[D][D], rim[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) {
      rre[i][j] = (i == j) ? 1.0 / D : 0.0;
      rim[i][j] = 0.0;
    }
  if constexpr (D == 2) {
    // the fixed point of the two-site map T1 o T2 directly: its real matrix is R1 R2; the candidate becomes the start of the
    // loop below, whose first step is then the acceptance test (iterations = 1).  The power method's iteration counts are
    // heavy-tailed at D = 2 (some Haar cells do not converge in 10 000 steps)
    auto getA1 = [&](int s, int i, int j) { return make_double2(a1re[s][i][j], a1im[s][i][j]); };
    auto getA2 = [&](int s, int i, int j) { return make_double2(a2re[s][i][j], a2im[s][i][j]); };
    double R1[4][4], R2[4][4], R[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        R1[a][c] = real_transfer_entry<2>(getA1, a, c);
        R2[a][c] = real_transfer_entry<2>(getA2, a, c);
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v = dfma(R1[a][k], R2[k][c], v);
        R[a][c] = v;
      }
    double u[4], pivmax;
    direct_fixed_point_d2(R, u, pivmax);
    const bool good = pivmax < 1e10 && fabs(u[0]) < 1e300 && fabs(u[1]) < 1e300 && fabs(u[2]) < 1e300 && fabs(u[3]) < 1e300;
    if (good) unpack_herm<2>(u, rre, rim);
  }
  int iters = 0, status = QMPS_ST_NOT_CONVERGED;
  const double tol2 = p.tol * p.tol;
  for (int k = 1; k <= p.max_iter; ++k) {
    double tre[D][D], tim[D][D], nre[D][D], nim[D][D];
    power_step<D>(a2re, a2im, rre, rim, tre, tim);
    power_step<D>(a1re, a1im, tre, tim, nre, nim);
    normalise_herm<D>(nre, nim);
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) {
        const double dr = nre[i][j] - rre[i][j], di = nim[i][j] - rim[i][j];
        d2 += (i == j) ? dr * dr : 2.0 * (dr * dr + di * di);
        rre[i][j] = nre[i][j];
        rim[i][j] = nim[i][j];
      }
    iters = k;
    if (d2 < tol2) { status = QMPS_ST_OK; break; }
  }
  // environment of the swapped cell
  double qre[D][D], qim[D][D];
  power_step<D>(a2re, a2im, rre, rim, qre, qim);
  normalise_herm<D>(qre, qim);
  if (status == QMPS_ST_OK && !(is_positive_definite<D>(rre, rim) && is_positive_definite<D>(qre, qim)))
    status = QMPS_ST_NOT_PD;
  double p1re[4][4], p1im[4][4], p2re[4][4], p2im[4][4];
  two_site_rdm<D>(a1re, a1im, a2re, a2im, rre, rim, p1re, p1im);
  two_site_rdm<D>(a2re, a2im, a1re, a1im, qre, qim, p2re, p2im);
  double tr1 = 0.0, tr2 = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) { tr1 += rre[i][i]; tr2 += qre[i][i]; }
  for (int q = 0; q < p.n_terms; ++q) {
    const double2* h = (const double2*)p.h + q * 16;
    const double e1 = rdm_energy(h, p1re, p1im) / tr1;
    const double e2 = rdm_energy(h, p2re, p2im) / tr2;
    p.E[b * p.n_terms + q] = 0.5 * (e1 + e2);
    if (p.E12 != nullptr) {
      p.E12[(b * p.n_terms + q) * 2 + 0] = e1;
      p.E12[(b * p.n_terms + q) * 2 + 1] = e2;
    }
  }
  p.iters[b] = iters;
  p.status[b] = status;
}

hipError_t launch_cell2(int D, const Cell2Args& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (D != 2) return hipErrorInvalidValue;  // the reference path is D = 2 only (ground_state.py:276)
  hipLaunchKernelGGL((cell2_lane_kernel<2>), dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace qmps
