// qmps_power_d4_core.h - the arithmetic of the D = 4 plain power iteration (QMPS_ENV_POWER), stated ONCE for its two kernels:
// env_power_d4_kernel (qmps_direct.hip: a 16-lane DPP row per evaluation, lane c owns coordinate c) and energy_lane_kernel<4>
// (qmps_energy_lane.hip, QMPS_POWER_LANE: one lane per evaluation, all sixteen coordinates in its registers).
//
// include/qmps_hip.h promises of the two routes "same iterates, same iteration counts and statuses".  The stopping test
// ||r_k - r_(k-1)||_F < tol is decided by the last bits of the distance wherever the residual falls by a factor 1 - gap per step
// (a transfer gap of 1e-3: a thousand steps within a factor e of tol), so the promise holds only if both kernels round alike:
// every operation of a step below is one IEEE operation in a fixed order - explicit fma, no contraction - and the sums over the
// sixteen coordinates are taken in the order of the DPP row reduction (row16_sum) and of the four accumulators of the row kernel.
//
// Coordinates (qmps_direct_core.h): c = 4 i + i', u_c = Re r[i][i'] (i <= i'), Im r[i'][i] (i > i').
#pragma once
#include <hip/hip_runtime.h>

#include "qmps_device.h"

namespace qmps {

// Row c = (i, i') of the real 16 x 16 transfer matrix (DirectD4::build for one row).  A(s, a, j) = A_s[a][j] as double2.
// With P(j,j') = sum_s (gamma A_s[i][j]) conj(A_s[i'][j']), gamma = 1 (i <= i') | i (i > i'):
// column (j,j): Re P(j,j);  (lo,hi): Re (P(lo,hi) + P(hi,lo));  (hi,lo): -Im (P(lo,hi) - P(hi,lo))
template <class Tensor>
__device__ __forceinline__ void power_d4_map_row(const Tensor& A, int i, int ip, double (&R)[16]) {
  const bool rot = i > ip;
  double tr[2][4], ti[2][4], br[2][4], bi[2][4];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double2 a = A(s, i, j), cc = A(s, ip, j);
      tr[s][j] = rot ? -a.y : a.x;
      ti[s][j] = rot ? a.x : a.y;
      br[s][j] = cc.x;
      bi[s][j] = cc.y;
    }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double v = tr[0][j] * br[0][j];
    v = dfma(ti[0][j], bi[0][j], v);
    v = dfma(tr[1][j], br[1][j], v);
    v = dfma(ti[1][j], bi[1][j], v);
    R[5 * j] = v;
  }
#pragma unroll
  for (int lo = 0; lo < 4; ++lo)
#pragma unroll
    for (int hi = lo + 1; hi < 4; ++hi) {
      double re = tr[0][lo] * br[0][hi], im = tr[0][lo] * bi[0][hi];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s > 0) {
          re = dfma(tr[s][lo], br[s][hi], re);
          im = dfma(tr[s][lo], bi[s][hi], im);
        }
        re = dfma(ti[s][lo], bi[s][hi], re);
        re = dfma(tr[s][hi], br[s][lo], re);
        re = dfma(ti[s][hi], bi[s][lo], re);
        im = dfma(-ti[s][lo], br[s][hi], im);
        im = dfma(ti[s][hi], br[s][lo], im);
        im = dfma(-tr[s][hi], bi[s][lo], im);
      }
      R[4 * lo + hi] = re;
      R[4 * hi + lo] = im;
    }
}

// coordinate (i, i') of a caller's guess, symmetrised: Re r[i][i'] (i <= i') | Im r[i'][i] (i > i')
__device__ __forceinline__ double power_d4_guess_coord(const double2* rin, int i, int ip) {
  const double2 rw = rin[4 * i + ip], cl = rin[4 * ip + i];       // r[i][i'], r[i'][i]
  return i <= ip ? 0.5 * (rw.x + cl.x) : 0.5 * (cl.y - rw.y);
}

// one coordinate's share of ||r_k - r_(k-1)||_F^2 = sum_diag d^2 + 2 sum_offdiag d^2: two multiplications, and the additions of the
// reduction that follows must not absorb the second (lane c would then hold fma(d_c, wt d_c, share of lane c + 8): another number in
// every lane of the row, and not the one the other kernel computes)
__device__ __forceinline__ double power_d4_distance_share(double wt, double d) {
#pragma clang fp contract(off)
  const double wd = wt * d;
  return wd * d;
}

// One lane per evaluation: the whole iteration on sixteen coordinates in registers, operation by operation what a row of
// env_power_d4_kernel does.  The map is written as rebuilt row by row in every step; it does not depend on the step, the compiler
// hoists it, and its 256 entries then fill the lane's registers and spill (512 VGPRs, ~1 KB of scratch): this is the A/B route,
// not the fast one.
// u: the start vector (trace 1) in, the last iterate out.  Iterate k is accepted when ||r_k - r_(k-1)||_F < tol, iterations = k <= max_iter.
template <class Tensor>
__device__ __forceinline__ void power_d4_lane_solve(const Tensor& A, double (&u)[16], int max_iter, double tol2, int& iters, bool& converged) {
#pragma clang fp contract(off)
  converged = false;
  for (int k = 1; k <= max_iter; ++k) {
    double y[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      double R[16];
      power_d4_map_row(A, c >> 2, c & 3, R);
      double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;      // the four accumulators of the row kernel's sixteen v_fmac_f64_dpp
#pragma unroll
      for (int b = 0; b < 16; b += 4) {
        y0 = dfma(u[b], R[b], y0);
        y1 = dfma(u[b + 1], R[b + 1], y1);
        y2 = dfma(u[b + 2], R[b + 2], y2);
        y3 = dfma(u[b + 3], R[b + 3], y3);
      }
      y[c] = (y0 + y1) + (y2 + y3);
    }
    const double t0 = y[0] + y[10], t1 = y[5] + y[15];
    const double inv = fast_rcp(t0 + t1);
    double w[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const double yn = y[c] * inv;
      w[c] = power_d4_distance_share((c >> 2) == (c & 3) ? 1.0 : 2.0, yn - u[c]);
      u[c] = yn;
    }
    // row16_sum as lane 0 of the row sees it (every lane of the row sees the same bits: each stage adds a pair commutatively)
    double x[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) x[c] = w[c] + w[c + 8];
    const double d2 = ((x[0] + x[4]) + (x[2] + x[6])) + ((x[1] + x[5]) + (x[3] + x[7]));
    iters = k;
    if (d2 < tol2) {
      converged = true;
      break;
    }
  }
}

}  // namespace qmps
