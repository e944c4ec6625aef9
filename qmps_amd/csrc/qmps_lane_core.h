// qmps_lane_core.h - the one-evaluation-per-lane mathematics of qmps's classical inner loop (gfx950 only): every operand of every
// v_fma_f64 is a VGPR of the lane that owns the evaluation.  Shared by energy_lane_kernel (qmps_energy_lane.hip),
// energy_pair_d4_kernel (qmps_energy_pair_d4.hip: the Cholesky test), cell2_lane_kernel (qmps_cell2.hip) and
// rotosolve_fused_d2_kernel (qmps_energy_lane.hip).  Everything here is __device__ __forceinline__: no out-of-line device code.
//
// Hot path (per evaluation; reference = fergusfinn/qmps, cited file:line):
//   A[2][D][D]  --(dominant fixed point of r -> sum_s A_s r A_s^+ ; replaces the xmps eigen-solve behind
//                  get_env_exact, qmps/tools.py:176-182; `krylov`, Power Method.ipynb cells 5-6)-->  r
//   (A, r, h)   --(closed form of State + psi^+ (1 x h x 1) psi, qmps/represent.py:258-262,
//                  qmps/ground_state.py:159-167)-->  E
//
// Plain power iteration (identical in oracle/qmps_oracle.c and oracle/qmps_oracle.py):
//   r_0 = 1/D (or the caller's warm start);  r' = herm(sum_s A_s r A_s^+);  r' /= tr r';
//   stop when ||r' - r||_F^2 < tol^2;  status 0 converged / 1 hit max_iter / 2 r not PD.
#pragma once
#include <hip/hip_runtime.h>

#include "qmps_kernels.h"     // QMPS_ST_*
#include "qmps_device.h"

namespace qmps {

// Packed Hermitian accessors: only entries with j >= i are stored; the diagonal is real.
template <int D>
__device__ __forceinline__ double h_re(const double (&re)[D][D], int i, int j) {
  return i <= j ? re[i][j] : re[j][i];
}
template <int D>
__device__ __forceinline__ double h_im(const double (&im)[D][D], int i, int j) {
  return i < j ? im[i][j] : -im[j][i];  // never called with i == j
}

// One power step, one evaluation per lane:  n = sum_s A_s r A_s^+  (upper triangle only).
template <int D>
__device__ __forceinline__ void power_step(const double (&are)[2][D][D], const double (&aim)[2][D][D],
                                           const double (&rre)[D][D], const double (&rim)[D][D],
                                           double (&nre)[D][D], double (&nim)[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) {
      nre[i][j] = 0.0;
      nim[i][j] = 0.0;
    }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      // row i of X_s = A_s r
      double xre[D], xim[D];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double xr = 0.0, xi = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double ar = are[s][i][k], ai = aim[s][i][k];
          const double rr = h_re<D>(rre, k, j);
          xr = dfma(ar, rr, xr);
          xi = dfma(ai, rr, xi);
          if (k != j) {
            const double ri = h_im<D>(rim, k, j);
            xr = dfma(-ai, ri, xr);
            xi = dfma(ar, ri, xi);
          }
        }
        xre[j] = xr;
        xim[j] = xi;
      }
      // n[i][j] += sum_k X[i][k] conj(A_s[j][k]),  j >= i
#pragma unroll
      for (int j = i; j < D; ++j) {
        double nr = nre[i][j], ni = nim[i][j];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          nr = dfma(xre[k], are[s][j][k], nr);
          nr = dfma(xim[k], aim[s][j][k], nr);
          if (j > i) {
            ni = dfma(xim[k], are[s][j][k], ni);
            ni = dfma(-xre[k], aim[s][j][k], ni);
          }
        }
        nre[i][j] = nr;
        nim[i][j] = ni;
      }
    }
  }
}

// Cholesky positive-definiteness test of a packed Hermitian matrix (LAPACK zpotrf criterion:
// a pivot that is not > 0 fails).  Mirrors cholesky(r) at qmps/tools.py:182.
template <int D>
__device__ __forceinline__ bool is_positive_definite(const double (&rre)[D][D], const double (&rim)[D][D]) {
  double lre[D][D], lim[D][D];  // lower factor, L[i][j], j <= i
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double d = rre[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= lre[j][k] * lre[j][k] + lim[j][k] * lim[j][k];
    ok = ok && (d > 0.0);
    const double ljj = __builtin_sqrt(d > 0.0 ? d : 1.0);
    const double inv = 1.0 / ljj;
    lre[j][j] = ljj;
    lim[j][j] = 0.0;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      // r[i][j] with i > j  = conj(r[j][i])
      double cr = rre[j][i], ci = -rim[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) {
        // L[i][k] * conj(L[j][k])
        cr -= lre[i][k] * lre[j][k] + lim[i][k] * lim[j][k];
        ci -= lim[i][k] * lre[j][k] - lre[i][k] * lim[j][k];
      }
      lre[i][j] = cr * inv;
      lim[i][j] = ci * inv;
    }
  }
  return ok;
}

// Two-site reduced density matrix, upper triangle (tau <= sigma), one evaluation per lane:
//   rho[tau][sigma] = tr(B_tau r B_sigma^+),  B_{2 s1 + s2} = A_s1 A_s2   (NOT yet divided by tr r)
// computed as  X_t2 = A_t2 r ;  R = X_t2 A_s2^+ ;  Z = A_t1 R ;  rho = sum_ik Z[i][k] conj(A_s1[i][k]).
// Generalised to a two-site unit cell: left-site tensor L (are/aim) and right-site tensor Rt (bre/bim):
//   rho[(t1 t2)][(s1 s2)] = tr(L_t1 Rt_t2 r Rt_s2^+ L_s1^+);  single-site cell: L == Rt.
template <int D>
__device__ __forceinline__ void two_site_rdm(const double (&are)[2][D][D], const double (&aim)[2][D][D],
                                             const double (&bre)[2][D][D], const double (&bim)[2][D][D],
                                             const double (&rre)[D][D], const double (&rim)[D][D],
                                             double (&pre)[4][4], double (&pim)[4][4]) {
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    // X = A_t2 r (full)
    double xre[D][D], xim[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        double xr = 0.0, xi = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double ar = bre[t2][i][k], ai = bim[t2][i][k];
          const double rr = h_re<D>(rre, k, j);
          xr = dfma(ar, rr, xr);
          xi = dfma(ai, rr, xi);
          if (k != j) {
            const double ri = h_im<D>(rim, k, j);
            xr = dfma(-ai, ri, xr);
            xi = dfma(ar, ri, xi);
          }
        }
        xre[i][j] = xr;
        xim[i][j] = xi;
      }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      // R = X A_s2^+ (full)
      double Rre[D][D], Rim[D][D];
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
          double cr = 0.0, ci = 0.0;
#pragma unroll
          for (int k = 0; k < D; ++k) {
            cr = dfma(xre[i][k], bre[s2][j][k], cr);
            cr = dfma(xim[i][k], bim[s2][j][k], cr);
            ci = dfma(xim[i][k], bre[s2][j][k], ci);
            ci = dfma(-xre[i][k], bim[s2][j][k], ci);
          }
          Rre[i][j] = cr;
          Rim[i][j] = ci;
        }
#pragma unroll
      for (int t1 = 0; t1 < 2; ++t1) {
        const int tau = 2 * t1 + t2;
        // is any (s1) with tau <= sigma ?
        if (tau > 2 + s2) continue;
        // rho[tau][sigma] = sum_i sum_k Z[i][k] conj(A_s1[i][k]),  Z = A_t1 R, one row at a time
        double acc_re[2] = {0.0, 0.0}, acc_im[2] = {0.0, 0.0};
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
          for (int k = 0; k < D; ++k) {
            double zr = 0.0, zi = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) {
              const double ar = are[t1][i][j], ai = aim[t1][i][j];
              zr = dfma(ar, Rre[j][k], zr);
              zr = dfma(-ai, Rim[j][k], zr);
              zi = dfma(ar, Rim[j][k], zi);
              zi = dfma(ai, Rre[j][k], zi);
            }
#pragma unroll
            for (int s1 = 0; s1 < 2; ++s1) {
              const int sigma = 2 * s1 + s2;
              if (tau <= sigma) {
                acc_re[s1] = dfma(zr, are[s1][i][k], acc_re[s1]);
                acc_re[s1] = dfma(zi, aim[s1][i][k], acc_re[s1]);
                if (tau < sigma) {
                  acc_im[s1] = dfma(zi, are[s1][i][k], acc_im[s1]);
                  acc_im[s1] = dfma(-zr, aim[s1][i][k], acc_im[s1]);
                }
              }
            }
          }
        }
#pragma unroll
        for (int s1 = 0; s1 < 2; ++s1) {
          const int sigma = 2 * s1 + s2;
          if (tau <= sigma) {
            pre[tau][sigma] = acc_re[s1];
            pim[tau][sigma] = acc_im[s1];
          }
        }
      }
    }
  }
}

// LDS slab of energy_lane_kernel<D>: the wave's 64 tensors, one padded row each.
template <int D>
struct LaneCfg {
  static constexpr int kRowBytes = 32 * D * D;          // one tensor A[2][D][D] complex128
  static constexpr int kRowPad = kRowBytes + 16;        // +16 B: conflict-free ds_read_b128 by row
  static constexpr int kLdsBytes = 64 * kRowPad;        // one wave's slab
  static constexpr int kChunks = kRowBytes / 16;        // 16-B pieces per tensor == loads per lane
};

__device__ __forceinline__ double rdm_energy(const double2* h, const double (&pre)[4][4], const double (&pim)[4][4]) {
  double e = 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double2 hv = h[s * 4 + t];
      const double rr = (t <= s) ? pre[t][s] : pre[s][t];
      e = dfma(hv.x, rr, e);
      if (t != s) {
        const double ri = (t < s) ? pim[t][s] : -pim[s][t];
        e = dfma(-hv.y, ri, e);
      }
    }
  return e;
}

// normalise a freshly computed power step in place and return ||n - r||_F^2
template <int D>
__device__ __forceinline__ double normalise_and_diff(double (&nre)[D][D], double (&nim)[D][D],
                                                     const double (&rre)[D][D], const double (&rim)[D][D]) {
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) tr += nre[i][i];
  const double inv = 1.0 / tr;
  double dd = 0.0, od = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) {
      nre[i][j] *= inv;
      const double dr = nre[i][j] - rre[i][j];
      if (i == j) {
        nim[i][j] = 0.0;
        dd = dfma(dr, dr, dd);
      } else {
        nim[i][j] *= inv;
        const double di = nim[i][j] - rim[i][j];
        od = dfma(dr, dr, od);
        od = dfma(di, di, od);
      }
    }
  return dfma(2.0, od, dd);
}

// ------------------------------------------------------------------------------------------
// Real Hermitian coordinates.  r -> sum_s A_s r A_s^+ maps Hermitian matrices to Hermitian matrices,
// so on the orthonormal real coordinates
//   x_a = r_ii (a = i < D),  sqrt2 Re r_ij (a = D + p),  sqrt2 Im r_ij (a = D + P + p),  p <-> (i<j)
// it is a REAL D^2 x D^2 matrix R (the complex transfer matrix E = B R B^+ for a unitary B): one
// squaring costs 2 (D^2)^3 real flops instead of 8 (D^2)^3, and ||x - x'||_2 == ||r - r'||_F.
// ------------------------------------------------------------------------------------------
template <int D>
struct HermBasis {
  static constexpr int N = D * D, P = D * (D - 1) / 2;
  __host__ __device__ static constexpr int kind(int a) { return a < D ? 0 : (a < D + P ? 1 : 2); }
  __host__ __device__ static constexpr int pair(int a) { return a < D ? 0 : (a < D + P ? a - D : a - D - P); }
  __host__ __device__ static constexpr int row(int a) {  // i of the (i, j) the coordinate refers to
    if (a < D) return a;
    int p = pair(a), i = 0;
    while (p >= D - 1 - i) { p -= D - 1 - i; ++i; }
    return i;
  }
  __host__ __device__ static constexpr int col(int a) {
    if (a < D) return a;
    int p = pair(a), i = 0;
    while (p >= D - 1 - i) { p -= D - 1 - i; ++i; }
    return i + 1 + p;
  }
};

// R[a][b] = coordinate a of T(H_b); GetA(s, i, j) returns A_s[i][j] as double2.
template <int D, class GetA>
__device__ __forceinline__ double real_transfer_entry(GetA A, int a, int b) {
  using HB = HermBasis<D>;
  const int ka = HB::kind(a), i = HB::row(a), ip = HB::col(a);
  const int kb = HB::kind(b), j = HB::row(b), jp = HB::col(b);
  // e1 = sum_s A_s[i][j] conj(A_s[ip][jp]),  e2 = sum_s A_s[i][jp] conj(A_s[ip][j])
  double e1r = 0.0, e1i = 0.0, e2r = 0.0, e2i = 0.0;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double2 x = A(s, i, j), y = A(s, ip, jp);
    e1r = dfma(x.x, y.x, e1r);
    e1r = dfma(x.y, y.y, e1r);
    e1i = dfma(x.y, y.x, e1i);
    e1i = dfma(-x.x, y.y, e1i);
    if (kb != 0) {
      const double2 u = A(s, i, jp), v = A(s, ip, j);
      e2r = dfma(u.x, v.x, e2r);
      e2r = dfma(u.y, v.y, e2r);
      e2i = dfma(u.y, v.x, e2i);
      e2i = dfma(-u.x, v.y, e2i);
    }
  }
  // M = T(H_b)[i][ip]:  diag b: e1;  re b: (e1 + e2)/sqrt2;  im b: i (e1 - e2)/sqrt2
  double mr, mi;
  if (kb == 0) { mr = e1r; mi = e1i; }
  else if (kb == 1) { mr = e1r + e2r; mi = e1i + e2i; }
  else { mr = -(e1i - e2i); mi = e1r - e2r; }
  double val = (ka == 2) ? mi : mr;
  const bool sa = ka != 0, sb = kb != 0;   // sqrt2 for a non-diagonal output, 1/sqrt2 for a non-diagonal input
  if (sa && !sb) val *= 1.4142135623730951;
  if (!sa && sb) val *= 0.70710678118654752;
  return val;
}

template <int D>
__device__ __forceinline__ void pack_herm(const double (&rre)[D][D], const double (&rim)[D][D], double (&x)[D * D]) {
  using HB = HermBasis<D>;
#pragma unroll
  for (int a = 0; a < D * D; ++a) {
    const int k = HB::kind(a), i = HB::row(a), j = HB::col(a);
    x[a] = k == 0 ? rre[i][i] : (k == 1 ? 1.4142135623730951 * rre[i][j] : 1.4142135623730951 * rim[i][j]);
  }
}

template <int D>
__device__ __forceinline__ void unpack_herm(const double (&x)[D * D], double (&rre)[D][D], double (&rim)[D][D]) {
  using HB = HermBasis<D>;
#pragma unroll
  for (int a = 0; a < D * D; ++a) {
    const int k = HB::kind(a), i = HB::row(a), j = HB::col(a);
    if (k == 0) { rre[i][i] = x[a]; rim[i][i] = 0.0; }
    else if (k == 1) rre[i][j] = 0.70710678118654752 * x[a];
    else rim[i][j] = 0.70710678118654752 * x[a];
  }
}

// D = 2 only: repeated-squaring tail, one evaluation per lane.  R = T^(2^m) as a real 4 x 4 matrix in
// registers, x_m = R x_C / tr, stop at ||x_m - x_{m-1}||^2 < tol^2;  iterations = done + 2^m.
// The fixed point of a trace-preserving map at D = 2 from its real 4 x 4 matrix R (HermBasis<2> coordinates: r_00, r_11,
// sqrt2 Re r_01, sqrt2 Im r_01): (R - 1 + e_1 t^T) u = e_1, t = the trace functional.  Trace preservation makes the two
// DIAGONAL rows of R - 1 sum to zero, so the functional sits on one of them and that row is the last pivot (order 0, 2, 3, 1),
// as at D = 4.  Unpivoted Gauss-Jordan in the lane; u comes back trace-normalised, pivmax = the largest |1 / pivot|
// (above 1e10: the fixed point is not unique / the system is singular to rounding - do not trust u).
__device__ __forceinline__ void direct_fixed_point_d2(const double (&R)[4][4], double (&u)[4], double& pivmax) {
  double M[4][5];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) M[a][b] = R[a][b] - (a == b ? 1.0 : 0.0);
    M[a][4] = a == 1 ? 1.0 : 0.0;
  }
  M[1][0] += 1.0;
  M[1][1] += 1.0;
  pivmax = 0.0;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int k = kk == 0 ? 0 : (kk == 1 ? 2 : (kk == 2 ? 3 : 1));
    const double pinv = fast_rcp(M[k][k]);
    pivmax = fmax(pivmax, fabs(pinv));
#pragma unroll
    for (int b = 0; b < 5; ++b)
      if (b != k) M[k][b] *= pinv;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a != k) {
        const double f = M[a][k];
#pragma unroll
        for (int b = 0; b < 5; ++b)
          if (b != k) M[a][b] = dfma(-f, M[k][b], M[a][b]);
      }
  }
  const double tinv = fast_rcp(M[0][4] + M[1][4]);
#pragma unroll
  for (int a = 0; a < 4; ++a) u[a] = M[a][4] * tinv;
}

__device__ __forceinline__ void squaring_tail_d2(const double (&are)[2][2][2], const double (&aim)[2][2][2],
                                                 double (&rre)[2][2], double (&rim)[2][2], bool& active, int& iters,
                                                 int& status, int done, int max_iter, double tol2, int skip,
                                                 bool direct = false) {
  auto getA = [&](int s, int i, int j) { return make_double2(are[s][i][j], aim[s][i][j]); };
  double R[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) R[a][b] = real_transfer_entry<2>(getA, a, b);
  double x0[4], xp[4];
  pack_herm<2>(rre, rim, x0);
#pragma unroll
  for (int a = 0; a < 4; ++a) xp[a] = x0[a];
  if (direct) {
    // QMPS_ENV_DIRECT at D = 2: the 4 x 4 fixed-point solve; accepted iff one power step moves it by less than tol (iterations =
    // done + 1) and no pivot was below 1e-10; everything else goes on to the squaring below.
    double u[4], y[4], pivmax;
    direct_fixed_point_d2(R, u, pivmax);
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v = dfma(R[a][k], u[k], v);
      y[a] = v;
    }
    const double yinv = fast_rcp(y[0] + y[1]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double d = y[a] * yinv - u[a];
      d2 = dfma(d, d, d2);
    }
    if (active && d2 < tol2 && pivmax < 1e10 && done + 1 <= max_iter) {
#pragma unroll
      for (int a = 0; a < 4; ++a) xp[a] = y[a] * yinv;
      iters = done + 1;
      status = QMPS_ST_OK;
      active = false;
    }
  }
  int m = 0;
  auto square = [&]() {
    double Q[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v = dfma(R[a][k], R[k][c], v);
        Q[a][c] = v;
      }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) R[a][c] = Q[a][c];
  };
  auto apply = [&](double (&y)[4]) {   // y = R x0 / tr
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v = dfma(R[a][k], x0[k], v);
      y[a] = v;
    }
    const double inv = 1.0 / (y[0] + y[1]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      y[a] *= inv;
#pragma unroll
      for (int k = 0; k < 4; ++k) R[a][k] *= inv;   // keep R at O(1) for non-isometric tensors
    }
  };
  // phase 1: `skip` squarings without tracking the iterate; the comparison chain then starts at z_skip
  while (m < skip && done + (1 << (m + 1)) <= max_iter && __any(active)) {
    square();
    ++m;
  }
  if (m > 0) {
    double y[4];
    apply(y);
    if (active) {
#pragma unroll
      for (int a = 0; a < 4; ++a) xp[a] = y[a];
      iters = done + (1 << m);
    }
  }
  while (done + (1 << (m + 1)) <= max_iter && m < 29) {
    if (!__any(active)) break;
    square();
    ++m;
    double y[4];
    apply(y);
    double d2 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double d = y[a] - xp[a];
      d2 = dfma(d, d, d2);
    }
    if (active) {
#pragma unroll
      for (int a = 0; a < 4; ++a) xp[a] = y[a];
      iters = done + (1 << m);
      if (d2 < tol2) {
        active = false;
        status = QMPS_ST_OK;
      }
    }
  }
  // The budget ran out between two powers of two (max_iter = 10 000: the chain's last comparison is z_8192 against z_4096, so an
  // evaluation the plain method finishes in 4 097 .. 10 000 steps used to end with status 1 although z_8192 IS its fixed point): the plain
  // method's own test on the last iterate, one application of T itself - || T z / tr - z || < tol - at the cost of one more iteration.
  const int taken = m > 0 ? (1 << m) : 0;
  if (__any(active) && done + taken + 1 <= max_iter) {
    double d2 = 0.0, y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) v = dfma(real_transfer_entry<2>(getA, a, k), xp[k], v);
      y[a] = v;
    }
    const double inv = 1.0 / (y[0] + y[1]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      y[a] *= inv;
      const double d = y[a] - xp[a];
      d2 = dfma(d, d, d2);
    }
    if (active && d2 < tol2) {
#pragma unroll
      for (int a = 0; a < 4; ++a) xp[a] = y[a];
      iters = done + taken + 1;
      status = QMPS_ST_OK;
      active = false;
    }
  }
  unpack_herm<2>(xp, rre, rim);
}

// trace-normalise a packed Hermitian matrix in place
template <int D>
__device__ __forceinline__ void normalise_herm(double (&nre)[D][D], double (&nim)[D][D]) {
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) tr += nre[i][i];
  const double inv = 1.0 / tr;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i; j < D; ++j) {
      nre[i][j] *= inv;
      nim[i][j] = (i == j) ? 0.0 : nim[i][j] * inv;
    }
}

}  // namespace qmps
