// qmps_direct_core.h - the per-evaluation mathematics of the DIRECT environment solve at D = 4, written once for
// two back-ends:
//   device : V = double - one lane of a DPP quad, four lanes per evaluation (qmps_direct.hip);
//   host   : V = four doubles in lock-step - TEST INFRASTRUCTURE ONLY (tests/csrc/direct_emu.cpp): it lets the CPU
//            test-suite check this very source against the oracle.  The product never runs it.
//
// What is computed (reference: the exact eigen-solve behind get_env_exact, qmps/tools.py:176-182, then
// State + psi^+ (1 x h x 1) psi, qmps/represent.py:258-262, qmps/ground_state.py:159-167):
//   the right environment r is the fixed point of T(r) = sum_s A_s r A_s^+.  For a left isometry T preserves the
//   trace, so in real coordinates u of the Hermitian matrix r the fixed point solves the REAL 16 x 16 system
//       (R - 1 + e_15 t^T) u = e_15        (t = trace functional; R = matrix of T)
//   by LU elimination without pivoting, the pivots taken round the quad, and back substitution (measured on 3000 Haar tensors in a
//   numpy model of the order: residual ||T(r) - r||_F < 8.1e-16), ACCEPTED only if one power step moves it by less than tol in Frobenius norm - the same criterion as
//   the iterative solvers, so status and tolerance semantics are unchanged; otherwise (not an isometry, degenerate
//   transfer spectrum, an unlucky pivot) the power method 2^m steps at a time takes over from r_0 = 1/D.
//
// Coordinates (plain, not orthonormal), index a = 4 i + i':
//   u[(i,i)] = r_ii ;  u[(i,i')] = Re r_ii' (i < i') ;  u[(i,i')] = Im r_i'i (i > i')
//   ||r - r'||_F^2 = sum_diag du^2 + 2 sum_offdiag du^2.
// Lane q of the quad owns the four coordinates a = (q, i'), i' = 0..3, i.e. rows 4 q .. 4 q + 3 of every matrix.
//
// Ops policy O (an object; holds the lane id and the tensor):
//   types   O::V (value), O::P (lane predicate)
//   lanes   o.q_eq(i), o.q_gt(i)                       predicates on the lane's row index q
//   quad    O::template bcast<L>(v), O::qsum(v)        value of lane L / sum over the quad, in every lane
//   select  O::sel(p, a, b);  O::rcp(v);  O::fma(a, b, c);  O::lt(a, b) -> P;  O::gt0(a) -> P
//           O::p_and(p, q), O::p_not(p), O::any(p) -> bool
//   tensor  o.own(s, j, re, im)   A_s[q][j]  (the lane's own row)
//           o.uni(s, i, j, re, im) A_s[i][j]  (the same value in every lane of the quad)
//           o.col(s, i, re, im)   A_s[i][q]  (the lane's own column; only power_step_sites / density_sites ask for it)
#pragma once

#include <stdint.h>

#include <utility>

namespace qmps {

// Which entries of the upper triangle of rho the Hamiltonian reads (E = Re sum h[s][t] rho[t][s]): bit 4 t + s (t <= s) - the real part of
// rho[t][s] - is set iff some term has Re h[s][t] != 0 or Re h[t][s] != 0, bit 16 + 4 t + s (t < s) - the imaginary part - iff some term has
// Im h[s][t] != 0 or Im h[t][s] != 0.  Exact comparisons: -0.0 is zero, NaN is needed.  h: n_terms x 16 complex numbers (re, im interleaved),
// Hermitian or not.  Plain C++: the host computes it once per Hamiltonian (qmps_set_hamiltonian).
constexpr uint32_t kRhoNeedAll = 0xFFFFFFFFu;
inline uint32_t rho_need_mask(const double* h, int n_terms) {
  uint32_t need = 0;
  for (int n = 0; n < n_terms; ++n)
    for (int s = 0; s < 4; ++s)
      for (int t = 0; t < 4; ++t) {
        const int lo = t < s ? t : s, hi = t < s ? s : t;
        const double re = h[32 * n + 2 * (4 * s + t)], im = h[32 * n + 2 * (4 * s + t) + 1];
        if (!(re == 0.0)) need |= 1u << (4 * lo + hi);
        if (lo != hi && !(im == 0.0)) need |= 1u << (16 + 4 * lo + hi);
      }
  return need;
}

// The site factors of rho (DirectD4::density_sites): with tau = 2 t1 + t2 and sigma = 2 s1 + s2,
//   rho[tau][sigma] = tr(N_{s1 t1} W_{t2 s2}),   N_{s1 t1} = A_s1^+ A_t1,   W_{t2 s2} = A_t2 r A_s2^+.
// The upper triangle (tau <= sigma, so t1 <= s1) reads N_00, N_10, N_11 and all four W; W_00 and W_11 are the two halves of the
// acceptance step and always there.  rho_site_factors: which of the other five the mask asks for - plain integer code, the same for every
// lane (scalar registers on the device).  rho_site_parts(f): the bits of `need` that read factor f.
constexpr uint32_t kSiteN00 = 1u, kSiteN10 = 2u, kSiteN11 = 4u, kSiteW01 = 8u, kSiteW10 = 16u;
constexpr uint32_t rho_site_parts(uint32_t factor) {
  uint32_t parts = 0;
  for (int tau = 0; tau < 4; ++tau)
    for (int sg = tau; sg < 4; ++sg) {
      const int t1 = tau >> 1, t2 = tau & 1, s1 = sg >> 1, s2 = sg & 1;
      const uint32_t n = s1 == 0 ? kSiteN00 : (t1 == 0 ? kSiteN10 : kSiteN11);
      const uint32_t w = t2 == s2 ? 0u : (t2 == 0 ? kSiteW01 : kSiteW10);
      if (factor == n || factor == w) parts |= (1u << (4 * tau + sg)) | (sg != tau ? 1u << (16 + 4 * tau + sg) : 0u);
    }
  return parts;
}
constexpr uint32_t rho_site_factors(uint32_t need) {
  return ((need & rho_site_parts(kSiteN00)) != 0u ? kSiteN00 : 0u) | ((need & rho_site_parts(kSiteN10)) != 0u ? kSiteN10 : 0u) |
         ((need & rho_site_parts(kSiteN11)) != 0u ? kSiteN11 : 0u) | ((need & rho_site_parts(kSiteW01)) != 0u ? kSiteW01 : 0u) |
         ((need & rho_site_parts(kSiteW10)) != 0u ? kSiteW10 : 0u);
}

#if defined(__HIPCC__)
#define QMPS_CORE_FN __device__ inline __attribute__((always_inline))
// instruction-scheduling fence: the compiler may not move anything across it.  The fully unrolled phases below are
// long straight-line blocks; without fences the scheduler hoists the operand reads / DPP moves of later steps and
// the register demand explodes (470 VGPRs without them).
#define QMPS_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define QMPS_CORE_FN inline __attribute__((always_inline))
#define QMPS_SCHED_FENCE() ((void)0)
#endif
// "this value exists here": in front of code that branches, the compiler otherwise sinks the arithmetic that produces a value into the
// branch that first reads it and leaves the LDS reads behind it in flight - their data then fills the register file across the branches
#if defined(__HIP_DEVICE_COMPILE__)
#define QMPS_COMPUTED_HERE(v) asm volatile("" : "+v"(v))
#else
#define QMPS_COMPUTED_HERE(v) ((void)0)
#endif

template <int... I, class F>
QMPS_CORE_FN void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
QMPS_CORE_FN void static_for(F&& f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}

template <class O>
struct DirectD4 {
  using V = typename O::V;
  using P = typename O::P;

  // the lane's own diagonal coordinate (q, q) out of its four values
  static QMPS_CORE_FN V own_diag(const O& o, const V (&x)[4]) {
    return O::sel(o.q_eq(0), x[0], O::sel(o.q_eq(1), x[1], O::sel(o.q_eq(2), x[2], x[3])));
  }

  // ---- 1. the lane's four rows of the real transfer matrix: Rc[i'][4 j + j'] = coordinate (q, i') of T(H_(j,j')) ----
  // With P(j,j') = sum_s (gamma A_s[q][j]) conj(A_s[i'][j']), gamma = 1 (q <= i': a real part) or i (q > i': minus an
  // imaginary part):  column (j,j): Re P(j,j);  column (lo,hi): Re (P(lo,hi) + P(hi,lo));
  // column (hi,lo): -Im (P(lo,hi) - P(hi,lo)).
  static QMPS_CORE_FN void build(const O& o, V (&Rc)[4][16]) {
    V ar[2][4], ai[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) o.own(s, j, ar[s][j], ai[s][j]);
#pragma unroll
    for (int ip = 0; ip < 4; ++ip) {
      const P rot = o.q_gt(ip);
      V tr[2][4], ti[2][4], br[2][4], bi[2][4];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // (no lane has q > 3: the last partner index needs no select)
          tr[s][j] = ip == 3 ? ar[s][j] : O::sel(rot, -ai[s][j], ar[s][j]);
          ti[s][j] = ip == 3 ? ai[s][j] : O::sel(rot, ar[s][j], ai[s][j]);
          o.uni(s, ip, j, br[s][j], bi[s][j]);
        }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        V v = tr[0][j] * br[0][j];
        v = O::fma(ti[0][j], bi[0][j], v);
        v = O::fma(tr[1][j], br[1][j], v);
        v = O::fma(ti[1][j], bi[1][j], v);
        Rc[ip][5 * j] = v;
      }
#pragma unroll
      for (int lo = 0; lo < 4; ++lo)
#pragma unroll
        for (int hi = lo + 1; hi < 4; ++hi) {
          V re = tr[0][lo] * br[0][hi], im = tr[0][lo] * bi[0][hi];
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            if (s > 0) {
              re = O::fma(tr[s][lo], br[s][hi], re);
              im = O::fma(tr[s][lo], bi[s][hi], im);
            }
            re = O::fma(ti[s][lo], bi[s][hi], re);
            re = O::fma(tr[s][hi], br[s][lo], re);
            re = O::fma(ti[s][hi], bi[s][lo], re);
            im = O::fma(-ti[s][lo], br[s][hi], im);
            im = O::fma(ti[s][hi], br[s][lo], im);
            im = O::fma(-tr[s][hi], bi[s][lo], im);
          }
          Rc[ip][4 * lo + hi] = re;
          Rc[ip][4 * hi + lo] = im;
        }
    }
  }

  // ---- 2. (R - 1 + e_15 t^T) u = e_15 by LU elimination without pivoting, rows distributed over the quad ----
  // The pivots go ROUND THE QUAD: step k pivots on row = column a(k) = 4 (k % 4) + k / 4 (lane k % 4, register k / 4), so the rows still to
  // come are the same registers in every lane: registers > k / 4 in all lanes, register k / 4 in the lanes > k % 4.  Only those are
  // eliminated (rows that were pivots already are rows of U and stay as they are): sum over k of rows x (15 - k) = 356 multiply-adds per
  // lane where eliminating above the pivot as well costs 480; in the order lane 0's rows, lane 1's, ... the lanes whose rows are done
  // would idle in lock-step and nothing would be saved.  The back substitution runs by columns: each unknown is broadcast as it appears
  // (that broadcast is the gathered copy) and every lane adds its column entry times the unknown to the sums of its unsolved rows.
  static constexpr int piv_coord(int k) { return 4 * (k & 3) + (k >> 2); }

  // M: the lane's rows of R on entry; destroyed.
  // ur: ALL sixteen coordinates of the solution in every lane, not normalised (ur[15] = 1).
  // pivmax: the largest |1 / pivot| of the elimination (the same in every lane of the quad) - see kMaxInversePivot
  static QMPS_CORE_FN void solve_gathered(const O& o, V (&M)[4][16], V (&ur)[16], V& pivmax) {
    V dinv[4];
    const V one = O::splat(1.0), zero = O::splat(0.0);
    V w[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) w[l] = O::sel(o.q_eq(l), one, zero);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int l = 0; l < 4; ++l) M[r][4 * l + r] = M[r][4 * l + r] - w[l];   // - identity: column 4 q + r
      dinv[r] = zero;
    }
    // + the trace functional on the LAST pivot row (lane 3, register 3), right-hand side e_15: the singular direction
    // of R - 1 is then resolved by the final pivot (measured on the 65536 Haar tensors of the benchmark: largest
    // residual ||T(r) - r||_F 1.1e-15, against 3.9e-13 with the functional on row 0).  No step adds a multiple of row 15 to another
    // row, so the right-hand side stays e_15 and is not carried: U u = e_15, solved up to the factor 1 / pivot_15 from u_15 = 1.
#pragma unroll
    for (int j = 0; j < 4; ++j) M[3][5 * j] = M[3][5 * j] + w[3];
    static_for<16>([&](auto K) {
      constexpr int k = decltype(K)::value, pl = k & 3, pr = k >> 2, a = piv_coord(k);
      // the pivot and the columns still to come of the pivot row, in every lane of the quad
      V prow[16];
      prow[a] = O::template bcast<pl>(M[pr][a]);
#pragma unroll
      for (int k2 = k + 1; k2 < 16; ++k2) prow[piv_coord(k2)] = O::template bcast<pl>(M[pr][piv_coord(k2)]);
      const V pinv = O::rcp(prow[a]);
      dinv[pr] = O::sel(o.q_eq(pl), pinv, dinv[pr]);
      // the pivot's own register: rows of the lanes behind the pivot lane only (the others are rows of U); it holds the next pivot row
      if (pl < 3) {
        const V f = O::sel(o.q_gt(pl), M[pr][a] * pinv, zero);
#pragma unroll
        for (int k2 = k + 1; k2 < 16; ++k2) M[pr][piv_coord(k2)] = O::fma(-f, prow[piv_coord(k2)], M[pr][piv_coord(k2)]);
      }
#pragma unroll
      for (int r = pr + 1; r < 4; ++r) {
        const V f = M[r][a] * pinv;
#pragma unroll
        for (int k2 = k + 1; k2 < 16; ++k2) M[r][piv_coord(k2)] = O::fma(-f, prow[piv_coord(k2)], M[r][piv_coord(k2)]);
      }
    });
    // back substitution, column j = 15 .. 1: s[r] += U[row][a(j)] u_a(j) for the rows in front of j in the pivot order - registers
    // < j / 4 in all lanes, register j / 4 in the lanes < j % 4 (no mask: the lanes >= j % 4 have read that sum for the last time) - the
    // sum that the next unknown waits for first; then u of the row in front: - s / pivot of its owner, to every lane.
    // (u_15 = 1: column 15 starts the sums as it is.)
    V s[4];
    ur[15] = one;
    static_for<15>([&](auto J) {
      constexpr int j = 15 - decltype(J)::value, pl = j & 3, pr = j >> 2, a = piv_coord(j);
      constexpr int nl = (j - 1) & 3, nr = (j - 1) >> 2;
#pragma unroll
      for (int r = pl > 0 ? pr : pr - 1; r >= 0; --r) {
        if constexpr (j == 15) s[r] = M[r][a];
        else s[r] = O::fma(M[r][a], ur[a], s[r]);
      }
      ur[piv_coord(j - 1)] = O::template bcast<nl>((-s[nr]) * dinv[nr]);
    });
    pivmax = O::qmax(O::vmax(O::vmax(O::vabs(dinv[0]), O::vabs(dinv[1])), O::vmax(O::vabs(dinv[2]), O::vabs(dinv[3]))));
  }

  // the lane's own coordinates out of all sixteen: x[r] = us[4 q + r]
  static QMPS_CORE_FN void own_coords(const O& o, const V (&us)[16], V (&x)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = O::sel(o.q_eq(0), us[r], O::sel(o.q_eq(1), us[4 + r], O::sel(o.q_eq(2), us[8 + r], us[12 + r])));
  }

  // solve_gathered's result as the lane's own four coordinates (not normalised): solve -> normalise -> gather gives the bits of
  // solve_gathered -> normalise_gathered.  The kernels call the pair; the CPU emulations of the test-suite call this one.
  static QMPS_CORE_FN void solve(const O& o, V (&M)[4][16], V (&x)[4], V& pivmax) {
    V ur[16];
    solve_gathered(o, M, ur, pivmax);
    own_coords(o, ur, x);
  }

  // scale to trace 1 with every coordinate in every lane: us = ur / tr, x = the lane's own four of them.  The sum has the association of
  // qsum (normalise), each product is the one normalise forms in the owner lane, and gather copies: the same bits.
  static QMPS_CORE_FN void normalise_gathered(const O& o, const V (&ur)[16], V (&us)[16], V (&x)[4]) {
    const V inv = O::rcp((ur[0] + ur[5]) + (ur[10] + ur[15]));
#pragma unroll
    for (int a = 0; a < 16; ++a) us[a] = ur[a] * inv;
    own_coords(o, us, x);
  }

  // A transfer map whose fixed point is NOT unique (degenerate dominant eigenvalue: product states, special angles of the
  // ansatz) makes the system singular to rounding; the elimination then returns SOME fixed point - it passes the acceptance
  // step like any other - which one being decided by rounding errors.  Such evaluations (a pivot below 1e-10) are handed to
  // the power method instead, which returns the projection of r_0 = 1/D onto the fixed-point space or reports that it does
  // not converge, exactly as the iterative solvers do.
  static constexpr double kMaxInversePivot = 1e10;

  // all sixteen coordinates in every lane: xs[4 l + r] = x[r] of lane l
  static QMPS_CORE_FN void gather(const V (&x)[4], V (&xs)[16]) {
    static_for<4>([&](auto L) {
      constexpr int l = decltype(L)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) xs[4 * l + r] = O::template bcast<l>(x[r]);
    });
  }

  // scale to trace 1 (the trace lives on the lanes' diagonal coordinates)
  static QMPS_CORE_FN V normalise(const O& o, V (&x)[4]) {
    const V tr = O::qsum(own_diag(o, x));
    const V inv = O::rcp(tr);
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = x[r] * inv;
    return inv;
  }

  // ||x - y||_F^2 of the two Hermitian matrices (the same in every lane of the quad)
  static QMPS_CORE_FN V dist2(const O& o, const V (&x)[4], const V (&y)[4]) {
    V d = O::splat(0.0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const V dd = y[r] - x[r];
      const V wt = O::sel(o.q_eq(r), O::splat(1.0), O::splat(2.0));
      d = O::fma(wt * dd, dd, d);
    }
    return O::qsum(d);
  }

  // ---- 3. one power step y = T(x)/tr straight from the tensor, and the squared Frobenius distance to x ----
  // us: the gathered coordinates of x.  Lane q forms row q of sum_s A_s r A_s^+ (X_s = A_s[q][:] r, then
  // X_s A_s^+) and keeps the real or imaginary part its coordinates call for.
  static QMPS_CORE_FN V power_step(const O& o, const V (&x)[4], const V (&us)[16], V (&y)[4]) {
    V xr[2][4], xi[2][4];
    own_rows_times_r(o, us, xr, xi);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      // r'[q][l] = sum_s sum_k X_s[k] conj(A_s[l][k])
      V cr = O::splat(0.0), ci = O::splat(0.0);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          V br, bi;
          o.uni(s, l, k, br, bi);
          cr = O::fma(xr[s][k], br, cr);
          cr = O::fma(xi[s][k], bi, cr);
          ci = O::fma(xi[s][k], br, ci);
          ci = O::fma(-xr[s][k], bi, ci);
        }
      y[l] = l == 3 ? cr : O::sel(o.q_gt(l), -ci, cr);     // u[(q,l)] = Re r'[q][l] (q <= l),  Im r'[l][q] = -Im r'[q][l] (q > l)
    }
    normalise(o, y);
    return dist2(o, x, y);
  }
  // X_s = A_s[q][:] r, s = 0, 1
  static QMPS_CORE_FN void own_rows_times_r(const O& o, const V (&us)[16], V (&xr)[2][4], V (&xi)[2][4]) {
    V ar[2][4], ai[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) o.own(s, j, ar[s][j], ai[s][j]);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        V cr = O::splat(0.0), ci = O::splat(0.0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const V rr = us[k <= l ? 4 * k + l : 4 * l + k];          // Re r[k][l]
          cr = O::fma(ar[s][k], rr, cr);
          ci = O::fma(ai[s][k], rr, ci);
          if (k != l) {
            const V ri = k < l ? us[4 * l + k] : -us[4 * k + l];    // Im r[k][l]
            cr = O::fma(-ai[s][k], ri, cr);
            ci = O::fma(ar[s][k], ri, ci);
          }
        }
        xr[s][l] = cr;
        xi[s][l] = ci;
      }
  }

  // ---- 3b. the same step with its two halves kept apart: row q of W_{t2 s2} = A_t2 r A_s2^+ = X_t2 A_s2^+, [t2][s2][l] ----
  // T(r) = W_00 + W_11; density_sites contracts the W with the tensor-only factors N (rho_site_factors), so the density matrix starts
  // from what the acceptance step has formed instead of from the tensor again.
  struct SiteW {
    V re[2][2][4], im[2][2][4];
  };
  // y = (W_00 + W_11)/tr and the distance to x, as power_step (another summation order: the halves are summed apart).  w: W_00 and W_11, and
  // whichever of W_01, W_10 the mask reads (rho_site_factors(need); wave-uniform tests) - the other one is NOT written.
  static QMPS_CORE_FN V power_step_sites(const O& o, const V (&x)[4], const V (&us)[16], uint32_t need, V (&y)[4], SiteW& w) {
    V xr[2][4], xi[2][4];
    own_rows_times_r(o, us, xr, xi);
    site_w(o, xr[0], xi[0], 0, w.re[0][0], w.im[0][0]);
    site_w(o, xr[1], xi[1], 1, w.re[1][1], w.im[1][1]);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const V cr = w.re[0][0][l] + w.re[1][1][l];
      y[l] = l == 3 ? cr : O::sel(o.q_gt(l), -(w.im[0][0][l] + w.im[1][1][l]), cr);
    }
    const uint32_t f = rho_site_factors(need);
    if (f & kSiteW01) site_w(o, xr[0], xi[0], 1, w.re[0][1], w.im[0][1]);
    if (f & kSiteW10) site_w(o, xr[1], xi[1], 0, w.re[1][0], w.im[1][0]);
    normalise(o, y);
    return dist2(o, x, y);
  }
  // (X A_s2^+)[l] = sum_k X[k] conj(A_s2[l][k])
  static QMPS_CORE_FN void site_w(const O& o, const V (&xr)[4], const V (&xi)[4], int s2, V (&wre)[4], V (&wim)[4]) {
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      V br, bi;
      o.uni(s2, l, 0, br, bi);
      V cr = O::fma(xi[0], bi, xr[0] * br), ci = O::fma(-xr[0], bi, xi[0] * br);
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        o.uni(s2, l, k, br, bi);
        cr = O::fma(xr[k], br, cr);
        cr = O::fma(xi[k], bi, cr);
        ci = O::fma(xi[k], br, ci);
        ci = O::fma(-xr[k], bi, ci);
      }
      wre[l] = cr;
      wim[l] = ci;
    }
  }
  // The W of another r (us) for the evaluations p; the others keep theirs, bit for bit - an evaluation whose environment changed after the
  // acceptance step (the power fall-back) takes the W of its final r.  The factors the mask reads, one at a time, each by the operations of
  // power_step_sites.
  static QMPS_CORE_FN void update_sites(const O& o, const V (&us)[16], uint32_t need, P p, SiteW& w) {
    V xr[2][4], xi[2][4];
    own_rows_times_r(o, us, xr, xi);
    const uint32_t f = rho_site_factors(need);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        if (t2 != s2 && !(f & (t2 == 0 ? kSiteW01 : kSiteW10))) continue;
        V tre[4], tim[4];
        site_w(o, xr[t2], xi[t2], s2, tre, tim);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          w.re[t2][s2][l] = O::sel(p, tre[l], w.re[t2][s2][l]);
          w.im[t2][s2][l] = O::sel(p, tim[l], w.im[t2][s2][l]);
        }
      }
  }

  // ---- 4. fall-back: the power method 2^m steps at a time from r_0 = 1/4, Rc <- Rc Rc in the quad layout ----
  // Reference formulation, run by the CPU emulation.  The device kernel runs the SAME recurrence one evaluation at a
  // time on the matrix cores (qmps_direct.hip: squaring_fallback; this form holds two 16 x 16 matrices per quad in
  // registers, which would cost the common path its register budget); tests/test_direct_gpu.py compares the two.
  static QMPS_CORE_FN void square(V (&Rc)[4][16]) {
    V out[4][16];
    static_for<16>([&](auto C) {
      constexpr int c = decltype(C)::value, cl = c >> 2, cr = c & 3;
      V rowc[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) rowc[j] = O::template bcast<cl>(Rc[cr][j]);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 16; ++j) out[r][j] = c == 0 ? Rc[r][c] * rowc[j] : O::fma(Rc[r][c], rowc[j], out[r][j]);
      QMPS_SCHED_FENCE();
    });
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j) Rc[r][j] = out[r][j];
  }

  // z_m = T^(2^m) r_0 / tr, stop at ||z_m - z_(m-1)||_F < tol;  steps = 2^m (as a value: it is per evaluation).
  // `active` lanes take part; converged ones are frozen.  Returns the still-unconverged predicate.
  static QMPS_CORE_FN P squaring(const O& o, V (&Rc)[4][16], P active, int max_iter, double tol2, V (&x)[4], V& steps) {
    V prev[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) prev[r] = O::sel(o.q_eq(r), O::splat(0.25), O::splat(0.0));
    int m = 0;
    while (O::any(active) && m < 29 && (2 << m) <= max_iter) {
      square(Rc);
      ++m;
      V z[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) z[r] = O::splat(0.25) * ((Rc[r][0] + Rc[r][5]) + (Rc[r][10] + Rc[r][15]));
      const V inv = normalise(o, z);
      // 1/tr(T^(2^m) r_0) ~ 1/lambda^(2^m): keeps the squared matrix at O(1) for tensors that are not isometries
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 16; ++j) Rc[r][j] = Rc[r][j] * inv;
      const P conv = O::lt(dist2(o, prev, z), O::splat(tol2));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        x[r] = O::sel(active, z[r], x[r]);
        prev[r] = z[r];
      }
      steps = O::sel(active, O::splat((double)(1 << m)), steps);
      active = O::p_and(active, O::p_not(conv));
    }
    return active;
  }

  // row q of B_tau = A_t1 A_t2, tau = 2 t1 + t2
  static QMPS_CORE_FN void b_rows(const O& o, V (&bre)[4][4], V (&bim)[4][4]) {
    V ar[2][4], ai[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) o.own(s, j, ar[s][j], ai[s][j]);
    // one row j of A_t2 at a time (8 values live instead of the whole matrix): B[(t1 t2)][k] += A_t1[q][j] A_t2[j][k]
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        V ur[4], ui[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o.uni(t2, j, k, ur[k], ui[k]);
#pragma unroll
        for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            V cr, ci;
            if (j == 0) {
              cr = ar[t1][0] * ur[k];
              ci = ar[t1][0] * ui[k];
            } else {
              cr = O::fma(ar[t1][j], ur[k], bre[2 * t1 + t2][k]);
              ci = O::fma(ar[t1][j], ui[k], bim[2 * t1 + t2][k]);
            }
            bre[2 * t1 + t2][k] = O::fma(-ai[t1][j], ui[k], cr);
            bim[2 * t1 + t2][k] = O::fma(ai[t1][j], ur[k], ci);
          }
      }
  }

  // ---- 5b. one energy without the density matrix (the energy-only contraction chain at high occupancy): with
  // C_sigma = sum_tau h[sigma,tau] B_tau (row q) and Z_sigma = C_sigma r,
  //   E = Re sum_sigma sum_l Z_sigma[l] conj(B_sigma[l])     ( = Re sum h[sigma,tau] tr(B_tau r B_sigma^+) )
  // - only the four B rows (b_rows, computed once for all terms) and r stay live (~150 registers against ~230 for the
  // rho route).  Returns the lane's share.
  static QMPS_CORE_FN V energy_lean(const V (&bre)[4][4], const V (&bim)[4][4], const V (&us)[16], const double* h) {
    V e = O::splat(0.0);
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) {
      V cr[4], ci[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        cr[l] = O::splat(0.0);
        ci[l] = O::splat(0.0);
      }
#pragma unroll
      for (int tau = 0; tau < 4; ++tau) {
        const V hr = O::splat(h[2 * (4 * sg + tau)]), hi = O::splat(h[2 * (4 * sg + tau) + 1]);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          cr[l] = O::fma(hr, bre[tau][l], cr[l]);
          cr[l] = O::fma(-hi, bim[tau][l], cr[l]);
          ci[l] = O::fma(hr, bim[tau][l], ci[l]);
          ci[l] = O::fma(hi, bre[tau][l], ci[l]);
        }
      }
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        // Z[l] = sum_k C[k] r[k][l];  r[k][l] for k <= l from (us[4k+l], us[4l+k]), the conjugate otherwise
        V zr = O::splat(0.0), zi = O::splat(0.0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const V rr = us[k <= l ? 4 * k + l : 4 * l + k];
          zr = O::fma(cr[k], rr, zr);
          zi = O::fma(ci[k], rr, zi);
          if (k != l) {
            const V ri = k < l ? us[4 * l + k] : -us[4 * k + l];
            zr = O::fma(-ci[k], ri, zr);
            zi = O::fma(cr[k], ri, zi);
          }
        }
        e = O::fma(zr, bre[sg][l], e);
        e = O::fma(zi, bim[sg][l], e);
      }
    }
    return e;
  }

  // r = L D L^H, replicated in the four lanes: rre / rim = r[k][l] (k <= l) out of the coordinates us, L strictly below the diagonal,
  // d the pivots as they come out; a pivot <= 0 divides as 1.  Returns "every pivot > 0".
  static QMPS_CORE_FN P ldl(const V (&us)[16], V (&rre)[4][4], V (&rim)[4][4], V (&lre)[4][4], V (&lim)[4][4], V (&d)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = k; l < 4; ++l) {
        rre[k][l] = us[4 * k + l];
        rim[k][l] = k == l ? O::splat(0.0) : us[4 * l + k];
      }
    P pd = O::gt0(rre[0][0]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      V dj = rre[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj = O::fma(-(lre[j][k] * lre[j][k] + lim[j][k] * lim[j][k]), d[k], dj);
      d[j] = dj;
      pd = O::p_and(pd, O::gt0(dj));
      const V inv = O::rcp(O::sel(O::gt0(dj), dj, O::splat(1.0)));
#pragma unroll
      for (int i = j + 1; i < 4; ++i) {
        V cr = rre[j][i], ci = -rim[j][i];   // r[i][j] = conj(r[j][i])
#pragma unroll
        for (int k = 0; k < j; ++k) {
          // L[i][k] conj(L[j][k]) d_k
          const V pr = lre[i][k] * lre[j][k] + lim[i][k] * lim[j][k];
          const V pi = lim[i][k] * lre[j][k] - lre[i][k] * lim[j][k];
          cr = O::fma(-pr, d[k], cr);
          ci = O::fma(-pi, d[k], ci);
        }
        lre[i][j] = cr * inv;
        lim[i][j] = ci * inv;
      }
    }
    return pd;
  }

  // ---- 5. positive-definiteness of r (LDL^H pivots > 0: the criterion of cholesky(r), qmps/tools.py:182) and the
  //         lane's share of the two-site density matrix rho[tau][sigma] = tr(B_tau r B_sigma^+), tau <= sigma ----
  // us: all sixteen coordinates of r (trace 1).  Lane q contributes row q of B_tau = A_t1 A_t2 (tau = 2 t1 + t2).
  static QMPS_CORE_FN P density(const O& o, const V (&us)[16], V (&pre)[4][4], V (&pim)[4][4]) {
    return density(o, us, kRhoNeedAll, pre, pim);
  }
  // need (rho_need_mask; the same for every lane of the wave): an entry whose bit is clear is not computed and left exactly 0.0 - in both
  // routes; the entries that are computed see the same operations in the same order whatever the mask
  static QMPS_CORE_FN P density(const O& o, const V (&us)[16], uint32_t need, V (&pre)[4][4], V (&pim)[4][4]) {
    V rre[4][4], rim[4][4], lre[4][4], lim[4][4], d[4];
    const P pd = ldl(us, rre, rim, lre, lim, d);
    V bre[4][4], bim[4][4];
    b_rows(o, bre, bim);
    // r = L D L^H:  rho[tau][sigma] = sum_k d_k G_tau[k] conj(G_sigma[k]) with G_tau = (row q of B_tau) L.  L is unit lower
    // triangular, so G costs 96 multiply-adds where Y_tau = B_tau r (below) costs 224.
#pragma unroll
    for (int tau = 0; tau < 4; ++tau)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        V cr = bre[tau][k], ci = bim[tau][k];
#pragma unroll
        for (int i = k + 1; i < 4; ++i) {
          cr = O::fma(bre[tau][i], lre[i][k], cr);
          cr = O::fma(-bim[tau][i], lim[i][k], cr);
          ci = O::fma(bre[tau][i], lim[i][k], ci);
          ci = O::fma(bim[tau][i], lre[i][k], ci);
        }
        bre[tau][k] = cr;      // (column k reads B[i], i > k: not overwritten yet)
        bim[tau][k] = ci;
      }
    computed_here(bre, bim);       // (the tests of rho_row follow)
#pragma unroll
    for (int tau = 0; tau < 4; ++tau) {
      V gre[4], gim[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gre[k] = bre[tau][k] * d[k];
        gim[k] = bim[tau][k] * d[k];
      }
      rho_row(tau, need, gre, gim, bre, bim, pre, pim);
    }
    // An r that fails the test is not what its factors give back (a pivot <= 0 was replaced by 1 above).  Those evaluations
    // take rho from Y_tau = (row q of B_tau) r instead: a rare branch, uniform over the wave on the device, in which every
    // evaluation keeps the route of its own test - no result depends on its wave-mates.
    QMPS_SCHED_FENCE();
    if (O::any(O::p_not(pd))) {
      b_rows(o, bre, bim);
      computed_here(bre, bim);
#pragma unroll
      for (int tau = 0; tau < 4; ++tau) {
        V yre[4], yim[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          V cr = O::splat(0.0), ci = O::splat(0.0);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            // r[k][l]: k <= l stored; k > l the conjugate of r[l][k]
            const V rr = k <= l ? rre[k][l] : rre[l][k];
            cr = O::fma(bre[tau][k], rr, cr);
            ci = O::fma(bim[tau][k], rr, ci);
            if (k != l) {
              const V ri = k < l ? rim[k][l] : -rim[l][k];
              cr = O::fma(-bim[tau][k], ri, cr);
              ci = O::fma(bre[tau][k], ri, ci);
            }
          }
          yre[l] = cr;
          yim[l] = ci;
          QMPS_COMPUTED_HERE(yre[l]);
          QMPS_COMPUTED_HERE(yim[l]);
        }
        V qre[4][4], qim[4][4];
        rho_row(tau, need, yre, yim, bre, bim, qre, qim);
#pragma unroll
        for (int sg = tau; sg < 4; ++sg) {
          pre[tau][sg] = O::sel(pd, pre[tau][sg], qre[tau][sg]);
          pim[tau][sg] = O::sel(pd, pim[tau][sg], qim[tau][sg]);
        }
      }
      QMPS_SCHED_FENCE();
    }
    return pd;
  }

  static QMPS_CORE_FN void computed_here(V (&bre)[4][4], V (&bim)[4][4]) {
#pragma unroll
    for (int tau = 0; tau < 4; ++tau)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        QMPS_COMPUTED_HERE(bre[tau][k]);
        QMPS_COMPUTED_HERE(bim[tau][k]);
      }
  }

  // rho[tau][sigma] += sum_l Y[l] conj(B_sigma[l]), sigma >= tau: the lane's share of row tau of rho
  static QMPS_CORE_FN void rho_row(int tau, const V (&yre)[4], const V (&yim)[4], const V (&bre)[4][4], const V (&bim)[4][4],
                                   V (&pre)[4][4], V (&pim)[4][4]) {
    rho_row(tau, kRhoNeedAll, yre, yim, bre, bim, pre, pim);
  }
  // ... of which only the parts `need` (rho_need_mask) asks for: a whole real or imaginary part (eight multiply-adds) per test
  static QMPS_CORE_FN void rho_row(int tau, uint32_t need, const V (&yre)[4], const V (&yim)[4], const V (&bre)[4][4],
                                   const V (&bim)[4][4], V (&pre)[4][4], V (&pim)[4][4]) {
#pragma unroll
    for (int sg = tau; sg < 4; ++sg) {
      V cr = O::splat(0.0);
      if ((need >> (4 * tau + sg)) & 1u) {
        cr = yre[0] * bre[sg][0];
        cr = O::fma(yim[0], bim[sg][0], cr);
#pragma unroll
        for (int l = 1; l < 4; ++l) {
          cr = O::fma(yre[l], bre[sg][l], cr);
          cr = O::fma(yim[l], bim[sg][l], cr);
        }
      }
      pre[tau][sg] = cr;
      pim[tau][sg] = O::splat(0.0);
    }
    // (the imaginary parts of the row behind one test of their own: a real Hamiltonian passes three tests, not six, and what the parts
    // share - the negated Y - stays inside)
    if ((need >> (16 + 4 * tau)) & 0xFu) {
#pragma unroll
      for (int sg = tau + 1; sg < 4; ++sg)
        if ((need >> (16 + 4 * tau + sg)) & 1u) {
          V ci = O::splat(0.0);
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            ci = O::fma(yim[l], bre[sg][l], ci);
            ci = O::fma(-yre[l], bim[sg][l], ci);
          }
          pim[tau][sg] = ci;
        }
    }
  }

  // ---- 5c. the same test and the same rho from the site factors: by cyclicity of the trace, for ANY tensor and ANY r,
  //   rho[tau][sigma] = tr(A_t1 A_t2 r A_s2^+ A_s1^+) = tr(N_{s1 t1} W_{t2 s2}),   N_{s1 t1} = A_s1^+ A_t1,   W_{t2 s2} = A_t2 r A_s2^+
  // and lane q's share is sum_l W_{t2 s2}[q][l] N_{s1 t1}[l][q]: row q of W (power_step_sites has it), column q of N (64 multiply-adds
  // from the tensor).  Where `density` pays 384 for B, G = B L and the pivot weights whatever the mask, this route pays 64 per factor
  // the mask reads on top of the acceptance step's W_00, W_11: 256 for TFIM and XXZ, 320 for every part.  r is not factored for rho, so
  // an r that fails the pivot test needs no route of its own.  One N is live at a time; a part the mask leaves out is exactly 0.0, and a
  // part that is computed sees the same operations in the same order whatever the mask.
  static QMPS_CORE_FN P density_sites(const O& o, const V (&us)[16], uint32_t need, const SiteW& w, V (&pre)[4][4], V (&pim)[4][4]) {
    P pd;
    {
      V rre[4][4], rim[4][4], lre[4][4], lim[4][4], d[4];
      pd = ldl(us, rre, rim, lre, lim, d);
    }
#pragma unroll
    for (int tau = 0; tau < 4; ++tau)
#pragma unroll
      for (int sg = tau; sg < 4; ++sg) {
        pre[tau][sg] = O::splat(0.0);
        pim[tau][sg] = O::splat(0.0);
      }
    static_for<3>([&](auto F) {
      constexpr int s1 = decltype(F)::value == 0 ? 0 : 1, t1 = decltype(F)::value == 2 ? 1 : 0;
      constexpr uint32_t parts = rho_site_parts(1u << decltype(F)::value);      // kSiteN00, kSiteN10, kSiteN11
      if (need & parts) {
        // column q of N_{s1 t1}: N[l][q] = sum_i conj(A_s1[i][l]) A_t1[i][q]
        V cr[4], ci[4], nre[4], nim[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o.col(t1, i, cr[i], ci[i]);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          V ur, ui;
          o.uni(s1, 0, l, ur, ui);
          V re = O::fma(ui, ci[0], ur * cr[0]), im = O::fma(-ui, cr[0], ur * ci[0]);
#pragma unroll
          for (int i = 1; i < 4; ++i) {
            o.uni(s1, i, l, ur, ui);
            re = O::fma(ur, cr[i], re);
            re = O::fma(ui, ci[i], re);
            im = O::fma(ur, ci[i], im);
            im = O::fma(-ui, cr[i], im);
          }
          nre[l] = re;
          nim[l] = im;
        }
#pragma unroll
        for (int l = 0; l < 4; ++l) {       // (the tests of the parts follow)
          QMPS_COMPUTED_HERE(nre[l]);
          QMPS_COMPUTED_HERE(nim[l]);
        }
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int tau = 2 * t1 + t2, sg = 2 * s1 + s2;
            if (tau > sg) continue;
            if ((need >> (4 * tau + sg)) & 1u) {
              V c = w.re[t2][s2][0] * nre[0];
              c = O::fma(-w.im[t2][s2][0], nim[0], c);
#pragma unroll
              for (int l = 1; l < 4; ++l) {
                c = O::fma(w.re[t2][s2][l], nre[l], c);
                c = O::fma(-w.im[t2][s2][l], nim[l], c);
              }
              pre[tau][sg] = c;
            }
          }
        // (the imaginary parts of the factor behind one test of their own: a real Hamiltonian passes three tests more, not nine)
        if ((need & parts) >> 16) {
#pragma unroll
          for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const int tau = 2 * t1 + t2, sg = 2 * s1 + s2;
              if (tau >= sg) continue;
              if ((need >> (16 + 4 * tau + sg)) & 1u) {
                V c = w.re[t2][s2][0] * nim[0];
                c = O::fma(w.im[t2][s2][0], nre[0], c);
#pragma unroll
                for (int l = 1; l < 4; ++l) {
                  c = O::fma(w.re[t2][s2][l], nim[l], c);
                  c = O::fma(w.im[t2][s2][l], nre[l], c);
                }
                pim[tau][sg] = c;
              }
            }
        }
      }
    });
    QMPS_SCHED_FENCE();
    return pd;
  }

  // E = Re sum_{s,t} h[s][t] rho[t][s] from the upper triangle of rho; h: 16 complex numbers (re, im interleaved),
  // the same for every lane
  static QMPS_CORE_FN V energy(const double* h, const V (&pre)[4][4], const V (&pim)[4][4]) {
    return energy(h, kRhoNeedAll, pre, pim);
  }
  // ... for a rho that density(need) left: without the multiply-adds of the imaginary parts when `need` holds none of them (every real
  // Hamiltonian) - one test for all twelve, two straight-line sums.  A part that `need` leaves out is exactly 0.0 and so is its h in every
  // term: whether it is multiplied or not, it adds +-0.0, which changes no bit of the sum - E is the full contraction's bit for bit.  (A test
  // per multiply-add, which the single real parts would need, costs the device more than the multiply-add: it is compiled to a select.)
  // H: const double*, or what reads like one (the device reads h through the constant address space: scalar loads)
  template <class H>
  static QMPS_CORE_FN V energy(H h, uint32_t need, const V (&pre)[4][4], const V (&pim)[4][4]) {
    V e = O::splat(0.0);
    if ((need >> 16) != 0u) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double hr = h[2 * (4 * s + t)], hi = h[2 * (4 * s + t) + 1];
          const V rr = t <= s ? pre[t][s] : pre[s][t];
          e = O::fma(O::splat(hr), rr, e);
          if (t != s) {
            const V ri = t < s ? pim[t][s] : -pim[s][t];
            e = O::fma(O::splat(-hi), ri, e);
          }
        }
        QMPS_COMPUTED_HERE(e);     // (a row of h at a time: all of it would not fit the device's scalar registers beside the rest)
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) e = O::fma(O::splat(h[2 * (4 * s + t)]), t <= s ? pre[t][s] : pre[s][t], e);
    }
    return e;
  }
};

}  // namespace qmps
