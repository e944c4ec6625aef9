// rho_reference.h - TEST INFRASTRUCTURE ONLY.  DirectD4::density / rho_row / energy as they stood before the "needed entries" mask
// (qmps_amd/csrc/qmps_direct_core.h), kept word for word as the reference of tests/test_rho_need_cpu.py: the masked routes - and the
// routes without a mask, which now forward to them with every bit set - must give these functions' results bit for bit.  An operation
// reordered in qmps_direct_core.h shows against this copy, where a comparison of the new code with itself under two masks would not.
#pragma once

#include "qmps_direct_core.h"

namespace qmps_test {

template <class O>
struct RhoReference {
  using V = typename O::V;
  using P = typename O::P;
  using Core = qmps::DirectD4<O>;

  // ---- 5. positive-definiteness of r (LDL^H pivots > 0: the criterion of cholesky(r), qmps/tools.py:182) and the
  //         lane's share of the two-site density matrix rho[tau][sigma] = tr(B_tau r B_sigma^+), tau <= sigma ----
  // us: all sixteen coordinates of r (trace 1).  Lane q contributes row q of B_tau = A_t1 A_t2 (tau = 2 t1 + t2).
  static QMPS_CORE_FN P density(const O& o, const V (&us)[16], V (&pre)[4][4], V (&pim)[4][4]) {
    // r[k][l], k <= l
    V rre[4][4], rim[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = k; l < 4; ++l) {
        rre[k][l] = us[4 * k + l];
        rim[k][l] = k == l ? O::splat(0.0) : us[4 * l + k];
      }
    // LDL^H (replicated in the four lanes)
    P pd = O::gt0(rre[0][0]);
    V lre[4][4], lim[4][4], d[4];
    {
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
    }
    V bre[4][4], bim[4][4];
    Core::b_rows(o, bre, bim);
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
#pragma unroll
    for (int tau = 0; tau < 4; ++tau) {
      V gre[4], gim[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gre[k] = bre[tau][k] * d[k];
        gim[k] = bim[tau][k] * d[k];
      }
      rho_row(tau, gre, gim, bre, bim, pre, pim);
    }
    // An r that fails the test is not what its factors give back (a pivot <= 0 was replaced by 1 above).  Those evaluations
    // take rho from Y_tau = (row q of B_tau) r instead: a rare branch, uniform over the wave on the device, in which every
    // evaluation keeps the route of its own test - no result depends on its wave-mates.
    QMPS_SCHED_FENCE();
    if (O::any(O::p_not(pd))) {
      Core::b_rows(o, bre, bim);
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
        }
        V qre[4][4], qim[4][4];
        rho_row(tau, yre, yim, bre, bim, qre, qim);
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

  // rho[tau][sigma] += sum_l Y[l] conj(B_sigma[l]), sigma >= tau: the lane's share of row tau of rho
  static QMPS_CORE_FN void rho_row(int tau, const V (&yre)[4], const V (&yim)[4], const V (&bre)[4][4], const V (&bim)[4][4],
                                   V (&pre)[4][4], V (&pim)[4][4]) {
#pragma unroll
    for (int sg = tau; sg < 4; ++sg) {
      V cr = yre[0] * bre[sg][0], ci = O::splat(0.0);
      cr = O::fma(yim[0], bim[sg][0], cr);
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        if (l > 0) {
          cr = O::fma(yre[l], bre[sg][l], cr);
          cr = O::fma(yim[l], bim[sg][l], cr);
        }
        if (sg != tau) {
          ci = O::fma(yim[l], bre[sg][l], ci);
          ci = O::fma(-yre[l], bim[sg][l], ci);
        }
      }
      pre[tau][sg] = cr;
      pim[tau][sg] = ci;
    }
  }

  // E = Re sum_{s,t} h[s][t] rho[t][s] from the upper triangle of rho; h: 16 complex numbers (re, im interleaved),
  // the same for every lane
  static QMPS_CORE_FN V energy(const double* h, const V (&pre)[4][4], const V (&pim)[4][4]) {
    V e = O::splat(0.0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
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
    return e;
  }
};

}  // namespace qmps_test
