// qmps_corrsum_one_site.h - the one-site source of the correlator sums (qmps_correlator_sums; the interface: qmps_corrsum_core.h).  An
// operator is O[2 t + s] = <t|O|s>.  With R_(t s) = A_s r A_t^+ and W_(t s) = A_t^+ A_s:
//   b_c = sum_(t s) O_c[t][s] R_(t s) - one[c] r      L_a = sum_(t s) O_a[t][s] W_(t s)      one[a] = O_a . tr R / tau
//   site[a][c] = (O_a O_c) . tr R / tau                G scaled by z / tau (the sum starts at n = 1)
#pragma once
#include "qmps_corrsum_core.h"

namespace qmps {

// sum_(t,s) O[t][s] w[t][s]
__device__ __forceinline__ double2 op_dot(const double2* O, const double2 (&w)[2][2]) {
  double2 v = make_double2(0.0, 0.0);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) cfma(O[t * 2 + s], w[t][s], v);
  return v;
}
// sum_(t,s) (O_a O_c)[t][s] w[t][s]
__device__ __forceinline__ double2 op_prod_dot(const double2* Oa, const double2* Oc, const double2 (&w)[2][2]) {
  double2 v = make_double2(0.0, 0.0);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      double2 pr = cmul(Oa[t * 2], Oc[s]);
      cfma(Oa[t * 2 + 1], Oc[2 + s], pr);
      cfma(pr, w[t][s], v);
    }
  return v;
}

struct OneSiteSource {
  static constexpr int kOpEntries = kOneSiteOpBytes / (int)sizeof(double2), kSiteValues = kOneSiteSiteValues;

  static __device__ __forceinline__ double2 readout_scale(double2 z, double2 inv) { return cmul(z, inv); }

  // the M right-hand sides b_c[i][j] behind the matrix entries of row (i, j), and lv[a] = L_a[j][i]
  template <int D, int M>
  static __device__ __forceinline__ void row_source(const double2* Ab, const double2* O, double2 rij, int i, int j, const double2 (&R)[2][2],
                                                    const double2 (&one)[M], double2 (&row)[D * D + M], double2 (&lv)[M]) {
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double2 e = op_dot(O + kOpEntries * c, R);
      cfms(one[c], rij, e);
      row[D * D + c] = e;
    }
    double2 W[2][2];
    left_products<D>(Ab, i, j, W);
#pragma unroll
    for (int a = 0; a < M; ++a) lv[a] = op_dot(O + kOpEntries * a, W);
  }

  // D = 8, 16: `one` and `site` of evaluation b from the traces tr[t][s] = tr R_(t s); thread `tid` stores entry `tid` of either
  static __device__ __forceinline__ void store(const CorrSumArgs& p, int64_t b, const double2* O, int m, const double2 (&tr)[2][2], double2 inv, int tid) {
    if (p.one != nullptr && tid < m) ((double2*)p.one)[b * m + tid] = cmul(op_dot(O + kOpEntries * tid, tr), inv);
    if (p.site != nullptr && tid < m * m)
      ((double2*)p.site)[b * (m * m) + tid] = cmul(op_prod_dot(O + kOpEntries * (tid / m), O + kOpEntries * (tid % m), tr), inv);
  }

  // D = 2, 4: one[a] into registers, `one` and `site` from them (the right-hand sides and lv need one row's R alone: row_source).
  // D = 2: the lane stores every entry
  template <int M>
  static __device__ __forceinline__ void lane(const CorrSumArgs& p, int64_t b, bool first, const double2* Ab, const double2* rb, const double2* O,
                                              const double2 (&R)[4][2][2], const double2 (&tr)[2][2], double2 inv, double2 (&one)[M],
                                              double2 (&W)[4][4 + M], double2 (&lv)[4][M]) {
#pragma unroll
    for (int a = 0; a < M; ++a) one[a] = cmul(op_dot(O + kOpEntries * a, tr), inv);
    if (first) {
      if (p.one != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a) ((double2*)p.one)[b * M + a] = one[a];
      }
      if (p.site != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
          for (int c = 0; c < M; ++c) ((double2*)p.site)[(b * M + a) * M + c] = cmul(op_prod_dot(O + kOpEntries * a, O + kOpEntries * c, tr), inv);
      }
    }
  }
  // D = 4: lane q stores entry q (a select per entry: the values sit in registers under constant indices)
  template <int M>
  static __device__ __forceinline__ void rows(const CorrSumArgs& p, int64_t b, bool first, const double2* Ab, const double2* rb, const double2* O,
                                              const double2 (&R)[2][2], const double2 (&tr)[2][2], double2 inv, int q, int g, double2 (&one)[M],
                                              double2 (&row)[16 + M], double2 (&lv)[M]) {
#pragma unroll
    for (int a = 0; a < M; ++a) one[a] = cmul(op_dot(O + kOpEntries * a, tr), inv);
    if (first) {
      if (p.one != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a)
          if (q == a) ((double2*)p.one)[b * M + a] = one[a];
      }
      if (p.site != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
          for (int c = 0; c < M; ++c)
            if (q == a * M + c) ((double2*)p.site)[(b * M + a) * M + c] = cmul(op_prod_dot(O + kOpEntries * a, O + kOpEntries * c, tr), inv);
      }
    }
  }

  // lv[a][q] = sum_ts O_a[ts] W_ts[q]: every thread combines the four values block_build left for its q in registers, then overwrites
  template <int D>
  static __device__ __forceinline__ void block_finish(BlockTiles<D>& S, const CorrSumArgs& p, int64_t b, bool first, const double2* O, int m,
                                                      double2 inv, const double2 (&tr)[2][2], int tid) {
    for (int q = tid; q < D * D; q += 256) {
      double2 w[2][2];
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.lv[ts][q];
#pragma unroll
      for (int a = 0; a < kMaxObservableOps; ++a) S.lv[a][q] = a < m ? op_dot(O + kOpEntries * a, w) : make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (first) store(p, b, O, m, tr, inv, tid);
  }

  template <int D>
  static __device__ __forceinline__ double2 block_rhs(const BlockTiles<D>& S, const double2* O, double2 inv, const double2 (&tr)[2][2], double2 rij,
                                                      int c, int row) {
    double2 w[2][2];
#pragma unroll
    for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.R[ts][row];
    double2 e = op_dot(O + kOpEntries * c, w);
    cfms(cmul(op_dot(O + kOpEntries * c, tr), inv), rij, e);
    return e;
  }
};

}  // namespace qmps
