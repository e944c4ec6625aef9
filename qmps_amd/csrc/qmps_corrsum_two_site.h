// qmps_corrsum_two_site.h - the two-site source of the correlator sums (qmps_correlator_sums_two_site; the interface: qmps_corrsum_core.h).
// An operator is O[2 t1 + t2][2 s1 + s2] = o[t1][t2][s1][s2], site 1 the left one (the index of h in qmps_set_hamiltonian).  With
// X_(t s) = A_s r A_t^+ and W_(t s) = A_t^+ A_s (what the one-site source builds too) everything is staged, never contracted per
// right-hand side through an 8 x 8 x D^2 object:
//   Z^c_(t1 s1) = sum_(t2 s2) o_c[t1 t2 s1 s2] X_(t2 s2)      E2_c = sum_(t1 s1) A_s1 Z^c_(t1 s1) A_t1^+      b_c = E2_c - one[c] r
//   V^a_(t2 s2) = sum_(t1 s1) o_a[t1 t2 s1 s2] W_(t1 s1)      L_a  = sum_(t2 s2) A_t2^+ V^a_(t2 s2) A_s2
//   rho[t1 t2 s1 s2] = tr(W_(t1 s1) X_(t2 s2))                one[a] = O_a . rho / tau      near[a][c][0] = (O_a O_c) . rho / tau
//   Q^c_(t u)  = sum_s A_s Z^c_(u s) A_t^+                    near[a][c][1] = O_a . tr(W_(t1 s1) Q^c_(t2 u)) / tau       (O_c one site to the right)
//   Q'^a_(s u) = sum_t A_s Z^a_(t u) A_t^+                    near[a][c][2] = O_c . tr(W_(t1 s1) Q'^a_(s2 u)) / tau     (O_c one site to the left)
// where `.` sums the sixteen products over (t1 t2 s1 s2) - with u in the place of s2 for Q and of t2 for Q'.  The helpers work on
// one matrix element at a time; TwoSiteSource decides per kernel shape where the D x D intermediates live (registers, or LDS between
// barriers).
#pragma once
#include "qmps_complex.h"
#include "qmps_corrsum_core.h"

namespace qmps {

// z[t1][s1] = sum_(t2,s2) o[t1 t2 s1 s2] x[t2][s2]: the right site contracted
__device__ __forceinline__ void op2_right(const double2* O, const double2 (&x)[2][2], double2 (&z)[2][2]) {
#pragma unroll
  for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
    for (int s1 = 0; s1 < 2; ++s1) {
      double2 v = make_double2(0.0, 0.0);
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) cfma(O[(2 * t1 + t2) * 4 + 2 * s1 + s2], x[t2][s2], v);
      z[t1][s1] = v;
    }
}
// v[t2][s2] = sum_(t1,s1) o[t1 t2 s1 s2] w[t1][s1]: the left site contracted
__device__ __forceinline__ void op2_left(const double2* O, const double2 (&w)[2][2], double2 (&v)[2][2]) {
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      double2 a = make_double2(0.0, 0.0);
#pragma unroll
      for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
        for (int s1 = 0; s1 < 2; ++s1) cfma(O[(2 * t1 + t2) * 4 + 2 * s1 + s2], w[t1][s1], a);
      v[t2][s2] = a;
    }
}
// sum_e O[e] c[e] over the sixteen entries
__device__ __forceinline__ double2 op2_dot(const double2* O, const double2* c) {
  double2 v = make_double2(0.0, 0.0);
#pragma unroll
  for (int e = 0; e < 16; ++e) cfma(O[e], c[e], v);
  return v;
}
// sum_e (O_a O_c)[e] c[e], O_a O_c the 4 x 4 matrix product
__device__ __forceinline__ double2 op2_prod_dot(const double2* Oa, const double2* Oc, const double2* c) {
  double2 v = make_double2(0.0, 0.0);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double2 pr = cmul(Oa[t * 4], Oc[s]);
#pragma unroll
      for (int u = 1; u < 4; ++u) cfma(Oa[t * 4 + u], Oc[u * 4 + s], pr);
      cfma(pr, c[t * 4 + s], v);
    }
  return v;
}
// c[(2 t1 + t2) 4 + 2 s1 + s2] += w[t1][s1] y[t2][s2]: one element's share of the sixteen traces tr(W_(t1 s1) Y_(t2 s2))
__device__ __forceinline__ void cross_add(const double2 (&w)[2][2], const double2 (&y)[2][2], double2 (&c)[16]) {
#pragma unroll
  for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int s1 = 0; s1 < 2; ++s1)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) cfma(w[t1][s1], y[t2][s2], c[(2 * t1 + t2) * 4 + 2 * s1 + s2]);
}
__device__ __forceinline__ void cross_zero(double2 (&c)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = make_double2(0.0, 0.0);
}

// (A_s Z A_t^+)[i][j], Z row-major at Zm[k D + l]; A(s, i, k) reads the tensor
template <int D, class Tensor>
__device__ __forceinline__ double2 sandwich(const Tensor& A, const double2* Zm, int s, int t, int i, int j) {
  constexpr int kOuter = D <= 2 ? D : 1, kInner = D <= 4 ? D : 4;      // D = 2: straight-line code on registers; above: loops over LDS
  double2 v = make_double2(0.0, 0.0);
#pragma unroll kOuter
  for (int k = 0; k < D; ++k) {
    double2 u = make_double2(0.0, 0.0);
#pragma unroll kInner
    for (int l = 0; l < D; ++l) cfma_conj(Zm[k * D + l], A(t, j, l), u);
    cfma(A(s, i, k), u, v);
  }
  return v;
}
// (A_t^+ V A_s)[j][i] with V given transposed, Vt[l D + k] = V[k][l] (the storage of W and of lv: element (i, j) holds [j][i])
template <int D, class Tensor>
__device__ __forceinline__ double2 sandwich_left(const Tensor& A, const double2* Vt, int s, int t, int i, int j) {
  constexpr int kOuter = D <= 2 ? D : 1, kInner = D <= 4 ? D : 4;      // D = 2: straight-line code on registers; above: loops over LDS
  double2 v = make_double2(0.0, 0.0);
#pragma unroll kOuter
  for (int l = 0; l < D; ++l) {
    double2 u = make_double2(0.0, 0.0);
#pragma unroll kInner
    for (int k = 0; k < D; ++k) cfma_conj(Vt[l * D + k], A(t, k, j), u);
    cfma(A(s, l, i), u, v);
  }
  return v;
}
// The four D x D matrices of a stage lie `stride` apart: Zt + (2 p + q) stride is Z_(p q) (or V_(p q), transposed).
// E2[i][j] = sum_(p q) (A_q Z_(p q) A_p^+)[i][j]
template <int D, class Tensor>
__device__ __forceinline__ double2 two_site_source(const Tensor& A, const double2* Zt, int stride, int i, int j) {
  constexpr int kTerms = D <= 2 ? 4 : 1;
  double2 v = make_double2(0.0, 0.0);
#pragma unroll kTerms
  for (int pq = 0; pq < 4; ++pq) {
    const double2 x = sandwich<D>(A, Zt + pq * stride, pq & 1, pq >> 1, i, j);
    v.x += x.x;
    v.y += x.y;
  }
  return v;
}
// L[j][i] = sum_(p q) (A_p^+ V_(p q) A_q)[j][i]
template <int D, class Tensor>
__device__ __forceinline__ double2 two_site_left(const Tensor& A, const double2* Vt, int stride, int i, int j) {
  constexpr int kTerms = D <= 2 ? 4 : 1;
  double2 v = make_double2(0.0, 0.0);
#pragma unroll kTerms
  for (int pq = 0; pq < 4; ++pq) {
    const double2 x = sandwich_left<D>(A, Vt + pq * stride, pq & 1, pq >> 1, i, j);
    v.x += x.x;
    v.y += x.y;
  }
  return v;
}
// Q_(t u)[i][j] = sum_s (A_s Z_(u s) A_t^+)[i][j] for right = true (stored at [t][u]), Q'_(s u)[i][j] = sum_t (A_s Z_(t u) A_t^+)[i][j]
// for right = false (stored at [u][s], the bra place first): either way the place of `cross_add`'s y[t2][s2]
template <int D, class Tensor>
__device__ __forceinline__ double2 two_site_overlap(const Tensor& A, const double2* Zt, int stride, bool right, int first, int second, int i, int j) {
  constexpr int kTerms = D <= 2 ? 2 : 1;
  double2 v = make_double2(0.0, 0.0);
#pragma unroll kTerms
  for (int x = 0; x < 2; ++x) {
    // right: first = t, second = u, x = s;  left: first = u, second = s, x = t
    const double2 e = right ? sandwich<D>(A, Zt + (2 * second + x) * stride, x, first, i, j) : sandwich<D>(A, Zt + (2 * x + first) * stride, second, x, i, j);
    v.x += e.x;
    v.y += e.y;
  }
  return v;
}

// LDS of the block kernels beside BlockTiles: the stage in flight (Z^c, then V^a), the matrices of the near terms (afterwards L_a on
// its way to lv), the sources E2_c, and the sixteen traces of a cross product with `one`.  12 N + 20 complex values: 12 608 bytes at
// D = 8, 49 472 at D = 16.
template <int D>
struct TwoSiteTiles {
  static constexpr int N = D * D;
  double2 T[4][N];
  double2 Q[4][N];
  double2 E[kMaxObservableOps][N];
  double2 cross[16];
  double2 one[kMaxObservableOps];
};
template <int D>
struct TileTensor {
  const BlockTiles<D>* S;
  __device__ __forceinline__ double2 operator()(int s, int i, int k) const { return S->A[s][i][k]; }
};

// out[(2 t1 + t2) 4 + 2 s1 + s2] = sum_q Wt[2 t1 + s1][q] Yt[2 t2 + s2][q] = tr(W_(t1 s1) Y_(t2 s2)): 16 lanes per trace.  256 threads.
template <int N>
__device__ __forceinline__ void block_cross(const double2 (*Wt)[N], const double2 (*Yt)[N], double2* out, int tid) {
  const int e = tid >> 4, part = tid & 15;
  const int ws = ((e >> 3) & 1) * 2 + ((e >> 1) & 1), ys = ((e >> 2) & 1) * 2 + (e & 1);
  double2 v = make_double2(0.0, 0.0);
  for (int q = part; q < N; q += 16) cfma(Wt[ws][q], Yt[ys][q], v);
  v = make_double2(row16_sum(v.x), row16_sum(v.y));
  if (part == 0) out[e] = v;
}

struct TwoSiteSource {
  static constexpr int kOpEntries = kTwoSiteOpBytes / (int)sizeof(double2), kSiteValues = kTwoSiteSiteValues;

  static __device__ __forceinline__ double2 readout_scale(double2 z, double2 inv) { return cmul(cmul(z, z), inv); }

  // The lane kernel: everything in registers, every loop unrolled.  Fills the right-hand sides W[q][N + c] and lv; the j = 0 item
  // stores one and near.
  template <int M>
  static __device__ __forceinline__ void lane(const CorrSumArgs& p, int64_t b, bool first, const double2* Ab, const double2* rb, const double2* O,
                                              const double2 (&R)[4][2][2], const double2 (&tr)[2][2], double2 inv, double2 (&one)[M],
                                              double2 (&W)[4][4 + M], double2 (&lv)[4][M]) {
    constexpr int D = 2, N = 4;
    const GlobalTensor<D> At{Ab};
    double2 Wm[N][2][2], T[4][N];
#pragma unroll
    for (int q = 0; q < N; ++q) left_products<D>(Ab, q / D, q % D, Wm[q]);
    {
      double2 rho[16];
      cross_zero(rho);
#pragma unroll
      for (int q = 0; q < N; ++q) cross_add(Wm[q], R[q], rho);
#pragma unroll
      for (int a = 0; a < M; ++a) one[a] = cmul(op2_dot(O + kOpEntries * a, rho), inv);
      double2* near = (double2*)p.site;
      if (first) {
        if (p.one != nullptr) {
#pragma unroll
          for (int a = 0; a < M; ++a) ((double2*)p.one)[b * M + a] = one[a];
        }
        // the near terms in a pass of their own, before the right-hand sides exist: Z^c is built again below (16 complex FMAs per
        // element), which is cheaper than keeping the sixteen traces live beside the system
        if (near != nullptr) {
#pragma unroll
          for (int a = 0; a < M; ++a)
#pragma unroll
            for (int c = 0; c < M; ++c) near[((b * M + a) * M + c) * kSiteValues] = cmul(op2_prod_dot(O + kOpEntries * a, O + kOpEntries * c, rho), inv);
          // (c indexes no register array here: it stays a loop)
#pragma unroll 1
          for (int c = 0; c < M; ++c) {
#pragma unroll
            for (int q = 0; q < N; ++q) {
              double2 zq[2][2];
              op2_right(O + kOpEntries * c, R[q], zq);
#pragma unroll
              for (int ts = 0; ts < 4; ++ts) T[ts][q] = zq[ts >> 1][ts & 1];
            }
#pragma unroll
            for (int side = 0; side < 2; ++side) {
              cross_zero(rho);
#pragma unroll
              for (int q = 0; q < N; ++q) {
                double2 y[2][2];
#pragma unroll
                for (int f = 0; f < 2; ++f)
#pragma unroll
                  for (int g = 0; g < 2; ++g) y[f][g] = two_site_overlap<D>(At, &T[0][0], N, side == 0, f, g, q / D, q % D);
                cross_add(Wm[q], y, rho);
              }
              // side 0: O_c one site to the right of O_a, near[a][c][1]; side 1: this operator is the left argument, near[c][a][2]
#pragma unroll
              for (int a = 0; a < M; ++a) {
                const double2 v = cmul(op2_dot(O + kOpEntries * a, rho), inv);
                if (side == 0) near[((b * M + a) * M + c) * kSiteValues + 1] = v;
                else near[((b * M + c) * M + a) * kSiteValues + 2] = v;
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int q = 0; q < N; ++q) {
        double2 zq[2][2];
        op2_right(O + kOpEntries * c, R[q], zq);
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) T[ts][q] = zq[ts >> 1][ts & 1];
      }
#pragma unroll
      for (int q = 0; q < N; ++q) {
        double2 e = two_site_source<D>(At, &T[0][0], N, q / D, q % D);
        cfms(one[c], rb[q], e);
        W[q][N + c] = e;
      }
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
#pragma unroll
      for (int q = 0; q < N; ++q) {
        double2 v[2][2];
        op2_left(O + kOpEntries * a, Wm[q], v);
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) T[ts][q] = v[ts >> 1][ts & 1];
      }
#pragma unroll
      for (int q = 0; q < N; ++q) lv[q][a] = two_site_left<D>(At, &T[0][0], N, q / D, q % D);
    }
  }

  // The rows kernel: lane q = (i, j) of item g of the workgroup owns element [i][j] of every D x D intermediate; a stage whose
  // successor needs whole matrices (Z^c, then V^a) goes through the item's tile sT between two barriers.  Every lane of the workgroup
  // runs every barrier; `first` (the live j = 0 item: all 16 lanes of a row agree) only guards the near terms and the stores.
  template <int M>
  static __device__ __forceinline__ void rows(const CorrSumArgs& p, int64_t b, bool first, const double2* Ab, const double2* rb, const double2* O,
                                              const double2 (&R)[2][2], const double2 (&tr)[2][2], double2 inv, int q, int g, double2 (&one)[M],
                                              double2 (&row)[16 + M], double2 (&lv)[M]) {
    constexpr int D = 4, N = 16;
    __shared__ double2 sStage[kRowsItems][4][N];     // the stage in flight: Z^c, then V^a
    double2 (*sT)[N] = sStage[g];
    const int i = q / D, j = q % D;
    const GlobalTensor<D> At{Ab};
    double2 Wm[2][2], c16[16];
    left_products<D>(Ab, i, j, Wm);
    cross_zero(c16);
    cross_add(Wm, R, c16);
    row16_sum16(c16);
#pragma unroll
    for (int a = 0; a < M; ++a) one[a] = cmul(op2_dot(O + kOpEntries * a, c16), inv);
    double2* near = (double2*)p.site;
    if (first) {
      if (p.one != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a)
          if (q == a) ((double2*)p.one)[b * M + a] = one[a];
      }
      if (near != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
          for (int c = 0; c < M; ++c)
            if (q == a * M + c) near[((b * M + a) * M + c) * kSiteValues] = cmul(op2_prod_dot(O + kOpEntries * a, O + kOpEntries * c, c16), inv);
      }
    }
    // the near terms in a pass of their own (c indexes no register array here: a loop); every lane stages Z^c and runs the barriers
    if (near != nullptr) {
#pragma unroll 1
      for (int c = 0; c < M; ++c) {
        {
          double2 zq[2][2];
          op2_right(O + kOpEntries * c, R, zq);
#pragma unroll
          for (int ts = 0; ts < 4; ++ts) sT[ts][q] = zq[ts >> 1][ts & 1];
        }
        __syncthreads();
        if (first) {
#pragma unroll 1
          for (int side = 0; side < 2; ++side) {
            double2 y[2][2];
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
              for (int g = 0; g < 2; ++g) y[f][g] = two_site_overlap<D>(At, &sT[0][0], N, side == 0, f, g, i, j);
            cross_zero(c16);
            cross_add(Wm, y, c16);
            row16_sum16(c16);
            // side 0: O_c one site to the right of O_a, near[a][c][1]; side 1: this operator is the left argument, near[c][a][2]
#pragma unroll
            for (int a = 0; a < M; ++a)
              if (q == a) near[side == 0 ? ((b * M + a) * M + c) * kSiteValues + 1 : ((b * M + c) * M + a) * kSiteValues + 2] = cmul(op2_dot(O + kOpEntries * a, c16), inv);
          }
        }
        __syncthreads();
      }
    }
    const double2 rij = rb[q];
#pragma unroll
    for (int c = 0; c < M; ++c) {
      {
        double2 zq[2][2];
        op2_right(O + kOpEntries * c, R, zq);
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) sT[ts][q] = zq[ts >> 1][ts & 1];
      }
      __syncthreads();
      double2 e = two_site_source<D>(At, &sT[0][0], N, i, j);
      cfms(one[c], rij, e);
      row[N + c] = e;
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
      {
        double2 v[2][2];
        op2_left(O + kOpEntries * a, Wm, v);
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) sT[ts][q] = v[ts >> 1][ts & 1];
      }
      __syncthreads();
      lv[a] = two_site_left<D>(At, &sT[0][0], N, i, j);
      __syncthreads();
    }
  }

  // nothing per row: every stage above needs whole matrices, not one element
  template <int D, int M>
  static __device__ __forceinline__ void row_source(const double2* Ab, const double2* O, double2 rij, int i, int j, const double2 (&R)[2][2],
                                                    const double2 (&one)[M], double2 (&row)[D * D + M], double2 (&lv)[M]) {}

  // the tiles of a block kernel: LDS of the two-site instantiations only
  template <int D>
  static __device__ __forceinline__ TwoSiteTiles<D>& tiles() {
    __shared__ TwoSiteTiles<D> U;
    return U;
  }

  // After block_build (S.R = X, S.lv = W): U.one and U.E[c] = E2_c for block_rhs, S.lv[a] = L_a for the kernel, one and near to global
  // memory from the j = 0 item (`first`, the same in every thread).  256 threads; every thread runs every barrier.
  template <int D>
  static __device__ __forceinline__ void block_finish(BlockTiles<D>& S, const CorrSumArgs& p, int64_t b, bool first, const double2* O, int m,
                                                      double2 inv, const double2 (&tr)[2][2], int tid) {
    constexpr int N = D * D;
    TwoSiteTiles<D>& U = tiles<D>();
    const TileTensor<D> At{&S};
    double2* near = (double2*)p.site;
    const bool want_near = first && near != nullptr;
    block_cross<N>(S.lv, S.R, U.cross, tid);
    __syncthreads();
    if (tid < m) {
      const double2 o = cmul(op2_dot(O + kOpEntries * tid, U.cross), inv);
      U.one[tid] = o;
      if (first && p.one != nullptr) ((double2*)p.one)[b * m + tid] = o;
    }
    if (want_near && tid < m * m) near[(b * (m * m) + tid) * kSiteValues] = cmul(op2_prod_dot(O + kOpEntries * (tid / m), O + kOpEntries * (tid % m), U.cross), inv);
    __syncthreads();
    for (int c = 0; c < m; ++c) {
      for (int q = tid; q < N; q += 256) {
        double2 x[2][2], zq[2][2];
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) x[ts >> 1][ts & 1] = S.R[ts][q];
        op2_right(O + kOpEntries * c, x, zq);
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) U.T[ts][q] = zq[ts >> 1][ts & 1];
      }
      __syncthreads();
      for (int q = tid; q < N; q += 256) U.E[c][q] = two_site_source<D>(At, &U.T[0][0], N, q / D, q % D);
      if (want_near) {
        for (int side = 0; side < 2; ++side) {
          for (int e = tid; e < 4 * N; e += 256) {
            const int fg = e / N, q = e % N;
            U.Q[fg][q] = two_site_overlap<D>(At, &U.T[0][0], N, side == 0, fg >> 1, fg & 1, q / D, q % D);
          }
          __syncthreads();
          block_cross<N>(S.lv, U.Q, U.cross, tid);
          __syncthreads();
          // side 0: O_c one site to the right of O_a, near[a][c][1]; side 1: this operator is the left argument, near[c][a][2]
          if (tid < m) near[side == 0 ? ((b * m + tid) * m + c) * kSiteValues + 1 : ((b * m + c) * m + tid) * kSiteValues + 2] = cmul(op2_dot(O + kOpEntries * tid, U.cross), inv);
        }
      }
      __syncthreads();
    }
    for (int a = 0; a < m; ++a) {
      for (int q = tid; q < N; q += 256) {
        double2 w[2][2], v[2][2];
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.lv[ts][q];
        op2_left(O + kOpEntries * a, w, v);
#pragma unroll
        for (int ts = 0; ts < 4; ++ts) U.T[ts][q] = v[ts >> 1][ts & 1];
      }
      __syncthreads();
      for (int q = tid; q < N; q += 256) U.Q[a][q] = two_site_left<D>(At, &U.T[0][0], N, q / D, q % D);
      __syncthreads();
    }
    for (int q = tid; q < N; q += 256)
#pragma unroll
      for (int a = 0; a < kMaxObservableOps; ++a) S.lv[a][q] = a < m ? U.Q[a][q] : make_double2(0.0, 0.0);
    __syncthreads();
  }

  template <int D>
  static __device__ __forceinline__ double2 block_rhs(const BlockTiles<D>& S, const double2* O, double2 inv, const double2 (&tr)[2][2], double2 rij,
                                                      int c, int row) {
    const TwoSiteTiles<D>& U = tiles<D>();
    double2 e = U.E[c][row];
    cfms(U.one[c], rij, e);
    return e;
  }
};

}  // namespace qmps
