// qmps_corrsum_two_site.h - the two-site source of the correlator sums (qmps_correlator_sums_two_site; kernels: qmps_corrsum.hip).
// An operator is O[2 t1 + t2][2 s1 + s2] = o[t1][t2][s1][s2], site 1 the left one (the index of h in qmps_set_hamiltonian).  With
// X_(t s) = A_s r A_t^+ and W_(t s) = A_t^+ A_s (what the one-site source builds too) everything is staged, never contracted per
// right-hand side through an 8 x 8 x D^2 object:
//   Z^c_(t1 s1) = sum_(t2 s2) o_c[t1 t2 s1 s2] X_(t2 s2)      E2_c = sum_(t1 s1) A_s1 Z^c_(t1 s1) A_t1^+      b_c = E2_c - one[c] r
//   V^a_(t2 s2) = sum_(t1 s1) o_a[t1 t2 s1 s2] W_(t1 s1)      L_a  = sum_(t2 s2) A_t2^+ V^a_(t2 s2) A_s2
//   rho[t1 t2 s1 s2] = tr(W_(t1 s1) X_(t2 s2))                one[a] = O_a . rho / tau      near[a][c][0] = (O_a O_c) . rho / tau
//   Q^c_(t u)  = sum_s A_s Z^c_(u s) A_t^+                    near[a][c][1] = O_a . tr(W_(t1 s1) Q^c_(t2 u)) / tau       (O_c one site to the right)
//   Q'^a_(s u) = sum_t A_s Z^a_(t u) A_t^+                    near[a][c][2] = O_c . tr(W_(t1 s1) Q'^a_(s2 u)) / tau     (O_c one site to the left)
// where `.` sums the sixteen products over (t1 t2 s1 s2) - with u in the place of s2 for Q and of t2 for Q'.  The helpers work on
// one matrix element at a time; the kernels decide where the D x D intermediates live (registers, or LDS between barriers).
#pragma once
#include "qmps_complex.h"

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

}  // namespace qmps
