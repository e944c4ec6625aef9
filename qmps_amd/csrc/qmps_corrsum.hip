// qmps_corrsum.hip - correlator sums of the resident states (qmps_correlator_sums): for every evaluation b and every point z_j
//   G[j][a][c] = z_j tr(L_a (1 - z_j Tt)^(-1)(b_c)) / tau,   Tt(x) = T(x) - r tr(x) / tau,   b_c = E_{O_c}(r) - one[c] r,   tau = tr r,
//   E_O(x) = sum_{t,s} O[t][s] A_s x A_t^+,  T = E_1,  L_a = sum_{t,s} O_a[t][s] A_t^+ A_s,  one[a] = tr(E_{O_a}(r)) / tau,
//   site[a][c] = tr(E_{O_a O_c}(r)) / tau
// - the sum over n >= 1 of z^n times the connected two-point function, without truncation - in ONE launch.  A work item is one (b, j):
// a dense solve of order N = D^2 with n_ops right-hand sides.  Matrices are vectorised row-major (x[i][j] at i D + j), so the system
// matrix is  M[(i,j)][(k,l)] = delta - z (sum_s A_s[i][k] conj(A_s[j][l]) - delta_kl r[i][j] / tau);  it is built on the device.
//
// The elimination, the same in all four kernels (tests/structure_factor_cases.py `port` restates it in float64 numpy): Gauss-Jordan
// with partial (row) pivoting.  At step k the pivot is the row of largest |re| + |im| in column k among the rows not yet used (the
// lowest row at a tie; a NaN counts as infinite); rows stay where they are and remember the column they were pivot of.  The pivot row
// is scaled by the reciprocal of the pivot, every other row - used ones included - is eliminated in columns k + 1 .. N + n_ops - 1.
// With one row per lane / thread all rows advance in lock step, so eliminating above the pivot as well costs no time and leaves no
// back substitution: afterwards x_c[column of row] = rhs_c[row] and  G = z / tau sum_rows L_a[j][i](column of row) rhs_c[row].
// A pivot that is zero or not finite marks the item: its G is NaN; nothing else is affected.  tau zero or not finite gives NaN in
// every output of the evaluation (the reciprocal is NaN and spreads).
//
//   D = 2   one lane per item, matrix and right-hand sides in registers, pivot row picked by selects (no scratch)
//   D = 4   16 consecutive lanes per item, lane q owns row q (16 + n_ops complex values in registers); pivot search by DPP row
//           rotations, the scaled pivot row goes through LDS (one write, one broadcast read per value).  Lanes past the last item
//           compute a copy of it and store nothing
//   D = 8   one workgroup of 256 threads per item, the 64 x (64 + n_ops) matrix in LDS, column-major (lanes read consecutive rows:
//           no bank conflict; the pivot row is a broadcast read); wave w owns the columns = w mod 4
//   D = 16  one workgroup of 256 threads (thread = row) per item, the 256 x (256 + n_ops) matrix column-major in a global workspace
//           of one slab per workgroup; a fixed grid of at most kMaxSlabs workgroups strides over the items (workspace <= 256 MiB)
// L_a, one and b_c are built once per item, not per right-hand side or step; their cost, O(D^3), is small next to the O(D^6) solve.
// Every loop has a trip count fixed by D, n_ops and the item count; there are no atomics, counters or waits between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_observable.h"
#include "qmps_corrsum_two_site.h"

namespace qmps {

namespace {

// What fills the right-hand sides and lv, the read-out scale and what the j = 0 item stores: one-site operators as described above,
// or two-site ones (qmps_correlator_sums_two_site; formulas and builders in qmps_corrsum_two_site.h): b_c = E2_(O_c)(r) - one[c] r,
// L_a two-site, G scaled by z^2 / tau (the sum starts at n = 2), `site` receives near[a][c][0..2].  The matrix, the pivot search,
// the elimination and the read-out are the same code for both.
enum class Source { one_site, two_site };

template <Source SRC>
__device__ __forceinline__ double2 readout_scale(double2 z, double2 inv) {
  if constexpr (SRC == Source::two_site) return cmul(cmul(z, z), inv);
  else return cmul(z, inv);
}

// the tensor of one evaluation in global memory, A(s, i, k) = A_s[i][k]
template <int D>
struct GlobalTensor {
  const double2* p;
  __device__ __forceinline__ double2 operator()(int s, int i, int k) const { return p[(s * D + i) * D + k]; }
};

// the size a pivot candidate is ranked by: |re| + |im|, infinite for a NaN (it is then chosen and marks the item)
__device__ __forceinline__ double pivot_size(const double2 a) {
  const double v = fabs(a.x) + fabs(a.y);
  return v == v ? v : INFINITY;
}
__device__ __forceinline__ bool pivot_usable(const double v) { return v > 0.0 && v < INFINITY; }
__device__ __forceinline__ double2 csel(bool c, double2 a, double2 b) { return make_double2(c ? a.x : b.x, c ? a.y : b.y); }
__device__ __forceinline__ double2 cnan() { return make_double2(NAN, NAN); }

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

// ---- D = 2, 4: A and r read from global memory ---------------------------------------------------------------------------------
// R[t][s] = (A_s r A_t^+)[i][j]
template <int D>
__device__ __forceinline__ void pair_products(const double2* Ab, const double2* rb, int i, int j, double2 (&R)[2][2]) {
  double2 y[2][D];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int l = 0; l < D; ++l) {
      double2 v = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < D; ++k) cfma(Ab[(s * D + i) * D + k], rb[k * D + l], v);
      y[s][l] = v;
    }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      double2 v = make_double2(0.0, 0.0);
#pragma unroll
      for (int l = 0; l < D; ++l) cfma_conj(y[s][l], Ab[(t * D + j) * D + l], v);
      R[t][s] = v;
    }
}
// W[t][s] = (A_t^+ A_s)[j][i]
template <int D>
__device__ __forceinline__ void left_products(const double2* Ab, int i, int j, double2 (&W)[2][2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      double2 v = make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < D; ++k) cfma_cj(Ab[(t * D + k) * D + j], Ab[(s * D + k) * D + i], v);
      W[t][s] = v;
    }
}
// row (i, j) of the system: the D^2 matrix entries and, for one-site operators, the M right-hand sides b_c[i][j] and lv[a] = L_a[j][i]
// (the two-site source fills those itself: its stages need whole matrices, not one element)
template <int D, int M, Source SRC>
__device__ __forceinline__ void build_row(const double2* Ab, const double2* rb, const double2* O, double2 z, double2 inv, int i, int j,
                                          const double2 (&R)[2][2], const double2 (&one)[M], double2 (&row)[D * D + M], double2 (&lv)[M]) {
  constexpr int N = D * D;
  const double2 rij = rb[i * D + j], rs = cmul(rij, inv);
  const int q = i * D + j;
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int l = 0; l < D; ++l) {
      double2 t = make_double2(0.0, 0.0);
      cfma_conj(Ab[i * D + k], Ab[j * D + l], t);
      cfma_conj(Ab[(D + i) * D + k], Ab[(D + j) * D + l], t);
      if (k == l) {
        t.x -= rs.x;
        t.y -= rs.y;
      }
      double2 m = make_double2(k * D + l == q ? 1.0 : 0.0, 0.0);
      cfms(z, t, m);
      row[k * D + l] = m;
    }
  if constexpr (SRC == Source::one_site) {
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double2 e = op_dot(O + 4 * c, R);
      cfms(one[c], rij, e);
      row[N + c] = e;
    }
    double2 W[2][2];
    left_products<D>(Ab, i, j, W);
#pragma unroll
    for (int a = 0; a < M; ++a) lv[a] = op_dot(O + 4 * a, W);
  }
}

// The two-site source of the lane kernel: everything in registers, every loop unrolled.  Fills one, the right-hand sides W[q][N + c]
// and lv; the j = 0 item stores one and near.
template <int M>
__device__ __forceinline__ void lane_two_site(const CorrSumArgs& p, int64_t b, bool first, const double2* Ab, const double2* rb, const double2* O,
                                              const double2 (&R)[4][2][2], double2 inv, double2 (&one)[M], double2 (&W)[4][4 + M], double2 (&lv)[4][M]) {
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
    for (int a = 0; a < M; ++a) one[a] = cmul(op2_dot(O + 16 * a, rho), inv);
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
          for (int c = 0; c < M; ++c) near[((b * M + a) * M + c) * 3] = cmul(op2_prod_dot(O + 16 * a, O + 16 * c, rho), inv);
        // (c indexes no register array here: it stays a loop)
#pragma unroll 1
        for (int c = 0; c < M; ++c) {
#pragma unroll
          for (int q = 0; q < N; ++q) {
            double2 zq[2][2];
            op2_right(O + 16 * c, R[q], zq);
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
              const double2 v = cmul(op2_dot(O + 16 * a, rho), inv);
              if (side == 0) near[((b * M + a) * M + c) * 3 + 1] = v;
              else near[((b * M + c) * M + a) * 3 + 2] = v;
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
      op2_right(O + 16 * c, R[q], zq);
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
      op2_left(O + 16 * a, Wm[q], v);
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) T[ts][q] = v[ts >> 1][ts & 1];
    }
#pragma unroll
    for (int q = 0; q < N; ++q) lv[q][a] = two_site_left<D>(At, &T[0][0], N, q / D, q % D);
  }
}

template <int M, Source SRC>
__global__ __launch_bounds__(64) void corrsum_lane_kernel(CorrSumArgs p) {
  constexpr int D = 2, N = 4;
  const int64_t it = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (it >= p.B * p.n_z) return;
  const int64_t b = it / p.n_z;
  const int jz = (int)(it % p.n_z);
  const double2* Ab = (const double2*)p.A + b * (2 * N);
  const double2* rb = (const double2*)p.r + b * N;
  const double2* O = (const double2*)p.ops;
  const double2 z = ((const double2*)p.z)[jz];

  double2 R[N][2][2], tr[2][2];
#pragma unroll
  for (int q = 0; q < N; ++q) pair_products<D>(Ab, rb, q / D, q % D, R[q]);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) tr[t][s] = make_double2(R[0][t][s].x + R[3][t][s].x, R[0][t][s].y + R[3][t][s].y);
  const double2 inv = crecip(make_double2(rb[0].x + rb[3].x, rb[0].y + rb[3].y));
  double2 one[M];
  double2 W[N][N + M], lv[N][M];
  if constexpr (SRC == Source::one_site) {
#pragma unroll
    for (int a = 0; a < M; ++a) one[a] = cmul(op_dot(O + 4 * a, tr), inv);
    if (jz == 0) {
      if (p.one != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a) ((double2*)p.one)[b * M + a] = one[a];
      }
      if (p.site != nullptr) {
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
          for (int c = 0; c < M; ++c) ((double2*)p.site)[(b * M + a) * M + c] = cmul(op_prod_dot(O + 4 * a, O + 4 * c, tr), inv);
      }
    }
  } else {
    lane_two_site<M>(p, b, jz == 0, Ab, rb, O, R, inv, one, W, lv);
  }
#pragma unroll
  for (int q = 0; q < N; ++q) build_row<D, M, SRC>(Ab, rb, O, z, inv, q / D, q % D, R[q], one, W[q], lv[q]);

  bool used[N] = {false, false, false, false}, bad = false;
  int colof[N] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double best = -1.0;
    int pr = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const double v = used[q] ? -1.0 : pivot_size(W[q][k]);
      if (v > best) {
        best = v;
        pr = q;
      }
    }
    bad = bad || !pivot_usable(best);
    double2 piv[N + M];
#pragma unroll
    for (int c = k; c < N + M; ++c) piv[c] = csel(pr == 0, W[0][c], csel(pr == 1, W[1][c], csel(pr == 2, W[2][c], W[3][c])));
    const double2 ip = crecip(piv[k]);
#pragma unroll
    for (int c = k + 1; c < N + M; ++c) piv[c] = cmul(piv[c], ip);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const bool is = pr == q;
      used[q] = used[q] || is;
      colof[q] = is ? k : colof[q];
      const double2 f = W[q][k];
#pragma unroll
      for (int c = k + 1; c < N + M; ++c) {
        double2 v = W[q][c];
        cfms(f, piv[c], v);
        W[q][c] = csel(is, piv[c], v);
      }
    }
  }
  const double2 scale = readout_scale<SRC>(z, inv);
#pragma unroll
  for (int a = 0; a < M; ++a)
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double2 v = make_double2(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < N; ++q) {
        // L_a at the column row q was pivot of
        const double2 l = csel(colof[q] == 0, lv[0][a], csel(colof[q] == 1, lv[1][a], csel(colof[q] == 2, lv[2][a], lv[3][a])));
        cfma(l, W[q][N + c], v);
      }
      ((double2*)p.G)[(it * M + a) * M + c] = bad ? cnan() : cmul(scale, v);
    }
}

// ---- D = 4: 16 lanes per item -------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ int row_ror_i(int v) {
  return __builtin_amdgcn_mov_dpp(v, 0x120 + N, 0xf, 0xf, true);
}
__device__ __forceinline__ double row16_max(double v) {
  v = fmax(v, row_ror<8>(v));
  v = fmax(v, row_ror<4>(v));
  v = fmax(v, row_ror<2>(v));
  v = fmax(v, row_ror<1>(v));
  return v;
}
__device__ __forceinline__ int row16_min_i(int v) {
  v = min(v, row_ror_i<8>(v));
  v = min(v, row_ror_i<4>(v));
  v = min(v, row_ror_i<2>(v));
  v = min(v, row_ror_i<1>(v));
  return v;
}

// sum over the 16 lanes of an item of each of the sixteen cross terms
__device__ __forceinline__ void row16_sum16(double2 (&c)[16]) {
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = make_double2(row16_sum(c[e].x), row16_sum(c[e].y));
}

// The two-site source of the rows kernel: lane q = (i, j) owns element [i][j] of every D x D intermediate; a stage whose successor
// needs whole matrices (Z^c, then V^a) goes through the item's tile sT between two barriers.  Every lane of the workgroup runs every
// barrier; `first` (the live j = 0 item: all 16 lanes of a row agree) only guards the near terms and the stores.
template <int M>
__device__ __forceinline__ void rows_two_site(const CorrSumArgs& p, int64_t b, bool first, const double2* Ab, const double2* rb, const double2* O,
                                              const double2 (&R)[2][2], double2 inv, int q, double2 (*sT)[16], double2 (&one)[M],
                                              double2 (&row)[16 + M], double2 (&lv)[M]) {
  constexpr int D = 4, N = 16;
  const int i = q / D, j = q % D;
  const GlobalTensor<D> At{Ab};
  double2 Wm[2][2], c16[16];
  left_products<D>(Ab, i, j, Wm);
  cross_zero(c16);
  cross_add(Wm, R, c16);
  row16_sum16(c16);
#pragma unroll
  for (int a = 0; a < M; ++a) one[a] = cmul(op2_dot(O + 16 * a, c16), inv);
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
          if (q == a * M + c) near[((b * M + a) * M + c) * 3] = cmul(op2_prod_dot(O + 16 * a, O + 16 * c, c16), inv);
    }
  }
  // the near terms in a pass of their own (c indexes no register array here: a loop); every lane stages Z^c and runs the barriers
  if (near != nullptr) {
#pragma unroll 1
    for (int c = 0; c < M; ++c) {
      {
        double2 zq[2][2];
        op2_right(O + 16 * c, R, zq);
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
            if (q == a) near[side == 0 ? ((b * M + a) * M + c) * 3 + 1 : ((b * M + c) * M + a) * 3 + 2] = cmul(op2_dot(O + 16 * a, c16), inv);
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
      op2_right(O + 16 * c, R, zq);
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
      op2_left(O + 16 * a, Wm, v);
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) sT[ts][q] = v[ts >> 1][ts & 1];
    }
    __syncthreads();
    lv[a] = two_site_left<D>(At, &sT[0][0], N, i, j);
    __syncthreads();
  }
}

template <int M, Source SRC>
__global__ __launch_bounds__(64) void corrsum_rows_kernel(CorrSumArgs p) {
  constexpr int D = 4, N = 16, EV = 4;
  __shared__ double2 sPiv[EV][N + M];
  __shared__ double2 sL[EV][M][N];
  const int lane = threadIdx.x, g = lane / N, q = lane % N, i = q / D, j = q % D;
  const int64_t items = p.B * p.n_z, it0 = (int64_t)blockIdx.x * EV + g;
  const bool live = it0 < items;
  const int64_t it = live ? it0 : items - 1;
  const int64_t b = it / p.n_z;
  const int jz = (int)(it % p.n_z);
  const double2* Ab = (const double2*)p.A + b * (2 * N);
  const double2* rb = (const double2*)p.r + b * N;
  const double2* O = (const double2*)p.ops;
  const double2 z = ((const double2*)p.z)[jz];

  double2 R[2][2], tr[2][2];
  pair_products<D>(Ab, rb, i, j, R);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) tr[t][s] = make_double2(row16_sum(i == j ? R[t][s].x : 0.0), row16_sum(i == j ? R[t][s].y : 0.0));
  double2 inv;
  {
    const double2 rqq = rb[q * (i == j ? 1 : 0)];      // diagonal lanes read their own entry, the others r[0][0] (unused)
    inv = crecip(make_double2(row16_sum(i == j ? rqq.x : 0.0), row16_sum(i == j ? rqq.y : 0.0)));
  }
  double2 one[M];
  if constexpr (SRC == Source::one_site) {
#pragma unroll
    for (int a = 0; a < M; ++a) one[a] = cmul(op_dot(O + 4 * a, tr), inv);
    if (live && jz == 0) {
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
            if (q == a * M + c) ((double2*)p.site)[(b * M + a) * M + c] = cmul(op_prod_dot(O + 4 * a, O + 4 * c, tr), inv);
      }
    }
  }

  double2 row[N + M];
  {
    double2 lv[M];
    if constexpr (SRC == Source::two_site) {
      __shared__ double2 sT[EV][4][N];     // the stage in flight: Z^c, then V^a
      rows_two_site<M>(p, b, live && jz == 0, Ab, rb, O, R, inv, q, sT[g], one, row, lv);
    }
    build_row<D, M, SRC>(Ab, rb, O, z, inv, i, j, R, one, row, lv);
#pragma unroll
    for (int a = 0; a < M; ++a) sL[g][a][q] = lv[a];
  }

  bool used = false, bad = false;
  int colof = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double v = used ? -1.0 : pivot_size(row[k]);
    const double vmax = row16_max(v);
    const int pr = row16_min_i(v == vmax ? q : N);
    bad = bad || !pivot_usable(vmax);
    const bool is = pr == q;
    if (is) {
      const double2 ip = crecip(row[k]);
#pragma unroll
      for (int c = k + 1; c < N + M; ++c) {
        row[c] = cmul(row[c], ip);
        sPiv[g][c] = row[c];
      }
      used = true;
      colof = k;
    }
    __syncthreads();
    if (!is) {
      const double2 f = row[k];
#pragma unroll
      for (int c = k + 1; c < N + M; ++c) cfms(f, sPiv[g][c], row[c]);
    }
    __syncthreads();
  }

  const double2 scale = readout_scale<SRC>(z, inv);
  double2 out = make_double2(0.0, 0.0);
#pragma unroll
  for (int a = 0; a < M; ++a) {
    const double2 l = sL[g][a][colof];
#pragma unroll
    for (int c = 0; c < M; ++c) {
      const double2 w = cmul(l, row[N + c]);
      const double2 s = make_double2(row16_sum(w.x), row16_sum(w.y));
      out = csel(q == a * M + c, s, out);
    }
  }
  if (live && q < M * M) ((double2*)p.G)[it * (M * M) + q] = bad ? cnan() : cmul(scale, out);
}

// ---- D = 8, 16: one workgroup of 256 threads per item ------------------------------------------------------------------------------
// (largest pivot_size, lowest row that has it) over the wave, in every lane
__device__ __forceinline__ void wave_argmax(double& v, int& idx) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    const bool take = ov > v || (ov == v && oi < idx);
    v = take ? ov : v;
    idx = take ? oi : idx;
  }
}

// What both block kernels build in LDS before the matrix: A, r, R[ts][(i,j)] = (A_s r A_t^+)[i][j], lv[a][(i,j)] = L_a[j][i]; returns
// 1 / tau and the traces tr[t][s] = tr(A_s r A_t^+) in every thread.  256 threads.
template <int D>
struct BlockTiles {
  static constexpr int N = D * D, P = D + 1;
  double2 A[2][D][P];
  double2 r[D][P];
  double2 Y[2][D][P];
  double2 R[4][N];
  double2 lv[kMaxObservableOps][N];
};

template <int D, Source SRC>
__device__ __forceinline__ void block_build(BlockTiles<D>& S, const double2* Ab, const double2* rb, const double2* O, int n_ops, int tid,
                                            double2& inv, double2 (&tr)[2][2]) {
  constexpr int N = D * D;
  for (int e = tid; e < 2 * N; e += 256) S.A[e / N][(e % N) / D][e % D] = Ab[e];
  for (int e = tid; e < N; e += 256) S.r[e / D][e % D] = rb[e];
  __syncthreads();
  for (int e = tid; e < 2 * N; e += 256) {
    const int s = e / N, i = (e % N) / D, l = e % D;
    double2 v = make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < D; ++k) cfma(S.A[s][i][k], S.r[k][l], v);
    S.Y[s][i][l] = v;
  }
  __syncthreads();
  for (int e = tid; e < 4 * N; e += 256) {
    const int ts = e / N, t = ts >> 1, s = ts & 1, q = e % N, i = q / D, j = q % D;
    double2 v = make_double2(0.0, 0.0), w = make_double2(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < D; ++l) cfma_conj(S.Y[s][i][l], S.A[t][j][l], v);
    S.R[ts][q] = v;
    // (A_t^+ A_s)[j][i], parked in lv[ts] (kMaxObservableOps == 4 slots) until the operators are applied below
#pragma unroll
    for (int k = 0; k < D; ++k) cfma_cj(S.A[t][k][j], S.A[s][k][i], w);
    S.lv[ts][q] = w;
  }
  __syncthreads();
  double2 tau = make_double2(0.0, 0.0);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) tr[t][s] = make_double2(0.0, 0.0);
  for (int i = 0; i < D; ++i) {
    const double2 d = S.r[i][i];
    tau.x += d.x;
    tau.y += d.y;
#pragma unroll
    for (int ts = 0; ts < 4; ++ts) {
      const double2 x = S.R[ts][i * D + i];
      tr[ts >> 1][ts & 1].x += x.x;
      tr[ts >> 1][ts & 1].y += x.y;
    }
  }
  inv = crecip(tau);
  if constexpr (SRC == Source::two_site) return;      // W stays parked in lv: block_two_site turns it into V^a and L_a
  // lv[a][q] = sum_ts O_a[ts] w_ts[q]: every thread combines the four stashed values of its q in registers, then overwrites
  for (int q = tid; q < N; q += 256) {
    double2 w[2][2];
#pragma unroll
    for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.lv[ts][q];
#pragma unroll
    for (int a = 0; a < kMaxObservableOps; ++a) S.lv[a][q] = a < n_ops ? op_dot(O + 4 * a, w) : make_double2(0.0, 0.0);
  }
  __syncthreads();
}

// ---- the two-site source of the block kernels ------------------------------------------------------------------------------------------
// LDS beside BlockTiles: the stage in flight (Z^c, then V^a), the matrices of the near terms (afterwards L_a on its way to lv), the
// sources E2_c, and the sixteen traces of a cross product with `one`.  12 N + 20 complex values: 12 608 bytes at D = 8, 49 472 at D = 16.
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

// After block_build<D, two_site> (S.R = X, S.lv = W): U.one, U.E[c] = E2_c and S.lv[a] = L_a for the kernel, one and near to
// global memory from the j = 0 item (`first`, the same in every thread).  256 threads; every thread runs every barrier.
template <int D>
__device__ __forceinline__ void block_two_site(BlockTiles<D>& S, TwoSiteTiles<D>& U, const CorrSumArgs& p, int64_t b, bool first, const double2* O, int m,
                                               double2 inv, int tid) {
  constexpr int N = D * D;
  const TileTensor<D> At{&S};
  double2* near = (double2*)p.site;
  const bool want_near = first && near != nullptr;
  block_cross<N>(S.lv, S.R, U.cross, tid);
  __syncthreads();
  if (tid < m) {
    const double2 o = cmul(op2_dot(O + 16 * tid, U.cross), inv);
    U.one[tid] = o;
    if (first && p.one != nullptr) ((double2*)p.one)[b * m + tid] = o;
  }
  if (want_near && tid < m * m) near[(b * (m * m) + tid) * 3] = cmul(op2_prod_dot(O + 16 * (tid / m), O + 16 * (tid % m), U.cross), inv);
  __syncthreads();
  for (int c = 0; c < m; ++c) {
    for (int q = tid; q < N; q += 256) {
      double2 x[2][2], zq[2][2];
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) x[ts >> 1][ts & 1] = S.R[ts][q];
      op2_right(O + 16 * c, x, zq);
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
        if (tid < m) near[side == 0 ? ((b * m + tid) * m + c) * 3 + 1 : ((b * m + c) * m + tid) * 3 + 2] = cmul(op2_dot(O + 16 * tid, U.cross), inv);
      }
    }
    __syncthreads();
  }
  for (int a = 0; a < m; ++a) {
    for (int q = tid; q < N; q += 256) {
      double2 w[2][2], v[2][2];
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.lv[ts][q];
      op2_left(O + 16 * a, w, v);
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

// entry ((i,j), (k,l)) of 1 - z Tt from the tiles
template <int D>
__device__ __forceinline__ double2 matrix_entry(const BlockTiles<D>& S, double2 z, double2 rs, int i, int j, int k, int l) {
  double2 t = make_double2(0.0, 0.0);
  cfma_conj(S.A[0][i][k], S.A[0][j][l], t);
  cfma_conj(S.A[1][i][k], S.A[1][j][l], t);
  if (k == l) {
    t.x -= rs.x;
    t.y -= rs.y;
  }
  double2 m = make_double2(i == k && j == l ? 1.0 : 0.0, 0.0);
  cfms(z, t, m);
  return m;
}

// `one` and `site` of evaluation b from the traces (the item with j = 0 stores them)
__device__ __forceinline__ void store_one_site(const CorrSumArgs& p, int64_t b, const double2* O, const double2 (&tr)[2][2], double2 inv, int tid) {
  const int m = p.n_ops;
  if (p.one != nullptr && tid < m) ((double2*)p.one)[b * m + tid] = cmul(op_dot(O + 4 * tid, tr), inv);
  if (p.site != nullptr && tid < m * m) ((double2*)p.site)[b * (m * m) + tid] = cmul(op_prod_dot(O + 4 * (tid / m), O + 4 * (tid % m), tr), inv);
}

template <Source SRC>
__global__ __launch_bounds__(256) void corrsum_lds_kernel(CorrSumArgs p) {
  constexpr int D = 8, N = 64, NC = N + kMaxObservableOps;
  __shared__ double2 sW[NC][N];          // column-major: sW[column][row]
  __shared__ BlockTiles<D> S;
  __shared__ double2 sPiv[NC];
  const int tid = threadIdx.x, row = tid % N, part = tid / N, i = row / D, j = row % D;
  const int64_t it = blockIdx.x;
  const int64_t b = it / p.n_z;
  const int jz = (int)(it % p.n_z);
  const int m = p.n_ops, nc = N + m;
  const double2* O = (const double2*)p.ops;
  const double2 z = ((const double2*)p.z)[jz];
  double2 inv, tr[2][2];
  block_build<D, SRC>(S, (const double2*)p.A + b * (2 * N), (const double2*)p.r + b * N, O, m, tid, inv, tr);
  if constexpr (SRC == Source::one_site) {
    if (jz == 0) store_one_site(p, b, O, tr, inv, tid);
    const double2 rij = S.r[i][j], rs = cmul(rij, inv);
    for (int c = part; c < N; c += 4) sW[c][row] = matrix_entry<D>(S, z, rs, i, j, c / D, c % D);
    if (part < m) {
      double2 w[2][2];
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.R[ts][row];
      double2 e = op_dot(O + 4 * part, w);
      cfms(cmul(op_dot(O + 4 * part, tr), inv), rij, e);
      sW[N + part][row] = e;
    }
  } else {
    __shared__ TwoSiteTiles<D> U;
    block_two_site<D>(S, U, p, b, jz == 0, O, m, inv, tid);
    const double2 rij = S.r[i][j], rs = cmul(rij, inv);
    for (int c = part; c < N; c += 4) sW[c][row] = matrix_entry<D>(S, z, rs, i, j, c / D, c % D);
    if (part < m) {
      double2 e = U.E[part][row];
      cfms(U.one[part], rij, e);
      sW[N + part][row] = e;
    }
  }
  __syncthreads();

  bool used = false, bad = false;
  int colof = 0;
  for (int k = 0; k < N; ++k) {
    const double2 f = sW[k][row];
    double v = used ? -1.0 : pivot_size(f);
    int pr = row;
    wave_argmax(v, pr);                  // every wave searches the whole column: the same answer in all four
    bad = bad || !pivot_usable(v);
    const bool is = pr == row;
    const double2 ip = crecip(sW[k][pr]);
    for (int c = k + 1 + tid; c < nc; c += 256) sPiv[c] = cmul(sW[c][pr], ip);
    __syncthreads();
    for (int c = k + 1 + part; c < nc; c += 4) {
      const double2 pv = sPiv[c];
      double2 x = sW[c][row];
      cfms(f, pv, x);
      sW[c][row] = csel(is, pv, x);
    }
    used = used || is;
    colof = is ? k : colof;
    __syncthreads();
  }

  // wave c sums column N + c against every L_a
  if (part < m) {
    const double2 x = sW[N + part][row];
    const double2 scale = readout_scale<SRC>(z, inv);
    for (int a = 0; a < m; ++a) {
      const double2 w = cmul(S.lv[a][colof], x);
      const double2 s = make_double2(wave_sum(w.x), wave_sum(w.y));
      if (row == 0) ((double2*)p.G)[(it * m + a) * m + part] = bad ? cnan() : cmul(scale, s);
    }
  }
}

constexpr int kSlabColumns = 256 + kMaxObservableOps;
constexpr size_t kSlabBytes = (size_t)kSlabColumns * 256 * sizeof(double2);

template <Source SRC>
__global__ __launch_bounds__(256) void corrsum_global_kernel(CorrSumArgs p) {
  constexpr int D = 16, N = 256;
  __shared__ BlockTiles<D> S;
  __shared__ double2 sPiv[kSlabColumns];
  __shared__ double sRedV[4];
  __shared__ int sRedI[4];
  __shared__ double sSum[4][2 * kMaxObservableOps * kMaxObservableOps];
  const int tid = threadIdx.x, row = tid, i = row / D, j = row % D, wave = tid >> 6;
  const int m = p.n_ops, nc = N + m;
  const double2* O = (const double2*)p.ops;
  double2* Wg = (double2*)((char*)p.work + (size_t)blockIdx.x * kSlabBytes);      // column-major: Wg[column * N + row]
  const int64_t items = p.B * p.n_z;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t b = it / p.n_z;
    const int jz = (int)(it % p.n_z);
    const double2 z = ((const double2*)p.z)[jz];
    double2 inv, tr[2][2];
    block_build<D, SRC>(S, (const double2*)p.A + b * (2 * N), (const double2*)p.r + b * N, O, m, tid, inv, tr);
    if constexpr (SRC == Source::one_site) {
      if (jz == 0) store_one_site(p, b, O, tr, inv, tid);
      const double2 rij = S.r[i][j], rs = cmul(rij, inv);
      for (int c = 0; c < N; ++c) Wg[c * N + row] = matrix_entry<D>(S, z, rs, i, j, c / D, c % D);
      double2 w[2][2];
#pragma unroll
      for (int ts = 0; ts < 4; ++ts) w[ts >> 1][ts & 1] = S.R[ts][row];
      for (int c = 0; c < m; ++c) {
        double2 e = op_dot(O + 4 * c, w);
        cfms(cmul(op_dot(O + 4 * c, tr), inv), rij, e);
        Wg[(N + c) * N + row] = e;
      }
    } else {
      __shared__ TwoSiteTiles<D> U;
      block_two_site<D>(S, U, p, b, jz == 0, O, m, inv, tid);
      const double2 rij = S.r[i][j], rs = cmul(rij, inv);
      for (int c = 0; c < N; ++c) Wg[c * N + row] = matrix_entry<D>(S, z, rs, i, j, c / D, c % D);
      for (int c = 0; c < m; ++c) {
        double2 e = U.E[c][row];
        cfms(U.one[c], rij, e);
        Wg[(N + c) * N + row] = e;
      }
    }
    __syncthreads();

    bool used = false, bad = false;
    int colof = 0;
    for (int k = 0; k < N; ++k) {
      const double2 f = Wg[k * N + row];
      double v = used ? -1.0 : pivot_size(f);
      int pr = row;
      wave_argmax(v, pr);
      if ((tid & 63) == 0) {
        sRedV[wave] = v;
        sRedI[wave] = pr;
      }
      __syncthreads();
      v = sRedV[0];
      pr = sRedI[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const double ov = sRedV[w];
        const int oi = sRedI[w];
        if (ov > v) {                    // rows of a later wave are higher: a tie keeps the earlier one
          v = ov;
          pr = oi;
        }
      }
      bad = bad || !pivot_usable(v);
      const bool is = pr == row;
      const double2 ip = crecip(Wg[k * N + pr]);
      for (int c = k + 1 + tid; c < nc; c += 256) sPiv[c] = cmul(Wg[c * N + pr], ip);
      __syncthreads();
#pragma unroll 4
      for (int c = k + 1; c < nc; ++c) {
        const double2 pv = sPiv[c];
        double2 x = Wg[c * N + row];
        cfms(f, pv, x);
        Wg[c * N + row] = csel(is, pv, x);
      }
      used = used || is;
      colof = is ? k : colof;
      __syncthreads();
    }

    for (int c = 0; c < m; ++c) {
      const double2 x = Wg[(N + c) * N + row];
      for (int a = 0; a < m; ++a) {
        const double2 w = cmul(S.lv[a][colof], x);
        const double sx = wave_sum(w.x), sy = wave_sum(w.y);
        if ((tid & 63) == 0) {
          sSum[wave][2 * (a * m + c)] = sx;
          sSum[wave][2 * (a * m + c) + 1] = sy;
        }
      }
    }
    __syncthreads();
    if (tid < m * m) {
      double2 s = make_double2(0.0, 0.0);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        s.x += sSum[w][2 * tid];
        s.y += sSum[w][2 * tid + 1];
      }
      ((double2*)p.G)[it * (m * m) + tid] = bad ? cnan() : cmul(readout_scale<SRC>(z, inv), s);
    }
    __syncthreads();                     // the tiles and the slab are rebuilt for the next item
  }
}

template <int M, Source SRC>
void launch_small(int D, const CorrSumArgs& a, int64_t items, hipStream_t st) {
  if (D == 2) hipLaunchKernelGGL((corrsum_lane_kernel<M, SRC>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((corrsum_rows_kernel<M, SRC>), dim3((unsigned)((items + 3) / 4)), dim3(64), 0, st, a);
}

template <Source SRC>
hipError_t launch_source(int D, const CorrSumArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.n_ops < 1 || a.n_ops > kMaxObservableOps || a.n_z < 1) return hipErrorInvalidValue;
  const int64_t items = a.B * a.n_z;
  switch (D) {
    case 2:
    case 4:
      switch (a.n_ops) {
        case 1: launch_small<1, SRC>(D, a, items, st); break;
        case 2: launch_small<2, SRC>(D, a, items, st); break;
        case 3: launch_small<3, SRC>(D, a, items, st); break;
        default: launch_small<4, SRC>(D, a, items, st); break;
      }
      break;
    case 8: hipLaunchKernelGGL(corrsum_lds_kernel<SRC>, dim3((unsigned)items), dim3(256), 0, st, a); break;
    case 16:
      if (a.work == nullptr || a.n_slabs < 1 || a.n_slabs > kCorrSumMaxSlabs) return hipErrorInvalidValue;
      hipLaunchKernelGGL(corrsum_global_kernel<SRC>, dim3((unsigned)(items < a.n_slabs ? items : a.n_slabs)), dim3(256), 0, st, a);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

int64_t correlator_sums_slabs(int D, int64_t items) {
  if (D != 16) return 0;
  return items < kCorrSumMaxSlabs ? items : kCorrSumMaxSlabs;
}
size_t correlator_sums_slab_bytes() { return kSlabBytes; }

hipError_t launch_correlator_sums(int D, const CorrSumArgs& a, hipStream_t st) { return launch_source<Source::one_site>(D, a, st); }
hipError_t launch_correlator_sums_two_site(int D, const CorrSumArgs& a, hipStream_t st) { return launch_source<Source::two_site>(D, a, st); }

}  // namespace qmps
