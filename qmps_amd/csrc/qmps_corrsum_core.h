// qmps_corrsum_core.h - what every kernel of the correlator sums shares and no source owns (kernels: qmps_corrsum_small.hip,
// qmps_corrsum_block.hip; sources of the right-hand sides: qmps_corrsum_one_site.h, qmps_corrsum_two_site.h; the formulas and the four
// kernel shapes: qmps_corrsum.hip): the system matrix, the pivot search and the tiles of the block kernels.
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
// A source (OneSiteSource, TwoSiteSource) is a type of static members that answers, and nothing else about it appears in a kernel:
//   kOpEntries, kSiteValues   complex entries of an operator; values `site` takes per operator pair
//   readout_scale(z, inv)     what the sum over the rows is multiplied by
//   lane<M>(...)              D = 2: from A, r, R, tr R and inv: one[a], and whatever of the right-hand-side columns W[q][N + c] and of
//                             lv[q][a] needs whole matrices
//   rows<M>(...)              D = 4: the same for the row of lane q, through whatever LDS stage it needs; every lane runs every barrier
//   row_source<D, M>(...)     D = 2, 4, behind the matrix entries of a row (build_row): what of its right-hand sides and lv[a] needs
//                             this row's R alone
//   block_finish<D>(...)      D = 8, 16: after block_build, S.lv[a] = L_a for all kMaxObservableOps slots (zero past n_ops); ends in a barrier
//   block_rhs<D>(...)         D = 8, 16: right-hand side c of one row, as a value
// lane, rows and block_finish store `one` and `site` from the j = 0 item (`first`).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_observable.h"

namespace qmps {

constexpr int kRowsItems = 4;      // D = 4: items (16 lanes each) of a workgroup

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
// row (i, j) of the system: the D^2 matrix entries, then what the source can fill from this row's R alone
template <int D, int M, class Src>
__device__ __forceinline__ void build_row(const double2* Ab, const double2* rb, const double2* O, double2 z, double2 inv, int i, int j,
                                          const double2 (&R)[2][2], const double2 (&one)[M], double2 (&row)[D * D + M], double2 (&lv)[M]) {
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
  Src::template row_source<D, M>(Ab, O, rij, i, j, R, one, row, lv);
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

// What both block kernels build in LDS before the matrix: A, r, R[ts][(i,j)] = (A_s r A_t^+)[i][j], lv[a][(i,j)] = L_a[j][i]
template <int D>
struct BlockTiles {
  static constexpr int N = D * D, P = D + 1;
  double2 A[2][D][P];
  double2 r[D][P];
  double2 Y[2][D][P];
  double2 R[4][N];
  double2 lv[kMaxObservableOps][N];
};

// Fills S.A, S.r and S.R and returns 1 / tau and the traces tr[t][s] = tr(A_s r A_t^+) in every thread.  It ends where the sources
// diverge, and hands over: R[2 t + s] holds X_(t s) = A_s r A_t^+, and lv[2 t + s] holds W_(t s) = A_t^+ A_s as element (i, j) =
// W[j][i] (kMaxObservableOps == 4 slots) - the source's block_finish turns the four W into L_a in place.  256 threads.
template <int D>
__device__ __forceinline__ void block_build(BlockTiles<D>& S, const double2* Ab, const double2* rb, int tid, double2& inv, double2 (&tr)[2][2]) {
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

}  // namespace qmps
