// qmps_corrsum_small.hip - the correlator-sum kernels of the small bond dimensions (formulas: qmps_corrsum.hip; the elimination and
// the source interface: qmps_corrsum_core.h), one instantiation per number of operators M and source:
//   D = 2   one lane per item, matrix and right-hand sides in registers, pivot row picked by selects (no scratch)
//   D = 4   16 consecutive lanes per item, lane q owns row q (16 + n_ops complex values in registers); pivot search by DPP row
//           rotations, the scaled pivot row goes through LDS (one write, one broadcast read per value).  Lanes past the last item
//           compute a copy of it and store nothing
#include "qmps_corrsum_internal.h"
#include "qmps_corrsum_one_site.h"
#include "qmps_corrsum_two_site.h"

namespace qmps {

namespace {

template <int M, class Src>
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
  Src::template lane<M>(p, b, jz == 0, Ab, rb, O, R, tr, inv, one, W, lv);
#pragma unroll
  for (int q = 0; q < N; ++q) build_row<D, M, Src>(Ab, rb, O, z, inv, q / D, q % D, R[q], one, W[q], lv[q]);

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
  const double2 scale = Src::readout_scale(z, inv);
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

template <int M, class Src>
__global__ __launch_bounds__(64) void corrsum_rows_kernel(CorrSumArgs p) {
  constexpr int D = 4, N = 16, EV = kRowsItems;
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

  double2 row[N + M];
  {
    double2 lv[M];
    Src::template rows<M>(p, b, live && jz == 0, Ab, rb, O, R, tr, inv, q, g, one, row, lv);
    build_row<D, M, Src>(Ab, rb, O, z, inv, i, j, R, one, row, lv);
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

  const double2 scale = Src::readout_scale(z, inv);
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

template <int M, class Src>
void launch_m(int D, const CorrSumArgs& a, int64_t items, hipStream_t st) {
  if (D == 2) hipLaunchKernelGGL((corrsum_lane_kernel<M, Src>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((corrsum_rows_kernel<M, Src>), dim3((unsigned)((items + kRowsItems - 1) / kRowsItems)), dim3(64), 0, st, a);
}

}  // namespace

template <class Src>
void launch_small(int D, const CorrSumArgs& a, int64_t items, hipStream_t st) {
  switch (a.n_ops) {
    case 1: launch_m<1, Src>(D, a, items, st); break;
    case 2: launch_m<2, Src>(D, a, items, st); break;
    case 3: launch_m<3, Src>(D, a, items, st); break;
    default: launch_m<4, Src>(D, a, items, st); break;
  }
}
template void launch_small<OneSiteSource>(int, const CorrSumArgs&, int64_t, hipStream_t);
template void launch_small<TwoSiteSource>(int, const CorrSumArgs&, int64_t, hipStream_t);

}  // namespace qmps
