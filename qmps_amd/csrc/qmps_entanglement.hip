// qmps_entanglement.hip - Schmidt spectra of the resident states (qmps_entanglement): a batched complex-Hermitian Jacobi eigensolver.
//   p = eigenvalues of herm(r) / tr r, descending;  S = - sum_(p > 0) p ln p;  V = the unit eigenvectors (optional, template parameter).
// One rotation, pivot (p, q), a_pq = |a_pq| w:  tau = (a_qq - a_pp) / (2 |a_pq|),  t = sign(tau) / (|tau| + sqrt(1 + tau^2)),
// c = 1 / sqrt(1 + t^2),  s = t c,  J e_p = c e_p - s conj(w) e_q,  J e_q = s e_p + c conj(w) e_q,  A <- J^+ A J,  V <- V J:
// a_pq becomes exactly zero, a_pp -= t |a_pq|, a_qq += t |a_pq|.  Two kinds of pivot are set to zero without a rotation:
//  - |a_pq|^2 < 2^-960: it is zero, or its square is about to leave the normal range, where 1 / |a_pq| loses its digits;
//  - |a_pq|^2 <= 2^-102 |a_pp a_qq| (the relative criterion of Demmel and Veselic with 2 ulp): between tied eigenvalues a_pq and
//    a_qq - a_pp are both rounding noise, the rotation has a large angle and leaves fresh noise of the same size in its rows and
//    columns, and a cluster of k tied eigenvalues then hovers at off(A) ~ 0.3 k ulp against the sqrt(k) ulp of the termination test
//    for tens of sweeps.  All pivots dropped in a sweep form a matrix E with |E|_F^2 <= 2^-102 sum a_pp a_qq <= 2^-102 (tr A)^2:
//    they move an eigenvalue of the unit-trace matrix by at most 2^-51, a small part of the D 2^-52 scale of the accuracy.
// A sweep is the D - 1 rounds of the round-robin schedule (circle method, index D - 1 fixed), D / 2 disjoint pivots each.  An
// evaluation is done when off(A)^2 <= 2^-104 sum a_ii^2 after a sweep or when a sweep rotated nothing; a wave goes on until all its
// evaluations are done, at most kSweepCap<D> sweeps (NaN for an evaluation that is not done by then).
//   D = 2, 4: one lane per evaluation, diagonal and upper triangle (D^2 reals) and V in registers, every index static.
//   D = 8, 16: (D/2)^2 lanes per evaluation (4 / 1 evaluations per wave), A and V in padded LDS tiles; lane (k, l) owns the 2 x 2
//   block (pivot k's rows) x (pivot l's columns) of the round and rows 2k, 2k+1 of V in pivot l's columns.
// r enters and the results leave through LDS, so that every global access is a contiguous run.  Workgroups are single waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qmps_kernels.h"
#include "qmps_complex.h"

namespace qmps {

namespace {

constexpr double kTiny2 = 0x1p-960;     // |a_pq|^2 below this: the pivot is zeroed without a rotation
constexpr double kDrop2 = 0x1p-102;     // ... and so is one with |a_pq|^2 <= kDrop2 |a_pp a_qq|
constexpr double kDone = 0x1p-104;      // off(A)^2 <= kDone sum a_ii^2
// sweeps: a float64 port of this scheme needed at most 1 / 4 / 12 / 14 at D = 2 / 4 / 8 / 16 on the cases of
// tests/entanglement_cases.py and on Haar-rotated clusters of k = 2 .. D tied eigenvalues with zero, tiny and graded tails
// (profiles/EXPERIMENTS.md); the caps are twice that and more (at D = 2 the one rotation is the closed form: off(A) is exactly zero
// after it).  A wave leaves as soon as its evaluations are done, so a cap costs nothing until it is needed.
template <int D> constexpr int kSweepCap = D == 2 ? 1 : D == 4 ? 10 : D == 8 ? 24 : 30;

struct Rotation {
  double c, s, t_abs;   // t |a_pq|
  double2 w;
  bool on;
};

// the rotation that annihilates a_pq between the diagonal entries dp, dq
__device__ __forceinline__ Rotation make_rotation(const double dp, const double dq, const double2 apq) {
  Rotation R;
  const double n2 = dfma(apq.x, apq.x, apq.y * apq.y);
  R.on = n2 >= kTiny2 && n2 > kDrop2 * fabs(dp * dq);
  R.c = 1.0;
  R.s = 0.0;
  R.t_abs = 0.0;
  R.w = make_double2(1.0, 0.0);
  if (R.on) {
    const double inv = 1.0 / sqrt(n2), ab = n2 * inv;
    const double tau = 0.5 * (dq - dp) * inv, ta = fmin(fabs(tau), 1e150);
    const double t = copysign(fast_rcp(ta + sqrt(dfma(ta, ta, 1.0))), tau);
    R.c = 1.0 / sqrt(dfma(t, t, 1.0));
    R.s = t * R.c;
    R.t_abs = t * ab;
    R.w = make_double2(apq.x * inv, apq.y * inv);
  }
  return R;
}
// columns p, q of a row (x, y) under J:  x' = c x - s conj(w) y,  y' = s x + c conj(w) y;   sw = s w, cw = c w
__device__ __forceinline__ void rotate_columns(double2& x, double2& y, const double c, const double s, const double2 sw, const double2 cw) {
  const double2 u = cmulc(sw, y), v = cmulc(cw, y);
  y = make_double2(dfma(s, x.x, v.x), dfma(s, x.y, v.y));
  x = make_double2(dfma(c, x.x, -u.x), dfma(c, x.y, -u.y));
}
// rows p, q of a column (x, y) under J^+:  x' = c x - s w y,  y' = s x + c w y
__device__ __forceinline__ void rotate_rows(double2& x, double2& y, const double c, const double s, const double2 sw, const double2 cw) {
  const double2 u = cmul(sw, y), v = cmul(cw, y);
  y = make_double2(dfma(s, x.x, v.x), dfma(s, x.y, v.y));
  x = make_double2(dfma(c, x.x, -u.x), dfma(c, x.y, -u.y));
}
__device__ __forceinline__ double2 conj2(const double2 a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ bool finite2(const double2 a) { return fabs(a.x) < INFINITY && fabs(a.y) < INFINITY; }

// pivot k of round m of the round-robin schedule of D indices, p < q
template <int D>
__host__ __device__ constexpr int pivot_p(int m, int k) {
  const int a = k == 0 ? m : (m + k) % (D - 1), b = k == 0 ? D - 1 : (m - k + D - 1) % (D - 1);
  return a < b ? a : b;
}
template <int D>
__host__ __device__ constexpr int pivot_q(int m, int k) {
  const int a = k == 0 ? m : (m + k) % (D - 1), b = k == 0 ? D - 1 : (m - k + D - 1) % (D - 1);
  return a < b ? b : a;
}

// ---- D = 2, 4: one lane per evaluation ------------------------------------------------------------------------------------------------
template <int D, bool VEC>
__global__ __launch_bounds__(64) void entanglement_lane_kernel(EntanglementArgs g) {
  constexpr int N = D * D, P = N + 1;          // one evaluation per padded row of the tile
  __shared__ double2 sT[64 * P];
  __shared__ double sP[64 * D];
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * 64;
  const int nb = g.B - b0 < 64 ? (int)(g.B - b0) : 64;
  const bool live = lane < nb;
  {
    const double2* src = (const double2*)g.r + b0 * N;
#pragma unroll
    for (int m = 0; m < N; ++m) {
      const int idx = m * 64 + lane;
      if (idx < nb * N) sT[(idx / N) * P + idx % N] = src[idx];
    }
  }
  __syncthreads();

  double d[D];
  double2 a[D][D];                             // upper triangle only
  double2 V[VEC ? D : 1][VEC ? D : 1];
  bool bad = !live;
  {
    double2 x[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        x[i][j] = live ? sT[lane * P + i * D + j] : make_double2(0.0, 0.0);
        bad |= !finite2(x[i][j]);
      }
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) tr += x[i][i].x;
    const double scale = 1.0 / tr;
    bad |= !(fabs(tr) < INFINITY) || !(fabs(scale) < INFINITY);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      d[i] = bad ? 1.0 : x[i][i].x * scale;
#pragma unroll
      for (int j = i + 1; j < D; ++j)
        a[i][j] = bad ? make_double2(0.0, 0.0) : make_double2(0.5 * (x[i][j].x + x[j][i].x) * scale, 0.5 * (x[i][j].y - x[j][i].y) * scale);
    }
  }
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) V[i][j] = make_double2(i == j ? 1.0 : 0.0, 0.0);
  }

  bool done = bad;
  for (int sweep = 0; sweep < kSweepCap<D>; ++sweep) {
    if (__ballot(!done) == 0) break;
    if (!done) {
      bool rotated = false;
#pragma unroll
      for (int m = 0; m < D - 1; ++m)
#pragma unroll
        for (int k = 0; k < D / 2; ++k) {
          const int p = pivot_p<D>(m, k), q = pivot_q<D>(m, k);      // constants once the loops are unrolled
          const Rotation R = make_rotation(d[p], d[q], a[p][q]);
          a[p][q] = make_double2(0.0, 0.0);
          if (R.on) {
            rotated = true;
            const double2 sw = make_double2(R.s * R.w.x, R.s * R.w.y), cw = make_double2(R.c * R.w.x, R.c * R.w.y);
            d[p] -= R.t_abs;
            d[q] += R.t_abs;
#pragma unroll
            for (int r = 0; r < D; ++r) {
              if (r == p || r == q) continue;
              double2 x = r < p ? a[r][p] : conj2(a[p][r]), y = r < q ? a[r][q] : conj2(a[q][r]);      // A[r][p], A[r][q]
              rotate_columns(x, y, R.c, R.s, sw, cw);
              if (r < p) a[r][p] = x; else a[p][r] = conj2(x);
              if (r < q) a[r][q] = y; else a[q][r] = conj2(y);
            }
            if constexpr (VEC) {
#pragma unroll
              for (int i = 0; i < D; ++i) rotate_columns(V[i][p], V[i][q], R.c, R.s, sw, cw);
            }
          }
        }
      double off2 = 0.0, d2 = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        d2 = dfma(d[i], d[i], d2);
#pragma unroll
        for (int j = i + 1; j < D; ++j) off2 += dfma(a[i][j].x, a[i][j].x, a[i][j].y * a[i][j].y);
      }
      done = 2.0 * off2 <= kDone * d2 || !rotated;
    }
  }
  const bool fail = bad || !done;

  // descending, the columns of V with their eigenvalues (sorting network, static indices)
  auto order = [&](auto I, auto J) {
    constexpr int i = decltype(I)::value, j = decltype(J)::value;
    const bool swap = d[i] < d[j];
    const double di = d[i], dj = d[j];
    d[i] = swap ? dj : di;
    d[j] = swap ? di : dj;
    if constexpr (VEC) {
#pragma unroll
      for (int r = 0; r < D; ++r) {
        const double2 vi = V[r][i], vj = V[r][j];
        V[r][i] = swap ? vj : vi;
        V[r][j] = swap ? vi : vj;
      }
    }
  };
  using std::integral_constant;
  if constexpr (D == 2) {
    order(integral_constant<int, 0>{}, integral_constant<int, 1>{});
  } else {
    order(integral_constant<int, 0>{}, integral_constant<int, 1>{});
    order(integral_constant<int, 2>{}, integral_constant<int, 3>{});
    order(integral_constant<int, 0>{}, integral_constant<int, 2>{});
    order(integral_constant<int, 1>{}, integral_constant<int, 3>{});
    order(integral_constant<int, 1>{}, integral_constant<int, 2>{});
  }
  double S = 0.0;
#pragma unroll
  for (int k = D - 1; k >= 0; --k) S -= d[k] > 0.0 ? d[k] * log(d[k]) : 0.0;       // smallest terms first
  if (live) g.S[b0 + lane] = fail ? NAN : S;

  __syncthreads();
#pragma unroll
  for (int k = 0; k < D; ++k) sP[lane * D + k] = fail ? NAN : d[k];
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int k = 0; k < D; ++k) sT[lane * P + i * D + k] = fail ? make_double2(NAN, NAN) : V[i][k];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < D; ++m) {
    const int idx = m * 64 + lane;
    if (idx < nb * D) g.p[b0 * D + idx] = sP[idx];
  }
  if constexpr (VEC) {
    double2* dst = (double2*)g.V + b0 * N;
#pragma unroll
    for (int m = 0; m < N; ++m) {
      const int idx = m * 64 + lane;
      if (idx < nb * N) dst[idx] = sT[(idx / N) * P + idx % N];
    }
  }
}

// ---- D = 8, 16: (D/2)^2 lanes per evaluation, A and V in LDS ------------------------------------------------------------------------
// sum over the lanes of one evaluation, in every lane of it
template <int D>
__device__ __forceinline__ double eval_sum(double v) {
  if constexpr (D == 8) return row16_sum(v);
  else return wave_sum(v);
}

template <int D, bool VEC>
__global__ __launch_bounds__(64) void entanglement_block_kernel(EntanglementArgs g) {
  constexpr int H = D / 2, T = H * H, EV = 64 / T, N = D * D, P = D + 1, M = N / T;
  __shared__ double2 sA[EV][D][P];
  __shared__ double2 sV[EV][D][P];             // r as it is loaded, then V
  __shared__ double sPar[EV][H][4];            // c, s, w of the round's rotations
  __shared__ double sEig[EV][D];
  __shared__ double sTerm[EV][D];
  __shared__ int sSrc[EV][D];
  const int lane = threadIdx.x, e = lane / T, tl = lane % T, k = tl / H, l = tl % H;
  const int64_t b0 = (int64_t)blockIdx.x * EV, b = b0 + e;
  const bool live = b < g.B;

  double2 x[M];
  double tr = 0.0, n_bad = 0.0;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int el = tl + T * m, i = el / D, j = el % D;
    x[m] = live ? ((const double2*)g.r)[b * N + el] : make_double2(0.0, 0.0);
    sV[e][i][j] = x[m];
    n_bad += finite2(x[m]) ? 0.0 : 1.0;
    tr += i == j ? x[m].x : 0.0;
  }
  tr = eval_sum<D>(tr);
  n_bad = eval_sum<D>(n_bad);
  const double scale = 1.0 / tr;
  const bool bad = !live || !(n_bad == 0.0) || !(fabs(tr) < INFINITY) || !(fabs(scale) < INFINITY);
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int el = tl + T * m, i = el / D, j = el % D;
    const double2 y = sV[e][j][i];
    x[m] = bad ? make_double2(i == j ? 1.0 : 0.0, 0.0) : make_double2(0.5 * (x[m].x + y.x) * scale, 0.5 * (x[m].y - y.y) * scale);
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int el = tl + T * m, i = el / D, j = el % D;
    sA[e][i][j] = x[m];
    if constexpr (VEC) sV[e][i][j] = make_double2(i == j ? 1.0 : 0.0, 0.0);
  }
  __syncthreads();

  bool done = bad;
  for (int sweep = 0; sweep < kSweepCap<D>; ++sweep) {
    if (__ballot(!done) == 0) break;
    double rotated = 0.0;
    for (int m = 0; m < D - 1; ++m) {
      const int pk = pivot_p<D>(m, k), qk = pivot_q<D>(m, k), pl = pivot_p<D>(m, l), ql = pivot_q<D>(m, l);
      if (!done && k == l) {
        // the diagonal block of pivot k: its rotation, for the lanes of row k and column k
        const double dp = sA[e][pk][pk].x, dq = sA[e][qk][qk].x;
        const Rotation R = make_rotation(dp, dq, sA[e][pk][qk]);
        rotated += R.on ? 1.0 : 0.0;
        sPar[e][k][0] = R.c;
        sPar[e][k][1] = R.s;
        sPar[e][k][2] = R.w.x;
        sPar[e][k][3] = R.w.y;
        sA[e][pk][pk] = make_double2(dp - R.t_abs, 0.0);
        sA[e][qk][qk] = make_double2(dq + R.t_abs, 0.0);
        sA[e][pk][qk] = make_double2(0.0, 0.0);
        sA[e][qk][pk] = make_double2(0.0, 0.0);
      }
      __syncthreads();
      // block (pivot kk's rows) x (pivot ll's columns), kk < ll: the lane below the diagonal reads the block above it, computes the
      // same numbers as the lane that owns it and stores their adjoint into its own block, so that the matrix stays Hermitian bit
      // for bit.  Two lanes read one block and one of them overwrites it: the barrier between the loads and the stores orders that.
      const bool upper = k < l;
      const int rp = upper ? pk : pl, rq = upper ? qk : ql, cp = upper ? pl : pk, cq = upper ? ql : qk;
      double2 a00 = make_double2(0.0, 0.0), a01 = a00, a10 = a00, a11 = a00;
      if (!done && k != l) {
        const int kk = upper ? k : l, ll = upper ? l : k;
        const double cr = sPar[e][kk][0], sr = sPar[e][kk][1], cc = sPar[e][ll][0], sc = sPar[e][ll][1];
        const double2 wr = make_double2(sPar[e][kk][2], sPar[e][kk][3]), wc = make_double2(sPar[e][ll][2], sPar[e][ll][3]);
        a00 = sA[e][rp][cp];
        a01 = sA[e][rp][cq];
        a10 = sA[e][rq][cp];
        a11 = sA[e][rq][cq];
        const double2 swc = make_double2(sc * wc.x, sc * wc.y), cwc = make_double2(cc * wc.x, cc * wc.y);
        const double2 swr = make_double2(sr * wr.x, sr * wr.y), cwr = make_double2(cr * wr.x, cr * wr.y);
        rotate_columns(a00, a01, cc, sc, swc, cwc);
        rotate_columns(a10, a11, cc, sc, swc, cwc);
        rotate_rows(a00, a10, cr, sr, swr, cwr);
        rotate_rows(a01, a11, cr, sr, swr, cwr);
      }
      __syncthreads();
      if (!done) {
        const double cl = sPar[e][l][0], sl = sPar[e][l][1];
        const double2 wl = make_double2(sPar[e][l][2], sPar[e][l][3]);
        if (k != l) {
          if (upper) {
            sA[e][rp][cp] = a00;
            sA[e][rp][cq] = a01;
            sA[e][rq][cp] = a10;
            sA[e][rq][cq] = a11;
          } else {
            sA[e][cp][rp] = conj2(a00);
            sA[e][cq][rp] = conj2(a01);
            sA[e][cp][rq] = conj2(a10);
            sA[e][cq][rq] = conj2(a11);
          }
        }
        if constexpr (VEC) {
          const double2 swl = make_double2(sl * wl.x, sl * wl.y), cwl = make_double2(cl * wl.x, cl * wl.y);
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            double2 vx = sV[e][2 * k + u][pl], vy = sV[e][2 * k + u][ql];
            rotate_columns(vx, vy, cl, sl, swl, cwl);
            sV[e][2 * k + u][pl] = vx;
            sV[e][2 * k + u][ql] = vy;
          }
        }
      }
      __syncthreads();
    }
    double off2 = 0.0, d2 = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int el = tl + T * m, i = el / D, j = el % D;
      const double2 v = sA[e][i][j];
      const double n2 = dfma(v.x, v.x, v.y * v.y);
      off2 += i == j ? 0.0 : n2;
      d2 += i == j ? n2 : 0.0;
    }
    off2 = eval_sum<D>(off2);
    d2 = eval_sum<D>(d2);
    rotated = eval_sum<D>(rotated);
    if (!done) done = off2 <= kDone * d2 || rotated == 0.0;
  }
  const bool fail = bad || !done;

  // descending order by ranks (ties by index); the entropy terms at their sorted places, summed smallest first by one lane
  if (tl < D) {
    const double dj = sA[e][tl][tl].x;
    int rank = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double di = sA[e][i][i].x;
      rank += (di > dj || (di == dj && i < tl)) ? 1 : 0;
    }
    // a failed evaluation may hold NaN on its diagonal, against which every comparison is false: its ranks are no permutation,
    // so it writes its NaN by index
    const int at = fail ? tl : rank;
    sEig[e][at] = fail ? NAN : dj;
    sTerm[e][at] = dj > 0.0 ? dj * log(dj) : 0.0;
    sSrc[e][at] = tl;
  }
  __syncthreads();
  if (tl == 0 && live) {
    double S = 0.0;
#pragma unroll
    for (int kk = D - 1; kk >= 0; --kk) S -= sTerm[e][kk];
    g.S[b] = fail ? NAN : S;
  }
  if (lane < EV * D && b0 * D + lane < g.B * D) g.p[b0 * D + lane] = sEig[lane / D][lane % D];
  if constexpr (VEC) {
    if (live) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int el = tl + T * m, i = el / D, kk = el % D;
        ((double2*)g.V)[b * N + el] = fail ? make_double2(NAN, NAN) : sV[e][i][sSrc[e][kk]];
      }
    }
  }
}

template <bool VEC>
hipError_t launch(int D, const EntanglementArgs& a, hipStream_t st) {
  switch (D) {
    case 2: hipLaunchKernelGGL((entanglement_lane_kernel<2, VEC>), dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a); break;
    case 4: hipLaunchKernelGGL((entanglement_lane_kernel<4, VEC>), dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a); break;
    case 8: hipLaunchKernelGGL((entanglement_block_kernel<8, VEC>), dim3((unsigned)((a.B + 3) / 4)), dim3(64), 0, st, a); break;
    case 16: hipLaunchKernelGGL((entanglement_block_kernel<16, VEC>), dim3((unsigned)a.B), dim3(64), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_entanglement(int D, const EntanglementArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (!a.r || !a.p || !a.S) return hipErrorInvalidValue;
  return a.V ? launch<true>(D, a, st) : launch<false>(D, a, st);
}

}  // namespace qmps
