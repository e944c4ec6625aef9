// qmps_correlator.hip - two-point functions of the resident states (qmps_correlators): for every evaluation the chains
//   x_c = E_{O_c}(r),  C[a][c][n-1] = tr(L_a T^(n-1)(x_c)) / tr r,  one[a] = tr(L_a r) / tr r,
//   E_O(x) = sum_{t,s} O[t][s] A_s x A_t^+,  T = E_1,  L_a = sum_{t,s} O_a[t][s] A_t^+ A_s   (tr(E_{O_a}(x)) = tr(L_a x)),
// in ONE launch whatever n_ops and n_max are.  A, r and the L_a are fetched / built once per evaluation, the chain state x stays in
// registers (D = 2, 4) or LDS (D = 8, 16) for the whole chain, the chains of the n_ops right operators run one after the other.
// Every loop has a fixed trip count (n_ops, n_max); there are no atomics, counters or waits between workgroups.
// Results leave through an LDS tile of a few steps, so that the stores are contiguous runs along n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_observable.h"

namespace qmps {

namespace {

// ---- D = 2, 4: D consecutive lanes per evaluation, lane q owns row q of x -----------------------------------------------------
// value of lane J of the own group of D lanes, in every lane of the group (DPP quad_perm)
template <int D, int J>
__device__ __forceinline__ double group_bcast(double v) {
  if constexpr (D == 4) return quad_bcast<J>(v);
  else return quad_perm<(J) | (J << 2) | ((2 + J) << 4) | ((2 + J) << 6)>(v);
}
template <int D>
__device__ __forceinline__ double group_sum(double v) {
  if constexpr (D == 4) return quad_sum(v);
  else return v + quad_perm<0xB1>(v);
}

constexpr int kRowTile = 8;   // steps gathered in LDS before they are stored: runs of 128 bytes along n

template <int D>
__global__ __launch_bounds__(64) void correlator_rows_kernel(CorrelatorArgs p) {
  constexpr int EV = 64 / D;       // evaluations per workgroup (one wave)
  __shared__ double2 sL[kMaxObservableOps][D][64];             // L_a[i][q] of the lane that owns row q: [a][i][lane]
  __shared__ double2 sRow[2][D][64];                 // A_s[q][j] of the lane: [s][j][lane]
  __shared__ double2 sR[D][64];                      // r[q][j] of the lane, the start of every chain
  __shared__ double2 sOut[EV][kMaxObservableOps][kRowTile];
  const int lane = threadIdx.x, q = lane % D, e = lane / D;
  const int64_t b0 = (int64_t)blockIdx.x * EV;
  // lanes past the batch compute a copy of the last evaluation (every lane takes part in the DPP moves) and store nothing
  const int64_t b = b0 + e < p.B ? b0 + e : p.B - 1;
  const double2* Ab = (const double2*)p.A + b * (2 * D * D);
  const double2* O = (const double2*)p.ops;          // [n_ops][2][2], uniform addresses
  const int n_ops = p.n_ops, n_max = p.n_max;

  double2 A[2][D][D];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) A[s][i][j] = Ab[(s * D + i) * D + j];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < D; ++j) sRow[s][j][lane] = Ab[(s * D + q) * D + j];
#pragma unroll
  for (int j = 0; j < D; ++j) sR[j][lane] = ((const double2*)p.r)[(b * D + q) * D + j];

  {
    // column q of M_ts = A_t^+ A_s and of every L_a, one row index i at a time (all sixteen M entries at once would not fit the registers)
    double2 Acol[2][D];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int k = 0; k < D; ++k) Acol[s][k] = Ab[(s * D + k) * D + q];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double2 M[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          double2 m = make_double2(0.0, 0.0);
#pragma unroll
          for (int k = 0; k < D; ++k) cfma_conj(Acol[s][k], A[t][k][i], m);
          M[t][s] = m;
        }
      for (int a = 0; a < n_ops; ++a) {
        double2 l = make_double2(0.0, 0.0);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int s = 0; s < 2; ++s) cfma(O[a * 4 + t * 2 + s], M[t][s], l);
        sL[a][i][lane] = l;
      }
    }
  }

  double2 inv;
  {
    // tr r: lane q holds r[q][q]
    double dx = 0.0, dy = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const double2 rj = sR[j][lane];
      dx = q == j ? rj.x : dx;
      dy = q == j ? rj.y : dy;
    }
    inv = crecip(make_double2(group_sum<D>(dx), group_sum<D>(dy)));
  }

  // y_t = x A_t^+ (row q)
  auto right_mul = [&](const double2 (&x)[D], double2 (&y)[2][D]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int l = 0; l < D; ++l) {
        double2 v = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < D; ++k) cfma_conj(x[k], A[t][l][k], v);
        y[t][l] = v;
      }
  };
  // row q of sum_s A_s z_s: row j of z_s comes from lane j of the group
  auto left_mul = [&](const double2 (&z)[2][D], double2 (&out)[D]) {
#pragma unroll
    for (int l = 0; l < D; ++l) out[l] = make_double2(0.0, 0.0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      auto row = [&](auto jc) {
        constexpr int J = decltype(jc)::value;
        const double2 arow = sRow[s][J][lane];
#pragma unroll
        for (int l = 0; l < D; ++l) {
          const double2 zz = make_double2(group_bcast<D, J>(z[s][l].x), group_bcast<D, J>(z[s][l].y));
          cfma(arow, zz, out[l]);
        }
      };
      row(std::integral_constant<int, 0>{});
      row(std::integral_constant<int, 1>{});
      if constexpr (D == 4) {
        row(std::integral_constant<int, 2>{});
        row(std::integral_constant<int, 3>{});
      }
    }
  };
  // tr(L_a x) / tr r, in every lane of the group
  auto read_out = [&](int a, const double2 (&x)[D]) {
    double2 v = make_double2(0.0, 0.0);
#pragma unroll
    for (int i = 0; i < D; ++i) cfma(sL[a][i][lane], x[i], v);
    return cmul(make_double2(group_sum<D>(v.x), group_sum<D>(v.y)), inv);
  };

  // (sL, sRow and sR need no barrier: every lane reads only what it wrote itself)
  if (p.one != nullptr) {
    double2 r[D];
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = sR[j][lane];
    for (int a = 0; a < n_ops; ++a) {
      const double2 v = read_out(a, r);
      if (q == 0 && b0 + e < p.B) ((double2*)p.one)[b * n_ops + a] = v;
    }
  }

  for (int c = 0; c < n_ops; ++c) {
    double2 x[D], y[2][D], z[2][D];
    // x = E_{O_c}(r): z_s = sum_t O_c[t][s] y_t
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = sR[j][lane];
    right_mul(x, y);
    {
      const double2 w00 = O[c * 4 + 0], w01 = O[c * 4 + 1], w10 = O[c * 4 + 2], w11 = O[c * 4 + 3];
#pragma unroll
      for (int l = 0; l < D; ++l) {
        z[0][l] = cmul(w00, y[0][l]);
        cfma(w10, y[1][l], z[0][l]);
        z[1][l] = cmul(w01, y[0][l]);
        cfma(w11, y[1][l], z[1][l]);
      }
    }
    left_mul(z, x);
    for (int n = 0; n < n_max; ++n) {
      const int k = n % kRowTile;
      for (int a = 0; a < n_ops; ++a) {
        const double2 v = read_out(a, x);
        if (q == 0) sOut[e][a][k] = v;
      }
      if (k == kRowTile - 1 || n == n_max - 1) {
        // the wave stores the tile: kRowTile consecutive lanes write one run of steps of one (evaluation, a)
        __syncthreads();
        const int nb = k + 1, n0 = n - k;
        for (int idx = lane; idx < EV * n_ops * kRowTile; idx += 64) {
          const int kk = idx % kRowTile, ea = idx / kRowTile, a = ea % n_ops, ee = ea / n_ops;
          const int64_t bb = b0 + ee;
          if (kk < nb && bb < p.B) ((double2*)p.C)[((bb * n_ops + a) * n_ops + c) * (int64_t)n_max + n0 + kk] = sOut[ee][a][kk];
        }
        __syncthreads();
      }
      if (n + 1 < n_max) {
        right_mul(x, y);
        left_mul(y, x);
      }
    }
  }
}

// ---- D = 8, 16: one workgroup of D x D threads per evaluation, thread (i, j) owns x[i][j] ------------------------------------
constexpr int kBlockTile = 16;   // steps gathered in LDS before they are stored: runs of 256 bytes along n

// sums of cnt <= 8 values over the workgroup, results in every thread
template <int D>
__device__ __forceinline__ void block_sum_n(double (&v)[2 * kMaxObservableOps], int cnt, double (*red)[2 * kMaxObservableOps], int tid) {
  constexpr int N = D * D;
#pragma unroll
  for (int u = 0; u < 2 * kMaxObservableOps; ++u)
    if (u < cnt) v[u] = wave_sum(v[u]);
  if (N > 64) {
    __syncthreads();
    if ((tid & 63) == 0) {
#pragma unroll
      for (int u = 0; u < 2 * kMaxObservableOps; ++u) red[tid >> 6][u] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2 * kMaxObservableOps; ++u) {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < N / 64; ++w) s += red[w][u];
      v[u] = s;
    }
  }
}

template <int D>
__global__ __launch_bounds__(D* D) void correlator_block_kernel(CorrelatorArgs p) {
  constexpr int N = D * D, P = D + 1, NW = (N + 63) / 64;
  __shared__ double2 sA[2][D][P];
  __shared__ double2 sX[D][P];
  __shared__ double2 sZ[2][D][P];
  __shared__ double sRed[NW][2 * kMaxObservableOps];
  __shared__ double2 sOut[kMaxObservableOps][kBlockTile];
  const int tid = threadIdx.x, i = tid / D, j = tid % D;
  const int64_t b = blockIdx.x;
  if (b >= p.B) return;
  const double2* O = (const double2*)p.ops;
  const int n_ops = p.n_ops, n_max = p.n_max;
  {
    const double2* a = (const double2*)p.A + b * (2 * N);
    sA[0][i][j] = a[tid];
    sA[1][i][j] = a[N + tid];
  }
  const double2 r = ((const double2*)p.r)[b * N + tid];
  __syncthreads();

  // this thread's entry L_a[j][i] of every L_a: tr(L_a x) = sum_(i, j) L_a[j][i] x[i][j]
  double2 Lji[kMaxObservableOps];
  {
    double2 M[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        double2 m = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < D; ++k) cfma_conj(sA[s][k][i], sA[t][k][j], m);
        M[t][s] = m;
      }
#pragma unroll
    for (int a = 0; a < kMaxObservableOps; ++a) {
      double2 l = make_double2(0.0, 0.0);
      if (a < n_ops) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int s = 0; s < 2; ++s) cfma(O[a * 4 + t * 2 + s], M[t][s], l);
      }
      Lji[a] = l;
    }
  }
  double v[2 * kMaxObservableOps];
#pragma unroll
  for (int u = 0; u < 2 * kMaxObservableOps; ++u) v[u] = 0.0;
  v[0] = i == j ? r.x : 0.0;
  v[1] = i == j ? r.y : 0.0;
  block_sum_n<D>(v, 2, sRed, tid);
  const double2 inv = crecip(make_double2(v[0], v[1]));

  // sum_(t, s) W[t][s] A_s x A_t^+ for the x in sX: z_t = sum_s W[t][s] A_s x through LDS, then z_t A_t^+
  auto apply = [&](const double2 w00, const double2 w01, const double2 w10, const double2 w11, const bool identity) {
    double2 y0 = make_double2(0.0, 0.0), y1 = make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double2 xc = sX[k][j];
      cfma(sA[0][i][k], xc, y0);
      cfma(sA[1][i][k], xc, y1);
    }
    if (identity) {
      sZ[0][i][j] = y0;
      sZ[1][i][j] = y1;
    } else {
      double2 z0 = cmul(w00, y0), z1 = cmul(w10, y0);
      cfma(w01, y1, z0);
      cfma(w11, y1, z1);
      sZ[0][i][j] = z0;
      sZ[1][i][j] = z1;
    }
    __syncthreads();
    double2 out = make_double2(0.0, 0.0);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int k = 0; k < D; ++k) cfma_conj(sZ[t][i][k], sA[t][j][k], out);
    return out;
  };
  // tr(L_a x) / tr r for every a, in every thread
  auto read_out = [&](const double2 x) {
#pragma unroll
    for (int a = 0; a < kMaxObservableOps; ++a) {
      const double2 w = cmul(Lji[a], x);
      v[2 * a] = w.x;
      v[2 * a + 1] = w.y;
    }
    block_sum_n<D>(v, 2 * n_ops, sRed, tid);
  };

  if (p.one != nullptr) {
    read_out(r);
#pragma unroll
    for (int a = 0; a < kMaxObservableOps; ++a)
      if (a < n_ops && tid == 0) ((double2*)p.one)[b * n_ops + a] = cmul(make_double2(v[2 * a], v[2 * a + 1]), inv);
  }

  const double2 zero = make_double2(0.0, 0.0);
  for (int c = 0; c < n_ops; ++c) {
    __syncthreads();
    sX[i][j] = r;
    __syncthreads();
    double2 x = apply(O[c * 4 + 0], O[c * 4 + 1], O[c * 4 + 2], O[c * 4 + 3], false);
    for (int n = 0; n < n_max; ++n) {
      const int k = n % kBlockTile;
      read_out(x);
      if (tid == 0) {
#pragma unroll
        for (int a = 0; a < kMaxObservableOps; ++a)
          if (a < n_ops) sOut[a][k] = cmul(make_double2(v[2 * a], v[2 * a + 1]), inv);
      }
      if (k == kBlockTile - 1 || n == n_max - 1) {
        __syncthreads();
        const int nb = k + 1, n0 = n - k, a = tid / kBlockTile, kk = tid % kBlockTile;
        if (a < n_ops && kk < nb) ((double2*)p.C)[((b * n_ops + a) * n_ops + c) * (int64_t)n_max + n0 + kk] = sOut[a][kk];
        __syncthreads();
      }
      if (n + 1 < n_max) {
        sX[i][j] = x;
        __syncthreads();
        x = apply(zero, zero, zero, zero, true);
      }
    }
  }
}

}  // namespace

hipError_t launch_correlators(int D, const CorrelatorArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.n_ops < 1 || a.n_ops > kMaxObservableOps || a.n_max < 1) return hipErrorInvalidValue;
  switch (D) {
    case 2: hipLaunchKernelGGL(correlator_rows_kernel<2>, dim3((unsigned)((a.B + 31) / 32)), dim3(64), 0, st, a); break;
    case 4: hipLaunchKernelGGL(correlator_rows_kernel<4>, dim3((unsigned)((a.B + 15) / 16)), dim3(64), 0, st, a); break;
    case 8: hipLaunchKernelGGL(correlator_block_kernel<8>, dim3((unsigned)a.B), dim3(64), 0, st, a); break;
    case 16: hipLaunchKernelGGL(correlator_block_kernel<16>, dim3((unsigned)a.B), dim3(256), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace qmps
