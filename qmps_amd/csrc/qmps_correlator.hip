// qmps_correlator.hip - two-point functions of the resident states (qmps_correlators): for every evaluation the chains
//   x_c = E_{O_c}(r),  C[a][c][n-1] = tr(L_a T^(n-1)(x_c)) / tr r,  one[a] = tr(L_a r) / tr r,
//   E_O(x) = sum_{t,s} O[t][s] A_s x A_t^+,  T = E_1,  L_a = sum_{t,s} O_a[t][s] A_t^+ A_s   (tr(E_{O_a}(x)) = tr(L_a x)),
// in ONE launch whatever n_ops and n_max are.  A, r and the L_a are fetched / built once per evaluation, the chain state x stays in
// registers (D = 2, 4) or LDS (D = 8, 16) for the whole chain, the chains of the n_ops right operators run one after the other.
// Every loop has a fixed trip count (n_ops, n_max); there are no atomics, counters or waits between workgroups.
// Results leave through an LDS tile of a few steps, so that the stores are contiguous runs along n.
// String order (qmps_string_correlators): the same kernels instantiated with another chain type.  With a one-site string S the step
// of every chain is E_S in the place of T,
//   C[a][c][n-1] = tr(L_a E_S^(n-1)(x_c)) / tr r = <O_a(0) S(1) .. S(n-1) O_c(n)>,   str[n-1] = tr(E_S^n(r)) / tr r = <S(1) .. S(n)>,
// which costs the mixing of the weights S[t][s] into every step; str is one more chain from r, read out by the plain trace.
// The chain is a type (PlainChain, StringChain): an instantiation holds one kind of step, and the plain one does what it always did.
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

// a b with the FMA order written out: the second product of the real part and the first of the imaginary part are rounded on their
// own.  (cmul leaves to the compiler which product of each part is fused; these are the bits qmps_correlators has always returned.)
__device__ __forceinline__ double2 cmul_rows(const double2 a, const double2 b) {
  return make_double2(dfma(a.x, b.x, -(a.y * b.y)), dfma(a.y, b.x, a.x * b.y));
}
// z_s = sum_t W[t][s] y_t: the weights of E_W between the right and the left multiplication of the row kernels
template <int D>
__device__ __forceinline__ void mix_rows(const double2 w00, const double2 w01, const double2 w10, const double2 w11, const double2 (&y)[2][D],
                                         double2 (&z)[2][D]) {
#pragma unroll
  for (int l = 0; l < D; ++l) {
    z[0][l] = cmul_rows(w00, y[0][l]);
    cfma(w10, y[1][l], z[0][l]);
    z[1][l] = cmul_rows(w01, y[0][l]);
    cfma(w11, y[1][l], z[1][l]);
  }
}

// ---- the chain: what one step x -> E(x) of a chain puts between its two multiplications ---------------------------------------
// A kernel is instantiated with one of the two types, so the n loop of an instantiation holds one kind of step and no test.
// `mixed` (row kernels): the y_t the left multiplication takes; `step` (block kernels): the call of `apply` for the x in LDS.
struct PlainChain {        // T = E_1: the y_t go on as they are
  static constexpr bool kString = false;
  __device__ explicit PlainChain(const CorrelatorArgs&) {}
  __device__ __forceinline__ int n_chains(const CorrelatorArgs& p) const { return p.n_ops; }
  template <int D>
  __device__ __forceinline__ const double2 (&mixed(const double2 (&y)[2][D], double2 (&)[2][D]) const)[2][D] {
    return y;
  }
  template <class Apply>
  __device__ __forceinline__ double2 step(Apply&& apply) const {
    const double2 zero = make_double2(0.0, 0.0);
    return apply(zero, zero, zero, zero, true);
  }
};
struct StringChain {       // E_S: the four entries of S, uniform, live in scalar registers for the whole kernel
  static constexpr bool kString = true;
  double2 w00, w01, w10, w11;
  __device__ explicit StringChain(const CorrelatorArgs& p)
      : w00(((const double2*)p.string)[0]), w01(((const double2*)p.string)[1]), w10(((const double2*)p.string)[2]), w11(((const double2*)p.string)[3]) {}
  // the chains of the operators and, where str is wanted, the pure string chain behind them
  __device__ __forceinline__ int n_chains(const CorrelatorArgs& p) const { return p.n_ops + (p.str != nullptr ? 1 : 0); }
  template <int D>
  __device__ __forceinline__ const double2 (&mixed(const double2 (&y)[2][D], double2 (&z)[2][D]) const)[2][D] {
    mix_rows<D>(w00, w01, w10, w11, y, z);
    return z;
  }
  template <class Apply>
  __device__ __forceinline__ double2 step(Apply&& apply) const {
    return apply(w00, w01, w10, w11, false);
  }
};

constexpr int kRowTile = 8;   // steps gathered in LDS before they are stored: runs of 128 bytes along n

template <int D, class Chain>
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
  const Chain chain(p);

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

  // The chains of the n_ops right operators, one after the other: x = E_(O_c)(r), then n_max times the n_ops read-outs, each followed
  // by one step of the chain; the values of (evaluation bb, read-out a) are the row (bb n_out + a) row_len of `rows`.
  // String launches that return str walk one more chain, the pure string chain: it starts from r with the string itself as its first
  // operator and has one read-out, the plain trace of x - tr(L x) with the identity in the place of L_0, which no chain needs any more.
  const int n_chains = chain.n_chains(p);
  for (int c = 0; c < n_chains; ++c) {
    const bool pure = Chain::kString && c == n_ops;      // (false at compile time in the plain instantiation)
    const double2* W = pure ? (const double2*)p.string : O + c * 4;
    const int n_out = pure ? 1 : n_ops;
    double2* rows = pure ? (double2*)p.str : (double2*)p.C + (int64_t)c * n_max;
    const int64_t row_len = pure ? (int64_t)n_max : (int64_t)n_ops * n_max;
    if (pure) {
#pragma unroll
      for (int i = 0; i < D; ++i) sL[0][i][lane] = make_double2(i == q ? 1.0 : 0.0, 0.0);
    }
    double2 x[D], y[2][D], z[2][D];
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = sR[j][lane];
    right_mul(x, y);
    mix_rows<D>(W[0], W[1], W[2], W[3], y, z);
    left_mul(z, x);
    for (int n = 0; n < n_max; ++n) {
      const int k = n % kRowTile;
      for (int a = 0; a < n_out; ++a) {
        const double2 v = read_out(a, x);
        if (q == 0) sOut[e][a][k] = v;
      }
      if (k == kRowTile - 1 || n == n_max - 1) {
        // the wave stores the tile: kRowTile consecutive lanes write one run of steps of one (evaluation, a)
        __syncthreads();
        const int nb = k + 1, n0 = n - k;
        for (int idx = lane; idx < EV * n_out * kRowTile; idx += 64) {
          const int kk = idx % kRowTile, ea = idx / kRowTile, a = ea % n_out, ee = ea / n_out;
          const int64_t bb = b0 + ee;
          if (kk < nb && bb < p.B) rows[(bb * n_out + a) * row_len + n0 + kk] = sOut[ee][a][kk];
        }
        __syncthreads();
      }
      if (n + 1 < n_max) {
        right_mul(x, y);
        left_mul(chain.template mixed<D>(y, z), x);
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

template <int D, class Chain>
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
  const Chain chain(p);
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
  // tr(L_a x) for the first n_out of the L_a, in v of every thread
  auto read_out = [&](const double2 x, const int n_out) {
#pragma unroll
    for (int a = 0; a < kMaxObservableOps; ++a) {
      const double2 w = cmul(Lji[a], x);
      v[2 * a] = w.x;
      v[2 * a + 1] = w.y;
    }
    block_sum_n<D>(v, 2 * n_out, sRed, tid);
  };

  if (p.one != nullptr) {
    read_out(r, n_ops);
#pragma unroll
    for (int a = 0; a < kMaxObservableOps; ++a)
      if (a < n_ops && tid == 0) ((double2*)p.one)[b * n_ops + a] = cmul(make_double2(v[2 * a], v[2 * a + 1]), inv);
  }

  // The chains of the n_ops right operators, one after the other: x = E_(O_c)(r), then n_max times the n_ops read-outs, each followed
  // by one step of the chain; the values of read-out a are the row a row_len of `rows`.  String launches that return str walk one more
  // chain, the pure string chain: it starts from r with the string itself as its first operator and has one read-out, the plain trace
  // of x - tr(L x) with the identity in the place of L_0, which no chain needs any more.
  const int n_chains = chain.n_chains(p);
  for (int c = 0; c < n_chains; ++c) {
    const bool pure = Chain::kString && c == n_ops;      // (false at compile time in the plain instantiation)
    const double2* W = pure ? (const double2*)p.string : O + c * 4;
    const int n_out = pure ? 1 : n_ops;
    double2* rows = pure ? (double2*)p.str + b * (int64_t)n_max : (double2*)p.C + (b * n_ops * n_ops + c) * (int64_t)n_max;
    const int64_t row_len = pure ? (int64_t)n_max : (int64_t)n_ops * n_max;
    if (pure) Lji[0] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    __syncthreads();
    sX[i][j] = r;
    __syncthreads();
    double2 x = apply(W[0], W[1], W[2], W[3], false);
    for (int n = 0; n < n_max; ++n) {
      const int k = n % kBlockTile;
      read_out(x, n_out);
      if (tid == 0) {
#pragma unroll
        for (int a = 0; a < kMaxObservableOps; ++a)
          if (a < n_out) sOut[a][k] = cmul(make_double2(v[2 * a], v[2 * a + 1]), inv);
      }
      if (k == kBlockTile - 1 || n == n_max - 1) {
        __syncthreads();
        const int nb = k + 1, n0 = n - k, a = tid / kBlockTile, kk = tid % kBlockTile;
        if (a < n_out && kk < nb) rows[a * row_len + n0 + kk] = sOut[a][kk];
        __syncthreads();
      }
      if (n + 1 < n_max) {
        sX[i][j] = x;
        __syncthreads();
        x = chain.step(apply);
      }
    }
  }
}

template <class Chain>
hipError_t launch_chain(int D, const CorrelatorArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (a.n_ops < 1 || a.n_ops > kMaxObservableOps || a.n_max < 1) return hipErrorInvalidValue;
  if (Chain::kString != (a.string != nullptr) || (!Chain::kString && a.str != nullptr)) return hipErrorInvalidValue;
  switch (D) {
    case 2: hipLaunchKernelGGL((correlator_rows_kernel<2, Chain>), dim3((unsigned)((a.B + 31) / 32)), dim3(64), 0, st, a); break;
    case 4: hipLaunchKernelGGL((correlator_rows_kernel<4, Chain>), dim3((unsigned)((a.B + 15) / 16)), dim3(64), 0, st, a); break;
    case 8: hipLaunchKernelGGL((correlator_block_kernel<8, Chain>), dim3((unsigned)a.B), dim3(64), 0, st, a); break;
    case 16: hipLaunchKernelGGL((correlator_block_kernel<16, Chain>), dim3((unsigned)a.B), dim3(256), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_correlators(int D, const CorrelatorArgs& a, hipStream_t st) { return launch_chain<PlainChain>(D, a, st); }
hipError_t launch_string_correlators(int D, const CorrelatorArgs& a, hipStream_t st) { return launch_chain<StringChain>(D, a, st); }

}  // namespace qmps
