// qmps_overlap_block.hip - time-evolution overlap objective, the generic tile kernel (gfx950 only).
//
// The map T(x) = sum_s C_s x Bm_s^+ and the power method on it: see qmps_overlap.hip.
//   overlap_block_kernel<D>    D = 8 (D = 4, 16 fall-backs): thread (i, j) of a D x D tile per evaluation (D = 4: four evaluations per
//                              wave, one per DPP row), tiles of C_s, Bm_s, x, Y_s = x Bm_s^+ in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_complex.h"

namespace qmps {

// ADJ: power method on the adjoint map y -> sum_s C_s^+ y Bm_s (its dominant eigenvalue is conj(eta), its fixed point the LEFT
// eigenvector of T for the Frobenius pairing: <y, T x> = <T^+ y, x>); eta_out receives eta itself
// (the body as a device function: the workgroups of one launch may run different instantiations - overlap_block_pair_kernel)
template <int D, bool ADJ>
__device__ __forceinline__ void overlap_block_body(const OverlapArgs& p, int64_t block) {
  constexpr int N = D * D, P = D + 1;
  constexpr int THREADS = N < 64 ? 64 : N, ITEMS = THREADS / N, WAVES = THREADS / 64;
  __shared__ double2 sC[ITEMS][4][D][P], sB[ITEMS][4][D][P], sX[ITEMS][D][P], sY[ITEMS][4][D][P];
  __shared__ double red[4][WAVES > 1 ? WAVES : 1];
  const int tid = threadIdx.x, e = tid / N, l = tid % N, i = l / D, j = l % D;
  const int64_t b = block * ITEMS + e;
  if (ITEMS == 1 && b < p.B && overlap_skipped(p, b)) return;      // (one evaluation per workgroup: a uniform exit)
  const bool valid = b < p.B;
  const int64_t bb = valid ? b : p.B - 1;       // surplus lanes of the last workgroup shadow a real evaluation
  // sum over the N threads of one evaluation (up to four values at a time), result in every one of them
  auto group_sum4 = [&](double (&v)[4]) {
    if constexpr (N == 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = row16_sum(v[q]);
    } else if constexpr (N == 64) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = wave_sum(v[q]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = wave_sum(v[q]);
      __syncthreads();
      if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[q][tid >> 6] = v[q];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) t += red[q][w];
        v[q] = t;
      }
    }
  };
  // ---- set-up: inputs through the Y tiles, then C_s = sum_t WW[s][t] A_t1 A_t2 and Bm_s = B_s1 B_s2
  {
    const double2* Ap = (const double2*)p.A + overlap_ref_index(p, bb) * (2 * N);
    const double2* Bp = (const double2*)p.Bt + bb * (2 * N);
    sY[e][0][i][j] = Ap[l];
    sY[e][1][i][j] = Ap[N + l];
    sY[e][2][i][j] = Bp[l];
    sY[e][3][i][j] = Bp[N + l];
  }
  __syncthreads();
  {
    double2 aa[4], bm[4];
#pragma unroll
    for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        double2 u = make_double2(0.0, 0.0), v = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          cfma(sY[e][t1][i][k], sY[e][t2][k][j], u);
          cfma(sY[e][2 + t1][i][k], sY[e][2 + t2][k][j], v);
        }
        aa[2 * t1 + t2] = u;
        bm[2 * t1 + t2] = v;
      }
    const double2* W = (const double2*)p.WW;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double2 c = make_double2(0.0, 0.0);
#pragma unroll
      for (int t = 0; t < 4; ++t) cfma(W[s * 4 + t], aa[t], c);
      sC[e][s][i][j] = c;
      sB[e][s][i][j] = bm[s];
    }
  }
  double2 x_cold = overlap_cold_start(i, j, D);      // (generic: see overlap_cold_start)
  {
    double v[4] = {x_cold.x * x_cold.x + x_cold.y * x_cold.y, 0.0, 0.0, 0.0};
    group_sum4(v);
    const double inv = 1.0 / __builtin_sqrt(v[0]);
    x_cold = make_double2(x_cold.x * inv, x_cold.y * inv);
  }
  double2 x = x_cold;
  const int64_t slot_off = overlap_slot_offset(p);
  if (p.x_in != nullptr) {      // warm start: the resident fixed point of this candidate's slot (all zero: none yet)
    const double2 w = ((const double2*)((const char*)p.x_in + slot_off))[(p.x_in_group > 0 ? bb / p.x_in_group : bb) * N + l];
    double v[4] = {w.x * w.x + w.y * w.y, 0.0, 0.0, 0.0};
    group_sum4(v);
    if (v[0] > 1e-200 && v[0] < 1e200) {
      const double inv = 1.0 / __builtin_sqrt(v[0]);
      x = make_double2(w.x * inv, w.y * inv);
    }
  }
  double2 eta = make_double2(0.0, 0.0);
  int iters = 0, status = QMPS_ST_NOT_CONVERGED;
  bool active = true;
  const double tol2 = overlap_tol2(p, b < p.B ? b : p.B - 1);
  // deflation steps (below): one evaluation per wave only - the branch must be uniform over the lanes of a reduction
  constexpr bool kDeflate = D == 8;
  double2 rp = make_double2(0.0, 0.0), sg_prev = make_double2(0.0, 0.0);
  double w0_prev = 0.0, n_prev = 0.0, sig_max2 = 0.0;
  int last_deflation = 0;
  bool deflate_on = p.no_deflation == 0;
  // hand-over to the Krylov fall-back (one evaluation per workgroup only: the decision must be uniform)
  const int give_up_after = (ITEMS == 1 && p.r_out != nullptr && p.kry_counter != nullptr) ? p.krylov_after : 0;
  int k_ref = 0;
  float l_ref = 0.0f;
  __syncthreads();
  for (int k = 1; k <= p.max_rounds; ++k) {
    if (!__syncthreads_or(active ? 1 : 0)) break;
    sX[e][i][j] = x;
    __syncthreads();
    // Y_s = x Bm_s^+   (ADJ: x Bm_s)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double2 y = make_double2(0.0, 0.0);
#pragma unroll
      for (int kk = 0; kk < D; ++kk) {
        if constexpr (ADJ) cfma(sX[e][i][kk], sB[e][s][kk][j], y);
        else cfma_conj(sX[e][i][kk], sB[e][s][j][kk], y);
      }
      sY[e][s][i][j] = y;
    }
    __syncthreads();
    // x' = sum_s C_s Y_s   (ADJ: C_s^+ Y_s)
    double2 xn = make_double2(0.0, 0.0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int kk = 0; kk < D; ++kk) {
        if constexpr (ADJ) cfma_conj(sY[e][s][kk][j], sC[e][s][kk][i], xn);
        else cfma(sC[e][s][i][kk], sY[e][s][kk][j], xn);
      }
    // eta = <x, x'>, ||x'||^2, then the residual ||x' - eta x||^2   (||x||_F = 1)
    double v[4] = {x.x * xn.x + x.y * xn.y, x.x * xn.y - x.y * xn.x, xn.x * xn.x + xn.y * xn.y, 0.0};
    group_sum4(v);
    const double2 et = make_double2(v[0], v[1]);
    const double nn = v[2];
    const double dr = xn.x - (et.x * x.x - et.y * x.y), di = xn.y - (et.x * x.y + et.y * x.x);
    // (the spare slots of this reduction: <r_{k-1}, r_k> for the estimate of the second eigenvalue, see below)
    double w[4] = {dr * dr + di * di, rp.x * dr + rp.y * di, rp.x * di - rp.y * dr, 0.0};
    group_sum4(w);
    if (active) {
      eta = et;
      iters = k;
      const double e2 = et.x * et.x + et.y * et.y;
      if (w[0] < tol2 && kDeflate && sig_max2 > 0.0 && !(e2 > sig_max2 * (1.0 + 1e-3))) {
        // converged - to an eigenvalue that does not dominate one of those a deflation step removed (a nearly degenerate
        // dominant pair: the shift took out the wrong one).  Start again, plain power method only.
        deflate_on = false;
        sig_max2 = 0.0;
        w0_prev = 0.0;
        k_ref = 0;
        rp = make_double2(0.0, 0.0);
        x = x_cold;
      } else if (w[0] < tol2) {
        status = QMPS_ST_OK;
        active = false;
      } else {
        bool deflated = false;
        if constexpr (kDeflate) {
          // Slow convergence = a second eigenvalue eta_2 close to eta_1 in modulus.  The residual r_k = (T - eta_k) x_k is then
          // dominated by that eigenvector, r_k ~ (eta_2 / n_{k-1}) r_{k-1} with n = ||T x||, so two successive residuals give
          // eta_2 for free; ONE step with the shifted map, x <- (T - sigma) x = T x - sigma x, removes that component (Wielandt).
          // It also amplifies every other component by |eta_j - sigma| / |eta_1 - sigma|, so it is taken only when the plain
          // iteration is slow, the estimate has settled, and not again before the plain steps have damped what it stirred up.
          // The result is still the power method's: convergence is declared by the same residual test on plain steps only.
          const double2 sg = w0_prev > 0.0 ? make_double2(n_prev * w[1] / w0_prev, n_prev * w[2] / w0_prev) : make_double2(0.0, 0.0);
          const double ds = (sg.x - sg_prev.x) * (sg.x - sg_prev.x) + (sg.y - sg_prev.y) * (sg.y - sg_prev.y), s2 = sg.x * sg.x + sg.y * sg.y;
          // (the estimate settled to 1e-4, and what it names is smaller in modulus than the current Rayleigh quotient - never
          // shift out something that may be the dominant eigenvalue; the check above is the safety net behind this one)
          if (deflate_on && k >= 24 && k - last_deflation >= 12 && w[0] > 0.64 * w0_prev && ds < 1e-8 * s2 && s2 < 0.998 * e2 && s2 > 0.25 * e2) {
            double2 xd = make_double2(xn.x - (sg.x * x.x - sg.y * x.y), xn.y - (sg.x * x.y + sg.y * x.x));
            double q[4] = {xd.x * xd.x + xd.y * xd.y, 0.0, 0.0, 0.0};
            group_sum4(q);
            if (q[0] > 1e-280) {
              const double inv = 1.0 / __builtin_sqrt(q[0]);
              x = make_double2(xd.x * inv, xd.y * inv);
              deflated = true;
              last_deflation = k;
              sig_max2 = s2 > sig_max2 ? s2 : sig_max2;
            }
          }
          sg_prev = sg;
          w0_prev = deflated ? 0.0 : w[0];
          n_prev = __builtin_sqrt(nn);
          rp = make_double2(dr, di);
        }
        if (!deflated) {
          const double inv = nn > 0.0 ? 1.0 / __builtin_sqrt(nn) : 0.0;
          x = make_double2(xn.x * inv, xn.y * inv);
        } else {
          k_ref = 0;
        }
        // a long tail ahead: stop here (status 1, k < max_rounds) - overlap_krylov_kernel takes the candidate over from x
        if (power_gives_up(k, w[0], tol2, give_up_after, k_ref, l_ref) && k < p.max_rounds) {
          active = false;
          if (tid == 0) atomicAdd(p.kry_counter + 2, 1);
        }
      }
    }
  }
  if (!valid) return;
  if (l == 0) overlap_store(p, b, eta.x, ADJ ? -eta.y : eta.y, iters, status);
  if (p.r_out != nullptr) ((double2*)((char*)p.r_out + slot_off))[b * N + l] = x;
}

template <int D, bool ADJ = false>
__global__ __launch_bounds__((D * D < 64) ? 64 : D * D) void overlap_block_kernel(OverlapArgs p) {
  overlap_block_body<D, ADJ>(p, blockIdx.x);
}

// RIGHT and LEFT fixed points in one launch (qmps_overlap_gradient at D = 8): workgroups [0, n_right) run the map of `pr`, the
// others the adjoint map of `pl` - the iteration chains are latency-bound, the left solve rides along on idle SIMDs
template <int D>
__global__ __launch_bounds__((D * D < 64) ? 64 : D * D) void overlap_block_pair_kernel(OverlapArgs pr, OverlapArgs pl, int n_right) {
  if ((int)blockIdx.x < n_right) overlap_block_body<D, false>(pr, blockIdx.x);
  else overlap_block_body<D, true>(pl, (int64_t)blockIdx.x - n_right);
}

hipError_t launch_overlap_pair_d8(const OverlapArgs& right, const OverlapArgs& left, hipStream_t st, bool krylov_now) {
  if (right.B <= 0) return hipSuccess;
  hipLaunchKernelGGL((overlap_block_pair_kernel<8>), dim3((unsigned)(right.B + left.B)), dim3(64), 0, st, right, left, (int)right.B);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  return krylov_now ? launch_krylov_after(8, right, &left, st) : hipSuccess;
}

hipError_t launch_overlap_block(int D, const OverlapArgs& a, hipStream_t st) {
  switch (D) {
    case 4:
      if (a.adjoint) hipLaunchKernelGGL((overlap_block_kernel<4, true>), dim3((unsigned)((a.B + 3) / 4)), dim3(64), 0, st, a);
      else hipLaunchKernelGGL((overlap_block_kernel<4>), dim3((unsigned)((a.B + 3) / 4)), dim3(64), 0, st, a);
      break;
    case 8:
      if (a.adjoint) hipLaunchKernelGGL((overlap_block_kernel<8, true>), dim3((unsigned)a.B), dim3(64), 0, st, a);
      else hipLaunchKernelGGL((overlap_block_kernel<8>), dim3((unsigned)a.B), dim3(64), 0, st, a);
      break;
    case 16:
      if (a.adjoint) hipLaunchKernelGGL((overlap_block_kernel<16, true>), dim3((unsigned)a.B), dim3(256), 0, st, a);
      else hipLaunchKernelGGL((overlap_block_kernel<16>), dim3((unsigned)a.B), dim3(256), 0, st, a);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace qmps
