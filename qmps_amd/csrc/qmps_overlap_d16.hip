// qmps_overlap_d16.hip - time-evolution overlap objective at bond dimension D = 16 on the matrix cores (gfx950 only).
//
// The map T(x) = sum_s C_s x Bm_s^+ and the power method on it: see qmps_overlap.hip.  A complex 16 x 16 x 16 product is 3 real
// v_mfma_f64_16x16x4_f64 chains (cmma16_3m); per step Y_s = x Bm_s^+ and x' += C_s Y_s for the four s, register to register but for
// ONE LDS transpose of x (C-layout of a product == B-layout of the next; Bm_s^+ in B-layout == conj of Bm_s in A-layout).  The
// wave-level steps are those of qmps_tile16.h.
//
//   overlap_mfma_d16x4_kernel       FOUR WAVES PER EVALUATION, wave w owns the physical index s = w: what launch_overlap_mfma_d16 runs at
//                                   every batch size (beyond 2 048 evaluations the workgroups draw them from a queue in HBM).
//   overlap_mfma_d16x4_pair_kernel  the same for the right and the left solves of a gradient in one launch, the surplus workgroups
//                                   building the central-difference neighbours' tensors.
//   overlap_mfma_d16_kernel         ONE WAVE PER EVALUATION: batches above 2 048 without a queue (QMPS_D16_ONE_WAVE) - and what the
//                                   tests compare the split kernels with.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_complex.h"
#include "qmps_tile16.h"
#include "qmps_circuit_wave.h"

namespace qmps {

namespace {

// The power iterations below test convergence on every SECOND step only (and on the last one): the three wave-wide sums and the
// residual pass of a test are a third of a step's latency once the products take 24 instead of 32 matrix instructions; between
// tests the iterate is not normalised (it shrinks by |eta| ~ 0.5 .. 1 per step).  `rounds` counts every step.
__device__ __forceinline__ bool overlap_check_step(int k, int max_rounds) { return (k & 1) == 0 || k == max_rounds; }

}  // namespace

// ------------------------------------------------------------------------------------------
// one wave per evaluation
// ------------------------------------------------------------------------------------------
template <bool ADJ>
__global__ __launch_bounds__(256) void overlap_mfma_d16_kernel(OverlapArgs p) {
  constexpr int D = 16, WAVES = 4;
  __shared__ double2 sT_all[WAVES][D * kTile16Ld];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  double2* sT = sT_all[wave];
  const double tol2 = p.tol * p.tol;
  const int64_t slot_off = overlap_slot_offset(p);
  for (int64_t b = (int64_t)blockIdx.x * WAVES + wave; b < p.B; b += (int64_t)gridDim.x * WAVES) {
    if (overlap_skipped(p, b)) continue;
    const double2* Ap = (const double2*)p.A + overlap_ref_index(p, b) * (2 * D * D);
    const double2* Bp = (const double2*)p.Bt + b * (2 * D * D);
    const double2* W = (const double2*)p.WW;
    // ---- set-up: AA_t = A_t1 A_t2 and BB_t = B_t1 B_t2 (C-layout), C_s = sum_t WW[s][t] AA_t; both sets to A-layout
    double cre[4][4], cim[4][4];     // C_s in A-layout (the P operand of x' += C_s Y_s)
    double bre[4][4], bimn[4][4];    // conj(Bm_s) in A-layout == Bm_s^+ in B-layout (the Q operand of Y_s = x Bm_s^+)
    // ADJ (y -> sum_s C_s^+ y Bm_s): the Q operand of Y_s = y Bm_s is Bm_s in B-layout - the C-layout the product B_s1 B_s2 comes
    // out in - and the P operand of y' += C_s^+ Y_s is C_s^+ in A-layout = conj of C_s in C-layout: no LDS transpose in the set-up
    {
      double pa[2][4], pai[2][4], pb[2][4], pbi[2][4];   // A_s, B_s in A-layout
      v4f64 qa[2], qai[2], qb[2], qbi[2];                 // A_s, B_s in B-layout (= C-layout)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const double2 va = Ap[(s * D + c) * D + 4 * kk + g], vb = Bp[(s * D + c) * D + 4 * kk + g];
          pa[s][kk] = va.x; pai[s][kk] = va.y;
          pb[s][kk] = vb.x; pbi[s][kk] = vb.y;
          const double2 wa = Ap[(s * D + 4 * kk + g) * D + c], wb = Bp[(s * D + 4 * kk + g) * D + c];
          qa[s][kk] = wa.x; qai[s][kk] = wa.y;
          qb[s][kk] = wb.x; qbi[s][kk] = wb.y;
        }
      v4f64 aar[4], aai[4];
#pragma unroll
      for (int t1 = 0; t1 < 2; ++t1)
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
          v4f64 zr = {0, 0, 0, 0}, zi = {0, 0, 0, 0};
          cmma16(pa[t1], pai[t1], qa[t2], qai[t2], zr, zi);
          aar[2 * t1 + t2] = zr;
          aai[2 * t1 + t2] = zi;
          v4f64 yr = {0, 0, 0, 0}, yi = {0, 0, 0, 0};
          cmma16(pb[t1], pbi[t1], qb[t2], qbi[t2], yr, yi);
          if constexpr (ADJ) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              bre[2 * t1 + t2][kk] = yr[kk];
              bimn[2 * t1 + t2][kk] = yi[kk];
            }
          } else {
            double tr[4], ti[4];
            tile16_to_a_layout(sT, yr, yi, tr, ti);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              bre[2 * t1 + t2][kk] = tr[kk];
              bimn[2 * t1 + t2][kk] = -ti[kk];
            }
          }
        }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        v4f64 zr = {0, 0, 0, 0}, zi = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double2 w = W[s * 4 + t];
          zr += w.x * aar[t] - w.y * aai[t];
          zi += w.x * aai[t] + w.y * aar[t];
        }
        if constexpr (ADJ) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            cre[s][kk] = zr[kk];
            cim[s][kk] = -zi[kk];
          }
        } else {
          tile16_to_a_layout(sT, zr, zi, cre[s], cim[s]);
        }
      }
    }
    // ---- power method, x in C-layout, ||x||_F = 1
    v4f64 xr, xi;
    tile16_cold_start(xr, xi);
    if (p.x_in != nullptr)       // warm start: the resident fixed point of this candidate's slot (all zero: none yet)
      tile16_warm_start((const double2*)((const char*)p.x_in + slot_off) + (p.x_in_group > 0 ? b / p.x_in_group : b) * (D * D), xr, xi);
    double eta_r = 0.0, eta_i = 0.0;
    int iters = 0, status = QMPS_ST_NOT_CONVERGED;
    for (int k = 1; k <= p.max_rounds; ++k) {
      double xar[4], xai[4];
      tile16_to_a_layout(sT, xr, xi, xar, xai);
      v4f64 nr = {0, 0, 0, 0}, ni = {0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        v4f64 yr = {0, 0, 0, 0}, yi = {0, 0, 0, 0};
        const v4f64 qre = {bre[s][0], bre[s][1], bre[s][2], bre[s][3]};
        const v4f64 qim = {bimn[s][0], bimn[s][1], bimn[s][2], bimn[s][3]};
        cmma16_3m(xar, xai, qre, qim, yr, yi);           // Y_s = x Bm_s^+
        cmma16_3m(cre[s], cim[s], yr, yi, nr, ni);       // x' += C_s Y_s
      }
      iters = k;
      if (!overlap_check_step(k, p.max_rounds)) {        // no test on this step: carry the (unnormalised) iterate on
        xr = nr;
        xi = ni;
        continue;
      }
      double xx, nn, rs_sum;
      const double res2 = tile16_power_test(xr, xi, nr, ni, eta_r, eta_i, xx, nn, rs_sum);     // ||T x - eta x||^2 / ||x||^2
      if (res2 < tol2) {
        status = QMPS_ST_OK;
        const double inv = xx > 0.0 ? 1.0 / __builtin_sqrt(xx) : 0.0;      // the fixed point handed out has unit norm
        xr *= inv;
        xi *= inv;
        break;
      }
      const double inv = nn > 0.0 ? 1.0 / __builtin_sqrt(nn) : 0.0;
      xr = nr * inv;
      xi = ni * inv;
    }
    if (lane == 0) overlap_store(p, b, eta_r, ADJ ? -eta_i : eta_i, iters, status);
    if (p.r_out != nullptr) {
      double2* ro = (double2*)((char*)p.r_out + slot_off) + b * (D * D);
#pragma unroll
      for (int q = 0; q < 4; ++q) ro[(4 * q + g) * D + c] = make_double2(xr[q], xi[q]);
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------
// D = 16, FOUR WAVES PER EVALUATION (small batches: BASELINE.json configs[4] shards its trajectories over the GPUs, a GPU
// holds tens to hundreds of candidates).  Wave w of the workgroup owns the physical index s = w: it keeps only C_w and
// Bm_w, computes n_w = C_w (x Bm_w^+) - 32 of the step's 128 MFMAs - and the four partial maps are summed through LDS (same
// order in every wave, so all four hold bit-identical x' and take the same decisions).  One wave per evaluation leaves a
// quarter of the SIMDs idle at B = 768 and, worse, lets the launch wait for its slowest candidate at one wave's pace; here
// the stragglers run on four SIMDs each.
// ------------------------------------------------------------------------------------------
// (the body as a device function: the workgroups of one launch may run different instantiations - overlap_mfma_d16x4_pair_kernel)
// DEFL: with deflation steps (cold starts - the instantiation for warm-started batches is the lean loop: the bookkeeping of the
// deflation steps costs 6 - 8 % of a step even where it never fires, measured on the evolve workload whose batches are all warm)
template <bool ADJ, bool DEFL>
__device__ __forceinline__ void overlap_mfma_d16x4_body(const OverlapArgs& p, int64_t b_first, int64_t b_stride, double2 (*sT_all)[16 * kTile16Ld],
                                                        double2 (*sX_all)[16 * 16]) {
  constexpr int D = 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  double2* sT = sT_all[wave];
  const int64_t slot_off = overlap_slot_offset(p);
  // p.queue != nullptr: the workgroups PULL their evaluations from a counter in HBM (dynamic: a workgroup that drew a slow
  // candidate - hundreds of power steps against tens - does not hold up the candidates a static stride would have queued behind
  // it); the counter value travels to the four waves through the (then idle) first exchange word
  for (int64_t b = b_first;; b += b_stride) {
    if (p.queue != nullptr) {
      if (threadIdx.x == 0) ((int*)&sX_all[0][0])[0] = atomicAdd(p.queue, 1);
      __syncthreads();
      b = ((const int*)&sX_all[0][0])[0];
      __syncthreads();
    }
    if (b >= p.B) break;
    if (overlap_skipped(p, b)) continue;          // (uniform over the workgroup: all four waves see the same b)
    const double tol2 = overlap_tol2(p, b);
    const double2* Ap = (const double2*)p.A + overlap_ref_index(p, b) * (2 * D * D);
    const double2* Bp = (const double2*)p.Bt + b * (2 * D * D);
    const double2* W = (const double2*)p.WW;
    // ---- set-up (tile16_split_setup): wave w owns the physical index s = w
    double cre[4], cim[4];       // C_w in A-layout (ADJ: C_w^+)
    double bre[4], bimn[4];      // conj(Bm_w) in A-layout == Bm_w^+ in B-layout (ADJ: Bm_w in B-layout)
    tile16_split_setup(Ap, Bp, D, W, wave, ADJ, sT, sX_all, cre, cim, bre, bimn);
    // ---- power method, x in C-layout (alike in the four waves), ||x||_F = 1
    v4f64 xr, xi;
    tile16_cold_start(xr, xi);
    if (p.x_in != nullptr)       // warm start: the resident fixed point of this candidate's slot (all zero: none yet)
      tile16_warm_start((const double2*)((const char*)p.x_in + slot_off) + (p.x_in_group > 0 ? b / p.x_in_group : b) * (D * D), xr, xi);
    double eta_r = 0.0, eta_i = 0.0;
    int iters = 0, status = QMPS_ST_NOT_CONVERGED;
    // Deflation steps (see overlap_block_kernel: a slowly decaying second eigenvector is shifted out, x <- T x - sigma x).  Here
    // the tests come every second step: a test at step k that finds the iteration slow keeps its residual r_k = n_k - eta x_k;
    // step k + 1 works on x_{k+1} = n_k / |n_k|, so its product gives T r_k = (n_{k+1} - eta x_{k+1}) |n_k| and with it
    // sigma = <r_k, T r_k> / <r_k, r_k> - and holds both vectors of the shifted step.  All four waves hold the same numbers.
    bool defl_on = DEFL && p.no_deflation == 0, pending = false, have_prev_sigma = false;
    v4f64 rr = {0, 0, 0, 0}, ri = {0, 0, 0, 0};
    double rs_chk = 0.0, inv_chk = 0.0, res_prev = 0.0, sgr_prev = 0.0, sgi_prev = 0.0, sig_max2 = 0.0;
    int last_deflation = 0;
    const int give_up_after = (p.r_out != nullptr && p.kry_counter != nullptr) ? p.krylov_after : 0;       // hand-over to the Krylov fall-back (see OverlapArgs)
    int k_ref = 0;
    float l_ref = 0.0f;
    for (int k = 1; k <= p.max_rounds; ++k) {
      double xar[4], xai[4];
      tile16_to_a_layout(sT, xr, xi, xar, xai);
      v4f64 yr = {0, 0, 0, 0}, yi = {0, 0, 0, 0}, pr = {0, 0, 0, 0}, pi = {0, 0, 0, 0};
      const v4f64 qre = {bre[0], bre[1], bre[2], bre[3]};
      const v4f64 qim = {bimn[0], bimn[1], bimn[2], bimn[3]};
      cmma16_3m(xar, xai, qre, qim, yr, yi);           // Y_w = x Bm_w^+
      cmma16_3m(cre, cim, yr, yi, pr, pi);             // C_w Y_w
      // the four partial maps are exchanged through one of TWO sets of buffers, alternately: a wave may publish step k + 1
      // while another still reads step k, so a step needs ONE workgroup barrier (a set is reused two barriers later)
      double2 (*sXk)[16 * 16] = sX_all + 4 * (k & 1);
      tile16_publish(sXk[wave], pr, pi);
      __syncthreads();
      v4f64 nr = {0, 0, 0, 0}, ni = {0, 0, 0, 0};
#pragma unroll
      for (int w = 0; w < 4; ++w) {                 // the same order in every wave: bit-identical sums
        v4f64 tr, ti;
        tile16_fetch(sXk[w], tr, ti);
        nr += tr;
        ni += ti;
      }
      iters = k;
      if (!overlap_check_step(k, p.max_rounds)) {   // no test on this step (see overlap_check_step)
        if (DEFL && pending) {
          pending = false;
          double b0 = 0.0, b1 = 0.0;
          v4f64 tr_, ti_;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            tr_[q] = nr[q] - (eta_r * xr[q] - eta_i * xi[q]);
            ti_[q] = ni[q] - (eta_r * xi[q] + eta_i * xr[q]);
            b0 = dfma(rr[q], tr_[q], dfma(ri[q], ti_[q], b0));        // conj(r) (T r)
            b1 = dfma(rr[q], ti_[q], dfma(-ri[q], tr_[q], b1));
          }
          const double den = inv_chk * rs_chk;
          const double sgr = den > 0.0 ? lane0(wave_sum(b0)) / den : 0.0, sgi = den > 0.0 ? lane0(wave_sum(b1)) / den : 0.0;
          const double s2 = sgr * sgr + sgi * sgi, e2 = eta_r * eta_r + eta_i * eta_i;
          const double ds = (sgr - sgr_prev) * (sgr - sgr_prev) + (sgi - sgi_prev) * (sgi - sgi_prev);
          const bool settled = have_prev_sigma && ds < 1e-8 * s2;
          sgr_prev = sgr;
          sgi_prev = sgi;
          have_prev_sigma = true;
          if (settled && s2 < 0.998 * e2 && s2 > 0.25 * e2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const double ar = nr[q] - (sgr * xr[q] - sgi * xi[q]), ai = ni[q] - (sgr * xi[q] + sgi * xr[q]);
              xr[q] = ar;
              xi[q] = ai;
            }
            last_deflation = k;
            sig_max2 = s2 > sig_max2 ? s2 : sig_max2;
            have_prev_sigma = false;
            res_prev = 0.0;
            k_ref = 0;
            continue;
          }
        }
        xr = nr;
        xi = ni;
        continue;
      }
      double xx, nn, rs_sum;
      const double res2 = tile16_power_test(xr, xi, nr, ni, eta_r, eta_i, xx, nn, rs_sum);
      if (res2 < tol2) {
        const double e2 = eta_r * eta_r + eta_i * eta_i;
        if (DEFL && sig_max2 > 0.0 && !(e2 > sig_max2 * (1.0 + 1e-3))) {
          // converged - but not to an eigenvalue that dominates every shift applied (a nearly degenerate dominant pair: the shift
          // took out the wrong one): start again as a plain power method
          defl_on = false;
          sig_max2 = 0.0;
          pending = false;
          k_ref = 0;
          tile16_cold_start(xr, xi);
          continue;
        }
        status = QMPS_ST_OK;
        const double inv = xx > 0.0 ? 1.0 / __builtin_sqrt(xx) : 0.0;
        xr *= inv;
        xi *= inv;
        break;
      }
      const double inv = nn > 0.0 ? 1.0 / __builtin_sqrt(nn) : 0.0;
      // slow (the residual shrank by less than 0.8 per step since the last test)?  keep it for the estimate of the next step
      pending = DEFL && defl_on && k >= 24 && k - last_deflation >= 12 && res_prev > 0.0 && res2 > 0.41 * res_prev && k + 1 < p.max_rounds;
      if (DEFL && pending) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rr[q] = nr[q] - (eta_r * xr[q] - eta_i * xi[q]);
          ri[q] = ni[q] - (eta_r * xi[q] + eta_i * xr[q]);
        }
        rs_chk = rs_sum;
        inv_chk = inv;
      } else {
        have_prev_sigma = false;
      }
      res_prev = res2;
      xr = nr * inv;
      xi = ni * inv;
      // a long tail ahead: stop here (status 1, k < max_rounds) - overlap_krylov_kernel takes the candidate over from x
      if (k < p.max_rounds && power_gives_up(k, res2, tol2, give_up_after, k_ref, l_ref)) {
        if (threadIdx.x == 0) atomicAdd(p.kry_counter + 2, 1);
        break;
      }
    }
    if (wave == 0) {
      if (lane == 0) overlap_store(p, b, eta_r, ADJ ? -eta_i : eta_i, iters, status);
      if (p.r_out != nullptr) {
        double2* ro = (double2*)((char*)p.r_out + slot_off) + b * (D * D);
#pragma unroll
        for (int q = 0; q < 4; ++q) ro[(4 * q + g) * D + c] = make_double2(xr[q], xi[q]);
      }
    }
    __syncthreads();
  }
}

template <bool ADJ, bool DEFL>
__global__ __launch_bounds__(256, 3) void overlap_mfma_d16x4_kernel(OverlapArgs p) {
  __shared__ double2 sT_all[4][16 * kTile16Ld];   // wave-private transposes
  __shared__ double2 sX_all[8][16 * 16];          // exchange: two sets of one tile (tile16_publish) per wave
  overlap_mfma_d16x4_body<ADJ, DEFL>(p, blockIdx.x, gridDim.x, sT_all, sX_all);
}

// RIGHT and LEFT fixed points in one launch (qmps_overlap_gradient): workgroups [0, n_right) run the map of `pr`, the others the
// adjoint map of `pl` - twice the waves in flight for the same length of the (latency-bound) iteration chain
// Round 5: the workgroups behind the solves, [n_right + n_left, gridDim), BUILD THE CENTRAL-DIFFERENCE NEIGHBOURS' TENSORS of the same
// gradient evaluation (nb.params != nullptr; ShallowCNOT families: the wave-distributed circuit of qmps_circuit_wave.h, one wave
// per neighbour, two columns per pass).  The solves are a latency-bound chain on the matrix cores whose stragglers leave most of
// the chip idle; the builds are vector work with no dependence on them - in round 4 a kernel of their own on a second stream,
// which cost the critical path two cross-stream dependencies (~7 us each) per evaluation.  Solver workgroups come first in the
// grid, so they are dispatched first; the builders fill what is left and the tail.
template <bool DEFL>
__global__ __launch_bounds__(256, 3) void overlap_mfma_d16x4_pair_kernel(OverlapArgs pr, OverlapArgs pl, int n_right, int n_left, NeighbourBuildArgs nb) {
  __shared__ double2 sT_all[4][16 * kTile16Ld];
  __shared__ double2 sX_all[8][16 * 16];
  if ((int)blockIdx.x < n_right) overlap_mfma_d16x4_body<false, DEFL>(pr, blockIdx.x, n_right, sT_all, sX_all);
  else if ((int)blockIdx.x < n_right + n_left) overlap_mfma_d16x4_body<true, DEFL>(pl, blockIdx.x - n_right, n_left, sT_all, sX_all);
  else {
    const int lane = threadIdx.x & 63, a = lane & 31;
    const int P = nb.n_params;
    const int64_t n_neigh = nb.rows * 2 * P;
    for (int64_t b = ((int64_t)blockIdx.x - n_right - n_left) * 4 + (threadIdx.x >> 6); b < n_neigh; b += ((int64_t)gridDim.x - n_right - n_left) * 4) {
      const int64_t row = b / (2 * P);
      if (nb.active != nullptr && nb.active[row] == 0) continue;       // (a skipped trajectory's neighbours are never read)
      const int k = (int)(b - row * 2 * P), isel = k % P;
      // one sincos per angle and wave: lane l takes angle l (P <= 64)
      double cn = 1.0, sn = 0.0;
      if (lane < P) {
        double v = nb.params[row * P + lane];
        if (lane == isel) v += k < P ? nb.h : -nb.h;
        sincos(0.5 * v, &sn, &cn);
      }
      double2* out = (double2*)nb.out + b * 512;
#pragma unroll 1
      for (int w = 0; w < 8; ++w) {
        const int j = 2 * w + (lane >> 5);
        double re, im;
        if (nb.kind == 3) shallow_cnot_wave_column_d16<3>(cn, sn, P, j, re, im);
        else shallow_cnot_wave_column_d16<0>(cn, sn, P, j, re, im);
        out[((a & 1) * 16 + (a >> 1)) * 16 + j] = make_double2(re, im);      // A[s][i][j] = amplitude[2 i + s] of column j
      }
    }
  }
}

hipError_t launch_overlap_pair_d16(const OverlapArgs& right, const OverlapArgs& left, hipStream_t st, bool krylov_now, const NeighbourBuildArgs* build) {
  if (right.B <= 0) return hipSuccess;
  const int nr = (int)(right.B < 2048 ? right.B : 2048), nl = (int)(left.B < 2048 ? left.B : 2048);
  NeighbourBuildArgs nb;
  memset(&nb, 0, sizeof(nb));
  int n_build = 0;
  if (build != nullptr && build->params != nullptr && build->rows > 0) {
    nb = *build;
    const int64_t n_neigh = nb.rows * 2 * nb.n_params;
    n_build = (int)((n_neigh + 3) / 4 < 4096 ? (n_neigh + 3) / 4 : 4096);      // one wave per neighbour (a stride beyond 16 384 of them)
  }
  // (deflation steps for cold starts only, see overlap_mfma_d16x4_body)
  if (right.x_in == nullptr && right.no_deflation == 0) hipLaunchKernelGGL(overlap_mfma_d16x4_pair_kernel<true>, dim3((unsigned)(nr + nl + n_build)), dim3(256), 0, st, right, left, nr, nl, nb);
  else hipLaunchKernelGGL(overlap_mfma_d16x4_pair_kernel<false>, dim3((unsigned)(nr + nl + n_build)), dim3(256), 0, st, right, left, nr, nl, nb);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  return krylov_now ? launch_krylov_after(16, right, &left, st) : hipSuccess;
}

hipError_t launch_overlap_mfma_d16(const OverlapArgs& a, hipStream_t st) {
  // four waves per evaluation at every batch size (a queue in HBM hands out the evaluations when there are more of them than
  // workgroups); without a queue above 2 048 evaluations (QMPS_D16_ONE_WAVE): the one-wave-per-evaluation kernel
  if (overlap_d16_four_waves(a)) {
    const dim3 grid((unsigned)(a.B < 2048 ? a.B : 2048));
    const bool defl = a.x_in == nullptr && a.no_deflation == 0;       // cold starts only (see overlap_mfma_d16x4_body)
    if (a.adjoint && defl) hipLaunchKernelGGL((overlap_mfma_d16x4_kernel<true, true>), grid, dim3(256), 0, st, a);
    else if (a.adjoint) hipLaunchKernelGGL((overlap_mfma_d16x4_kernel<true, false>), grid, dim3(256), 0, st, a);
    else if (defl) hipLaunchKernelGGL((overlap_mfma_d16x4_kernel<false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((overlap_mfma_d16x4_kernel<false, false>), grid, dim3(256), 0, st, a);
  } else {
    int grid = (int)((a.B + 3) / 4);
    if (grid > 4096) grid = 4096;
    if (a.adjoint) hipLaunchKernelGGL(overlap_mfma_d16_kernel<true>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(overlap_mfma_d16_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace qmps
