// qmps_overlap_square.hip - time-evolution overlap objective at bond dimension D = 2 and D = 4: the kernels that SQUARE the matrix of
// the map (gfx950 only).  The map T(x) = sum_s C_s x Bm_s^+: see qmps_overlap.hip.
//   overlap_lane_kernel        D = 2: the 4 x 4 matrix of T, one evaluation per lane (qmps_overlap_d2.h).
//   overlap_square_d4_kernel   D = 4: the map is ONE complex 16 x 16 tile - squared on the matrix cores until it is rank one
//                              (O(log) rounds whatever the spectral gap), one wave per evaluation (qmps_overlap_d4.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_overlap_d2.h"
#include "qmps_overlap_d4.h"

namespace qmps {

// ------------------------------------------------------------------------------------------
// Kernel 3d: time-evolution overlap objective (qmps/new_time_evolve.py:193-221,
// scripts/loschmidt.py:209-239), D = 2, one evaluation per lane.
//   T(x) = sum_{s=0..3} C_s x Bm_s^+ ,  C = WW . merge(A, A) ,  Bm = merge(B, B)
// (qmps/time_evolve_tools.py:20-23); the 6-qubit circuit of the reference measures
// 2 |psi[0]| = |eta|, eta the dominant eigenvalue of T, and the objective is -sqrt(|eta|).
// eta is found by power iteration applied 2^m steps at a time: the 4 x 4 complex matrix of T is
// squared (Frobenius-normalised each round), its dominant right vector v read off the largest column,
// eta = <v, T v>/<v, v>, stop when ||T v - eta v|| < tol ||v||.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void overlap_lane_kernel(OverlapArgs p) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= p.B || overlap_skipped(p, b)) return;
  const double2* Ap = (const double2*)p.A + overlap_ref_index(p, b) * 8;
  const double2* Bp = (const double2*)p.Bt + b * 8;
  OverlapLaneResult o;
  overlap_lane_solve([&](int k) { return Ap[k]; }, [&](int k) { return Bp[k]; }, (const double2*)p.WW, p.max_rounds, p.tol, o);
  overlap_store(p, b, o.eta_r, o.eta_i, o.rounds, o.status);
  if (p.r_out != nullptr) {
    double n2 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) n2 += o.vr[a] * o.vr[a] + o.vi[a] * o.vi[a];
    const double inv = n2 > 0.0 ? 1.0 / __builtin_sqrt(n2) : 0.0;
    double2* ro = (double2*)((char*)p.r_out + overlap_slot_offset(p));
#pragma unroll
    for (int a = 0; a < 4; ++a) ro[b * 4 + a] = make_double2(o.vr[a] * inv, o.vi[a] * inv);
  }
}

hipError_t launch_overlap(const OverlapArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(overlap_lane_kernel, dim3((unsigned)((a.B + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// D = 4 on the matrix cores: the mixed transfer map IS one complex 16 x 16 tile,
//   E[(i,i'),(j,j')] = sum_{s<4} C_s[i][j] conj(Bm_s[i'][j']),
// so the power method is taken 2^m steps at a time by SQUARING it (one wave per evaluation, 16 v_mfma_f64_16x16x4 per
// round, Frobenius-normalised): O(log) rounds whatever the spectral gap - the plain power method needed up to 27 386
// steps inside a batch of 65 536 time-step candidates.  M = E^(2^m)/scale tends to the rank-one u v^+; a rank-one
// matrix satisfies M M = tr(M) M, which is the convergence test (||M M - tr(M) M||_F < tol ||M M||_F, elementwise in
// the accumulator layout, no gather), and then eta = tr(M E)/tr(M) (= v^+ E u / v^+ u).  The right fixed point, when
// asked for, is the largest column of M.  rounds = squarings used; status 1 = not rank one within max_rounds (two
// dominant eigenvalues of equal modulus) or tr(M) = 0.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 3) void overlap_square_d4_kernel(OverlapArgs p) {
  constexpr int WAVES = 4;
  __shared__ double2 sT_all[WAVES][kSquareD4Scratch];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  double2* sT = sT_all[wave];
  const double tol2 = p.tol * p.tol;
  for (int64_t b = (int64_t)blockIdx.x * WAVES + wave; b < p.B; b += (int64_t)gridDim.x * WAVES) {
    if (overlap_skipped(p, b)) continue;
    // (set-up, squaring rounds, eta: qmps_overlap_d4.h)
    double eta_r, eta_i;
    int rounds, status;
    v4f64 mr, mi;
    overlap_square_d4_item((const double2*)p.A + overlap_ref_index(p, b) * 32, (const double2*)p.Bt + b * 32, (const double2*)p.WW, sT, p.max_rounds, tol2,
                           eta_r, eta_i, rounds, status, mr, mi);
    if (lane == 0) overlap_store(p, b, eta_r, eta_i, rounds, status);
    // (the left solve's record: eta, rounds, status and statistics.  No objective: f_out[B ..] holds the neighbours' objectives of
    // qmps_overlap_gradient, and a skipped trajectory's must stay - this used to overwrite the first B of them, which the probes put
    // right for every trajectory but a skipped one)
    if (p.l_out != nullptr && lane == 0) overlap_store(p, b + p.B, eta_r, eta_i, rounds, status, false);
    if ((p.r_out != nullptr && p.adjoint) || p.l_out != nullptr) {
      // LEFT fixed point (T^+ y = conj(eta) y): M -> u v^+, so every row of M is a multiple of v^+; y = conj of the largest row
      void* lo = p.l_out != nullptr ? p.l_out : p.r_out;
      double rn[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) rn[q] = row16_sum(dfma(mr[q], mr[q], mi[q] * mi[q]));      // |row 4 q + g|^2, in the 16 lanes of row group g
      __builtin_amdgcn_wave_barrier();
      if (c == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sT[4 * q + g] = make_double2(rn[q], 0.0);
      }
      __builtin_amdgcn_wave_barrier();
      int best = 0;
      double bn = -1.0;
      for (int k = 0; k < 16; ++k) {
        const double v = sT[k].x;
        if (v > bn) { bn = v; best = k; }
      }
      __builtin_amdgcn_wave_barrier();
      if (g == (best & 3)) {
        double vr = 0.0, vi = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q == (best >> 2)) { vr = mr[q]; vi = mi[q]; }
        sT[16 + c] = make_double2(vr, -vi);
      }
      __builtin_amdgcn_wave_barrier();
      const double inv = bn > 0.0 ? 1.0 / __builtin_sqrt(bn) : 0.0;
      if (lane < 16) {
        const double2 u = sT[16 + lane];
        ((double2*)((char*)lo + overlap_slot_offset(p)))[b * 16 + lane] = make_double2(u.x * inv, u.y * inv);
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (p.r_out != nullptr && !p.adjoint) {
      // right fixed point = the largest column of M, unit Frobenius norm
      double cn = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) cn = dfma(mr[q], mr[q], dfma(mi[q], mi[q], cn));
      cn = group4_sum(cn);                       // norm^2 of column c, in every row group
      __builtin_amdgcn_wave_barrier();
      if (g == 0) sT[c] = make_double2(cn, 0.0);
      __builtin_amdgcn_wave_barrier();
      int best = 0;
      double bn = -1.0;
      for (int k = 0; k < 16; ++k) {
        const double v = sT[k].x;
        if (v > bn) { bn = v; best = k; }
      }
      __builtin_amdgcn_wave_barrier();
      if (c == best) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sT[16 + 4 * q + g] = make_double2(mr[q], mi[q]);
      }
      __builtin_amdgcn_wave_barrier();
      const double inv = bn > 0.0 ? 1.0 / __builtin_sqrt(bn) : 0.0;
      if (lane < 16) {
        const double2 u = sT[16 + lane];
        ((double2*)((char*)p.r_out + overlap_slot_offset(p)))[b * 16 + lane] = make_double2(u.x * inv, u.y * inv);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
}

hipError_t launch_overlap_square_d4(const OverlapArgs& a, hipStream_t st) {
  int grid = (int)((a.B + 3) / 4);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(overlap_square_d4_kernel, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace qmps
