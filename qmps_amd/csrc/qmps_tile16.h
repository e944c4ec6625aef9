// qmps_tile16.h - the wave-level steps of the 16 x 16 matrix-core eigen-solves (gfx950 only): the ONE definition of each, for the D = 16
// overlap kernels (qmps_overlap_d16.hip), the D = 16 device-resident BFGS (qmps_evolve_d16.hip), the Krylov fall-back
// (qmps_overlap_krylov.hip), the D = 16 gradient contraction (qmps_overlap_grad.hip) and the D = 4 squaring solve (qmps_overlap_d4.h).
// Not here: the largest-column / largest-row extractions of overlap_square_d4_kernel and rayleigh_ritz_wave - as a shared helper the column
// extraction cost the Krylov kernels a register (D = 8: 224 -> 225 VGPRs), so each stays written out in its kernel.
// The kernels built from them are compared bit for bit by the tests: the order of the operations in a helper is part of what they compute.
//
// Layouts of a 16 x 16 matrix over the lanes (g, c) = (lane >> 4, lane & 15) of a wave (v_mfma_f64_16x16x4):
//   accumulator (C-) layout, also the B operand:  register q  = element [row 4 q + g][col c]
//   A-layout:                                     slab kk     = element [row c][k = 4 kk + g]
// Large register state (v4f64, double[4]) goes in and out by reference, as in cmma16.
#pragma once
#include <hip/hip_runtime.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_complex.h"

namespace qmps {

constexpr int kTile16Ld = 17;      // padded row of a wave's transpose tile [16][17]

// accumulator layout -> A-layout through the wave-private LDS tile sT [16][17]
__device__ __forceinline__ void tile16_to_a_layout(double2* sT, const v4f64& re, const v4f64& im, double (&are)[4], double (&aim)[4]) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < 4; ++q) sT[(4 * q + g) * kTile16Ld + c] = make_double2(re[q], im[q]);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double2 t = sT[c * kTile16Ld + 4 * kk + g];
    are[kk] = t.x;
    aim[kk] = t.y;
  }
}

// ---- exchange tiles: one accumulator-layout matrix in 256 entries of LDS, register q of a lane at tile16_at(q, lane)
constexpr __device__ __forceinline__ int tile16_at(int q, int lane) { return q * 64 + lane; }
__device__ __forceinline__ void tile16_publish(double2* tile, const v4f64& re, const v4f64& im) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) tile[tile16_at(q, lane)] = make_double2(re[q], im[q]);
}
__device__ __forceinline__ void tile16_fetch(const double2* tile, v4f64& re, v4f64& im) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double2 t = tile[tile16_at(q, lane)];
    re[q] = t.x;
    im[q] = t.y;
  }
}

// AA = A_t1 A_t2 in the accumulator layout, the tensor A [2][16][ld] (HBM: ld = 16, LDS: ld = 17) read straight into the operand layouts
__device__ __forceinline__ void tile16_merge_pair(const double2* A, int ld, int t1, int t2, v4f64& zr, v4f64& zi) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  double pa[4], pai[4];
  v4f64 qa, qai;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double2 va = A[(t1 * 16 + c) * ld + 4 * kk + g], wa = A[(t2 * 16 + 4 * kk + g) * ld + c];
    pa[kk] = va.x; pai[kk] = va.y;
    qa[kk] = wa.x; qai[kk] = wa.y;
  }
  cmma16(pa, pai, qa, qai, zr, zi);
}

// C_w = sum_t WW[w][t] AA_t from the four published products (exchange tiles sX[0 .. 3]), in the accumulator layout
// (element by element on purpose: here the compiler forms fma(w.x, a.x, -(w.y a.y)) and adds it to the sum; written on whole v4f64 vectors it
// contracts the same products in another order and C_w moves in the last bit)
__device__ __forceinline__ void tile16_mix_pairs(const double2* W, int w, double2 (*sX)[256], v4f64& sr, v4f64& si) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const double2 ww = W[w * 4 + t];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double2 v = sX[t][tile16_at(q, lane)];
      sr[q] += ww.x * v.x - ww.y * v.y;
      si[q] += ww.x * v.y + ww.y * v.x;
    }
  }
}

// Set-up of a map T(x) = sum_s C_s x Bm_s^+ shared by FOUR WAVES (a team; called by all of them, two workgroup barriers inside): wave w owns
// the physical index s = w = 2 t1 + t2.  It forms AA_w = A_t1 A_t2 (published in sX[w]) and Bm_w = B_t1 B_t2 (kept), then
// C_w = sum_t WW[w][t] AA_t.  Out: C_w in the A-layout (the P operand of x' += C_w Y_w) and conj(Bm_w) in the A-layout == Bm_w^+ in the
// B-layout (the Q operand of Y_w = x Bm_w^+).  adj (the map y -> sum_s C_s^+ y Bm_s): the Q operand is Bm_w in the B-layout - the
// accumulator layout the product comes out in - and the P operand C_w^+ in the A-layout = conj of C_w in the accumulator layout: no
// transpose at all.  Ap, Bp: tensors [2][16][ld]; sT: this wave's transpose tile; sX: the team's four exchange tiles, free again on return.
__device__ __forceinline__ void tile16_split_setup(const double2* Ap, const double2* Bp, int ld, const double2* W, int w, bool adj, double2* sT,
                                                   double2 (*sX)[256], double (&cre)[4], double (&cim)[4], double (&bre)[4], double (&bimn)[4]) {
  const int t1 = w >> 1, t2 = w & 1;
  v4f64 zr = {0, 0, 0, 0}, zi = {0, 0, 0, 0};
  tile16_merge_pair(Ap, ld, t1, t2, zr, zi);
  tile16_publish(sX[w], zr, zi);
  v4f64 yr = {0, 0, 0, 0}, yi = {0, 0, 0, 0};
  tile16_merge_pair(Bp, ld, t1, t2, yr, yi);
  if (adj) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      bre[kk] = yr[kk];
      bimn[kk] = yi[kk];
    }
  } else {
    double ti[4];
    tile16_to_a_layout(sT, yr, yi, bre, ti);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) bimn[kk] = -ti[kk];
  }
  __syncthreads();
  v4f64 sr = {0, 0, 0, 0}, si = {0, 0, 0, 0};
  tile16_mix_pairs(W, w, sX, sr, si);
  if (adj) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      cre[kk] = sr[kk];
      cim[kk] = -si[kk];
    }
  } else {
    tile16_to_a_layout(sT, sr, si, cre, cim);
  }
  __syncthreads();               // the exchange tiles are free again
}

// Start vector of a power method in the accumulator layout: overlap_cold_start ...
__device__ __forceinline__ void tile16_cold_start(v4f64& xr, v4f64& xi) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double2 x0 = overlap_cold_start(4 * q + g, c, 16);      // (generic: see overlap_cold_start)
    xr[q] = x0.x;
    xi[q] = x0.y;
  }
}
// ... replaced by the matrix at `warm` ([16][16] row-major), normalised, if its norm is usable (all zero: no fixed point yet)
__device__ __forceinline__ void tile16_warm_start(const double2* warm, v4f64& xr, v4f64& xi) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  v4f64 wr, wi;
  double n2 = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double2 t = warm[(4 * q + g) * 16 + c];
    wr[q] = t.x; wi[q] = t.y;
    n2 = dfma(t.x, t.x, dfma(t.y, t.y, n2));
  }
  n2 = lane0(wave_sum(n2));
  if (n2 > 1e-200 && n2 < 1e200) {
    const double inv = 1.0 / __builtin_sqrt(n2);
    xr = wr * inv;
    xi = wi * inv;
  }
}

// Convergence test of a power step x -> n = T x (x not necessarily normalised): eta = <x, n> / <x, x>, xx = <x, x>, nn = <n, n>,
// rs = ||n - eta x||^2; returns rs / xx, the squared residual relative to ||x||^2.  rs and the return value are wave-uniform.
__device__ __forceinline__ double tile16_power_test(const v4f64& xr, const v4f64& xi, const v4f64& nr, const v4f64& ni, double& eta_r, double& eta_i,
                                                    double& xx, double& nn, double& rs) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    a0 = dfma(xr[q], nr[q], a0);
    a0 = dfma(xi[q], ni[q], a0);
    a1 = dfma(xr[q], ni[q], a1);
    a1 = dfma(-xi[q], nr[q], a1);
    a2 = dfma(nr[q], nr[q], a2);
    a2 = dfma(ni[q], ni[q], a2);
    a3 = dfma(xr[q], xr[q], a3);
    a3 = dfma(xi[q], xi[q], a3);
  }
  xx = wave_sum(a3);
  const double ixx = xx > 0.0 ? 1.0 / xx : 0.0;
  eta_r = wave_sum(a0) * ixx;
  eta_i = wave_sum(a1) * ixx;
  nn = wave_sum(a2);
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double dr = nr[q] - (eta_r * xr[q] - eta_i * xi[q]), di = ni[q] - (eta_r * xi[q] + eta_i * xr[q]);
    s = dfma(dr, dr, s);
    s = dfma(di, di, s);
  }
  rs = lane0(wave_sum(s));
  return rs * ixx;
}

}  // namespace qmps
