// qmps_env_square_d4.hip - kernel 1c (gfx950 only): D = 4 repeated squaring, ONE WAVE PER ITEM, v_mfma_f64_16x16x4_f64.
// In real Hermitian coordinates the transfer map of a D = 4 tensor is exactly one real 16 x 16 MFMA
// tile R.  R_m = R^(2^m) by squaring: 4 MFMAs per round.  The accumulator layout
// (row = 4 reg + lane/16, col = lane%16) IS the B-operand layout of the next product; the A-operand
// layout (row = lane%16, k = 4 kk + lane/16) comes from a padded LDS image.
// After `skip` squarings the power method continues with R_m itself: z <- R_m z / tr (one mat-vec = 2^m
// power steps, VALU), stop at ||z' - z||^2 < tol^2; every `period` unconverged mat-vecs R_m is squared
// once more.  iterations = power steps applied to the start matrix (done + 2^skip + 2^m + ...).
// Items: the worklist written by the lane kernel, or (work_idx == nullptr) all of 0 .. B-1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"

namespace qmps {

// Coordinates (kernel-local): a = 4 i + i' packs a Hermitian 4 x 4 matrix r into a real one -
//   x[(i,i)] = r_ii,   x[(i,i')] = sqrt2 Re r_ii' (i < i'),   x[(i,i')] = sqrt2 Im r_i'i (i > i')
// (orthonormal, so ||x - x'||_2 = ||r - r'||_F).  Lane (g, c) owns rows a = (reg, g), reg = 0..3, and column
// b = (c / 4, c % 4): row index `reg` is static, so the tensor reads below need four LDS addresses.
#ifndef QMPS_SQ_MINBLOCKS
#define QMPS_SQ_MINBLOCKS 5
#endif
__global__ __launch_bounds__(256, QMPS_SQ_MINBLOCKS) void env_square_d4_kernel(SquareArgs p) {
  constexpr int D = 4, N = 16, LD = 17;
  constexpr int WAVES = 4;
  constexpr double RS2 = 0.70710678118654752, S2 = 1.4142135623730951;
  __shared__ double2 sA_all[WAVES][2][2 * N];   // two tiles per wave: the next item's tensor lands while this one is solved
  __shared__ double sR_all[WAVES][N * LD + N];
  // the wave index is wave-uniform: keep it (and every item id / address derived from it) in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int j = c >> 2, jp = c & 3;
  double* sR = sR_all[wave];
  double* sZ = sR + N * LD;          // 16-double strip behind the padded image
  const int64_t n_items = p.work_idx != nullptr ? (int64_t)*p.work_count : p.B;
  const double tol2 = p.tol * p.tol;
  // lane constants of the matrix build (see below)
  // P = (cpx a.x + cpy a.y,  cpy a.x - cpx a.y),  Q likewise with e:  diagonal column (1, 0 | 0, 0),
  // real-part column (1, 0 | 1, 0)/sqrt2,  imaginary-part column (0, -1 | 0, 1)/sqrt2
  const double cpx = j == jp ? 1.0 : (j < jp ? RS2 : 0.0), cpy = j > jp ? -RS2 : 0.0;
  const double cqx = j < jp ? RS2 : 0.0, cqy = j > jp ? RS2 : 0.0;
  double row_scale[4];
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) row_scale[reg] = reg == g ? 1.0 : (reg < g ? S2 : -S2);
  // every wave walks its own items (wave-private LDS regions, no workgroup barriers); the next item's tensor is
  // fetched straight into the other LDS tile (global_load_lds_dwordx4: 32 lanes x 16 B = the 512-byte tile, lane-linear,
  // no VGPRs, no ds_write) while the current one is being solved
  const int64_t stride = (int64_t)gridDim.x * WAVES;
  int64_t w = (int64_t)blockIdx.x * WAVES + wave;
  auto item_id = [&](int64_t ww) { return p.work_idx != nullptr ? (int64_t)p.work_idx[ww] : ww; };
  auto fetch = [&](int64_t ww, int buf) {
    if (lane < 2 * N)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const double2*)p.A + item_id(ww) * (2 * N) + lane),
                                       (__attribute__((address_space(3))) void*)&sA_all[wave][buf][0], 16, 0, 0);
  };
  int buf = 0;
  if (w < n_items) fetch(w, 0);
  for (; w < n_items; w += stride, buf ^= 1) {
    const int64_t b = item_id(w);
    const double2* sA = sA_all[wave][buf];
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): this item's tile has landed
    __builtin_amdgcn_wave_barrier();
    if (w + stride < n_items) fetch(w + stride, buf ^ 1);
    // R[a][b] = tr(H_a T(H_b)), T(X) = sum_s A_s X A_s^+, in accumulator layout: lane holds R[(reg, g)][(j, j')].
    // G = T(H_b) is Hermitian; its entry [reg][g] folds the column combination into per-lane operands:
    //   G[reg][g] = sum_s ( A_s[reg][j] P_s + A_s[reg][j'] Q_s ),  P_s = alpha conj(A_s[g][j']),  Q_s = beta conj(A_s[g][j])
    //   j == j': (alpha, beta) = (1, 0);   j < j': (1, 1)/sqrt2;   j > j': (-i, i)/sqrt2
    //   R = Re G (reg == g),  sqrt2 Re G (reg < g),  -sqrt2 Im G (reg > g: the sorted pair is (g, reg), G[g][reg] = conj)
    v4f64 R;
    {
      double pr[2], pi[2], qr[2], qi[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const double2 a = sA[(s2 * D + g) * D + jp], e = sA[(s2 * D + g) * D + j];
        // conj(a) * alpha: (a.x, -a.y) * col_a  or  (-a.y, -a.x)/sqrt2;   conj(e) * beta: (e.x, -e.y) * col_b  or  (e.y, e.x)/sqrt2
        // as lane-constant linear combinations (mul + fma each, no selects)
        pr[s2] = dfma(cpx, a.x, cpy * a.y);
        pi[s2] = dfma(cpy, a.x, -cpx * a.y);
        qr[s2] = dfma(cqx, e.x, cqy * e.y);
        qi[s2] = dfma(cqy, e.x, -cqx * e.y);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        double gr = 0.0, gi = 0.0;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const double2 x = sA[(s2 * D + reg) * D + j], u = sA[(s2 * D + reg) * D + jp];
          gr = dfma(x.x, pr[s2], gr);
          gr = dfma(-x.y, pi[s2], gr);
          gr = dfma(u.x, qr[s2], gr);
          gr = dfma(-u.y, qi[s2], gr);
          gi = dfma(x.x, pi[s2], gi);
          gi = dfma(x.y, pr[s2], gi);
          gi = dfma(u.x, qi[s2], gi);
          gi = dfma(u.y, qr[s2], gi);
        }
        R[reg] = (reg > g ? gi : gr) * row_scale[reg];
      }
    }
    // Vectors are kept ROW-DISTRIBUTED: lane (g, c) holds v[(reg, g)], reg = 0..3, alike for every c.
    // The A-operand fragments of R_m (af[kk] = R_m[c][4 kk + g], read back from the padded LDS image)
    // serve both the next squaring and the mat-vec y = R_m z:  per lane sum_kk af[kk] z[4 kk + g], summed
    // over the four row groups g -> y[c] in every group; a 128-byte LDS strip turns that back into the
    // row distribution (strip slot of coordinate a = 4 reg + g is 4 g + reg: one lane reads 4 neighbours)
    // and hands every lane the four diagonal coordinates (the trace) without a cross-lane reduction.
    const int spos = 4 * (c & 3) + (c >> 2);
    double af[4];
    auto fragments_of = [&](const v4f64& M, double (&f)[4]) {   // wave-private LDS region; LDS is in-order per wave
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sR[(4 * reg + g) * LD + c] = M[reg];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) f[kk] = sR[c * LD + 4 * kk + g];
    };
    auto square_of = [&](const v4f64& M, const double (&f)[4]) {
      // M M: 4 x v_mfma_f64_16x16x4_f64 (k-slabs), single accumulator chain.
      // (Measured alternative: 16 x v_mfma_f64_4x4x4_4b_f64 - 16 cycles each vs ~100 for the 16x16x4
      // form on gfx950, profiles/experiments/scratch/mfma_probe.hip - needs 16 LDS fragment reads and 40 more VGPRs
      // per round and came out 7 % slower end to end; its lane layout is in profiles/experiments/scratch/mfma4_layout.hip.)
      v4f64 acc = {0, 0, 0, 0};
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f[0], M[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f[1], M[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f[2], M[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(f[3], M[3], acc, 0, 0, 0);
      return acc;
    };
    auto fragments = [&]() { fragments_of(R, af); };
    auto square = [&]() { return square_of(R, af); };
    auto fast_inv = [](double t) {   // v_rcp_f64 + one Newton step: relative error ~1e-16 (a scale factor only)
      const double x = __builtin_amdgcn_rcp(t);
      return dfma(dfma(-t, x, 1.0), x, x);
    };
    auto strip_trace = [&]() { return (sZ[0] + sZ[5]) + (sZ[10] + sZ[15]); };   // slots of (0,0) (1,1) (2,2) (3,3)
    // step counts stay below 2^31 and strides below 2^30: 32-bit scalar arithmetic (no 64-bit VALU compares)
    const unsigned cap = (unsigned)p.max_iter;
    int m = 0, iters = p.done, status = QMPS_ST_NOT_CONVERGED;
    // phase 1: `skip` squarings, matrix pipe only (no item converges in < 2^skip steps)
    fragments();
    // the number of untracked squarings is known up front: two rounds per trip on two register sets (the accumulator of
    // one round is the B operand of the next, no copies), one odd round at the end
    int m1 = 0;
    while (m1 < p.skip && m1 < 29 && (unsigned)p.done + (2u << m1) <= cap) ++m1;
    for (int pair = 0; pair < (m1 >> 1); ++pair) {
      const v4f64 R2 = square_of(R, af);
      double af2[4];
      fragments_of(R2, af2);
      R = square_of(R2, af2);
      fragments_of(R, af);
    }
    if (m1 & 1) {
      const v4f64 R2 = square_of(R, af);
      R = R2;
      fragments_of(R, af);
    }
    m = m1;
    // start vector z (trace 1): a warm start / the lane kernel's iterate, else r_0 = |0><0| = e_0, for which
    // T^(2^m) e_0 is simply column 0 of R_m (held by the lanes c == 0)
    double xc[4];
    if (p.r_in != nullptr) {
      double tsel = 0.0;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const double2 u = ((const double2*)p.r_in)[b * N + reg * D + g];   // r[reg][g]
        const double2 l = ((const double2*)p.r_in)[b * N + g * D + reg];   // r[g][reg]
        xc[reg] = reg == g ? u.x : (reg < g ? RS2 * (u.x + l.x) : RS2 * (l.y - u.y));
        tsel = reg == g ? u.x : tsel;
      }
      const double tr0 = group4_sum_mfma(tsel);
      const bool usable = tr0 > 1e-300 && tr0 < 1e300;      // (zeros / NaN where nobody stored an environment: the default start e_0)
      const double inv0 = usable ? fast_inv(tr0) : 0.0;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) xc[reg] = usable ? xc[reg] * inv0 : ((4 * reg + g == 0) ? 1.0 : 0.0);
    } else if (m == 0) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) xc[reg] = (4 * reg + g == 0) ? 1.0 : 0.0;
    } else {
      __builtin_amdgcn_wave_barrier();
      if (c == 0) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sZ[4 * g + reg] = R[reg];
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) xc[reg] = sZ[4 * g + reg];
      const double inv0 = fast_inv(strip_trace());
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) xc[reg] *= inv0;
      iters = p.done + (1 << m);
    }
    // phase 2: power iteration with R_m = T^(2^m) (one mat-vec = 2^m steps; VALU + LDS strip), compared
    // iterate to iterate; after every `period` unconverged mat-vecs the matrix is squared once more.
    int count = 0;
    while ((unsigned)iters + (1u << m) <= cap) {
      double part = af[0] * xc[0];
      part = dfma(af[1], xc[1], part);
      part = dfma(af[2], xc[2], part);
      part = dfma(af[3], xc[3], part);
      const double yc = group4_sum_mfma(part);          // y[c], alike in every row group
      __builtin_amdgcn_wave_barrier();
      if (g == 0) sZ[spos] = yc;
      __builtin_amdgcn_wave_barrier();
      double y[4];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) y[reg] = sZ[4 * g + reg];
      const double inv = fast_inv(strip_trace());
      iters += 1 << m;
      double dpart = 0.0;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        y[reg] *= inv;
        const double d = y[reg] - xc[reg];
        dpart = dfma(d, d, dpart);
        xc[reg] = y[reg];
      }
      const double d2 = lane0(group4_sum_mfma(dpart));  // wave-uniform: one item per wave
      if (d2 < tol2) {
        status = QMPS_ST_OK;
        break;
      }
      if (++count == p.period && m < 29 && (unsigned)iters + (2u << m) <= cap) {
        // 1/tr(R_m z) ~ 1/lambda(R_m): keeps R_{m+1} at O(1) for non-isometric tensors too
        const v4f64 Rn = square();
        R = Rn * (inv * inv);
        ++m;
        fragments();
        count = 0;
      }
    }
    // unpack x (lane (g, c = 0) holds coordinates (reg, g)) to the complex r[i][i'] and store
    __builtin_amdgcn_wave_barrier();
    if (c == 0) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) sZ[4 * reg + g] = xc[reg];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < N) {
      const int i = lane >> 2, ip = lane & 3;
      const int lo = i < ip ? i : ip, hi = i < ip ? ip : i;
      double re = sZ[4 * lo + hi], im = sZ[4 * hi + lo];
      if (i == ip) im = 0.0;
      else {
        re *= RS2;
        im *= i < ip ? RS2 : -RS2;
      }
      ((double2*)p.r_out)[b * N + lane] = make_double2(re, im);
    }
    if (lane == 0) {
      p.iters[b] = iters;
      p.status[b] = status;
    }
  }
}

hipError_t launch_square_tail(int D, const SquareArgs& a, int grid, hipStream_t st) {
  if (D != 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(env_square_d4_kernel, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace qmps
