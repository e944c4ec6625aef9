// qmps_energy_lane.hip - kernel 1 (gfx950 only): D = 2, 4 - ONE EVALUATION PER LANE, one wave per workgroup.  The wave's 64
// tensors are read from HBM as one contiguous, fully coalesced slab (16 B per lane per load), transposed through a padded LDS
// tile; from then on every operand of every v_fma_f64 is a VGPR of the lane that needs it.  Plain power iteration (packed
// Hermitian r: 12 D^3 - 2 D^2 FMAs per step), Cholesky test, two-site-RDM energy epilogue (qmps_lane_core.h).  Also launch_energy,
// the dispatcher over D of the solve + energy launch.
//
// Kernel 3c', the whole-run D = 2 rotosolve (below), shares this translation unit: it evaluates through the same squaring_tail_d2 as
// energy_lane_kernel<2, true>.  Compiled apart from that kernel - squaring_tail_d2 is then only ever called with done = 0 - the
// rotosolve kernels come out with other scalar code around the call than the code that was tuned and measured.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmps_kernels.h"
#include "qmps_device.h"
#include "qmps_lane_core.h"
#include "qmps_power_d4_core.h"
#include "qmps_circuit.h"       // Reg, ansatz_circuit_cs, ansatz_param_scale, roto_shift_value
#include "qmps_roto_math.h"     // wrap_pi, double_sinusoid_step

namespace qmps {

// ROWMATH (D = 4, SOLVE, no squaring tail behind it): the plain power iteration with the arithmetic of env_power_d4_kernel
template <int D, bool SOLVE, bool ROWMATH = false>
__global__ __launch_bounds__(64) void energy_lane_kernel(LaneArgs p) {
  static_assert(!ROWMATH || (D == 4 && SOLVE), "ROWMATH: the D = 4 solve only");
  using Cfg = LaneCfg<D>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int lane = threadIdx.x;
  const int64_t wave_first = (int64_t)blockIdx.x * 64;
  int64_t b = wave_first + lane;
  bool valid = b < p.B;
  if (p.acc_zero != nullptr && blockIdx.x == 0) acc_clear(p.acc_zero, p.n_terms, lane, 64);   // accumulator of a later step
  double are[2][D][D], aim[2][D][D];

  if (p.idx_list != nullptr) {
    // ---- list mode: evaluation ids come from a device-side worklist (gathered loads, few items)
    const int64_t n_list = *p.idx_count;
    if (wave_first >= n_list) return;
    valid = wave_first + lane < n_list;
    b = valid ? (int64_t)p.idx_list[wave_first + lane] : (int64_t)p.idx_list[wave_first];
    const double2* a = (const double2*)p.A + b * (2 * D * D);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const double2 v = a[(s * D + i) * D + j];
          are[s][i][j] = v.x;
          aim[s][i][j] = v.y;
        }
  } else {
    // ---- HBM -> LDS: the wave's 64 tensors are one contiguous slab; 16 B per lane per load
    {
      const unsigned char* slab = (const unsigned char*)p.A + wave_first * Cfg::kRowBytes;
      const int64_t slab_bytes = (p.B - wave_first < 64 ? p.B - wave_first : 64) * (int64_t)Cfg::kRowBytes;
#pragma unroll
      for (int c = 0; c < Cfg::kChunks; ++c) {
        const int off = c * 1024 + lane * 16;
        double2 v = make_double2(0.0, 0.0);
        if (off < slab_bytes) v = *(const double2*)(slab + off);
        const int e = off / Cfg::kRowBytes, w = off % Cfg::kRowBytes;
        *(double2*)(lds + e * Cfg::kRowPad + w) = v;
      }
    }
    __syncthreads();
    // ---- LDS -> VGPR: each lane takes its own tensor
    const unsigned char* row = lds + lane * Cfg::kRowPad;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
          const double2 v = *(const double2*)(row + ((s * D + i) * D + j) * 16);
          are[s][i][j] = v.x;
          aim[s][i][j] = v.y;
        }
  }

  // ---- environment: r0 = 1/D or the caller's guess (packed Hermitian, trace-normalised)
  double rre[D][D], rim[D][D];
  if (p.r_in != nullptr && valid) {
    const double2* g = (const double2*)p.r_in + b * (D * D);
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) {
        const double2 u = g[i * D + j], l = g[j * D + i];
        rre[i][j] = 0.5 * (u.x + l.x);
        rim[i][j] = (i == j) ? 0.0 : 0.5 * (u.y - l.y);
        if (i == j) tr += rre[i][j];
      }
    // (a resident 'environment' nobody wrote - a window that never stored one, zeros, NaN - is no guess: the default start.  A warm launch on such a
    // window used to end with status != 0 for every evaluation: profiles/experiments/r05/stress_api_state.py, round 5)
    const bool usable = tr > 1e-300 && tr < 1e300;
    const double inv = usable ? 1.0 / tr : 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) {
        rre[i][j] = usable ? rre[i][j] * inv : ((i == j) ? 1.0 / D : 0.0);
        rim[i][j] = usable ? rim[i][j] * inv : 0.0;
      }
  } else {
    // default start: 1/D; squaring from the start (handoff == 0) uses |0><0| like the D = 4 matrix kernel
    const bool e0 = SOLVE && p.hybrid != 0 && p.handoff == 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) {
        rre[i][j] = (i == j) ? (e0 ? (i == 0 ? 1.0 : 0.0) : 1.0 / D) : 0.0;
        rim[i][j] = 0.0;
      }
  }

  int iters = 0, status = QMPS_ST_OK;
  bool handed_off = false;
  if (SOLVE) {
    status = QMPS_ST_NOT_CONVERGED;
    bool active = valid;
    const double tol2 = p.tol * p.tol;
    const bool hybrid = p.hybrid != 0 && p.handoff < p.max_iter;
    int plain = hybrid ? p.handoff : p.max_iter;
    if constexpr (ROWMATH) {
      // QMPS_ENV_POWER at D = 4 (QMPS_POWER_LANE, or a context without the work counter of env_power_d4_kernel): the iteration in the
      // real coordinates and with the operations of that kernel (qmps_power_d4_core.h) - the same iterates, iteration counts and
      // statuses bit for bit, which two differently rounded iterations cannot give where the residual creeps towards tol
      double u[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) u[c] = (c >> 2) == (c & 3) ? 0.25 : 0.0;
      if (p.r_in != nullptr && valid) {
        const double2* rin = (const double2*)p.r_in + b * 16;
        double ug[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) ug[c] = power_d4_guess_coord(rin, c >> 2, c & 3);
        const double t = (ug[0] + ug[10]) + (ug[5] + ug[15]);       // row16_sum of the diagonal coordinates
        const bool usable = t > 1e-300 && t < 1e300;
        const double inv = 1.0 / t;
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (usable) u[c] = ug[c] * inv;
      }
      bool converged = false;
      if (active)
        power_d4_lane_solve([&](int s, int a, int j) { return make_double2(are[s][a][j], aim[s][a][j]); }, u, p.max_iter, tol2, iters, converged);
      if (converged) status = QMPS_ST_OK;
      active = false;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) {
          rre[i][j] = u[4 * i + j];
          rim[i][j] = i == j ? 0.0 : u[4 * j + i];
        }
      plain = 0;
    }
    // two steps per trip, ping-pong r -> n -> r: frozen (converged) lanes are simply masked off
    for (int k = 1; k <= plain; k += 2) {
      if (!__any(active)) break;
      double nre[D][D], nim[D][D];
      if (active) {
        power_step<D>(are, aim, rre, rim, nre, nim);
        const double d2 = normalise_and_diff<D>(nre, nim, rre, rim);
        iters = k;
        if (d2 < tol2 || k == plain) {
          if (d2 < tol2) status = QMPS_ST_OK;
          active = false;
#pragma unroll
          for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = i; j < D; ++j) {
              rre[i][j] = nre[i][j];
              rim[i][j] = nim[i][j];
            }
        }
      }
      if (active) {
        power_step<D>(are, aim, nre, nim, rre, rim);
        const double d2 = normalise_and_diff<D>(rre, rim, nre, nim);
        iters = k + 1;
        if (d2 < tol2) {
          status = QMPS_ST_OK;
          active = false;
        }
      }
    }
    if (hybrid) {
      active = valid && status == QMPS_ST_NOT_CONVERGED;
      if (D == 2) {
        if constexpr (D == 2) squaring_tail_d2(are, aim, rre, rim, active, iters, status, plain, p.max_iter, tol2, p.skip, p.direct != 0);
      } else if (p.work_idx != nullptr) {
        // hand the slow items to the wave-per-item squaring kernel: wave-aggregated append
        const unsigned long long mask = __ballot(active);
        if (mask != 0ull) {
          int base = 0;
          if (lane == 0) base = atomicAdd(p.work_count, __popcll(mask));
          base = __shfl(base, 0, 64);
          if (active) {
            p.work_idx[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)b;
            handed_off = true;
          }
        }
      }
    }
    if (status == QMPS_ST_OK && !is_positive_definite<D>(rre, rim)) status = QMPS_ST_NOT_PD;
  } else if (p.check_pd) {
    if (valid) {
      status = p.status[b];
      if (status == QMPS_ST_OK && !is_positive_definite<D>(rre, rim)) status = QMPS_ST_NOT_PD;
    }
  }

  // ---- energy epilogue: rho (upper triangle) -> E_t = Re sum h_t[s][t] rho[t][s] / tr r
  double pre[4][4], pim[4][4];
  two_site_rdm<D>(are, aim, are, aim, rre, rim, pre, pim);
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) tr += rre[i][i];
  const double inv = 1.0 / tr;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int s = t; s < 4; ++s) {
      pre[t][s] *= inv;
      pim[t][s] = (t == s) ? 0.0 : pim[t][s] * inv;
    }
  for (int q = 0; q < p.n_terms; ++q) {
    const double2* h = (const double2*)p.h + q * 16;  // wave-uniform -> scalar loads
    const double e = rdm_energy(h, pre, pim);
    if (valid) p.E[b * p.n_terms + q] = e;
    if (p.partial != nullptr || p.acc != nullptr) {
      // fused first pass of the cost reduction: one partial per wave (deterministic order) - or the whole reduction
      // (exact fixed-point accumulator, qmps_kernels.h)
      const double s = wave_sum(valid ? e : 0.0);
      if (lane == 0) {
        if (p.partial != nullptr) p.partial[(int64_t)q * gridDim.x + blockIdx.x] = s;
        if (p.acc != nullptr) acc_arrive(p.acc, p.acc_shards, q, blockIdx.x, s, p.acc_bound, p.acc_scale);
      }
    }
  }
  if (!valid) return;
  if (SOLVE) {
    p.iters[b] = iters;
    p.status[b] = status;
  } else if (p.check_pd) {
    p.status[b] = status;
  }
  (void)handed_off;
  if (p.r_out != nullptr && SOLVE) {
    double2* o = (double2*)p.r_out + b * (D * D);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double re = h_re<D>(rre, i, j);
        const double im = (i == j) ? 0.0 : h_im<D>(rim, i, j);
        o[i * D + j] = make_double2(re, im);
      }
  }
  if (p.rho_out != nullptr) {
    double2* o = (double2*)p.rho_out + b * 16;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double re = (t <= s) ? pre[t][s] : pre[s][t];
        const double im = (t == s) ? 0.0 : ((t < s) ? pim[t][s] : -pim[s][t]);
        o[t * 4 + s] = make_double2(re, im);
      }
  }
}

template <int D>
static hipError_t launch_lane(const LaneArgs& a, bool solve, hipStream_t st) {
  const int grid = (int)((a.B + 63) / 64);
  const size_t lds = LaneCfg<D>::kLdsBytes;
  const bool tail = a.hybrid != 0 && a.handoff < a.max_iter;       // (the kernel's own `hybrid`)
  if (solve && D == 4 && !tail)
    hipLaunchKernelGGL((energy_lane_kernel<D, true, D == 4>), dim3(grid), dim3(64), lds, st, a);
  else if (solve)
    hipLaunchKernelGGL((energy_lane_kernel<D, true>), dim3(grid), dim3(64), lds, st, a);
  else
    hipLaunchKernelGGL((energy_lane_kernel<D, false>), dim3(grid), dim3(64), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_energy(int D, const LaneArgs& a, bool solve, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  switch (D) {
    case 2: return launch_lane<2>(a, solve, st);
    case 4: return launch_lane<4>(a, solve, st);
    case 8:
    case 16: return launch_energy_block(D, a, solve, st);
    default: return hipErrorInvalidValue;
  }
}

// ------------------------------------------------------------------------------------------
// Kernel 3c': the WHOLE rotosolve run of a D = 2 ansatz in one launch.  Restarts are independent, so the sequential loop
// over parameters and sweeps needs no grid-wide step: a quad of lanes owns one restart (lanes 0..2 = the shifts
// {0, +pi/2, -pi/2}, lane 3 idles along), builds its shifted state tensor in registers, solves the environment and the
// energy exactly as energy_lane_kernel<2, true> does with the squaring solver from the start (same device functions, same
// order: bit-identical energies), exchanges the three energies by DPP and applies the closed-form update to the restart's
// parameter vector in LDS.  One launch replaces (4 kernels + graph replay) x n_params x n_sweeps.
// ------------------------------------------------------------------------------------------
// NSH = 3: shifts {0, +pi/2, -pi/2}, closed-form update (qmps/rotosolve.py:154-181);  NSH = 6: the double-frequency rotosolve
// of Optimizer.optimize('Rotosolve') (qmps/tools.py:422-457) - lanes 0..2 evaluate shifts k and k + 3 of {0, pi, +-pi/2, +-pi/4},
// lane 0 fits a sin 2x + b cos 2x + c sin x + d cos x and moves the parameter to its global minimiser (not re-wrapped).
template <int KIND, int NSH>
__global__ __launch_bounds__(64) void rotosolve_fused_d2_kernel(RotoArgs p) {
  constexpr int D = 2;
  // lanes per restart: a quad for the three shifts of the single-frequency rule; EIGHT for the six shifts of the double-frequency one (round 6: the six
  // evaluations side by side - three lanes used to take two each, one after the other)
  constexpr int LPR = NSH == 6 ? 8 : 4, RPW = 64 / LPR;
  extern __shared__ double sP[];                 // [RPW restarts][P], then their cos / sin
  const int lane = threadIdx.x, rl = lane / LPR, k = lane % LPR;
  const int r = blockIdx.x * RPW + rl;
  const bool valid = r < p.R;
  const int rr = valid ? r : p.R - 1;
  const int P = p.P;
  double* mine = sP + rl * P;
  // cos / sin of the restart's (scaled) angles, kept beside them (round 6): an evaluation used to compute the sincos of EVERY angle inside the circuit,
  // once per column - 60 double-precision sincos per parameter update and lane with ShallowFull's 15 angles, ~18 of the update's 31 us; now ONE per
  // evaluation (the shifted angle) and one per update (the moved angle).  Same arguments, same function: the same bits.
  double2* mine_cs = (double2*)(sP + RPW * P) + rl * P;
  for (int l = k; l < P; l += LPR) {
    const double v = p.base[(int64_t)rr * P + l];
    mine[l] = v;
    double sn, cs_;
    sincos(ansatz_param_scale<KIND>(l) * v, &sn, &cs_);
    mine_cs[l] = make_double2(cs_, sn);
  }
  __builtin_amdgcn_wave_barrier();
  const double tol2 = p.tol * p.tol;
  const double shift = roto_shift_value(NSH, k >= NSH ? 0 : k);         // the group's spare lanes idle along with shift 0

  // one evaluation at (params + delta e_i): summed energy over the Hamiltonian terms, status
  auto evaluate = [&](int i, double delta, double& e_out, int& status_out) {
    double are[2][D][D], aim[2][D][D];
    double2 own = make_double2(1.0, 0.0);
    if (i >= 0) {
      double sn, cs_;
      sincos(ansatz_param_scale<KIND>(i) * (mine[i] + delta), &sn, &cs_);
      own = make_double2(cs_, sn);
    }
#pragma unroll
    for (int col = 0; col < D; ++col) {
      Reg<2> q;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        q.re[x] = (x == col) ? 1.0 : 0.0;
        q.im[x] = 0.0;
      }
      ansatz_circuit_cs<2, KIND>(q, [&](int l) {
        double2 v = mine_cs[l];               // (value selects: a select between `own` and an LDS element would put `own` in scratch)
        if (l == i) { v.x = own.x; v.y = own.y; }
        return v;
      }, P);
#pragma unroll
      for (int x = 0; x < 4; ++x) {           // A[s][i][j] = amplitude[2 i + s] of input |j>
        are[x & 1][x >> 1][col] = q.re[x];
        aim[x & 1][x >> 1][col] = q.im[x];
      }
    }
    double rre[D][D], rim[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = a; b < D; ++b) {
        rre[a][b] = (a == b && a == 0) ? 1.0 : 0.0;     // r_0 = |0><0|
        rim[a][b] = 0.0;
      }
    int iters = 0, status = QMPS_ST_NOT_CONVERGED;
    bool active = true;
    squaring_tail_d2(are, aim, rre, rim, active, iters, status, 0, p.max_iter, tol2, p.skip, p.direct != 0);
    if (status == QMPS_ST_OK && !is_positive_definite<D>(rre, rim)) status = QMPS_ST_NOT_PD;
    double pre[4][4], pim[4][4];
    two_site_rdm<D>(are, aim, are, aim, rre, rim, pre, pim);
    const double inv = 1.0 / (rre[0][0] + rre[1][1]);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int sg = t; sg < 4; ++sg) {
        pre[t][sg] *= inv;
        pim[t][sg] = (t == sg) ? 0.0 : pim[t][sg] * inv;
      }
    double e = 0.0;
    for (int q = 0; q < p.n_terms; ++q) e += rdm_energy((const double2*)p.h + q * 16, pre, pim);
    e_out = e;
    status_out = status;
  };
  auto quad_bcast = [&](double v, int src) {      // value of lane `src` of the restart's group, in every lane of the group
    if constexpr (LPR == 4) {
      int lo = __double2loint(v), hi = __double2hiint(v);
      switch (src) {
        case 0: lo = __builtin_amdgcn_mov_dpp(lo, 0x00, 0xf, 0xf, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x00, 0xf, 0xf, true); break;
        case 1: lo = __builtin_amdgcn_mov_dpp(lo, 0x55, 0xf, 0xf, true); hi = __builtin_amdgcn_mov_dpp(hi, 0x55, 0xf, 0xf, true); break;
        default: lo = __builtin_amdgcn_mov_dpp(lo, 0xAA, 0xf, 0xf, true); hi = __builtin_amdgcn_mov_dpp(hi, 0xAA, 0xf, 0xf, true); break;
      }
      return __hiloint2double(hi, lo);
    } else {
      return __shfl(v, (lane & ~(LPR - 1)) + src, 64);
    }
  };
  for (int sw = 0; sw < p.n_sweeps; ++sw) {
    for (int i = 0; i < P; ++i) {
      double e;
      int st;
      evaluate(i, shift, e, st);
      const double e0 = quad_bcast(e, 0), ep = quad_bcast(e, 1), em = quad_bcast(e, 2);
      // the unshifted evaluation of a sweep's first parameter IS the energy at the parameters the previous sweep left
      if (i == 0 && sw > 0 && valid && k == 0) p.hist[(int64_t)(sw - 1) * p.R + r] = e0;
      double okv = (st == QMPS_ST_OK || k >= NSH) ? 1.0 : 0.0;
      double e3 = 0.0, e4 = 0.0, e5 = 0.0;
      bool ok;
      if constexpr (NSH == 6) {
        e3 = quad_bcast(e, 3);
        e4 = quad_bcast(e, 4);
        e5 = quad_bcast(e, 5);
        ok = quad_bcast(okv, 0) * quad_bcast(okv, 1) * quad_bcast(okv, 2) * quad_bcast(okv, 3) * quad_bcast(okv, 4) * quad_bcast(okv, 5) != 0.0;
      } else {
        ok = quad_bcast(okv, 0) * quad_bcast(okv, 1) * quad_bcast(okv, 2) != 0.0;
      }
      __builtin_amdgcn_wave_barrier();
      if (ok && k == 0) {      // (an evaluation without a valid environment leaves this restart's parameter untouched)
        if constexpr (NSH == 3) {
          const double theta = -1.5707963267948966 - atan2(2.0 * e0 - ep - em, ep - em);
          mine[i] = wrap_pi(mine[i] + wrap_pi(theta));
        } else {
          // samples at {0, pi, +pi/2, -pi/2, +pi/4, -pi/4} = e0, ep, em, e3, e4, e5 (roto_update_kernel's fit, tools.py:434-447)
          const double Av = e0 + ep, Bv = e0 - ep, Cv = em + e3, Dv = em - e3, Ev = e4 - e5;
          const double a = 0.25 * (2.0 * Ev - 1.4142135623730951 * Dv), b = 0.25 * (Av - Cv), c = 0.5 * Dv, d = 0.5 * Bv;
          mine[i] += double_sinusoid_step(a, b, c, d, p.rule);
        }
        double sn, cs_;
        sincos(ansatz_param_scale<KIND>(i) * mine[i], &sn, &cs_);
        mine_cs[i] = make_double2(cs_, sn);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  {
    double e;
    int st;
    evaluate(-1, 0.0, e, st);                     // energy at the swept parameters (the reference records eps(params)): last sweep
    if (valid && k == 0) p.hist[(int64_t)(p.n_sweeps - 1) * p.R + r] = e;
  }
  __builtin_amdgcn_wave_barrier();
  if (valid)
    for (int l = k; l < P; l += LPR) p.base[(int64_t)r * P + l] = mine[l];
}

hipError_t launch_rotosolve_fused_d2(int kind, const RotoArgs& a, hipStream_t st) {
  const int rpw = a.nsh == 6 ? 8 : 16;                                                  // restarts per wave: eight lanes each (six shifts) | a quad each
  const dim3 grid((unsigned)((a.R + rpw - 1) / rpw)), block(64);
  const size_t lds = (size_t)rpw * a.P * (sizeof(double) + sizeof(double2));      // the restarts' angles and their cos / sin
  if (a.nsh == 6)
    switch (kind) {
      case 0: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<0, 6>), grid, block, lds, st, a); break;
      case 1: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<1, 6>), grid, block, lds, st, a); break;
      case 2: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<2, 6>), grid, block, lds, st, a); break;
      case 3: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<3, 6>), grid, block, lds, st, a); break;
      default: return hipErrorInvalidValue;
    }
  else
    switch (kind) {
      case 0: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<0, 3>), grid, block, lds, st, a); break;
      case 1: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<1, 3>), grid, block, lds, st, a); break;
      case 2: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<2, 3>), grid, block, lds, st, a); break;
      case 3: hipLaunchKernelGGL((rotosolve_fused_d2_kernel<3, 3>), grid, block, lds, st, a); break;
      default: return hipErrorInvalidValue;
    }
  return hipGetLastError();
}

}  // namespace qmps
