// qmps_complex.h - complex arithmetic on double2 and the complex 16 x 16 x 16 products on v_mfma_f64_16x16x4 (gfx950 only): the ONE
// definition of each, for every kernel translation unit.  The FMA order of each helper is part of what the kernels compute - a kernel
// that needs another order writes it out in its own body; it does not get a second helper of the same name.
#pragma once
#include <hip/hip_runtime.h>

#include "qmps_device.h"

namespace qmps {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }   // conj(a) b
__device__ __forceinline__ void cfma(double2 a, double2 b, double2& c) {   // c += a b
  c.x = dfma(a.x, b.x, c.x);
  c.x = dfma(-a.y, b.y, c.x);
  c.y = dfma(a.x, b.y, c.y);
  c.y = dfma(a.y, b.x, c.y);
}
__device__ __forceinline__ void cfms(double2 a, double2 b, double2& c) {   // c -= a b
  c.x = dfma(-a.x, b.x, c.x);
  c.x = dfma(a.y, b.y, c.x);
  c.y = dfma(-a.x, b.y, c.y);
  c.y = dfma(-a.y, b.x, c.y);
}
__device__ __forceinline__ void cfma_conj(double2 a, double2 b, double2& c) {   // c += a conj(b)
  c.x = dfma(a.x, b.x, c.x);
  c.x = dfma(a.y, b.y, c.x);
  c.y = dfma(a.y, b.x, c.y);
  c.y = dfma(-a.x, b.y, c.y);
}
__device__ __forceinline__ void cfma_cj(double2 a, double2 b, double2& c) {   // c += conj(a) b
  c.x = dfma(a.x, b.x, c.x);
  c.x = dfma(a.y, b.y, c.x);
  c.y = dfma(a.x, b.y, c.y);
  c.y = dfma(-a.y, b.x, c.y);
}

// C += P * Q, P in A-layout (pre/pim[kk] = P[row = c][k = 4 kk + g]), Q in B-layout (qre/qim[kk] = Q[k = 4 kk + g][col = c])
__device__ __forceinline__ void cmma16(const double (&pre)[4], const double (&pim)[4], const v4f64& qre, const v4f64& qim,
                                       v4f64& cre, v4f64& cim) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    cre = __builtin_amdgcn_mfma_f64_16x16x4f64(pre[kk], qre[kk], cre, 0, 0, 0);
    cim = __builtin_amdgcn_mfma_f64_16x16x4f64(pre[kk], qim[kk], cim, 0, 0, 0);
    cre = __builtin_amdgcn_mfma_f64_16x16x4f64(-pim[kk], qim[kk], cre, 0, 0, 0);
    cim = __builtin_amdgcn_mfma_f64_16x16x4f64(pim[kk], qre[kk], cim, 0, 0, 0);
  }
}

// The same product with THREE real products per k-slab instead of four (K1 = (Pr + Pi) Qr, K2 = Pr (Qi - Qr), K3 = Pi (Qr + Qi);
// Re = K1 - K3, Im = K1 + K2): 12 v_mfma_f64_16x16x4 per complex 16 x 16 x 16 product instead of 16, in three independent
// accumulator chains of four.  The matrix pipe is what bounds the power iteration (a v_mfma_f64_16x16x4 occupies it for ~100
// cycles on this part, profiles/EXPERIMENTS.md), the handful of extra additions run on the vector pipe beside it.  Rounding:
// norm-wise the same bound as the four-product form (|error| <= c eps |P| |Q|).
__device__ __forceinline__ void cmma16_3m(const double (&pre)[4], const double (&pim)[4], const v4f64& qre, const v4f64& qim,
                                          v4f64& cre, v4f64& cim) {
  v4f64 k1 = {0, 0, 0, 0}, k2 = {0, 0, 0, 0}, k3 = {0, 0, 0, 0};
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double ps = pre[kk] + pim[kk], qd = qim[kk] - qre[kk], qs = qre[kk] + qim[kk];
    k1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ps, qre[kk], k1, 0, 0, 0);
    k2 = __builtin_amdgcn_mfma_f64_16x16x4f64(pre[kk], qd, k2, 0, 0, 0);
    k3 = __builtin_amdgcn_mfma_f64_16x16x4f64(pim[kk], qs, k3, 0, 0, 0);
  }
  cre += k1 - k3;
  cim += k1 + k2;
}

}  // namespace qmps
