// qmps_observable.h - device helpers shared by the kernels of the observables of the resident states (qmps_correlator.hip,
// qmps_corrsum_small.hip, qmps_corrsum_block.hip); the operator limit kMaxObservableOps and the operator sizes they share with the
// host are in qmps_kernels.h
#pragma once
#include "qmps_complex.h"

namespace qmps {

// 1 / t, NaN when t is zero or not finite (the documented answer of an evaluation without a usable environment: tr r is such a t)
__device__ __forceinline__ double2 crecip(const double2 t) {
  const double s = fmax(fabs(t.x), fabs(t.y));
  if (!(s > 0.0) || !(s < INFINITY)) return make_double2(NAN, NAN);
  const double u = t.x / s, v = t.y / s, n = (u * u + v * v) * s;
  return make_double2(u / n, -v / n);
}

}  // namespace qmps
