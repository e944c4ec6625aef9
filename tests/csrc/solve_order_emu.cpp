// solve_order_emu.cpp - TEST INFRASTRUCTURE ONLY.  The 16 x 16 solve of the D = 4 kernel (DirectD4::solve_gathered / normalise_gathered and
// the route solve -> normalise -> gather of the older emulations: qmps_amd/csrc/qmps_direct_core.h) on the CPU, in the lock-step host policy
// of direct_emu.cpp, beside a test-only copy of the Gauss-Jordan elimination in the natural pivot order that the kernel ran before its
// pivots went round the quad.  Nothing in the product loads this file.
//
// Build: g++ <CXXFLAGS of tests/csrc/Makefile> -shared tests/csrc/solve_order_emu.cpp -o tests/csrc/libsolve_order_emu.so
#include "direct_emu.cpp"

namespace {

using OrderCore = qmps::DirectD4<HostOps>;

// The reference: full Gauss-Jordan elimination, pivot k = row k (lane k / 4, register k % 4), every lane updates all four of its rows at
// every step.  x: the lane's own coordinates, not normalised.
void gauss_jordan_natural(const HostOps& o, Q4 (&M)[4][16], Q4 (&x)[4], Q4& pivmax) {
  using O = HostOps;
  Q4 y[4], dinv[4], w[4];
  const Q4 one = O::splat(1.0), zero = O::splat(0.0);
  for (int l = 0; l < 4; ++l) w[l] = O::sel(o.q_eq(l), one, zero);
  for (int r = 0; r < 4; ++r) {
    for (int l = 0; l < 4; ++l) M[r][4 * l + r] = M[r][4 * l + r] - w[l];
    dinv[r] = zero;
  }
  for (int j = 0; j < 4; ++j) M[3][5 * j] = M[3][5 * j] + w[3];
  for (int k = 0; k < 16; ++k) {
    const int pl = k >> 2, pr = k & 3;
    Q4 prow[16];
    for (int j = k; j < 16; ++j) {
      const double v = M[pr][j].v[pl];
      prow[j] = O::splat(v);
    }
    const Q4 pinv = O::rcp(prow[k]);
    const P4 mine = o.q_eq(pl);
    dinv[pr] = O::sel(mine, pinv, dinv[pr]);
    for (int r = 0; r < 4; ++r) {
      Q4 f = M[r][k] * pinv;
      if (r == pr) f = O::sel(mine, zero, f);
      for (int j = k + 1; j < 16; ++j) M[r][j] = O::fma(-f, prow[j], M[r][j]);
      if (k == 15) y[r] = -f;
    }
  }
  y[3] = O::sel(o.q_eq(3), one, y[3]);
  for (int r = 0; r < 4; ++r) x[r] = y[r] * dinv[r];
  pivmax = O::qmax(O::vmax(O::vmax(O::vabs(dinv[0]), O::vabs(dinv[1])), O::vmax(O::vabs(dinv[2]), O::vabs(dinv[3]))));
}

void store(const Q4 (&x)[4], const Q4 (&us)[16], long b, double* x_out, double* us_out) {
  for (int q = 0; q < 4; ++q)
    for (int r = 0; r < 4; ++r) x_out[(b * 4 + q) * 4 + r] = x[r].v[q];
  for (int a = 0; a < 16; ++a)
    for (int q = 0; q < 4; ++q) us_out[(b * 16 + a) * 4 + q] = us[a].v[q];
}

}  // namespace

// B tensors A [B][2][4][4] c128 through three routes, each followed by one power step:
//   route 0  build, solve, normalise, gather                (what the older emulations call)
//   route 1  build, solve_gathered, normalise_gathered      (what the kernels call)
//   route 2  build, the natural-order Gauss-Jordan of this file, normalise, gather
// Outputs per route (leading index: route): x [3][B][4 lanes][4]: the lanes' own coordinates, normalised; us [3][B][16][4 lanes]: every
// coordinate as every lane holds it; pivmax [3][B]; d2 [3][B]: squared distance of one power step.
extern "C" int solve_order_emu_d4(long B, const double* A, double* x_out, double* us_out, double* pivmax_out, double* d2_out) {
  for (long b = 0; b < B; ++b) {
    HostOps o{A + b * 64};
    for (int route = 0; route < 3; ++route) {
      Q4 Rc[4][16], x[4], us[16], y[4], pivmax;
      OrderCore::build(o, Rc);
      if (route == 1) {
        Q4 ur[16];
        OrderCore::solve_gathered(o, Rc, ur, pivmax);
        OrderCore::normalise_gathered(o, ur, us, x);
      } else {
        if (route == 0) OrderCore::solve(o, Rc, x, pivmax);
        else gauss_jordan_natural(o, Rc, x, pivmax);
        OrderCore::normalise(o, x);
        OrderCore::gather(x, us);
      }
      const Q4 d2 = OrderCore::power_step(o, x, us, y);
      store(x, us, b, x_out + route * B * 16, us_out + route * B * 64);
      pivmax_out[route * B + b] = pivmax.v[0];
      d2_out[route * B + b] = d2.v[0];
    }
  }
  return 0;
}
