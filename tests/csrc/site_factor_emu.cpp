// site_factor_emu.cpp - TEST INFRASTRUCTURE ONLY.  The site-factor route of the two-site density matrix (DirectD4::power_step_sites /
// update_sites / density_sites: qmps_amd/csrc/qmps_direct_core.h) on the CPU, in the lock-step host policy of direct_emu.cpp with the one
// accessor the route adds (col: the lane's own column of the tensor).  Nothing in the product loads this file.
//
// Build: g++ <CXXFLAGS of tests/csrc/Makefile> -shared tests/csrc/site_factor_emu.cpp -o tests/csrc/libsite_factor_emu.so
#include "direct_emu.cpp"

namespace {

struct SiteOps : HostOps {
  void col(int s, int i, V& re, V& im) const {
    for (int q = 0; q < 4; ++q) {
      re.v[q] = A[2 * ((s * 4 + i) * 4 + q)];
      im.v[q] = A[2 * ((s * 4 + i) * 4 + q) + 1];
    }
  }
};

using SiteCore = qmps::DirectD4<SiteOps>;

// the coordinates of r [4][4] c128 (upper triangle read), in every lane
void coordinates(const double* r, Q4 (&us)[16]) {
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j) {
      us[4 * i + j] = HostOps::splat(r[2 * (i * 4 + j)]);
      if (i != j) us[4 * j + i] = HostOps::splat(r[2 * (i * 4 + j) + 1]);
    }
}

void shares(const Q4 (&pre)[4][4], const Q4 (&pim)[4][4], long b, double* pre_out, double* pim_out) {
  for (int t = 0; t < 4; ++t)
    for (int s = 0; s < 4; ++s)
      for (int q = 0; q < 4; ++q) {
        pre_out[((b * 4 + t) * 4 + s) * 4 + q] = t <= s ? pre[t][s].v[q] : 0.0;
        pim_out[((b * 4 + t) * 4 + s) * 4 + q] = t < s ? pim[t][s].v[q] : 0.0;
      }
}

}  // namespace

extern "C" uint32_t site_factors_emu(uint32_t need) { return qmps::rho_site_factors(need); }

// Density matrix and energies of B evaluations from their tensors A [B][2][4][4] c128 and environments r [B][4][4] c128, any tensor and any
// Hermitian r: power_step_sites (the W), density_sites, energy with the mask `need`.
// via_update == 0: W as power_step_sites leaves it.  1: W first from the environment 1/4, then update_sites with r for every lane - the
// fall-back's route.  2: W from r, then update_sites with the environment 1/4 for NO lane.  All three must agree bit for bit.
// Outputs: E [B][nt]; pre, pim [B][4][4][4]: the four lanes' shares of rho[t][s], t <= s (the rest 0.0); pd [B]; y [B][4][4]: the lanes'
// coordinates of the normalised power step (lane q, coordinate l); d2 [B]: its squared distance to r.
extern "C" int site_factor_emu_d4(long B, const double* A, const double* r, const double* h, int nt, uint32_t need, int via_update,
                                  double* E, double* pre_out, double* pim_out, int32_t* pd_out, double* y_out, double* d2_out) {
  using V = Q4;
  const P4 all = {{true, true, true, true}}, none = {{false, false, false, false}};
  for (long b = 0; b < B; ++b) {
    SiteOps o{{A + b * 64}};
    V us[16], flat[16], x[4], y[4];
    coordinates(r + b * 32, us);
    for (int a = 0; a < 16; ++a) flat[a] = HostOps::splat(a % 5 == 0 ? 0.25 : 0.0);
    for (int l = 0; l < 4; ++l)
      for (int q = 0; q < 4; ++q) x[l].v[q] = us[4 * q + l].v[0];
    SiteCore::SiteW W;
    V d2;
    if (via_update == 1) {
      V x0[4], y0[4];
      for (int l = 0; l < 4; ++l)
        for (int q = 0; q < 4; ++q) x0[l].v[q] = flat[4 * q + l].v[0];
      SiteCore::power_step_sites(o, x0, flat, need, y0, W);
      SiteCore::SiteW unused;
      d2 = SiteCore::power_step_sites(o, x, us, need, y, unused);
      SiteCore::update_sites(o, us, need, all, W);
    } else {
      d2 = SiteCore::power_step_sites(o, x, us, need, y, W);
      if (via_update == 2) SiteCore::update_sites(o, flat, need, none, W);
    }
    V pre[4][4], pim[4][4];
    const P4 pd = SiteCore::density_sites(o, us, need, W, pre, pim);
    pd_out[b] = pd.v[0];
    for (int t = 0; t < nt; ++t) E[b * nt + t] = HostOps::qsum(SiteCore::energy(h + 32 * t, need, pre, pim)).v[0];
    shares(pre, pim, b, pre_out, pim_out);
    for (int l = 0; l < 4; ++l)
      for (int q = 0; q < 4; ++q) y_out[(b * 4 + q) * 4 + l] = y[l].v[q];
    d2_out[b] = d2.v[0];
  }
  return 0;
}

// One batch through the sequence of core calls of the cold-start energy_direct_d4_kernel: direct_emu_d4 (direct_emu.cpp) with the acceptance
// step, the fall-back's hand-over and the density phase of the site-factor route.  Same arguments; `need` as the kernel takes it from the
// launch arguments.
extern "C" int site_factor_direct_d4(long B, const double* A, const double* h, int nt, uint32_t need, int max_iter, double tol, double* E,
                                     double* r_out, double* rho_out, int32_t* iters, int32_t* status) {
  using V = Q4;
  for (long b = 0; b < B; ++b) {
    SiteOps o{{A + b * 64}};
    V Rc[4][16], x[4], y[4], us[16];
    SiteCore::build(o, Rc);
    V pivmax;
    SiteCore::solve(o, Rc, x, pivmax);
    SiteCore::normalise(o, x);
    SiteCore::gather(x, us);
    SiteCore::SiteW W;
    const V d2 = SiteCore::power_step_sites(o, x, us, need, y, W);
    const double tol2 = tol * tol;
    const P4 ok = HostOps::p_and(HostOps::lt(d2, HostOps::splat(tol2)), HostOps::lt(pivmax, HostOps::splat(SiteCore::kMaxInversePivot)));
    V steps = HostOps::splat(1.0);
    int st = 0;
    if (!ok.v[0]) {
      V sq = HostOps::splat(0.0);
      SiteCore::build(o, Rc);
      const P4 left = SiteCore::squaring(o, Rc, HostOps::p_not(ok), max_iter - 1, tol2, x, sq);
      steps = HostOps::splat(1.0) + sq;
      st = left.v[0] ? 1 : 0;
      if (st == 1 && steps.v[0] + 1.0 <= (double)max_iter) {
        V yb[4];
        SiteCore::gather(x, us);
        const V d2b = SiteCore::power_step(o, x, us, yb);
        if (d2b.v[0] < tol2) {
          for (int l = 0; l < 4; ++l) x[l] = yb[l];
          steps = steps + HostOps::splat(1.0);
          st = 0;
        }
      }
      SiteCore::gather(x, us);
      SiteCore::update_sites(o, us, need, HostOps::p_not(ok), W);
    }
    V pre[4][4], pim[4][4];
    const P4 pd = SiteCore::density_sites(o, us, need, W, pre, pim);
    if (st == 0 && !pd.v[0]) st = 2;
    for (int t = 0; t < nt; ++t) E[b * nt + t] = HostOps::qsum(SiteCore::energy(h + 32 * t, need, pre, pim)).v[0];
    iters[b] = (int32_t)steps.v[0];
    status[b] = st;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const double re = us[4 * lo + hi].v[0], im = i == j ? 0.0 : us[4 * hi + lo].v[0];
        r_out[2 * (b * 16 + i * 4 + j)] = re;
        r_out[2 * (b * 16 + i * 4 + j) + 1] = i <= j ? im : -im;
      }
    for (int t = 0; t < 4; ++t)
      for (int s = 0; s < 4; ++s) {
        const int lo = t < s ? t : s, hi = t < s ? s : t;
        const double re = HostOps::qsum(pre[lo][hi]).v[0], im = t == s ? 0.0 : HostOps::qsum(pim[lo][hi]).v[0];
        rho_out[2 * (b * 16 + t * 4 + s)] = re;
        rho_out[2 * (b * 16 + t * 4 + s) + 1] = t <= s ? im : -im;
      }
  }
  return 0;
}
