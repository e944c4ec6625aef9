// rho_need_emu.cpp - TEST INFRASTRUCTURE ONLY.  The "needed entries" mask of the two-site density matrix (qmps::rho_need_mask,
// DirectD4::density / energy with a mask: qmps_amd/csrc/qmps_direct_core.h) on the CPU, in the lock-step host policy of direct_emu.cpp,
// beside the routes without a mask.  Nothing in the product loads this file.
//
// Build: g++ <CXXFLAGS of tests/csrc/Makefile> -shared tests/csrc/rho_need_emu.cpp -o tests/csrc/librho_need_emu.so
#include "direct_emu.cpp"
#include "rho_reference.h"

extern "C" uint32_t rho_need_mask_emu(const double* h, int nt) { return qmps::rho_need_mask(h, nt); }

// Density matrix and energies of B evaluations from their tensors A [B][2][4][4] c128 and environments r [B][4][4] c128 (as direct_emu_d4
// returns them: the coordinates the kernel holds, exactly).  masked == 0: DirectD4::density / energy without a mask; masked == 1: with
// `need`; masked == -1: the reference, the functions as they stood before there was a mask (rho_reference.h).
// Outputs: E [B][nt]; pre, pim [B][4][4][4]: the four lanes' shares of rho[t][s], t <= s (the rest 0.0); pd [B]: the positive-definiteness
// flag.
extern "C" int rho_need_emu_d4(long B, const double* A, const double* r, const double* h, int nt, int masked, uint32_t need, double* E,
                               double* pre_out, double* pim_out, int32_t* pd_out) {
  using Core = qmps::DirectD4<HostOps>;
  using V = Q4;
  for (long b = 0; b < B; ++b) {
    HostOps o{A + b * 64};
    V us[16];
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j) {
        us[4 * i + j] = HostOps::splat(r[2 * (b * 16 + i * 4 + j)]);
        if (i != j) us[4 * j + i] = HostOps::splat(r[2 * (b * 16 + i * 4 + j) + 1]);
      }
    V pre[4][4], pim[4][4];
    using Ref = qmps_test::RhoReference<HostOps>;
    const P4 pd = masked < 0 ? Ref::density(o, us, pre, pim) : masked ? Core::density(o, us, need, pre, pim) : Core::density(o, us, pre, pim);
    pd_out[b] = pd.v[0];
    for (int t = 0; t < nt; ++t) {
      const double* ht = h + 32 * t;
      E[b * nt + t] = HostOps::qsum(masked < 0 ? Ref::energy(ht, pre, pim) : masked ? Core::energy(ht, need, pre, pim) : Core::energy(ht, pre, pim)).v[0];
    }
    for (int t = 0; t < 4; ++t)
      for (int s = 0; s < 4; ++s)
        for (int q = 0; q < 4; ++q) {
          pre_out[((b * 4 + t) * 4 + s) * 4 + q] = t <= s ? pre[t][s].v[q] : 0.0;
          pim_out[((b * 4 + t) * 4 + s) * 4 + q] = t < s ? pim[t][s].v[q] : 0.0;
        }
  }
  return 0;
}
