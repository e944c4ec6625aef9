// qmps_capi_corrsum.hip - C-ABI of the correlator sums of the resident states (kernels: qmps_corrsum.hip)
#include "qmps_ctx.h"

using namespace qmps_host;

extern "C" {

int qmps_correlator_sums(qmps_ctx* c, int64_t B, int n_ops, const double* ops, int n_z, const double* z, double* G_out, double* one_out,
                         double* site_out) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!ops) return fail(QMPS_ERR_ARG, "null ops");
  if (!z) return fail(QMPS_ERR_ARG, "null z");
  if (!G_out) return fail(QMPS_ERR_ARG, "null G_out");
  if (n_ops < 1 || n_ops > 4) return fail(QMPS_ERR_ARG, "n_ops=%d outside [1, 4] (four operators span the one-site operators)", n_ops);
  if (n_z < 1 || n_z > 1024) return fail(QMPS_ERR_ARG, "n_z=%d outside [1, 1024]", n_z);
  for (int j = 0; j < n_z; ++j) {
    const double n2 = z[2 * j] * z[2 * j] + z[2 * j + 1] * z[2 * j + 1];
    // (the slack is for e^(ik) as float64 rounds it; a NaN fails the comparison too)
    if (!(n2 <= 1.0 + 1e-12)) return fail(QMPS_ERR_ARG, "|z[%d]|^2 = %.17g outside the closed unit disc: the sum over n does not converge there", j, n2);
  }
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  // compare through a division: nothing is allocated or written before
  constexpr uint64_t kLimit = (uint64_t)1 << 30;
  const uint64_t per_eval = (uint64_t)n_z * n_ops * n_ops * 16;
  if ((uint64_t)B > kLimit / per_eval)
    return fail(QMPS_ERR_ARG, "result of %lld x %d x %d x %d complex values exceeds the limit of 1 GiB (2^30 bytes): split the batch or z", (long long)B, n_z,
                n_ops, n_ops);
  if (c->window + B > c->n_states)
    return fail(QMPS_ERR_STATE, "window [%lld, %lld) but only %lld states are resident", (long long)c->window, (long long)(c->window + B), (long long)c->n_states);
  if (!c->have_env) return fail(QMPS_ERR_STATE, "no resident environment: run qmps_energy_launch (without QMPS_FLAG_NO_ENV_OUT) or qmps_set_env_guess first");
  if (B == 0) return QMPS_OK;
  if (int rc = ensure_tensors(c)) return rc;
  // scratch: operators | z | G | one | site | D = 16: the matrices of the workgroups
  const int64_t slabs = qmps::correlator_sums_slabs(c->D, B * n_z);
  const size_t ops_bytes = 256, z_bytes = (size_t)n_z * 16, G_bytes = (size_t)B * per_eval, one_bytes = (size_t)B * n_ops * 16,
               site_bytes = one_bytes * n_ops, out_bytes = (G_bytes + one_bytes + site_bytes + 255) / 256 * 256,
               work_bytes = (size_t)slabs * qmps::correlator_sums_slab_bytes();
  if (int rc = ensure_scratch(c, ops_bytes + 16384 + out_bytes + work_bytes)) return rc;
  char* d_ops = (char*)c->d_scratch;
  char* d_z = d_ops + ops_bytes;
  char* d_G = d_z + 16384;
  char* d_one = d_G + G_bytes;
  char* d_site = d_one + one_bytes;
  HIP_TRY(hipMemcpyAsync(d_ops, ops, (size_t)n_ops * 64, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_z, z, z_bytes, hipMemcpyHostToDevice, c->stream));
  qmps::CorrSumArgs a{};
  a.A = win_A(c);
  a.r = win_r(c);
  a.ops = d_ops;
  a.z = d_z;
  a.G = d_G;
  a.one = one_out ? d_one : nullptr;
  a.site = site_out ? d_site : nullptr;
  a.work = slabs > 0 ? d_G + out_bytes : nullptr;
  a.B = B;
  a.n_ops = n_ops;
  a.n_z = n_z;
  a.n_slabs = (int)slabs;
  KernelTimer timer(c, !c->capturing && c->timing_period > 0);      // qmps_kernel_time reads the kernel alone
  HIP_TRY(timer.start());
  HIP_TRY(qmps::launch_correlator_sums(c->D, a, c->stream));
  if (timer.on) c->dominant = "correlator_sums";
  HIP_TRY(timer.stop());
  HIP_TRY(hipMemcpyAsync(G_out, d_G, G_bytes, hipMemcpyDeviceToHost, c->stream));
  if (one_out) HIP_TRY(hipMemcpyAsync(one_out, d_one, one_bytes, hipMemcpyDeviceToHost, c->stream));
  if (site_out) HIP_TRY(hipMemcpyAsync(site_out, d_site, site_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

}  // extern "C"
