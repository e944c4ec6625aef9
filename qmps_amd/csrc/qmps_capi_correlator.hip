// qmps_capi_correlator.hip - C-ABI of the two-point functions of the resident states (kernels: qmps_correlator.hip)
#include "qmps_ctx.h"

using namespace qmps_host;

extern "C" {

int qmps_correlators(qmps_ctx* c, int64_t B, int n_ops, const double* ops, int n_max, double* C_out, double* one_out) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!ops) return fail(QMPS_ERR_ARG, "null ops");
  if (!C_out) return fail(QMPS_ERR_ARG, "null C_out");
  if (n_ops < 1 || n_ops > 4) return fail(QMPS_ERR_ARG, "n_ops=%d outside [1, 4] (four operators span the one-site operators)", n_ops);
  if (n_max < 1 || n_max > 4096) return fail(QMPS_ERR_ARG, "n_max=%d outside [1, 4096]", n_max);
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  // B <= max_batch < 2^63 / (16 * 4096 * 16) is not given: compare through a division, nothing is allocated before
  constexpr uint64_t kLimit = (uint64_t)1 << 30;
  const uint64_t per_eval = (uint64_t)n_ops * n_ops * n_max * 16;
  if ((uint64_t)B > kLimit / per_eval)
    return fail(QMPS_ERR_ARG, "result of %lld x %d x %d x %d complex values exceeds the limit of 1 GiB (2^30 bytes): split the batch or n_max", (long long)B,
                n_ops, n_ops, n_max);
  if (c->window + B > c->n_states)
    return fail(QMPS_ERR_STATE, "window [%lld, %lld) but only %lld states are resident", (long long)c->window, (long long)(c->window + B), (long long)c->n_states);
  if (!c->have_env) return fail(QMPS_ERR_STATE, "no resident environment: run qmps_energy_launch (without QMPS_FLAG_NO_ENV_OUT) or qmps_set_env_guess first");
  if (B == 0) return QMPS_OK;
  if (int rc = ensure_tensors(c)) return rc;
  // scratch: operators | C | one
  const size_t ops_bytes = 256, C_bytes = (size_t)B * per_eval, one_bytes = (size_t)B * n_ops * 16;
  if (int rc = ensure_scratch(c, ops_bytes + C_bytes + one_bytes)) return rc;
  char* d_ops = (char*)c->d_scratch;
  char* d_C = d_ops + ops_bytes;
  char* d_one = d_C + C_bytes;
  HIP_TRY(hipMemcpyAsync(d_ops, ops, (size_t)n_ops * 64, hipMemcpyHostToDevice, c->stream));
  qmps::CorrelatorArgs a{};
  a.A = win_A(c);
  a.r = win_r(c);
  a.ops = d_ops;
  a.C = d_C;
  a.one = one_out ? d_one : nullptr;
  a.B = B;
  a.n_ops = n_ops;
  a.n_max = n_max;
  KernelTimer timer(c, !c->capturing && c->timing_period > 0);      // qmps_kernel_time reads the kernel alone
  HIP_TRY(timer.start());
  HIP_TRY(qmps::launch_correlators(c->D, a, c->stream));
  if (timer.on) c->dominant = "correlator";
  HIP_TRY(timer.stop());
  HIP_TRY(hipMemcpyAsync(C_out, d_C, C_bytes, hipMemcpyDeviceToHost, c->stream));
  if (one_out) HIP_TRY(hipMemcpyAsync(one_out, d_one, one_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

}  // extern "C"
