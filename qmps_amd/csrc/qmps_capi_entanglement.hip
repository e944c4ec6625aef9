// qmps_capi_entanglement.hip - C-ABI of the Schmidt spectra and entropies of the resident states (kernels: qmps_entanglement.hip)
#include "qmps_ctx.h"

using namespace qmps_host;

extern "C" {

int qmps_entanglement(qmps_ctx* c, int64_t B, double* p_out, double* S_out, double* V_out) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!p_out) return fail(QMPS_ERR_ARG, "null p_out");
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (c->window + B > c->n_states)
    return fail(QMPS_ERR_STATE, "window [%lld, %lld) but only %lld states are resident", (long long)c->window, (long long)(c->window + B), (long long)c->n_states);
  if (!c->have_env) return fail(QMPS_ERR_STATE, "no resident environment: run qmps_energy_launch (without QMPS_FLAG_NO_ENV_OUT) or qmps_set_env_guess first");
  if (B == 0) return QMPS_OK;
  // scratch: p | S | V
  const size_t p_bytes = (size_t)B * c->D * 8, S_bytes = (size_t)B * 8, V_bytes = V_out ? (size_t)B * env_bytes(c) : 0;
  if (int rc = ensure_scratch(c, p_bytes + S_bytes + V_bytes)) return rc;
  char* d_p = (char*)c->d_scratch;
  char* d_S = d_p + p_bytes;
  char* d_V = d_S + S_bytes;
  qmps::EntanglementArgs a{};
  a.r = win_r(c);
  a.p = (double*)d_p;
  a.S = (double*)d_S;
  a.V = V_out ? d_V : nullptr;
  a.B = B;
  KernelTimer timer(c, !c->capturing && c->timing_period > 0);      // qmps_kernel_time reads the kernel alone
  HIP_TRY(timer.start());
  HIP_TRY(qmps::launch_entanglement(c->D, a, c->stream));
  if (timer.on) c->dominant = "entanglement";
  HIP_TRY(timer.stop());
  HIP_TRY(hipMemcpyAsync(p_out, d_p, p_bytes, hipMemcpyDeviceToHost, c->stream));
  if (S_out) HIP_TRY(hipMemcpyAsync(S_out, d_S, S_bytes, hipMemcpyDeviceToHost, c->stream));
  if (V_out) HIP_TRY(hipMemcpyAsync(V_out, d_V, V_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

}  // extern "C"
