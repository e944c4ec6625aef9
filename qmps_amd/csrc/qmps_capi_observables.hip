// qmps_capi_observables.hip - C-ABI of the observables of the resident states: two-point functions and string order (kernels: qmps_correlator.hip),
// Schmidt spectra and entropies (qmps_entanglement.hip), density matrices and entropies of blocks of sites (qmps_block_rdm.hip, then the Jacobi kernels of qmps_entanglement.hip: the one call with two launches), correlator sums of one-site and of two-site operators (qmps_corrsum.hip and the kernel files it dispatches to).  Every call checks its own arguments,
// passes the shared front, carves its regions out of the scratch buffer, uploads its inputs, launches ONE kernel, reads its results
// back and synchronises ONE time.  A refused call writes nothing and allocates nothing.
#include "qmps_ctx.h"

using namespace qmps_host;

namespace {

// The checks every observable makes after those of its own arguments, in this order: the context, the window, the size of the
// result (bytes_per_eval per evaluation against 1 GiB; 0 = no limit), the resident states, the resident environment.  `empty` tells
// the caller that B == 0: it returns QMPS_OK without touching anything.  `other_axis`: what the size message offers to split
// besides the batch.
int resident_front(qmps_ctx* c, int64_t B, uint64_t bytes_per_eval, const char* other_axis, bool& empty) {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  // compare through a division: B * bytes_per_eval may not fit 64 bits, and nothing is allocated or written before
  constexpr uint64_t kLimit = (uint64_t)1 << 30;
  if (bytes_per_eval > 0 && (uint64_t)B > kLimit / bytes_per_eval)
    return fail(QMPS_ERR_ARG, "result of %lld x %llu bytes exceeds the limit of 1 GiB (2^30 bytes): split the batch or %s", (long long)B,
                (unsigned long long)bytes_per_eval, other_axis);
  if (int rc = check_resident(c, B)) return rc;
  if (!c->env.covers(c->window, c->window + B)) return fail(QMPS_ERR_STATE, "no resident environment for the window: run qmps_energy_launch (without QMPS_FLAG_NO_ENV_OUT) or qmps_set_env_guess first");
  empty = B == 0;
  return QMPS_OK;
}

int check_n_ops(int n_ops) {
  if (n_ops < 1 || n_ops > qmps::kMaxObservableOps)
    return fail(QMPS_ERR_ARG, "n_ops=%d outside [1, %d] (four operators span the one-site operators)", n_ops, qmps::kMaxObservableOps);
  return QMPS_OK;
}

// The one kernel launch of a call, between the timing events when kernel timing is on (qmps_kernel_time then reads the kernel alone)
template <class Args>
int timed_launch(qmps_ctx* c, const char* name, hipError_t (*launch)(int, const Args&, hipStream_t), const Args& a) {
  KernelTimer timer(c, !c->capturing && c->timing_period > 0);
  HIP_TRY(timer.start());
  HIP_TRY(launch(c->D, a, c->stream));
  if (timer.on) c->dominant = name;
  HIP_TRY(timer.stop());
  return QMPS_OK;
}

// Bump carver over c->d_scratch: a call names its regions in order and gets their offsets; `bytes` is what ensure_scratch has to
// provide before the offsets become addresses
struct ScratchLayout {
  size_t bytes = 0;
  size_t take(size_t n) {
    const size_t at = bytes;
    bytes += n;
    return at;
  }
  void align(size_t a) { bytes = (bytes + a - 1) / a * a; }
};

// qmps_correlator_sums and qmps_correlator_sums_two_site: one contract, one body.  `two_site`: operators of 4 x 4 entries, three
// near values per pair where the one-site call has one `site` value, the two-site kernels.
int correlator_sums_call(qmps_ctx* c, int64_t B, int n_ops, const double* ops, int n_z, const double* z, double* G_out, double* one_out,
                         double* site_out, bool two_site) {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!ops) return fail(QMPS_ERR_ARG, "null ops");
  if (!z) return fail(QMPS_ERR_ARG, "null z");
  if (!G_out) return fail(QMPS_ERR_ARG, "null G_out");
  if (int rc = check_n_ops(n_ops)) return rc;
  if (n_z < 1 || n_z > 1024) return fail(QMPS_ERR_ARG, "n_z=%d outside [1, 1024]", n_z);
  for (int j = 0; j < n_z; ++j) {
    const double n2 = z[2 * j] * z[2 * j] + z[2 * j + 1] * z[2 * j + 1];
    // (the slack is for e^(ik) as float64 rounds it; a NaN fails the comparison too)
    if (!(n2 <= 1.0 + 1e-12)) return fail(QMPS_ERR_ARG, "|z[%d]|^2 = %.17g outside the closed unit disc: the sum over n does not converge there", j, n2);
  }
  const uint64_t per_eval = (uint64_t)n_z * n_ops * n_ops * 16;
  bool empty = false;
  if (int rc = resident_front(c, B, per_eval, "z", empty)) return rc;
  if (empty) return QMPS_OK;
  if (int rc = ensure_tensors(c)) return rc;
  const int64_t slabs = qmps::correlator_sums_slabs(c->D, B * n_z);
  const size_t op_bytes = two_site ? qmps::kTwoSiteOpBytes : qmps::kOneSiteOpBytes, site_values = two_site ? qmps::kTwoSiteSiteValues : qmps::kOneSiteSiteValues;
  const size_t z_bytes = (size_t)n_z * 16, G_bytes = (size_t)B * per_eval, one_bytes = (size_t)B * n_ops * 16, site_bytes = one_bytes * n_ops * site_values;
  ScratchLayout s;
  const size_t ops_at = s.take(qmps::kMaxObservableOps * op_bytes), z_at = s.take(16384), G_at = s.take(G_bytes), one_at = s.take(one_bytes), site_at = s.take(site_bytes);
  // D = 16: the matrices of the workgroups, (G_bytes + one_bytes + site_bytes + 255) / 256 * 256 bytes behind G (the operators and z
  // take multiples of 256 bytes, so rounding the offset is rounding that sum)
  s.align(256);
  const size_t work_at = s.take((size_t)slabs * qmps::correlator_sums_slab_bytes());
  if (int rc = ensure_scratch(c, s.bytes)) return rc;
  char* base = (char*)c->d_scratch;
  char *d_ops = base + ops_at, *d_z = base + z_at, *d_G = base + G_at, *d_one = base + one_at, *d_site = base + site_at;
  HIP_TRY(hipMemcpyAsync(d_ops, ops, (size_t)n_ops * op_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_z, z, z_bytes, hipMemcpyHostToDevice, c->stream));
  qmps::CorrSumArgs a{};
  a.A = win_A(c);
  a.r = win_r(c);
  a.ops = d_ops;
  a.z = d_z;
  a.G = d_G;
  a.one = one_out ? d_one : nullptr;
  a.site = site_out ? d_site : nullptr;
  a.work = slabs > 0 ? base + work_at : nullptr;
  a.B = B;
  a.n_ops = n_ops;
  a.n_z = n_z;
  a.n_slabs = (int)slabs;
  if (int rc = two_site ? timed_launch(c, "correlator_sums_two_site", qmps::launch_correlator_sums_two_site, a)
                        : timed_launch(c, "correlator_sums", qmps::launch_correlator_sums, a))
    return rc;
  HIP_TRY(hipMemcpyAsync(G_out, d_G, G_bytes, hipMemcpyDeviceToHost, c->stream));
  if (one_out) HIP_TRY(hipMemcpyAsync(one_out, d_one, one_bytes, hipMemcpyDeviceToHost, c->stream));
  if (site_out) HIP_TRY(hipMemcpyAsync(site_out, d_site, site_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}

// qmps_correlators and qmps_string_correlators: one contract, one body.  `with_string`: the string call, whose `string` must not be
// null; it uploads the string behind the operators (still one upload), launches the kernels of the string chain and may return str.
int correlators_call(qmps_ctx* c, int64_t B, int n_ops, const double* ops, bool with_string, const double* string, int n_max, double* C_out,
                     double* one_out, double* str_out) {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!ops) return fail(QMPS_ERR_ARG, "null ops");
  if (with_string && !string) return fail(QMPS_ERR_ARG, "null string");
  if (!C_out) return fail(QMPS_ERR_ARG, "null C_out");
  if (int rc = check_n_ops(n_ops)) return rc;
  if (n_max < 1 || n_max > 4096) return fail(QMPS_ERR_ARG, "n_max=%d outside [1, 4096]", n_max);
  const uint64_t per_eval = ((uint64_t)n_ops * n_ops + (str_out ? 1 : 0)) * n_max * 16;
  bool empty = false;
  if (int rc = resident_front(c, B, per_eval, "n_max", empty)) return rc;
  if (empty) return QMPS_OK;
  if (int rc = ensure_tensors(c)) return rc;
  const size_t op_bytes = qmps::kOneSiteOpBytes, ops_bytes = (size_t)n_ops * op_bytes;
  const size_t C_bytes = (size_t)B * n_ops * n_ops * n_max * 16, one_bytes = (size_t)B * n_ops * 16, str_bytes = str_out ? (size_t)B * n_max * 16 : 0;
  ScratchLayout s;
  const size_t ops_at = s.take((qmps::kMaxObservableOps + 1) * op_bytes);
  s.align(256);      // the runs of the kernels' stores stay whole cache lines
  const size_t C_at = s.take(C_bytes), one_at = s.take(one_bytes), str_at = s.take(str_bytes);
  if (int rc = ensure_scratch(c, s.bytes)) return rc;
  char* base = (char*)c->d_scratch;
  char *d_ops = base + ops_at, *d_C = base + C_at, *d_one = base + one_at, *d_str = base + str_at;
  // the string travels behind the operators: one upload either way (the staging copy lives until the synchronisation below)
  double staged[(qmps::kMaxObservableOps + 1) * (qmps::kOneSiteOpBytes / sizeof(double))];
  const double* src = ops;
  size_t up_bytes = ops_bytes;
  if (with_string) {
    memcpy(staged, ops, ops_bytes);
    memcpy((char*)staged + ops_bytes, string, op_bytes);
    src = staged;
    up_bytes += op_bytes;
  }
  HIP_TRY(hipMemcpyAsync(d_ops, src, up_bytes, hipMemcpyHostToDevice, c->stream));
  qmps::CorrelatorArgs a{};
  a.A = win_A(c);
  a.r = win_r(c);
  a.ops = d_ops;
  a.C = d_C;
  a.one = one_out ? d_one : nullptr;
  a.B = B;
  a.n_ops = n_ops;
  a.n_max = n_max;
  a.string = with_string ? d_ops + ops_bytes : nullptr;
  a.str = str_out ? d_str : nullptr;
  if (int rc = with_string ? timed_launch(c, "string_correlator", qmps::launch_string_correlators, a)
                           : timed_launch(c, "correlator", qmps::launch_correlators, a))
    return rc;
  HIP_TRY(hipMemcpyAsync(C_out, d_C, C_bytes, hipMemcpyDeviceToHost, c->stream));
  if (one_out) HIP_TRY(hipMemcpyAsync(one_out, d_one, one_bytes, hipMemcpyDeviceToHost, c->stream));
  if (str_out) HIP_TRY(hipMemcpyAsync(str_out, d_str, str_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}

}  // namespace

extern "C" {

int qmps_correlators(qmps_ctx* c, int64_t B, int n_ops, const double* ops, int n_max, double* C_out, double* one_out) try {
  return correlators_call(c, B, n_ops, ops, false, nullptr, n_max, C_out, one_out, nullptr);
}
QMPS_API_CATCH

int qmps_string_correlators(qmps_ctx* c, int64_t B, int n_ops, const double* ops, const double* string, int n_max, double* C_out,
                            double* one_out, double* str_out) try {
  return correlators_call(c, B, n_ops, ops, true, string, n_max, C_out, one_out, str_out);
}
QMPS_API_CATCH

int qmps_entanglement(qmps_ctx* c, int64_t B, double* p_out, double* S_out, double* V_out) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!p_out) return fail(QMPS_ERR_ARG, "null p_out");
  bool empty = false;
  if (int rc = resident_front(c, B, 0, "", empty)) return rc;      // a few D x D matrices per evaluation: no size limit
  if (empty) return QMPS_OK;
  const size_t p_bytes = (size_t)B * c->D * 8, S_bytes = (size_t)B * 8, V_bytes = V_out ? (size_t)B * env_bytes(c) : 0;
  ScratchLayout s;
  const size_t p_at = s.take(p_bytes), S_at = s.take(S_bytes), V_at = s.take(V_bytes);
  if (int rc = ensure_scratch(c, s.bytes)) return rc;
  char* base = (char*)c->d_scratch;
  char *d_p = base + p_at, *d_S = base + S_at, *d_V = base + V_at;
  qmps::EntanglementArgs a{};
  a.r = win_r(c);
  a.p = (double*)d_p;
  a.S = (double*)d_S;
  a.V = V_out ? d_V : nullptr;
  a.B = B;
  if (int rc = timed_launch(c, "entanglement", qmps::launch_entanglement, a)) return rc;
  HIP_TRY(hipMemcpyAsync(p_out, d_p, p_bytes, hipMemcpyDeviceToHost, c->stream));
  if (S_out) HIP_TRY(hipMemcpyAsync(S_out, d_S, S_bytes, hipMemcpyDeviceToHost, c->stream));
  if (V_out) HIP_TRY(hipMemcpyAsync(V_out, d_V, V_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_block_entanglement(qmps_ctx* c, int64_t B, int n_sites, double* rho_out, double* p_out, double* S_out) try {
  if (n_sites < 1 || n_sites > qmps::kMaxBlockSites)
    return fail(QMPS_ERR_ARG, "n_sites=%d outside [1, %d] (the spectrum of a larger block is no Jacobi order of this library)", n_sites, qmps::kMaxBlockSites);
  if (!rho_out && !p_out && !S_out) return fail(QMPS_ERR_ARG, "null rho_out, p_out and S_out: nothing to return");
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  const int T = 1 << n_sites;
  const uint64_t per_eval = (uint64_t)T * T * 16;                   // the device-side rho, whether or not it is read back
  bool empty = false;
  if (int rc = resident_front(c, B, per_eval, "n_sites", empty)) return rc;
  if (empty) return QMPS_OK;
  if (int rc = ensure_tensors(c)) return rc;
  const bool spectrum = p_out || S_out;
  const size_t rho_bytes = (size_t)B * per_eval, p_bytes = spectrum ? (size_t)B * T * 8 : 0, S_bytes = spectrum ? (size_t)B * 8 : 0;
  ScratchLayout s;
  const size_t rho_at = s.take(rho_bytes), p_at = s.take(p_bytes), S_at = s.take(S_bytes);
  if (int rc = ensure_scratch(c, s.bytes)) return rc;
  char* base = (char*)c->d_scratch;
  char *d_rho = base + rho_at, *d_p = base + p_at, *d_S = base + S_at;
  qmps::BlockRdmArgs a{};
  a.A = win_A(c);
  a.r = win_r(c);
  a.rho = d_rho;
  a.B = B;
  a.n_sites = n_sites;
  if (int rc = timed_launch(c, "block_rdm", qmps::launch_block_rdm, a)) return rc;
  if (spectrum) {
    // the Jacobi kernels of qmps_entanglement at the order 2^n, on rho where it lies: herm(rho) / tr rho, its rule for NaN
    qmps::EntanglementArgs j{};
    j.r = d_rho;
    j.p = (double*)d_p;
    j.S = (double*)d_S;
    j.B = B;
    HIP_TRY(qmps::launch_entanglement(T, j, c->stream));
  }
  if (rho_out) HIP_TRY(hipMemcpyAsync(rho_out, d_rho, rho_bytes, hipMemcpyDeviceToHost, c->stream));
  if (p_out) HIP_TRY(hipMemcpyAsync(p_out, d_p, p_bytes, hipMemcpyDeviceToHost, c->stream));
  if (S_out) HIP_TRY(hipMemcpyAsync(S_out, d_S, S_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_correlator_sums(qmps_ctx* c, int64_t B, int n_ops, const double* ops, int n_z, const double* z, double* G_out, double* one_out,
                         double* site_out) try {
  return correlator_sums_call(c, B, n_ops, ops, n_z, z, G_out, one_out, site_out, false);
}
QMPS_API_CATCH

int qmps_correlator_sums_two_site(qmps_ctx* c, int64_t B, int n_ops, const double* ops, int n_z, const double* z, double* G_out, double* one_out,
                                  double* near_out) try {
  return correlator_sums_call(c, B, n_ops, ops, n_z, z, G_out, one_out, near_out, true);
}
QMPS_API_CATCH

}  // extern "C"
