// qmps_capi_brickwall.hip - the brick-wall (new_tdvp) calls of the C-ABI (declared in include/qmps_hip.h): expectation values,
// environments, the manifold contraction and the environment-optimisation objective.  One-shot calls: inputs are copied into the
// context's scratch arena, one launch of qmps_brickwall.hip, results copied back.  Context + helpers: qmps_capi.hip, qmps_ctx.h.
#include "qmps_ctx.h"

using namespace qmps_host;

// (every entry point below is declared extern "C" in include/qmps_hip.h: the definitions inherit the linkage)

namespace {
// bump allocator over the scratch arena: copies a host array in, returns the device address
struct Arena {
  qmps_ctx* c;
  size_t off = 0;
  void* put(const void* host, size_t bytes, hipError_t* err) {
    void* d = (char*)c->d_scratch + off;
    off += (bytes + 255) & ~(size_t)255;
    if (host) *err = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->stream);
    return d;
  }
};
}  // namespace

int qmps_bw_expval(qmps_ctx* c, int64_t B, int sites, const double* U1, const double* U2, const double* O, int o_shared,
                   double* out) try {
  if (int rc = bind(c)) return rc;
  if (B < 0 || !U1 || !U2 || !O || !out) return fail(QMPS_ERR_ARG, "bad arguments");
  if (sites != 2 && sites != 4) return fail(QMPS_ERR_ARG, "sites must be 2 or 4");
  const size_t no = sites == 2 ? 16 : 256;
  const size_t ob = (o_shared ? 1 : (size_t)B) * no * 16;
  if (int rc = ensure_scratch(c, (size_t)B * (256 + 256 + 16 + 256) + ob + 4096)) return rc;
  Arena a{c};
  hipError_t e = hipSuccess;
  qmps::BwArgs k;
  memset(&k, 0, sizeof(k));
  k.U1 = a.put(U1, (size_t)B * 256, &e); HIP_TRY(e);
  k.U2 = a.put(U2, (size_t)B * 256, &e); HIP_TRY(e);
  k.O = a.put(O, ob, &e); HIP_TRY(e);
  k.out = a.put(nullptr, (size_t)B * 16, &e);
  k.B = B; k.o_shared = o_shared ? 1 : 0;
  HIP_TRY(qmps::launch_bw(sites == 2 ? 0 : 1, k, c->stream));
  HIP_TRY(hipMemcpyAsync(out, k.out, (size_t)B * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_bw_env(qmps_ctx* c, int64_t B, int side, const double* U1, const double* U2, const double* U1p,
                const double* U2p, int max_rounds, double tol, double* mat_out, double* eta_out, double* vec_out,
                int32_t* status_out) try {
  if (int rc = bind(c)) return rc;
  if (B < 0 || !U1 || !U2 || !U1p || !U2p || !eta_out || !vec_out) return fail(QMPS_ERR_ARG, "bad arguments");
  if (side != 0 && side != 1) return fail(QMPS_ERR_ARG, "side must be 0 (right) or 1 (left)");
  if (max_rounds < 1 || max_rounds > 60 || !(tol > 0.0)) return fail(QMPS_ERR_ARG, "bad max_rounds / tol");
  if (int rc = ensure_scratch(c, (size_t)B * (4 * 256 + 256 + 16 + 64 + 16) + 8192)) return rc;
  Arena a{c};
  hipError_t e = hipSuccess;
  qmps::BwArgs k;
  memset(&k, 0, sizeof(k));
  k.U1 = a.put(U1, (size_t)B * 256, &e); HIP_TRY(e);
  k.U2 = a.put(U2, (size_t)B * 256, &e); HIP_TRY(e);
  k.U1p = a.put(U1p, (size_t)B * 256, &e); HIP_TRY(e);
  k.U2p = a.put(U2p, (size_t)B * 256, &e); HIP_TRY(e);
  k.mat_out = mat_out ? a.put(nullptr, (size_t)B * 256, &e) : nullptr;
  k.out = a.put(nullptr, (size_t)B * 16, &e);
  k.vec_out = a.put(nullptr, (size_t)B * 64, &e);
  k.status = (int32_t*)a.put(nullptr, (size_t)B * 4, &e);
  k.B = B; k.side = side; k.max_rounds = max_rounds; k.tol = tol;
  HIP_TRY(qmps::launch_bw(2, k, c->stream));
  if (mat_out) HIP_TRY(hipMemcpyAsync(mat_out, k.mat_out, (size_t)B * 256, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(eta_out, k.out, (size_t)B * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(vec_out, k.vec_out, (size_t)B * 64, hipMemcpyDeviceToHost, c->stream));
  if (status_out) HIP_TRY(hipMemcpyAsync(status_out, k.status, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_bw_manifold(qmps_ctx* c, int64_t B, const double* U1, const double* U2, const double* U1p, const double* U2p,
                     const double* Mr, const double* Ml, int m_shared, const double* W, int w_shared, double* out) try {
  if (int rc = bind(c)) return rc;
  if (B < 0 || !U1 || !U2 || !U1p || !U2p || !Mr || !Ml || !W || !out) return fail(QMPS_ERR_ARG, "bad arguments");
  const size_t mb = (m_shared ? 1 : (size_t)B) * 64, wb = (w_shared ? 1 : (size_t)B) * 4096;
  if (int rc = ensure_scratch(c, (size_t)B * (4 * 256 + 16) + 2 * mb + wb + 8192)) return rc;
  Arena a{c};
  hipError_t e = hipSuccess;
  qmps::BwArgs k;
  memset(&k, 0, sizeof(k));
  k.U1 = a.put(U1, (size_t)B * 256, &e); HIP_TRY(e);
  k.U2 = a.put(U2, (size_t)B * 256, &e); HIP_TRY(e);
  k.U1p = a.put(U1p, (size_t)B * 256, &e); HIP_TRY(e);
  k.U2p = a.put(U2p, (size_t)B * 256, &e); HIP_TRY(e);
  k.Mr = a.put(Mr, mb, &e); HIP_TRY(e);
  k.Ml = a.put(Ml, mb, &e); HIP_TRY(e);
  k.O = a.put(W, wb, &e); HIP_TRY(e);
  k.out = a.put(nullptr, (size_t)B * 16, &e);
  k.B = B; k.m_shared = m_shared ? 1 : 0; k.o_shared = w_shared ? 1 : 0;
  HIP_TRY(qmps::launch_bw(3, k, c->stream));
  HIP_TRY(hipMemcpyAsync(out, k.out, (size_t)B * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_opt_env_objective(qmps_ctx* c, int64_t B, const double* params, const double* h, double k, double* f_out,
                           double* parts_out) try {
  if (int rc = bind(c)) return rc;
  if (B < 0 || !params || !h || !f_out) return fail(QMPS_ERR_ARG, "bad arguments");
  if (int rc = ensure_scratch(c, (size_t)B * (240 + 8 + 32) + 4096)) return rc;
  Arena a{c};
  hipError_t e = hipSuccess;
  const double* d_p = (const double*)a.put(params, (size_t)B * 240, &e); HIP_TRY(e);
  const void* d_h = a.put(h, 256, &e); HIP_TRY(e);
  double* d_f = (double*)a.put(nullptr, (size_t)B * 8, &e);
  double* d_parts = parts_out ? (double*)a.put(nullptr, (size_t)B * 32, &e) : nullptr;
  HIP_TRY(qmps::launch_opt_env(d_p, d_h, k, d_f, d_parts, B, c->stream));
  HIP_TRY(hipMemcpyAsync(f_out, d_f, (size_t)B * 8, hipMemcpyDeviceToHost, c->stream));
  if (parts_out) HIP_TRY(hipMemcpyAsync(parts_out, d_parts, (size_t)B * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH
