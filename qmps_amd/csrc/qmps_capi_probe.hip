// qmps_capi_probe.hip - the peak probes of the C-ABI (declared in include/qmps_hip.h): FP64 vector, FP64 matrix-core and HBM copy
// rates of the context's device, best of five timed launches of the probe kernels in qmps_util.hip; and the builder probe
// qmps_ansatz_probe (the tensors the device ansatz builders write, for the tests).  Context + helpers: qmps_capi.hip, qmps_ctx.h.
#include "qmps_ctx.h"

using namespace qmps_host;

// (every entry point below is declared extern "C" in include/qmps_hip.h: the definitions inherit the linkage)

int qmps_probe_fp64_peak(qmps_ctx* c, double* tflops) try {
  if (int rc = bind(c)) return rc;
  if (!tflops) return fail(QMPS_ERR_ARG, "null tflops");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const int blocks = prop.multiProcessorCount * 8;  // 2 waves per SIMD
  const int iters = 20000;
  HIP_TRY(qmps::launch_probe_fp64(c->d_cost, blocks, 200, c->stream));  // warm-up
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(qmps::launch_probe_fp64(c->d_cost, blocks, iters, c->stream));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (ms < best) best = ms;
  }
  const double flops = 2.0 * 16.0 * iters * 256.0 * blocks;
  *tflops = flops / (best * 1e-3) * 1e-12;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_probe_fp64_mfma_peak(qmps_ctx* c, int waves_per_simd, double* tflops) try {
  if (int rc = bind(c)) return rc;
  if (!tflops || waves_per_simd < 1 || waves_per_simd > 8) return fail(QMPS_ERR_ARG, "bad arguments");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const int blocks = prop.multiProcessorCount * waves_per_simd;  // 256 threads = 4 waves = 1 per SIMD
  const int iters = 20000;
  HIP_TRY(qmps::launch_probe_mfma_f64(c->d_cost, blocks, 200, c->stream));
  float best = 1e30f;
  for (int rep = 0; rep < 5; ++rep) {
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(qmps::launch_probe_mfma_f64(c->d_cost, blocks, iters, c->stream));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (ms < best) best = ms;
  }
  const double flops = 4.0 * 2048.0 * iters * 4.0 * blocks;  // 4 MFMAs x 2048 flop, 4 waves per block
  *tflops = flops / (best * 1e-3) * 1e-12;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_probe_hbm_peak(qmps_ctx* c, double* gbps) try {
  if (int rc = bind(c)) return rc;
  if (!gbps) return fail(QMPS_ERR_ARG, "null gbps");
  const size_t bytes = (size_t)1 << 30;  // 1 GiB each way: well past the 256 MiB Infinity Cache
  void *src = nullptr, *dst = nullptr;
  HIP_TRY(hipMalloc(&src, bytes));
  if (hipMalloc(&dst, bytes) != hipSuccess) {
    (void)hipFree(src);
    return fail(QMPS_ERR_HIP, "hipMalloc failed in the HBM probe");
  }
  int rc = [&]() -> int {
    HIP_TRY(hipMemsetAsync(src, 1, bytes, c->stream));
    HIP_TRY(qmps::launch_probe_copy(src, dst, (int64_t)(bytes / 16), c->stream));
    float best = 1e30f;
    for (int rep = 0; rep < 5; ++rep) {
      HIP_TRY(hipEventRecord(c->ev0, c->stream));
      HIP_TRY(qmps::launch_probe_copy(src, dst, (int64_t)(bytes / 16), c->stream));
      HIP_TRY(hipEventRecord(c->ev1, c->stream));
      HIP_TRY(hipEventSynchronize(c->ev1));
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
      if (ms < best) best = ms;
    }
    *gbps = 2.0 * (double)bytes / (best * 1e-3) * 1e-9;
    return QMPS_OK;
  }();
  (void)hipFree(src);
  (void)hipFree(dst);
  return rc;
}
QMPS_API_CATCH

// The device ansatz builders on their own (tests/test_ansatz_gpu.py): the launch_ansatz* call the drivers make, into scratch memory.
// The context's resident states, parameters and flags are not touched.
int qmps_ansatz_probe(qmps_ctx* c, int64_t B, int kind, int n_params, const double* params, int nsh, int index, double fd_h,
                      const unsigned char* active, const double* fill, double* A_out) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  if (B < 1 || !params || !A_out) return fail(QMPS_ERR_ARG, "bad arguments");
  if (int rc = check_ansatz(c, kind, n_params)) return rc;
  const bool fd = fd_h != 0.0;
  if (!(fd_h == fd_h)) return fail(QMPS_ERR_ARG, "fd_h is not a number");
  if (fd ? nsh != 0 : (nsh != 0 && nsh != 3 && nsh != 6)) return fail(QMPS_ERR_ARG, "nsh=%d: 0 (plain or central differences), 3 or 6 (rotosolve shifts)", nsh);
  if (active && !fd) return fail(QMPS_ERR_ARG, "the mask belongs to the central-difference build");
  const int64_t per_row = fd ? 2 * (int64_t)n_params : (nsh > 0 ? nsh : 1);
  if (B % per_row) return fail(QMPS_ERR_ARG, "B=%lld is not a multiple of the %lld evaluations per parameter row", (long long)B, (long long)per_row);
  if (nsh > 0 && (index < 0 || index >= n_params)) return fail(QMPS_ERR_ARG, "index=%d outside [0, n_params=%d)", index, n_params);
  const int64_t rows = B / per_row;
  auto pad = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t pb = (size_t)rows * n_params * sizeof(double), ab = (size_t)B * tensor_bytes(c);
  if (int rc = ensure_scratch(c, pad(pb) + 256 + pad((size_t)rows) + ab)) return rc;
  double* d_p = (double*)c->d_scratch;
  int* d_i = (int*)((char*)c->d_scratch + pad(pb));
  unsigned char* d_m = (unsigned char*)d_i + 256;
  void* d_a = d_m + pad((size_t)rows);
  HIP_TRY(hipMemcpyAsync(d_p, params, pb, hipMemcpyHostToDevice, c->stream));
  if (nsh > 0) HIP_TRY(hipMemcpyAsync(d_i, &index, sizeof(int), hipMemcpyHostToDevice, c->stream));   // (the drivers keep it in HBM: qmps_ctx::roto_idx)
  if (active) HIP_TRY(hipMemcpyAsync(d_m, active, (size_t)rows, hipMemcpyHostToDevice, c->stream));
  std::vector<double> host_fill;
  if (fill) {
    host_fill.resize((size_t)B * 4 * c->D * c->D);
    for (size_t e = 0; e < host_fill.size(); e += 2) { host_fill[e] = fill[0]; host_fill[e + 1] = fill[1]; }
    HIP_TRY(hipMemcpyAsync(d_a, host_fill.data(), ab, hipMemcpyHostToDevice, c->stream));
  }
  if (fd) HIP_TRY(qmps::launch_ansatz_fd(c->D, kind, d_p, n_params, d_a, rows, fd_h, c->stream, active ? d_m : nullptr));
  else if (nsh > 0) HIP_TRY(qmps::launch_ansatz_shifted(c->D, kind, d_p, n_params, d_a, B, nsh, d_i, c->stream));
  else HIP_TRY(qmps::launch_ansatz(c->D, kind, d_p, n_params, d_a, B, c->stream));
  HIP_TRY(hipMemcpyAsync(A_out, d_a, ab, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));      // (also: the pageable host buffers above are done with)
  return QMPS_OK;
}
QMPS_API_CATCH
