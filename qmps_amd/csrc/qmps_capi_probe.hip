// qmps_capi_probe.hip - the peak probes of the C-ABI (declared in include/qmps_hip.h): FP64 vector, FP64 matrix-core and HBM copy
// rates of the context's device, best of five timed launches of the probe kernels in qmps_util.hip.  Context + helpers: qmps_capi.hip,
// qmps_ctx.h.
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
