// qmps_timeline.hip - tuning builds only (make EXTRA=-DQMPS_WAVE_TIMELINE): the probe behind tools/wave_timeline.py.  With that option
// lane 0 of every wave of energy_direct_d4_kernel stamps its phases into LaneArgs::timeline (qmps_direct.hip, QMPS_TL_STAMP; the words:
// kTimelineWords / kTl* in qmps_kernels.h), and this file exports the call that hands the kernel a buffer and returns the record.  It is
// no part of the C-ABI of include/qmps_hip.h: the shipped library compiles this file to nothing, and the tool binds the symbol by name.
#ifdef QMPS_WAVE_TIMELINE
#include "qmps_ctx.h"

using namespace qmps_host;

// `reps` launches of qmps_energy_launch(B, max_iter, tol, flags) over the window, all on the context stream - flags with QMPS_ENV_DIRECT; with
// QMPS_FLAG_ACCUMULATE_COST each followed by its qmps_cost_launch, as an optimiser step does - every wave stamping into the same
// buffer (the last launch's record stays), HIP events round them all.  words: [(B + 15) / 16][kTimelineWords]; us_per_launch: nullable.
extern "C" int qmps_wave_timeline(qmps_ctx* c, int64_t B, int max_iter, double tol, int flags, int reps, unsigned long long* words,
                                  double* us_per_launch) try {
  if (int rc = bind(c)) return rc;
  if (c->D != 4 || (flags & 0xff) != QMPS_ENV_DIRECT) return fail(QMPS_ERR_ARG, "qmps_wave_timeline: D = 4 with QMPS_ENV_DIRECT only");
  if (B < 1 || reps < 1 || !words) return fail(QMPS_ERR_ARG, "bad arguments");
  const size_t bytes = (size_t)((B + 15) / 16) * qmps::kTimelineWords * sizeof(unsigned long long);
  unsigned long long* d_tl = nullptr;
  HIP_TRY(hipMalloc((void**)&d_tl, bytes));
  int rc = [&]() -> int {
    Restore<unsigned long long*> stamped(c->d_timeline, d_tl);
    HIP_TRY(hipMemsetAsync(d_tl, 0, bytes, c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int rep = 0; rep < reps; ++rep) {
      if (int r = energy_launch(c, B, max_iter, tol, flags, false)) return r;
      if (flags & QMPS_FLAG_ACCUMULATE_COST)
        if (int r = qmps_cost_launch(c, B)) return r;
    }
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (us_per_launch) *us_per_launch = 1e3 * ms / reps;
    HIP_TRY(hipMemcpy(words, d_tl, bytes, hipMemcpyDeviceToHost));
    return QMPS_OK;
  }();
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d_tl);
  return rc;
}
QMPS_API_CATCH
#endif
