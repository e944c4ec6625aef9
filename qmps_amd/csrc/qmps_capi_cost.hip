// qmps_capi_cost.hip - the summed-cost exchange of the C-ABI (declared in include/qmps_hip.h) and its RCCL communicator, in reading
// order: setup_accumulator (an accumulating energy launch claims its ring position), close_group (a group of summed costs goes out
// in ONE all-reduce on a communication stream), the communicator, the plain all-reduces, then qmps_cost_launch / qmps_get_cost.
// The ring, its two communication streams and the fixed-point accumulators live in qmps_ctx (qmps_ctx.h), which also declares the
// two helpers for their callers: the energy paths (qmps_capi_energy.hip) and qmps_sync (qmps_capi.hip).
#include "qmps_ctx.h"

#include <time.h>

using namespace qmps_host;

namespace qmps_host {

// QMPS_FLAG_ACCUMULATE_COST: point the energy kernel at the accumulator of the ring position the following
// qmps_cost_launch will use.  adds = arrivals per term (waves or evaluations that add one word each), per_add =
// evaluations behind one arrival (bounds the partial sum: per_add ||h||_F).
int setup_accumulator(qmps_ctx* c, qmps::LaneArgs& a, int64_t B, int64_t adds, int per_add) {
  // The position the following qmps_cost_launch will use: its accumulator must be clear BEFORE the finish kernel of
  // this step starts to poll it on a communication stream (a stale word of the previous lap carries a full arrival
  // count).  Consecutive ring slots alternate between two communication streams, so every launch clears the same
  // position TWO slots ahead: the finish kernel of this step (same stream as that later slot's) completes only when
  // every wave of this kernel - the clearing one included - has arrived, and the later slot's finish kernel is queued
  // behind it.
  const int slot = (int)(c->groups % qmps_ctx::kCostSlots), pos = c->group_fill;
  const int nslot = (int)((c->groups + 2) % qmps_ctx::kCostSlots), npos = pos;
  c->acc_after_event[slot][pos] = false;
  c->acc_seq[slot][pos] = 0;      // (a launch on the lanes enters itself behind this call: energy_direct_d4)
  if (c->acc_dirty[slot][pos]) {
    // unusual call order (exchange period changed, a partly filled group, an accumulated cost that was dropped): clear
    // it now on the launch's stream, and order this position's finish kernel behind that by an event
    HIP_TRY(hipMemsetAsync(c->acc_at(slot, pos), 0, qmps::kAccWords * sizeof(long long), c->launch_stream));
    c->acc_dirty[slot][pos] = false;
    c->acc_after_event[slot][pos] = true;
  }
  // a slot of the ring is touched again only after its previous exchange has finished.  Asked on the HOST (that
  // exchange, kCostSlots - 2 groups ago, has normally finished long ago): a stream wait would put a barrier packet
  // on the compute stream in every step (+4 us measured), and the compute stream carries no event either
#ifdef QMPS_DEBUG_KNOBS
  static const bool dbg_nohostwait = getenv("QMPS_DBG_NOHOSTWAIT") != nullptr;   // timing dissection only (unsafe slot reuse)
#else
  constexpr bool dbg_nohostwait = false;
#endif
  if (c->comm && !dbg_nohostwait && c->groups + 2 >= qmps_ctx::kCostSlots) {
    c->slot_checks++;
    if (hipEventQuery(c->cost_reduced[nslot]) != hipSuccess) {
      (void)hipGetLastError();
      timespec t0, t1;
      clock_gettime(CLOCK_MONOTONIC, &t0);
      HIP_TRY(hipEventSynchronize(c->cost_reduced[nslot]));
      clock_gettime(CLOCK_MONOTONIC, &t1);
      c->slot_blocks++;
      c->slot_block_ms += (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
    }
  }
  int shards = 32;
  while (shards * (int64_t)qmps::kAccMaxWavesPerShard < adds && shards < qmps::kAccMaxShards) shards *= 2;
  if (shards * (int64_t)qmps::kAccMaxWavesPerShard < adds)
    return fail(QMPS_ERR_ARG, "B=%lld too large for QMPS_FLAG_ACCUMULATE_COST (at most %lld evaluations per launch on this path)", (long long)B,
                (long long)qmps::kAccMaxShards * qmps::kAccMaxWavesPerShard * per_add);
  a.acc = c->acc_at(slot, pos);
  a.acc_zero = c->acc_dirty[nslot][npos] ? c->acc_at(nslot, npos) : nullptr;
  a.acc_shards = shards;
  // partial sums (per_add evaluations each) beyond per_add ||h||_F bypass the fixed-point sum; scale 2^k with bound 2^k <= 2^51
  const double hf = c->h_fro > 1e-300 ? c->h_fro : 1.0;
  a.acc_bound = (double)per_add * hf * (1.0 + 1e-6);
  int k = (int)floor((double)qmps::kAccOffsetBits - 1e-9 - log2(a.acc_bound));
  if (k > 1000) k = 1000;
  if (k < -1000) k = -1000;
  a.acc_scale = ldexp(1.0, k);
  c->acc_shards[slot][pos] = shards;
  c->acc_expect[slot][pos] = adds;
  c->acc_scale[slot][pos] = a.acc_scale;
  c->acc_dirty[slot][pos] = true;
  c->acc_dirty[nslot][npos] = false;
  c->acc_pending = true; c->acc_B = B; c->acc_window = c->window; c->acc_slot = slot; c->acc_pos = pos;
  c->partials_B = -1;
  return QMPS_OK;
}

// close the current group: ONE ncclAllReduce of its `fill` x 16 doubles on the communication stream, ordered after the
// device-side sums by an event, so the exchange overlaps the next steps' kernels instead of stalling the compute stream
int close_group(qmps_ctx* c) {
  if (c->group_fill == 0) return QMPS_OK;
  const int slot = (int)(c->groups % qmps_ctx::kCostSlots);
  double* base = c->d_cost_ring + (size_t)slot * qmps_ctx::kMaxGroup * kMaxTerms;
  if (c->comm) {
#ifdef QMPS_DEBUG_KNOBS   // timing dissections only (they produce WRONG costs): compiled in with -DQMPS_DEBUG_KNOBS, never in the shipped library
    static const bool dbg_noevent = getenv("QMPS_DBG_NOEVENT") != nullptr, dbg_noar = getenv("QMPS_DBG_NOAR") != nullptr,
                      dbg_nofinish = getenv("QMPS_DBG_NOFINISH") != nullptr, dbg_nopoll = getenv("QMPS_DBG_NOPOLL") != nullptr;
#else
    constexpr bool dbg_noevent = false, dbg_noar = false, dbg_nofinish = false, dbg_nopoll = false;
#endif
    // positions whose cost lives in a fixed-point accumulator need no ordering on the compute stream: their finish
    // kernel polls the arrival counts.  Only costs written by reduction kernels on the compute stream need the event - and an
    // accumulator that a memset in front of its launch cleared, unless that launch went to a lane: the finish kernel of such a
    // position waits for the launch's own event, on whichever lane it ran (nothing is put on a compute stream for it).
    bool need_event = false;
    for (int pos = 0; pos < c->group_fill; ++pos)
      need_event = need_event || !c->acc_is[slot][pos] || (c->acc_after_event[slot][pos] && c->acc_seq[slot][pos] == 0);
    if (need_event && !dbg_noevent) {
      HIP_TRY(hipEventRecord(c->cost_ready[slot], c->stream));
      HIP_TRY(hipStreamWaitEvent(c->comm_stream_of(slot), c->cost_ready[slot], 0));
    }
    for (int pos = 0; pos < c->group_fill; ++pos)
      if (c->acc_is[slot][pos]) {   // fixed-point accumulators -> doubles, off the compute stream
        if (c->acc_seq[slot][pos] > 0 && !dbg_noevent)
          if (int rc = lane_wait(c, c->comm_stream_of(slot), c->acc_lane[slot][pos], c->acc_seq[slot][pos])) return rc;
        if (!dbg_nofinish)
          HIP_TRY(qmps::launch_cost_finish(c->acc_at(slot, pos), c->acc_shards[slot][pos], c->acc_expect[slot][pos], dbg_nopoll ? 0 : 1 << 22,
                                           1.0 / c->acc_scale[slot][pos], c->n_terms, base + (size_t)pos * kMaxTerms,
                                           c->d_acc_err, c->comm_stream_of(slot)));
        c->acc_is[slot][pos] = false;
      }
#ifdef QMPS_DEBUG_KNOBS
    // robustness drill for the exchange pipeline at world size 1, where the real all-reduce is instantaneous: a busy kernel in
    // front of it makes every exchange last QMPS_DBG_SLOW_AR probe iterations (~1300 = 40 us, longer than a step), so the ring
    // fills up, the host-side slot guard blocks and the finish kernels queue behind exchanges that are still in flight
    static const int slow_ar = getenv("QMPS_DBG_SLOW_AR") ? atoi(getenv("QMPS_DBG_SLOW_AR")) : 0;
    if (slow_ar > 0) HIP_TRY(qmps::launch_probe_fp64((double*)c->d_work_idx, 1, slow_ar, c->comm_stream_of(slot)));
#endif
    if (!dbg_noar)
      RCCL_TRY(ncclAllReduce(base, base, (size_t)c->group_fill * kMaxTerms, ncclDouble, ncclSum, c->comm_of(slot), c->comm_stream_of(slot)));
    HIP_TRY(hipEventRecord(c->cost_reduced[slot], c->comm_stream_of(slot)));
  }
  c->group_fill = 0;
  c->groups++;
  c->slot_waited = false;
  return QMPS_OK;
}

}  // namespace qmps_host

// (every entry point below is declared extern "C" in include/qmps_hip.h: the definitions inherit the linkage)

int qmps_comm_unique_id(char id[QMPS_UNIQUE_ID_BYTES]) try {
  if (!id) return fail(QMPS_ERR_ARG, "null id");
  static_assert(sizeof(ncclUniqueId) <= QMPS_UNIQUE_ID_BYTES, "ncclUniqueId larger than QMPS_UNIQUE_ID_BYTES");
  ncclUniqueId u;
  RCCL_TRY(ncclGetUniqueId(&u));
  memset(id, 0, QMPS_UNIQUE_ID_BYTES);
  memcpy(id, &u, sizeof(u));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_comm_init(qmps_ctx* c, const char id[QMPS_UNIQUE_ID_BYTES], int rank, int nranks) try {
  if (int rc = bind(c)) return rc;
  if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(QMPS_ERR_ARG, "bad communicator arguments");
  if (c->comm) return fail(QMPS_ERR_STATE, "communicator already initialised");
  ncclUniqueId u;
  memcpy(&u, id, sizeof(u));
  RCCL_TRY(ncclCommInitRank(&c->comm, nranks, u, rank));
  if (!tuning_knob("QMPS_ONE_COMM")) {
    // second communicator over the same ranks (collective, like the init itself); without it everything runs on the first
    ncclResult_t r2 = ncclCommSplit(c->comm, 0, rank, &c->comm2, nullptr);
    if (r2 != ncclSuccess) c->comm2 = nullptr;
    // every rank must take the same decision (slot -> communicator): agree on min over ranks of "I have the second one"
    HIP_TRY(hipStreamSynchronize(c->stream));
    double* flag = c->d_cost;
    const double mine = c->comm2 ? 1.0 : 0.0;
    double all = 0.0;
    HIP_TRY(hipMemcpyAsync(flag, &mine, sizeof(double), hipMemcpyHostToDevice, c->comm_stream));
    RCCL_TRY(ncclAllReduce(flag, flag, 1, ncclDouble, ncclMin, c->comm, c->comm_stream));
    HIP_TRY(hipMemcpyAsync(&all, flag, sizeof(double), hipMemcpyDeviceToHost, c->comm_stream));
    HIP_TRY(hipStreamSynchronize(c->comm_stream));
    if (all < 0.5 && c->comm2) {
      (void)ncclCommDestroy(c->comm2);
      c->comm2 = nullptr;
    }
  }
  c->rank = rank;
  c->nranks = nranks;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_comm_destroy(qmps_ctx* c) try {
  if (int rc = bind(c)) return rc;
  if (c->comm) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->comm_stream));
    HIP_TRY(hipStreamSynchronize(c->comm_stream2));
    if (c->comm2) RCCL_TRY(ncclCommDestroy(c->comm2));
    c->comm2 = nullptr;
    RCCL_TRY(ncclCommDestroy(c->comm));
    c->comm = nullptr;
    c->nranks = 1;
    c->rank = 0;
  }
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_comm_count(qmps_ctx* c, int* nranks) try {
  if (int rc = bind(c)) return rc;
  if (!nranks) return fail(QMPS_ERR_ARG, "null nranks");
  *nranks = 1;
  if (c->comm) RCCL_TRY(ncclCommCount(c->comm, nranks));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_allreduce_sum(qmps_ctx* c, double* inout, int n) try {
  if (int rc = bind(c)) return rc;
  if (!inout || n < 1 || n > kMaxTerms) return fail(QMPS_ERR_ARG, "n=%d outside [1,%d]", n, kMaxTerms);
  if (!c->comm) return fail(QMPS_ERR_STATE, "qmps_comm_init has not been called");
  memcpy(c->h_cost, inout, n * sizeof(double));
  HIP_TRY(hipMemcpyAsync(c->d_cost, c->h_cost, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  RCCL_TRY(ncclAllReduce(c->d_cost, c->d_cost, n, ncclDouble, ncclSum, c->comm, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_cost, c->d_cost, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(inout, c->h_cost, n * sizeof(double));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_allreduce_min(qmps_ctx* c, double* inout, int n) try {
  if (int rc = bind(c)) return rc;
  if (!inout || n < 1 || n > kMaxTerms) return fail(QMPS_ERR_ARG, "n=%d outside [1,%d]", n, kMaxTerms);
  if (!c->comm) return fail(QMPS_ERR_STATE, "qmps_comm_init has not been called");
  memcpy(c->h_cost, inout, n * sizeof(double));
  HIP_TRY(hipMemcpyAsync(c->d_cost, c->h_cost, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  RCCL_TRY(ncclAllReduce(c->d_cost, c->d_cost, n, ncclDouble, ncclMin, c->comm, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_cost, c->d_cost, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(inout, c->h_cost, n * sizeof(double));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_exchange_stats(qmps_ctx* c, int64_t* checks, int64_t* blocked, double* blocked_ms, int reset) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (checks) *checks = c->slot_checks;
  if (blocked) *blocked = c->slot_blocks;
  if (blocked_ms) *blocked_ms = c->slot_block_ms;
  if (reset) { c->slot_checks = 0; c->slot_blocks = 0; c->slot_block_ms = 0.0; }
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_exchange_period(qmps_ctx* c, int steps) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (steps < 1 || steps > qmps_ctx::kMaxGroup) return fail(QMPS_ERR_ARG, "exchange period must be in [1, %d]", qmps_ctx::kMaxGroup);
  if (int rc = bind(c)) return rc;
  if (int rc = close_group(c)) return rc;     // costs summed under the old period are exchanged now
  c->exchange_period = steps;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_cost_launch(qmps_ctx* c, int64_t B) try {
  if (int rc = bind_device(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "no energies resident");
  // device-side sum into this step's place in the current group of the ring (main stream) ...
  const int slot = (int)(c->groups % qmps_ctx::kCostSlots);
  double* dst = c->d_cost_ring + ((size_t)slot * qmps_ctx::kMaxGroup + c->group_fill) * kMaxTerms;
  c->acc_is[slot][c->group_fill] = false;
  const bool in_kernel = c->acc_pending && c->acc_B == B && c->acc_window == c->window && c->acc_slot == slot && c->acc_pos == c->group_fill;
  // A slot is reused only after its previous all-reduce has finished.  Costs written by a reduction kernel on the compute
  // stream need that as a stream dependency; a cost that lives in a fixed-point accumulator is converted on the slot's own
  // communication stream, behind that all-reduce, and puts nothing on the compute stream (no barrier packet per step).
  // A cost the energy kernel summed itself puts nothing on the context stream and reads nothing: the lanes stay apart (close_group
  // orders the finish kernel behind the launch).  A reduction kernel reads E or the partial sums behind both lanes.
  if (!in_kernel)
    if (int rc = join_lanes(c)) return rc;
  if (c->comm && !in_kernel && c->groups >= qmps_ctx::kCostSlots && !c->slot_waited) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->cost_reduced[slot], 0));
    c->slot_waited = true;
  }
  if (in_kernel) {
    // the energy kernel has summed the batch itself (exact fixed-point accumulator): nothing to launch
    c->acc_is[slot][c->group_fill] = true;
  } else if (c->partials_B == B)   // the energy kernel already left per-wave partial sums: only the final pass is needed
    HIP_TRY(qmps::launch_sum_final(c->d_partial, c->partials_n, c->n_terms, dst, c->stream));
  else {
    c->partials_B = -1;   // the generic two-pass reduction reuses d_partial
    HIP_TRY(qmps::launch_sum(win_E(c), B, c->n_terms, c->d_partial, kSumBlocks, dst, c->stream));
  }
  c->acc_pending = false;
  c->last_slot = slot;
  c->last_pos = c->group_fill;
  c->group_fill++;
  c->cost_launches++;
  // ... then, once per `exchange_period` steps, the exchange step
  if (c->group_fill >= c->exchange_period)
    if (int rc = close_group(c)) return rc;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_cost(qmps_ctx* c, double* cost) try {
  if (int rc = bind(c)) return rc;
  if (!cost) return fail(QMPS_ERR_ARG, "null cost");
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "no energies resident");
  if (c->cost_launches < 1) return fail(QMPS_ERR_STATE, "qmps_cost_launch has not been called");
  if (int rc = close_group(c)) return rc;     // a partly filled group is exchanged now
  hipStream_t st = c->comm ? c->comm_stream_of(c->last_slot) : c->stream;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->acc_is[c->last_slot][c->last_pos]) {
    // no communicator: the cost still lives in its fixed-point accumulator; sum the shards on the host (exact)
    HIP_TRY(hipMemcpyAsync(c->h_acc, c->acc_at(c->last_slot, c->last_pos), qmps::kAccWords * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double inv = 1.0 / c->acc_scale[c->last_slot][c->last_pos];
    for (int t = 0; t < c->n_terms; ++t) {
      long long cnt = 0, hi = 0, lo = 0;
      for (int sh = 0; sh < c->acc_shards[c->last_slot][c->last_pos]; ++sh) {
        long long k, v;
        qmps::acc_decode(c->h_acc[t * qmps::kAccMaxShards + sh], k, v);
        cnt += k;
        hi += v >> 20;
        lo += v & 0xFFFFF;
      }
      if (cnt != c->acc_expect[c->last_slot][c->last_pos])
        return fail(QMPS_ERR_STATE, "cost accumulator: %lld of %lld waves arrived", cnt, c->acc_expect[c->last_slot][c->last_pos]);
      cost[t] = ((double)hi * 1048576.0 + (double)lo) * inv + ((const double*)(c->h_acc + qmps::kAccOver))[t];
    }
    return QMPS_OK;
  }
  HIP_TRY(hipMemcpyAsync(c->h_cost, c->d_cost_ring + ((size_t)c->last_slot * qmps_ctx::kMaxGroup + c->last_pos) * kMaxTerms,
                         c->n_terms * sizeof(double), hipMemcpyDeviceToHost, st));
  int acc_err = 0;
  if (c->comm) HIP_TRY(hipMemcpyAsync(&acc_err, c->d_acc_err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (acc_err) {
    // a finish kernel gave up waiting for its energy kernel's waves (bounded poll): the cost it wrote is NaN
    (void)hipMemsetAsync(c->d_acc_err, 0, sizeof(int), st);
    return fail(QMPS_ERR_STATE, "cost accumulator: a step's energy kernel did not arrive within the polling bound (was it launched?)");
  }
  memcpy(cost, c->h_cost, c->n_terms * sizeof(double));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_allreduce_cost(qmps_ctx* c, int64_t B, double* cost) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!c->comm) return fail(QMPS_ERR_STATE, "qmps_comm_init has not been called");
  if (int rc = qmps_cost_launch(c, B)) return rc;
  return qmps_get_cost(c, cost);
}
QMPS_API_CATCH
