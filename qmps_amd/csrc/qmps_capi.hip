// qmps_capi.hip - the context of the C-ABI of libqmps_hip.so (declared in include/qmps_hip.h): the error string, library / device
// queries, the qmps_host helpers behind qmps_ctx.h (bind and the launch lanes among them), context lifetime (one device + one HIP stream
// + HBM buffers + pinned staging),
// the state, Hamiltonian, window and guess setters, the solver / handoff / roto-rule / timing-period settings, timers.
// The energy path and read-back: qmps_capi_energy.hip; the summed-cost exchange (RCCL): qmps_capi_cost.hip; the brick-wall calls:
// qmps_capi_brickwall.hip; the peak probes: qmps_capi_probe.hip; the time-evolution overlap objective: qmps_capi_overlap.hip; the
// evolve drivers: qmps_capi_evolve.hip; the rotosolve drivers: qmps_capi_roto.hip.
#include "qmps_ctx.h"
#include "qmps_direct_core.h"

using namespace qmps_host;

namespace {
thread_local char g_err[512] = "";
}  // namespace

namespace qmps_host {

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int bind_device(qmps_ctx* c) {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  HIP_TRY(hipSetDevice(c->device));
  return QMPS_OK;
}

int bind(qmps_ctx* c) {
  if (int rc = bind_device(c)) return rc;
  return join_lanes(c);
}

// The launch lanes (qmps_ctx.h, qmps_hazard.h).  Waiting for an event that has completed puts nothing on the stream.
int lane_wait(qmps_ctx* c, hipStream_t waiter, int lane, int64_t seq) {
  if (seq < 1) return QMPS_OK;
  if (c->lane_table.kept(lane, seq)) {
    HIP_TRY(hipStreamWaitEvent(waiter, c->lane_ev[lane][LaneTable::slot_of(seq)], 0));
  } else {      // its event has been taken over by a later launch of the lane: wait for the lane as it stands
    HIP_TRY(hipEventRecord(c->lane_fork, c->lane(lane)));
    HIP_TRY(hipStreamWaitEvent(waiter, c->lane_fork, 0));
  }
  return QMPS_OK;
}

namespace {
// what lanes_begin / lanes_join (qmps_hazard.h) ask for, on the context's streams
struct LaneIO {
  qmps_ctx* c;
  int wait(int waiter, int lane, int64_t seq) { return lane_wait(c, c->lane(waiter), lane, seq); }
  int fork() {
    HIP_TRY(hipEventRecord(c->lane_fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->lane_stream, c->lane_fork, 0));
    return QMPS_OK;
  }
};
}  // namespace

int join_lanes(qmps_ctx* c) {
  if (c->capturing) return QMPS_OK;      // (the drivers that capture have bound, and issue no lane launches)
  LaneIO io{c};
  return lanes_join(c->lane_table, io, c->main_touched);
}

int lane_begin(qmps_ctx* c, const LaunchFootprint& f, int* lane_out) {
  if (!c->lane_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&c->lane_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->lane_fork, hipEventDisableTiming));
    for (auto& lane : c->lane_ev)
      for (hipEvent_t& e : lane) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  const int lane = c->next_lane;
  c->next_lane = 1 - lane;
  LaneIO io{c};
  if (int rc = lanes_begin(c->lane_table, io, lane, f, c->main_touched)) return rc;
  *lane_out = lane;
  return QMPS_OK;
}

int lane_end(qmps_ctx* c, const LaunchFootprint& f, int lane, int64_t* seq) {
  *seq = c->lane_table.record(lane, f);
  HIP_TRY(hipEventRecord(c->lane_ev[lane][LaneTable::slot_of(*seq)], c->lane(lane)));
  return QMPS_OK;
}

int check_B(const qmps_ctx* c, int64_t B) {
  if (B < 0 || B > c->max_batch) return fail(QMPS_ERR_ARG, "B=%lld outside [0, max_batch=%lld]", (long long)B, (long long)c->max_batch);
  return QMPS_OK;
}

// launch / read-back calls: the window [window, window + B) must lie inside the buffers
int check_window(const qmps_ctx* c, int64_t B) {
  if (B < 0 || c->window + B > c->max_batch)
    return fail(QMPS_ERR_ARG, "window [%lld, %lld) outside [0, max_batch=%lld]", (long long)c->window, (long long)(c->window + B), (long long)c->max_batch);
  return QMPS_OK;
}

int check_resident(const qmps_ctx* c, int64_t B) {
  if (c->window + B > c->states.count)
    return fail(QMPS_ERR_STATE, "window [%lld, %lld) but only %lld states are resident", (long long)c->window, (long long)(c->window + B), (long long)c->states.count);
  return QMPS_OK;
}

// kinds the D = 4 direct kernel builds in front of the solve (three-qubit circuits with a per-layer gate list)
bool fusable_ansatz(const qmps_ctx* c, int kind) {
  static const bool off = documented_switch("QMPS_NO_FUSED_ANSATZ") != nullptr;   // A/B knob
  return !off && c->D == 4 && (kind == QMPS_ANSATZ_SHALLOW_CNOT || kind == QMPS_ANSATZ_SHALLOW_QAOA || kind == QMPS_ANSATZ_SHALLOW_CNOT3);
}

int ensure_pinned(qmps_ctx* c, size_t bytes) {
  if (bytes > c->h_pin_bytes) {
    // growth: a staged copy kernel of an earlier call may still be reading the old buffer, and a staged upload may be waiting in
    // it - drain the device, carry the contents over, then free (offsets into the buffer stay valid; nothing keeps raw pointers)
    const size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    char* fresh = nullptr;
    HIP_TRY(hipHostMalloc((void**)&fresh, want, hipHostMallocDefault));
    if (c->h_pin) {
      const hipError_t se = hipDeviceSynchronize();
      if (se != hipSuccess) { (void)hipHostFree(fresh); HIP_TRY(se); }
      memcpy(fresh, c->h_pin, c->h_pin_bytes);
      (void)hipHostFree(c->h_pin);
    }
    c->h_pin = fresh;
    c->h_pin_bytes = want;
  }
  return QMPS_OK;
}

// (kind, n_params) of an ansatz the device builders know (qmps/represent.py:268-404)
int check_ansatz(const qmps_ctx* c, int kind, int n_params) {
  if (n_params < 1 || n_params > 4096) return fail(QMPS_ERR_ARG, "n_params=%d outside [1,4096]", n_params);
  if (kind < 0 || kind > 6) return fail(QMPS_ERR_ARG, "unknown ansatz kind %d", kind);
  if (kind == QMPS_ANSATZ_SHALLOW_FULL && (c->D != 2 || n_params != 15))
    return fail(QMPS_ERR_ARG, "ShallowFullStateTensor is a two-qubit gate: D = 2, 15 parameters");
  if (kind == QMPS_ANSATZ_STATE_GATE && (c->D != 2 || n_params < 6))
    return fail(QMPS_ERR_ARG, "StateGate is a two-qubit gate: D = 2, 6 parameters");
  if (kind == QMPS_ANSATZ_EXACT_AFTER4 && n_params % 6) return fail(QMPS_ERR_ARG, "ExactAfter4 takes six angles per layer");
  if (kind == QMPS_ANSATZ_SHALLOW_CNOT_NONUNIFORM) {
    int nq = 1;
    while ((1 << (nq - 1)) < c->D) ++nq;      // n + 1 qubits
    if (n_params % (2 * nq)) return fail(QMPS_ERR_ARG, "ShallowCNOTStateTensor_nonuniform takes %d angles per layer at D = %d", 2 * nq, c->D);
  }
  if ((kind == QMPS_ANSATZ_SHALLOW_CNOT || kind == QMPS_ANSATZ_SHALLOW_QAOA) && n_params % 2)
    return fail(QMPS_ERR_ARG, "this ansatz takes (beta, gamma) pairs");
  if (kind == QMPS_ANSATZ_SHALLOW_CNOT3 && n_params % 3) return fail(QMPS_ERR_ARG, "this ansatz takes (beta, gamma, omega) triples");
  return QMPS_OK;
}

// d_A <- tensors of the resident ansatz parameters, if nothing has built them yet
int ensure_tensors(qmps_ctx* c) {
  const ResidentStates& s = c->states;
  if (s.has_tensors) return QMPS_OK;
  if (!s.ansatz || s.shifts != 0) return fail(QMPS_ERR_STATE, "no resident states");
  HIP_TRY(qmps::launch_ansatz(c->D, s.kind, s.borrowed() ? s.rows : c->d_params, s.P, c->d_A, s.count, c->stream));
  c->states.tensors_built();
  return QMPS_OK;
}

}  // namespace qmps_host

extern "C" {

int qmps_abi_version(void) { return QMPS_ABI_VERSION; }
int qmps_abi_minor(void) { return QMPS_ABI_MINOR; }

const char* qmps_last_error(void) { return g_err; }

// test hook for the "nothing throws across the ABI" contract (tests/test_cabi.py; needs no device): raises the exception a host
// allocation of absurd size would raise, inside the same function-try-block every other entry point has
int qmps_selftest_exception(int kind) try {
  if (kind == 1) throw std::bad_alloc();
  if (kind == 2) { std::vector<double> v; v.resize(v.max_size() + 1); return (int)v.size(); }     // std::length_error
  if (kind == 3) throw 42;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_device_count(int* count) try {
  if (!count) return fail(QMPS_ERR_ARG, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    n = 0;
  }
  *count = n;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_device_info(int device, char* name, int name_len, char* arch, int arch_len, int* compute_units,
                     int64_t* hbm_bytes) try {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (name && name_len > 0) snprintf(name, name_len, "%s", prop.name);
  if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", prop.gcnArchName);
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_create(int device, int D, int64_t max_batch, qmps_ctx** out) try {
  if (!out) return fail(QMPS_ERR_ARG, "null out");
  *out = nullptr;
  if (D != 2 && D != 4 && D != 8 && D != 16) return fail(QMPS_ERR_ARG, "bond dimension D=%d not in {2,4,8,16}", D);
  if (max_batch < 1) return fail(QMPS_ERR_ARG, "max_batch must be >= 1");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return fail(QMPS_ERR_NO_DEVICE, "no HIP device visible: libqmps_hip has no CPU fallback");
  }
  if (device < 0 || device >= n) return fail(QMPS_ERR_ARG, "device %d outside [0,%d)", device, n);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(QMPS_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device,
                prop.gcnArchName);
  qmps_ctx* c = new (std::nothrow) qmps_ctx();
  if (!c) return fail(QMPS_ERR_ARG, "out of host memory");
  c->device = device;
  c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->D = D;
  c->max_batch = max_batch;
  int rc = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->launch_stream = c->stream;
    c->lanes = qmps::launch_lanes();
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    for (int i = 0; i < qmps_ctx::kRing; ++i) {
      HIP_TRY(hipEventCreate(&c->kev0[i]));
      HIP_TRY(hipEventCreate(&c->kev1[i]));
    }
    HIP_TRY(hipMalloc(&c->d_A, (size_t)max_batch * tensor_bytes(c)));
    HIP_TRY(hipMalloc(&c->d_r, (size_t)max_batch * env_bytes(c)));
    HIP_TRY(hipMalloc(&c->d_h, (size_t)kMaxTerms * 256));
    HIP_TRY(hipMalloc((void**)&c->d_iters, (size_t)(max_batch + 2) * sizeof(int32_t)));     // (+ 2: read in 8-byte units by the staging copy)
    HIP_TRY(hipMalloc((void**)&c->d_status, (size_t)(max_batch + 2) * sizeof(int32_t)));
    c->partial_cap = (max_batch + 15) / 16 > kSumBlocks ? (max_batch + 15) / 16 : kSumBlocks;   // one partial per 16 (direct kernel), 32 (pair kernel) or 64 items
    HIP_TRY(hipMalloc((void**)&c->d_partial, (size_t)kMaxTerms * c->partial_cap * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->d_cost, kMaxTerms * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&c->d_cost_ring, (size_t)qmps_ctx::kCostSlots * qmps_ctx::kMaxGroup * kMaxTerms * sizeof(double)));
    HIP_TRY(hipMemsetAsync(c->d_cost_ring, 0, (size_t)qmps_ctx::kCostSlots * qmps_ctx::kMaxGroup * kMaxTerms * sizeof(double), c->stream));
    HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream2, hipStreamNonBlocking));
    for (int i = 0; i < qmps_ctx::kCostSlots; ++i) {
      HIP_TRY(hipEventCreateWithFlags(&c->cost_ready[i], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&c->cost_reduced[i], hipEventDisableTiming));
    }
    HIP_TRY(hipHostMalloc((void**)&c->h_cost, kMaxTerms * sizeof(double), hipHostMallocDefault));
    const size_t acc_bytes = (size_t)qmps_ctx::kCostSlots * qmps_ctx::kMaxGroup * qmps::kAccWords * sizeof(long long);
    HIP_TRY(hipMalloc((void**)&c->d_acc, acc_bytes));
    HIP_TRY(hipMemsetAsync(c->d_acc, 0, acc_bytes, c->stream));
    HIP_TRY(hipHostMalloc((void**)&c->h_acc, qmps::kAccWords * sizeof(long long), hipHostMallocDefault));
    HIP_TRY(hipMalloc((void**)&c->d_acc_err, sizeof(int)));
    HIP_TRY(hipMemsetAsync(c->d_acc_err, 0, sizeof(int), c->stream));
    // work counters of the overlap queue, the Krylov fall-backs and env_power_d4_kernel (qmps_ctx::QueueSlot) - allocated here,
    // never at a launch (a launch may sit inside a stream capture); the Krylov counters clear themselves after use, the others are
    // cleared in front of their launch
    HIP_TRY(hipMalloc((void**)&c->d_queue, qmps_ctx::kQueueInts * sizeof(int)));
    HIP_TRY(hipMemsetAsync(c->d_queue, 0, qmps_ctx::kQueueInts * sizeof(int), c->stream));
    HIP_TRY(hipMalloc((void**)&c->d_work_count, sizeof(int32_t)));
    HIP_TRY(hipMalloc((void**)&c->d_work_idx, (size_t)max_batch * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(c->d_work_count, 0, sizeof(int32_t), c->stream));
    c->handoff = 0;   // D = 2, 4: squaring from the start (fastest); D = 8, 16 have no squaring path
    c->default_solver = (D == 2 || D == 4 || D == 8) ? QMPS_ENV_DIRECT : QMPS_ENV_POWER_SQUARING;
    c->skip_rounds = (D == 2) ? QMPS_SKIP_ROUNDS_D2 : QMPS_SKIP_ROUNDS_D4;
    if (const char* e = tuning_knob("QMPS_SKIP_ROUNDS")) c->skip_rounds = atoi(e);   // tuning knob
    if (const char* e = tuning_knob("QMPS_MATVEC_PERIOD")) c->matvec_period = atoi(e);   // tuning knob
    c->no_pair = tuning_knob("QMPS_NO_PAIR") != nullptr;
    c->pair_in_step = tuning_knob("QMPS_LANE_IN_STEP") == nullptr;
    return QMPS_OK;
  }();
  if (rc != QMPS_OK) {
    char keep[512];
    snprintf(keep, sizeof(keep), "%s", g_err);
    qmps_destroy(c);
    snprintf(g_err, sizeof(g_err), "%s", keep);
    return rc;
  }
  *out = c;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_destroy(qmps_ctx* c) try {
  if (!c) return QMPS_OK;
  (void)hipSetDevice(c->device);
  for (qmps_ctx* g : c->lockstep) (void)qmps_destroy(g);        // (lock-step groups of qmps_evolve_bfgs)
  c->lockstep.clear();
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->lane_stream) (void)hipStreamSynchronize(c->lane_stream);
  if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
  if (c->comm_stream2) (void)hipStreamSynchronize(c->comm_stream2);
  if (c->roto_exec) (void)hipGraphExecDestroy(c->roto_exec);
  if (c->roto_graph) (void)hipGraphDestroy(c->roto_graph);
  if (c->comm2) (void)ncclCommDestroy(c->comm2);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  for (int i = 0; i < qmps_ctx::kCostSlots; ++i) {
    if (c->cost_ready[i]) (void)hipEventDestroy(c->cost_ready[i]);
    if (c->cost_reduced[i]) (void)hipEventDestroy(c->cost_reduced[i]);
  }
  if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
  for (hipEvent_t e : c->active_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->aux_fork) (void)hipEventDestroy(c->aux_fork);
  if (c->aux_join) (void)hipEventDestroy(c->aux_join);
  if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
  if (c->comm_stream2) (void)hipStreamDestroy(c->comm_stream2);
  void* bufs[] = {c->d_A, c->d_U, c->d_U2, c->d_params, c->d_ww, c->d_eta, c->d_ref, c->d_f, c->d_ostats, c->d_xwarm, c->d_y, c->d_queue, c->d_kry, c->d_active, c->d_scratch, c->d_h, c->d_r, c->d_rho, c->d_E, c->d_iters, c->d_status, c->d_partial, c->d_cost, c->d_cost_ring, c->d_work_count, c->d_work_idx, c->d_acc, c->d_acc_err, c->roto_base, c->roto_hist, c->roto_idx};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (c->h_cost) (void)hipHostFree(c->h_cost);
  if (c->h_pin) (void)hipHostFree(c->h_pin);
  if (c->h_mask) (void)hipHostFree(c->h_mask);
  if (c->d_lock) (void)hipFree(c->d_lock);
  if (c->h_ctl) (void)hipHostFree(c->h_ctl);
  if (c->step_ev0) (void)hipEventDestroy(c->step_ev0);
  if (c->step_ev1) (void)hipEventDestroy(c->step_ev1);
  if (c->d_tolarr) (void)hipFree(c->d_tolarr);
  if (c->h_acc) (void)hipHostFree(c->h_acc);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  for (int i = 0; i < qmps_ctx::kRing; ++i) {
    if (c->kev0[i]) (void)hipEventDestroy(c->kev0[i]);
    if (c->kev1[i]) (void)hipEventDestroy(c->kev1[i]);
  }
  for (auto& lane : c->lane_ev)
    for (hipEvent_t e : lane)
      if (e) (void)hipEventDestroy(e);
  if (c->lane_fork) (void)hipEventDestroy(c->lane_fork);
  if (c->lane_stream) (void)hipStreamDestroy(c->lane_stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_sync(qmps_ctx* c) try {
  if (int rc = bind(c)) return rc;
  if (int rc = close_group(c)) return rc;     // costs still waiting for their exchange go out now
  HIP_TRY(hipStreamSynchronize(c->stream));      // (behind lane 1 since bind)
  HIP_TRY(hipStreamSynchronize(c->comm_stream));
  HIP_TRY(hipStreamSynchronize(c->comm_stream2));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_states(qmps_ctx* c, int64_t B, const double* states, int kind) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  if (!states && B > 0) return fail(QMPS_ERR_ARG, "null states");
  if (kind == QMPS_INPUT_TENSOR) {
    HIP_TRY(hipMemcpyAsync(c->d_A, states, (size_t)B * tensor_bytes(c), hipMemcpyHostToDevice, c->stream));
  } else if (kind == QMPS_INPUT_UNITARY) {
    if (!c->d_U) HIP_TRY(hipMalloc(&c->d_U, (size_t)c->max_batch * 2 * tensor_bytes(c)));
    HIP_TRY(hipMemcpyAsync(c->d_U, states, (size_t)B * 2 * tensor_bytes(c), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(qmps::launch_unitary_to_tensor(c->d_U, c->d_A, c->D, B, c->stream));
  } else {
    return fail(QMPS_ERR_ARG, "unknown input kind %d", kind);
  }
  // the caller's host buffer may be pageable and re-used right after the call returns
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->states.hold_tensors(B);
  c->window = 0;
  c->have_guess = false;
  forget_results(c);
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_window(qmps_ctx* c, int64_t first) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (first < 0 || first > c->states.count) return fail(QMPS_ERR_ARG, "window start %lld outside the %lld resident states", (long long)first, (long long)c->states.count);
  c->window = first;
  c->partials_B = -1;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_states_ansatz(qmps_ctx* c, int64_t B, int kind, int n_params, const double* params) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  if (!params && B > 0) return fail(QMPS_ERR_ARG, "null params");
  if (int rc = check_ansatz(c, kind, n_params)) return rc;
  if (int rc = ensure_params(c, n_params)) return rc;
  {
    const size_t pb = (size_t)B * n_params * sizeof(double);
    if (c->defer_sync && pb <= (8u << 20)) {
      // one-round-trip callers: through pinned memory, moved by a kernel on the context stream (no copy-queue hop)
      if (int rc = ensure_pinned(c, (16u << 20))) return rc;
      memcpy(c->h_pin, params, pb);
      if (c->mask_stash_n > 0) {         // a mask of qmps_overlap_set_active waiting in its staging slot rides along
        const int64_t n = c->mask_stash_n;
        c->mask_stash_n = 0;
        HIP_TRY(qmps::launch_stage_copy2(c->h_pin, c->d_params, (int64_t)(pb / 8), c->mask_stash, c->d_active, (n + 7) / 8, c->stream));
      } else {
        HIP_TRY(qmps::launch_stage_copy(c->h_pin, c->d_params, (int64_t)(pb / 8), c->stream));
      }
    } else {
      HIP_TRY(hipMemcpyAsync(c->d_params, params, pb, hipMemcpyHostToDevice, c->stream));
    }
    if (c->fork_after_copy) {            // qmps_overlap_gradient: its second stream needs the parameters only
      HIP_TRY(hipEventRecord(c->fork_after_copy, c->stream));
      c->fork_after_copy = nullptr;
    }
  }
  c->states.hold_ansatz(B, kind, n_params);
  // D = 4: the direct kernel builds the tensors itself (8 P bytes per evaluation instead of 512); d_A is filled on demand
  if (!fusable_ansatz(c, kind))
    if (int rc = ensure_tensors(c)) return rc;
  if (!c->defer_sync) HIP_TRY(hipStreamSynchronize(c->stream));
  c->window = 0;
  c->have_guess = false;
  forget_results(c);
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_states_su(qmps_ctx* c, int64_t B, const double* params) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  if (!params && B > 0) return fail(QMPS_ERR_ARG, "null params");
  const int N = 2 * c->D, np_ = N * N - 1;
  if (int rc = ensure_params(c, np_)) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_params, params, (size_t)B * np_ * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(qmps::launch_su_exp(N, c->d_params, B, np_, c->d_A, 1, c->stream));
  if (!c->defer_sync) HIP_TRY(hipStreamSynchronize(c->stream));
  c->states.hold_tensors(B);
  c->window = 0;
  c->have_guess = false;
  forget_results(c);
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_su_unitaries(qmps_ctx* c, int64_t B, int N, const double* params, double* U_out) try {
  if (int rc = bind(c)) return rc;
  if (B < 0 || !params || !U_out) return fail(QMPS_ERR_ARG, "bad arguments");
  if (N != 4 && N != 8 && N != 16 && N != 32) return fail(QMPS_ERR_ARG, "N=%d not in {4, 8, 16, 32}", N);
  const size_t pb = (size_t)B * (N * N - 1) * sizeof(double), ub = (size_t)B * N * N * 16;
  if (int rc = ensure_scratch(c, ((pb + 255) & ~(size_t)255) + ub + 256)) return rc;
  double* d_p = (double*)c->d_scratch;
  void* d_u = (char*)c->d_scratch + ((pb + 255) & ~(size_t)255);
  HIP_TRY(hipMemcpyAsync(d_p, params, pb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(qmps::launch_su_exp(N, d_p, B, N * N - 1, d_u, 0, c->stream));
  HIP_TRY(hipMemcpyAsync(U_out, d_u, ub, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_states(qmps_ctx* c, int64_t B, double* A) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  if (!A) return fail(QMPS_ERR_ARG, "null A");
  if (B > c->states.count) return fail(QMPS_ERR_STATE, "only %lld states are resident", (long long)c->states.count);
  if (int rc = ensure_tensors(c)) return rc;
  HIP_TRY(hipMemcpyAsync(A, c->d_A, (size_t)B * tensor_bytes(c), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_hamiltonian(qmps_ctx* c, int n_terms, const double* h) try {
  if (int rc = bind(c)) return rc;
  if (n_terms < 1 || n_terms > kMaxTerms) return fail(QMPS_ERR_ARG, "n_terms=%d outside [1,%d]", n_terms, kMaxTerms);
  if (!h) return fail(QMPS_ERR_ARG, "null h");
  if (int rc = ensure_E(c, n_terms)) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_h, h, (size_t)n_terms * 256, hipMemcpyHostToDevice, c->stream));
  if (!c->defer_sync) HIP_TRY(hipStreamSynchronize(c->stream));
  c->h_fro = 0.0;
  for (int t = 0; t < n_terms; ++t) {
    double f = 0.0;
    for (int i = 0; i < 32; ++i) f += h[32 * t + i] * h[32 * t + i];
    f = sqrt(f);
    if (f > c->h_fro) c->h_fro = f;
  }
  c->rho_need = qmps::rho_need_mask(h, n_terms);
  if (n_terms != c->n_terms) {
    // The in-kernel clear of a cost accumulator covers the CURRENT number of terms only: after a change of that number a slot that counts as clean
    // may still hold the arrivals of a term it was last used with ("cost accumulator: 46 of 23 waves arrived" on the first accumulating launch after
    // going from one Hamiltonian term to two; found by profiles/experiments/r05/stress_api_state.py, round 5).  Every position of the ring is marked
    // dirty: setup_accumulator clears a dirty position completely before it is used.
    for (int sl = 0; sl < qmps_ctx::kCostSlots; ++sl)
      for (int ps = 0; ps < qmps_ctx::kMaxGroup; ++ps) c->acc_dirty[sl][ps] = true;
  }
  if (n_terms != c->n_terms) c->energies.clear();     // d_E is laid out [evaluation][term]: the resident rows no longer line up
  c->n_terms = n_terms;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_env_guess(qmps_ctx* c, int64_t B, const double* r0) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  c->window = 0;
  if (!r0) {
    c->have_guess = false;
    return QMPS_OK;
  }
  HIP_TRY(hipMemcpyAsync(c->d_r, r0, (size_t)B * env_bytes(c), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->have_guess = true;
  c->env.add(0, B);
  c->env_guessed.add(0, B);
  c->env_start.add(0, B);
  c->have_overlap_x = false;
  c->grad_warm_T = 0;          // d_r no longer holds the right fixed points of a gradient batch
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_kernel_timing_period(qmps_ctx* c, int period) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (period < 0) return fail(QMPS_ERR_ARG, "period must be >= 0");
  c->timing_period = period;
  c->samples = 0;          // earlier samples belong to another schedule
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_handoff(qmps_ctx* c, int handoff) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (handoff < 0) return fail(QMPS_ERR_ARG, "handoff must be >= 0");
  c->handoff = handoff;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_default_solver(qmps_ctx* c, int solver) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (solver != QMPS_ENV_POWER && solver != QMPS_ENV_POWER_SQUARING && solver != QMPS_ENV_DIRECT)
    return fail(QMPS_ERR_ARG, "unknown solver %d", solver);
  c->default_solver = solver;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_set_roto_rule(qmps_ctx* c, int rule) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (rule != QMPS_ROTO_REFERENCE && rule != QMPS_ROTO_GLOBAL_ARGMIN) return fail(QMPS_ERR_ARG, "unknown rotosolve rule %d", rule);
  c->roto_rule = rule;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_roto_rule_probe(qmps_ctx* c, int64_t n, const double* abcd, int rule, double* theta) try {
  if (int rc = bind(c)) return rc;
  if (!abcd || !theta || n < 1 || n > (1 << 24)) return fail(QMPS_ERR_ARG, "bad arguments");
  if (rule != QMPS_ROTO_REFERENCE && rule != QMPS_ROTO_GLOBAL_ARGMIN) return fail(QMPS_ERR_ARG, "unknown rotosolve rule %d", rule);
  if (int rc = ensure_scratch(c, (size_t)n * 5 * sizeof(double))) return rc;
  double* d_in = (double*)c->d_scratch;
  double* d_out = d_in + 4 * n;
  HIP_TRY(hipMemcpyAsync(d_in, abcd, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(qmps::launch_roto_rule_probe(d_in, n, rule, d_out, c->stream));
  HIP_TRY(hipMemcpyAsync(theta, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_roto_rule(qmps_ctx* c, int* rule) try {
  if (!c || !rule) return fail(QMPS_ERR_ARG, "null argument");
  *rule = c->roto_rule;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_handoff(qmps_ctx* c, int* handoff) try {
  if (!c || !handoff) return fail(QMPS_ERR_ARG, "null argument");
  *handoff = c->handoff;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_squaring_schedule(qmps_ctx* c, int* skip_rounds, int* matvec_period) try {
  if (!c || !skip_rounds || !matvec_period) return fail(QMPS_ERR_ARG, "null argument");
  *skip_rounds = c->skip_rounds;
  *matvec_period = c->D == 4 ? c->matvec_period : 0;
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_kernel_time(qmps_ctx* c, int n_last, float* avg_ms, char* name, int name_len) try {
  if (int rc = bind(c)) return rc;
  if (!avg_ms || n_last < 1) return fail(QMPS_ERR_ARG, "bad arguments");
  if (c->samples < 1) return fail(QMPS_ERR_STATE, "no timed energy launch yet (qmps_set_kernel_timing_period)");
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the timed launches among the last n_last ones
  int64_t n = c->timing_period > 0 ? (n_last + c->timing_period - 1) / c->timing_period : 1;
  if (n < 1) n = 1;
  if (n > c->samples) n = c->samples;
  if (n > qmps_ctx::kRing) n = qmps_ctx::kRing;
  double sum = 0.0;
  for (int64_t k = 0; k < n; ++k) {
    const int slot = (int)((c->samples - 1 - k) % qmps_ctx::kRing);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->kev0[slot], c->kev1[slot]));
    sum += ms;
  }
  *avg_ms = (float)(sum / (double)n);
  if (name && name_len > 0) snprintf(name, name_len, "%s", c->dominant);
  return QMPS_OK;
}
QMPS_API_CATCH

// Both events stand on the context stream behind a join of the lanes (bind), and lane 1 starts nothing new before the first of them
// (main_touched): the interval covers the work of both lanes issued between the two calls, and none from before.
int qmps_timer_begin(qmps_ctx* c) try {
  if (int rc = bind(c)) return rc;
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_timer_end(qmps_ctx* c, float* ms) try {
  if (int rc = bind(c)) return rc;
  if (!ms) return fail(QMPS_ERR_ARG, "null ms");
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return QMPS_OK;
}
QMPS_API_CATCH

}  // extern "C"
