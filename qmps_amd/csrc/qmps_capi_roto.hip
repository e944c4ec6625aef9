// qmps_capi_roto.hip - the rotosolve drivers of the C-ABI (declared in include/qmps_hip.h): qmps_rotosolve / qmps_double_rotosolve on the
// energy (a function per path: the whole-run kernels of D = 2 and D = 8, the step-by-step path with its cached sweep graph) and
// qmps_evolve_rotosolve on the time-evolution overlap objective, on the same work buffers and sweep-graph plumbing.  The launches they
// enqueue: qmps_capi_energy.hip, qmps_capi_overlap.hip (the overlap launches on the kernel route of the call: overlap_route); the BFGS evolve drivers: qmps_capi_evolve.hip; context + helpers: qmps_capi.hip,
// qmps_ctx.h.
#include "qmps_ctx.h"
#include "qmps_overlap_internal.h"

using namespace qmps_host;

namespace {

#ifdef QMPS_D8_PROFILE        // scratch instrumentation build (profiles/experiments/scratch/d8_profile.py): 16 phase clocks behind the history
constexpr size_t kHistExtra = 16 + 3 * 4096;
#else
constexpr size_t kHistExtra = 0;
#endif

// The constants of one run: R restarts (trajectories of the evolve driver) of P parameters, nsh shifts per parameter; max_iter / tol
// of every fixed-point solve; the context's work buffers (parameter vectors, history, the four ints the kernels advance)
struct RotoRun {
  int64_t R;
  int kind, P, n_sweeps, max_iter;
  double tol;
  int nsh;
  double *base, *hist;
  int* idx;
};

int ready_buffers(qmps_ctx* c, size_t base_bytes, size_t hist_bytes) {
  if (int rc = grow(c->roto_base, c->roto_base_bytes, base_bytes)) return rc;
  if (int rc = grow(c->roto_hist, c->roto_hist_bytes, hist_bytes)) return rc;
  if (!c->roto_idx) HIP_TRY(hipMalloc((void**)&c->roto_idx, 4 * sizeof(int)));
  return QMPS_OK;
}

bool use_sweep_graph(int P) { return documented_switch("QMPS_NO_GRAPH") == nullptr && P <= 256; }

// one_sweep's launches into *graph, instantiated as *exec.  c->capturing is cleared on every way out, and an error of the sweep
// itself is reported in preference to the one it makes hipStreamEndCapture return.
template <class Sweep>
int capture_sweep(qmps_ctx* c, const Sweep& one_sweep, hipGraph_t* graph, hipGraphExec_t* exec) {
  int e;
  hipError_t ce;
  {
    Restore<bool> capturing(c->capturing, true);
    HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    e = one_sweep();
    ce = hipStreamEndCapture(c->stream, graph);
  }
  if (e) return e;
  HIP_TRY(ce);
  HIP_TRY(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
  return QMPS_OK;
}

// D = 2 with the library's default solver: the whole run is ONE launch (restarts are independent, see
// rotosolve_fused_d2_kernel); afterwards one ordinary evaluation of the final parameters leaves the context's
// resident tensors / energies / statuses exactly as the step-by-step path does.
bool d2_whole_run(const qmps_ctx* c, const RotoRun& r) {
  return (r.nsh == 3 || r.nsh == 6) && c->D == 2 && c->handoff == 0 && (c->default_solver == QMPS_ENV_POWER_SQUARING || c->default_solver == QMPS_ENV_DIRECT) &&
         r.P <= 64 && documented_switch("QMPS_NO_FUSED_ROTO") == nullptr;
}

// D = 8 (ShallowCNOT families, direct solver): the whole run in ONE launch as well - a workgroup per restart, a wave per
// shift (qmps_roto_d8.hip); afterwards one ordinary evaluation of the final parameters, as above
// (six shifts: every wave evaluates two of them in turn).  A restart occupies a CU for the whole run, so this is the path of
// the SMALL runs (BASELINE.json configs[3]: 256 restarts): measured against the step-by-step path, us per update,
// three shifts: R = 256: 19.9 / 34, 512: 40.8 / 45.4, 1 024: 77 / 63, 21 845: 1 552 / 785; six shifts: R = 128: 40.6 / 35.6, 256: 41.0 / 44.1.
bool d8_whole_run(const qmps_ctx* c, const RotoRun& r) {
  const bool d8_fused_pays = r.nsh == 3 ? r.R <= 512 : (r.R <= 256 && 6 * r.R > 1024);
  return c->D == 8 && (r.nsh == 3 || r.nsh == 6) && d8_fused_pays && c->default_solver == QMPS_ENV_DIRECT &&
         (r.kind == QMPS_ANSATZ_SHALLOW_CNOT || r.kind == QMPS_ANSATZ_SHALLOW_CNOT3) && r.P <= 64 && documented_switch("QMPS_NO_FUSED_ROTO") == nullptr;
}

// Every sweep of every restart inside one launch of `launch`, then the evaluation of the final vectors.  skip / direct: the solver
// fields of RotoArgs (D = 2 follows the context's solver, D = 8 is the direct solve).
int whole_run(qmps_ctx* c, const RotoRun& r, hipError_t (*launch)(int, const qmps::RotoArgs&, hipStream_t), int skip, int direct) {
  qmps::RotoArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.base = r.base; ra.h = c->d_h; ra.hist = r.hist;
  ra.R = (int)r.R; ra.P = r.P; ra.n_terms = c->n_terms; ra.n_sweeps = r.n_sweeps; ra.max_iter = r.max_iter;
  ra.skip = skip; ra.tol = r.tol; ra.direct = direct; ra.nsh = r.nsh; ra.rule = c->roto_rule;
  HIP_TRY(launch(r.kind, ra, c->stream));
  HIP_TRY(qmps::launch_ansatz(c->D, r.kind, r.base, r.P, c->d_A, r.R, c->stream));
  c->states.hold_tensors(r.R);
  forget_results(c);      // the launch below states what the R final vectors leave resident
  return energy_launch(c, r.R, r.max_iter, r.tol, c->default_solver, false);
}

// One parameter update = shift build -> ansatz -> environment + energy -> closed-form update; one sweep = n_params updates.  The
// parameter index and the sweep counter live in HBM and are advanced by the update kernel, so the sweep is captured ONCE into a
// hipGraph and replayed n_sweeps times: it is launch-bound at small R (a graph launch costs ~15 us: per update it was a third of
// the time, per sweep it is noise).
int step_by_step(qmps_ctx* c, const RotoRun& r) {
  // D = 4 with the direct solver: shift build and ansatz happen INSIDE the energy kernel (evaluation nsh r + k builds
  // the tensor of restart r with shift k on parameter *idx straight into LDS): two kernels per parameter update
  const bool fused = c->default_solver == QMPS_ENV_DIRECT && fusable_ansatz(c, r.kind);
  auto evaluate = [&](int shifts) -> int {      // shifts = nsh: the shifted batch;  0: the R base vectors
    const int64_t n = shifts > 0 ? (int64_t)shifts * r.R : r.R;
    if (fused) {
      c->states.hold_ansatz(n, r.kind, r.P, r.base, r.idx, shifts);      // (rows borrowed from the run: rotosolve_impl gives them back on every way out)
    } else {
      // shifted tensors straight from the base vectors (the shift build is folded into the ansatz kernel)
      HIP_TRY(qmps::launch_ansatz_shifted(c->D, r.kind, r.base, r.P, c->d_A, n, shifts, r.idx, c->stream));
      c->states.hold_tensors(n);
    }
    return energy_launch(c, n, r.max_iter, r.tol, c->default_solver, false);
  };
  auto one_sweep = [&]() -> int {
    for (int i = 0; i < r.P; ++i) {
      if (int e = evaluate(r.nsh)) return e;
      // the shift-0 row of a sweep's first batch is the evaluation of the vectors the PREVIOUS sweep left: its record
      if (i == 0) HIP_TRY(qmps::launch_roto_record(c->d_E, r.hist, (int)r.R, c->n_terms, r.idx + 2, r.nsh, c->stream));
      HIP_TRY(qmps::launch_roto_update(r.base, c->d_E, c->d_status, (int)r.R, r.P, r.idx, c->n_terms, r.nsh, c->roto_rule, c->stream));
    }
    return QMPS_OK;
  };
  const bool use_graph = use_sweep_graph(r.P);
  if (use_graph) {
    qmps_ctx::RotoKey key;
    key.R = r.R; key.kind = r.kind; key.P = r.P; key.nsh = r.nsh; key.max_iter = r.max_iter; key.n_terms = c->n_terms; key.rho_need = c->rho_need;
    key.solver = c->default_solver; key.handoff = c->handoff; key.rule = c->roto_rule; key.tol = r.tol; key.fused = fused;
    key.base = r.base; key.hist = r.hist; key.params = c->d_params; key.E = c->d_E;
    if (!(c->roto_exec && key == c->roto_key)) {
      if (c->roto_exec) (void)hipGraphExecDestroy(c->roto_exec);
      if (c->roto_graph) (void)hipGraphDestroy(c->roto_graph);
      c->roto_exec = nullptr; c->roto_graph = nullptr;
      if (int e = capture_sweep(c, one_sweep, &c->roto_graph, &c->roto_exec)) return e;
      c->roto_key = key;
    }
  }
  for (int sw = 0; sw < r.n_sweeps; ++sw) {
    if (use_graph) HIP_TRY(hipGraphLaunch(c->roto_exec, c->stream));
    else if (int e = one_sweep()) return e;
  }
  // the last sweep's record, and the resident state the call leaves: one evaluation of the final vectors
  if (int e = evaluate(0)) return e;
  HIP_TRY(qmps::launch_roto_record(c->d_E, r.hist, (int)r.R, c->n_terms, r.idx + 2, 1, c->stream));
  // The context's view of what is resident - a replayed graph runs no host code, so it is stated here, not inherited from
  // the capture: the R final parameter vectors, their energies / statuses / environments
  c->window = 0;
  forget_results(c);
  c->env.add(0, r.R); c->env_start.add(0, r.R); c->energies.add(0, r.R); c->counts.add(0, r.R);
  c->partials_B = -1;
  c->acc_pending = false;
  if (fused) {
    // as a qmps_set_states_ansatz of the final parameters would leave it: rows resident in d_params, tensors on demand
    HIP_TRY(hipMemcpyAsync(c->d_params, r.base, (size_t)r.R * r.P * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->states.hold_ansatz(r.R, r.kind, r.P);
  } else {
    c->states.hold_tensors(r.R);
  }
  return QMPS_OK;
}

// The run's results (final parameters, energy history) come back through the context's pinned buffer when they fit: the
// first LARGE copy into pageable memory makes the runtime set up its internal staging, ~8 ms once per process (measured
// in the first 160-sweep call after an 8-sweep one: 27.7 instead of 19.5 us per parameter update at D = 8).
int download_results(qmps_ctx* c, const RotoRun& r, size_t hist_doubles, double* params, double* E_hist) {
  const size_t pb = (size_t)r.R * r.P * sizeof(double), hb = hist_doubles * sizeof(double);
  const bool staged = pb + hb <= (2u << 20);      // (small results only: a 7 MB history copied twice cost the D = 4 run of 21 845 restarts 16 %)
  if (staged)
    if (int e = ensure_pinned(c, (16u << 20))) return e;
  HIP_TRY(hipMemcpyAsync(staged ? (void*)c->h_pin : params, r.base, pb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(staged ? (void*)(c->h_pin + pb) : E_hist, r.hist, hb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (staged) {
    memcpy(params, c->h_pin, pb);
    memcpy(E_hist, c->h_pin + pb, hb);
  }
  return QMPS_OK;
}

// start vectors in, counters cleared, then the run on the path that serves it
int upload_and_run(qmps_ctx* c, const RotoRun& r, const double* params) {
  HIP_TRY(hipMemcpyAsync(r.base, params, (size_t)r.R * r.P * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(r.idx, 0, 3 * sizeof(int), c->stream));   // parameter index, arrival counter, finished sweeps
  if (kHistExtra) HIP_TRY(hipMemsetAsync(r.hist + (size_t)r.R * r.n_sweeps, 0, kHistExtra * sizeof(double), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  Restore<bool> cold(c->have_guess, false);      // every solve of the run starts cold; the caller's guess outlives it, also on an error
  if (d2_whole_run(c, r)) return whole_run(c, r, qmps::launch_rotosolve_fused_d2, c->skip_rounds, c->default_solver == QMPS_ENV_DIRECT ? 1 : 0);
  if (d8_whole_run(c, r)) return whole_run(c, r, qmps::launch_rotosolve_fused_d8, 0, 1);
  return step_by_step(c, r);
}

int rotosolve_impl(qmps_ctx* c, int64_t R, int kind, int n_params, double* params, int n_sweeps, int max_iter, double tol,
                   double* E_hist, int nsh) {
  if (int rc = bind(c)) return rc;
  if (R < 1 || nsh * R > c->max_batch) return fail(QMPS_ERR_ARG, "%d R = %lld evaluations exceed max_batch = %lld", nsh, (long long)(nsh * R), (long long)c->max_batch);
  c->window = 0;
  if (!params || !E_hist) return fail(QMPS_ERR_ARG, "null argument");
  if (n_sweeps < 1) return fail(QMPS_ERR_ARG, "n_sweeps must be >= 1");
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "qmps_set_hamiltonian has not been called");
  if (int rc = check_ansatz(c, kind, n_params)) return rc;
  if (int rc = ensure_params(c, n_params)) return rc;
  if (int rc = ready_buffers(c, (size_t)R * n_params * sizeof(double), ((size_t)R * n_sweeps + kHistExtra) * sizeof(double))) return rc;
  const RotoRun r{R, kind, n_params, n_sweeps, max_iter, tol, nsh, c->roto_base, c->roto_hist, c->roto_idx};
  int rc = upload_and_run(c, r, params);
  // (the instrumented D = 8 kernel's clocks sit behind the history and come back with it)
  if (rc == QMPS_OK) rc = download_results(c, r, (size_t)R * n_sweeps + (kHistExtra && d8_whole_run(c, r) ? kHistExtra : 0), params, E_hist);
  (void)hipStreamSynchronize(c->stream);
  if (c->states.borrowed()) c->states.hold_tensors(0);     // an error left the context pointing at the run's own buffers
  if (rc != QMPS_OK && c->roto_exec) {     // do not trust a sweep captured by a failed run
    (void)hipGraphExecDestroy(c->roto_exec);
    if (c->roto_graph) (void)hipGraphDestroy(c->roto_graph);
    c->roto_exec = nullptr; c->roto_graph = nullptr;
  }
  return rc;
}

// The time steps of qmps_evolve_rotosolve: r.R trajectories, r.max_iter = max_rounds of the overlap solves; slot_bytes: one warm-start
// slot (0: the solver squares, no warm start).  The sweep graph is the caller's to destroy, once the stream has drained.
int evolve_run(qmps_ctx* c, const OverlapRoute& route, const RotoRun& r, int n_steps, size_t slot_bytes, double* params, const double* WW, double* params_hist, double* f_hist,
               hipGraph_t* graph, hipGraphExec_t* exec) {
  const int64_t T = r.R;
  const int P = r.P;
  const size_t vec_bytes = (size_t)T * P * sizeof(double);
  double* d_phist = (double*)c->d_scratch;
  HIP_TRY(hipMemcpyAsync(r.base, params, vec_bytes, hipMemcpyHostToDevice, c->stream));
  const int idx0[4] = {0, 0, 0, P};      // parameter index, arrival counter, finished sweeps, slot of the unshifted evaluation
  HIP_TRY(hipMemcpyAsync(r.idx, idx0, sizeof(idx0), hipMemcpyHostToDevice, c->stream));
  if (int e = set_ww(c, WW)) return e;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->window = 0;
  forget_resident_state(c);
  c->energies.clear();        // d_E is the run's objective buffer: what qmps_get_energies would return are overlap objectives
  c->states.hold_tensors(0);      // d_A is the run's candidate buffer from here on; the caller states what the run leaves
  auto evaluate = [&](int shifts) -> int {      // shifts = nsh: the shifted batch of parameter *idx;  0: the T base vectors
    const int64_t n = shifts > 0 ? (int64_t)shifts * T : T;
    HIP_TRY(qmps::launch_ansatz_shifted(c->D, r.kind, r.base, P, c->d_A, n, shifts, r.idx, c->stream));
    qmps::OverlapArgs a;
    memset(&a, 0, sizeof(a));
    a.A = c->d_ref; a.Bt = c->d_A; a.WW = c->d_ww; a.eta = c->d_eta; a.f_out = c->d_E;
    a.iters = c->d_iters; a.status = c->d_status; a.B = n; a.group = shifts > 0 ? shifts : 1;
    a.max_rounds = r.max_iter; a.tol = r.tol; a.stats = c->d_ostats;
    if (slot_bytes) {
      a.x_in = c->d_xwarm; a.r_out = c->d_xwarm;
      a.slot_ptr = shifts > 0 ? r.idx : r.idx + 3; a.slot_stride = (int64_t)slot_bytes;
    }
    return launch_overlap_kernels(c, route, a);
  };
  auto one_sweep = [&]() -> int {
    for (int i = 0; i < P; ++i) {
      if (int e = evaluate(r.nsh)) return e;
      HIP_TRY(qmps::launch_roto_update(r.base, c->d_E, c->d_status, (int)T, P, r.idx, 1, r.nsh, c->roto_rule, c->stream));
    }
    // the sweep's record: the objective of the updated vectors against this time step's reference states
    if (int e = evaluate(0)) return e;
    HIP_TRY(qmps::launch_roto_record(c->d_E, r.hist, (int)T, 1, r.idx + 2, 1, c->stream));
    return QMPS_OK;
  };
  const bool use_graph = use_sweep_graph(P);
  if (use_graph)
    if (int e = capture_sweep(c, one_sweep, graph, exec)) return e;
  for (int step = 0; step < n_steps; ++step) {
    // the states the step starts from are the reference: A_t = tensor(params_t)  (new_time_evolve.py:281-283)
    HIP_TRY(qmps::launch_ansatz(c->D, r.kind, r.base, P, c->d_ref, T, c->stream));
    for (int sw = 0; sw < r.n_sweeps; ++sw) {
      if (use_graph) HIP_TRY(hipGraphLaunch(*exec, c->stream));
      else if (int e = one_sweep()) return e;
    }
    HIP_TRY(hipMemcpyAsync(d_phist + (size_t)step * T * P, r.base, vec_bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(params, r.base, vec_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(f_hist, r.hist, (size_t)T * n_steps * r.n_sweeps * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (params_hist) HIP_TRY(hipMemcpyAsync(params_hist, d_phist, (size_t)n_steps * vec_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}

}  // namespace

int qmps_rotosolve(qmps_ctx* c, int64_t R, int kind, int n_params, double* params, int n_sweeps, int max_iter,
                   double tol, double* E_hist) try {
  return rotosolve_impl(c, R, kind, n_params, params, n_sweeps, max_iter, tol, E_hist, 3);
}
QMPS_API_CATCH

int qmps_double_rotosolve(qmps_ctx* c, int64_t R, int kind, int n_params, double* params, int n_sweeps, int max_iter,
                          double tol, double* E_hist) try {
  return rotosolve_impl(c, R, kind, n_params, params, n_sweeps, max_iter, tol, E_hist, 6);
}
QMPS_API_CATCH

int qmps_evolve_rotosolve(qmps_ctx* c, int64_t T, int kind, int n_params, double* params, const double* WW, int n_steps,
                          int n_sweeps, int nsh, int max_rounds, double tol, double* params_hist, double* f_hist) try {
  if (int rc = bind(c)) return rc;
  const OverlapRoute route = overlap_route(c);
  if (!params || !WW || !f_hist) return fail(QMPS_ERR_ARG, "null argument");
  if (nsh != 3 && nsh != 6) return fail(QMPS_ERR_ARG, "nsh must be 3 (single-frequency) or 6 (double-frequency)");
  if (T < 1 || nsh * T > c->max_batch) return fail(QMPS_ERR_ARG, "%d T = %lld candidates exceed max_batch = %lld", nsh, (long long)(nsh * T), (long long)c->max_batch);
  if (n_steps < 1 || n_sweeps < 1) return fail(QMPS_ERR_ARG, "n_steps and n_sweeps must be >= 1");
  if (int rc = check_ansatz(c, kind, n_params)) return rc;
  const int cap = route.squares ? 60 : (1 << 24);
  if (max_rounds < 1 || max_rounds > cap || !(tol > 0.0)) return fail(QMPS_ERR_ARG, "bad max_rounds / tol (D = %d: max_rounds in [1, %d])", c->D, cap);
  const size_t vec_bytes = (size_t)T * n_params * sizeof(double);
  if (int rc = ready_buffers(c, vec_bytes, (size_t)T * n_steps * n_sweeps * sizeof(double))) return rc;
  if (int rc = ensure_refs(c, T)) return rc;
  if (int rc = ensure_E(c, c->n_terms > 0 ? c->n_terms : 1)) return rc;
  if (int rc = ensure_overlap_outputs(c)) return rc;
  if (int rc = ensure_scratch(c, (size_t)n_steps * vec_bytes)) return rc;    // parameter history
  // fixed points of the power method (D = 8, 16), one set per parameter plus one for the unshifted evaluation of a sweep:
  // the candidates of parameter i come back to the same slot in the next sweep and in the next time step - by then the
  // parameters have moved by one sweep's updates, so the resident fixed point is the natural warm start
  const size_t slot_bytes = route.squares ? 0 : (size_t)nsh * T * env_bytes(c);
  if (slot_bytes) {
    if (int rc = grow(c->d_xwarm, c->xwarm_bytes, (size_t)(n_params + 1) * slot_bytes)) return rc;
    HIP_TRY(hipMemsetAsync(c->d_xwarm, 0, (size_t)(n_params + 1) * slot_bytes, c->stream));       // all zero = cold start
  }
  const RotoRun r{T, kind, n_params, n_sweeps, max_rounds, tol, nsh, c->roto_base, c->roto_hist, c->roto_idx};
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  const int rc = evolve_run(c, route, r, n_steps, slot_bytes, params, WW, params_hist, f_hist, &graph, &exec);
  (void)hipStreamSynchronize(c->stream);
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
  // what the call leaves resident: the T final candidates (tensors, eta, objective, status) against the last step's references
  c->states.hold_tensors(rc == QMPS_OK ? T : 0);
  c->overlap_refs = rc == QMPS_OK ? T : 0;
  c->overlap_group = 0;
  return rc;
}
QMPS_API_CATCH
