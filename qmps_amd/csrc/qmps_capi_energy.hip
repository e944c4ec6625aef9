// qmps_capi_energy.hip - the energy path of the C-ABI (declared in include/qmps_hip.h): qmps_energy_launch with a function per solver
// path and their dispatcher, the energy-only pass, read-back (energies, status, environments, density matrices), the one-shot batch
// calls and the two-site unit cell.  Asynchronous launches on the context stream - the fused D = 4 direct kernel alternately on the two
// launch lanes (qmps_hazard.h); the setters they follow and the shared helpers: qmps_capi.hip, qmps_ctx.h.  Where an accumulated cost
// goes (setup_accumulator, qmps_cost_launch): qmps_capi_cost.hip.  The rotosolve drivers built on these launches: qmps_capi_roto.hip.
#include "qmps_ctx.h"
#include "qmps_direct_core.h"

using namespace qmps_host;

// (every entry point below is declared extern "C" in include/qmps_hip.h: the definitions inherit the linkage)

namespace {

// the arguments every launch starts from: the window's buffers; solve == false: the energy pass over the resident environments
qmps::LaneArgs make_args(qmps_ctx* c, int64_t B, int max_iter, double tol, bool solve) {
  qmps::LaneArgs a;
  memset(&a, 0, sizeof(a));
  a.A = win_A(c);
  a.h = c->d_h;
  a.r_in = solve ? (c->have_guess && window_has_start(c, B) ? win_r(c) : nullptr) : win_r(c);   // (a guess covers the slots it was given for)
  a.r_out = solve ? win_r(c) : nullptr;
  a.rho_out = c->want_rho ? (char*)c->d_rho + (size_t)c->window * 256 : nullptr;
  a.rho_need = a.rho_out != nullptr ? qmps::kRhoNeedAll : c->rho_need;   // rho itself: every entry; otherwise what h reads
  a.E = win_E(c);
  a.iters = win_iters(c);
  a.status = win_status(c);
  a.B = B;
  a.n_terms = c->n_terms;
  a.max_iter = max_iter;
  a.tol = tol;
  return a;
}

// The paths of qmps_energy_launch: a = make_args of the launch (B, max_iter, tol; QMPS_FLAG_WARM_RESIDENT and the fused ansatz already
// applied), flags as passed (the requested solver in the low byte), t the timing bracket of the dominant kernel(s)
using EnergyPathFn = int (*)(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t);

// Where the cost of the launch goes: the accumulator of the following qmps_cost_launch (QMPS_FLAG_ACCUMULATE_COST; adds = arrivals
// per term, per_add = evaluations behind one arrival), or per-wave partial sums in d_partial, `adds` entries per term, which
// qmps_cost_launch reduces instead of E while partials_B == a.B
int cost_sink(qmps_ctx* c, qmps::LaneArgs& a, bool accumulate, int64_t adds, int per_add) {
  if (accumulate) return setup_accumulator(c, a, a.B, adds, per_add);
  a.partial = c->d_partial;
  c->partials_B = a.B;
  c->partials_n = (int)adds;
  return QMPS_OK;
}

// D = 8, 16: the power launch with the Krylov fall-back of the environment solve (include/qmps_hip.h "fixed-point solvers").
// Evaluations whose power iteration predicts a long tail (|lambda_2| -> 1: shallow circuits) are finished by the Arnoldi kernel of
// qmps_overlap_krylov.hip on the environment map, then accepted - energy, Cholesky test, status - by a finishing pass of the same
// energy kernel.  krylov == false: the power launch alone.  launch: launch_energy_mfma or launch_energy.
int power_with_krylov(qmps_ctx* c, qmps::LaneArgs& a, bool krylov, hipError_t (*launch)(int, const qmps::LaneArgs&, bool, hipStream_t)) {
  if (krylov) {
    a.krylov_after = krylov_after();
    a.kry_counter = c->d_queue + qmps_ctx::kEnergyKrylov;
  }
  HIP_TRY(launch(c->D, a, true, c->stream));
  if (!krylov || a.krylov_after <= 0) return QMPS_OK;
  qmps::OverlapArgs k;
  memset(&k, 0, sizeof(k));
  k.Bt = a.A; k.r_out = a.r_out; k.iters = a.iters; k.status = a.status; k.B = a.B; k.max_rounds = a.max_iter; k.tol = a.tol;
  k.env_mode = 1; k.krylov_after = a.krylov_after; k.kry_counter = a.kry_counter;
  HIP_TRY(qmps::launch_overlap_krylov(c->D, k, k.kry_counter, c->stream));
  qmps::LaneArgs f = a;
  f.r_in = a.r_out; f.only_pending = 1; f.krylov_after = 0; f.acc_zero = nullptr; f.direct = 0;
  f.max_iter = 64;
  HIP_TRY(launch(c->D, f, true, c->stream));
  return QMPS_OK;
}

// D = 4: direct fixed-point solve + acceptance power step + energies in ONE kernel (a DPP quad per evaluation); one read of A, one
// store of E (and, unless switched off, of r) per evaluation.  a.r_in (qmps_set_env_guess / QMPS_FLAG_WARM_RESIDENT): evaluations
// whose guess passes the acceptance test skip the solve.
// on_lanes (qmps_energy_launch decides): the launch goes to the next of the two compute lanes, behind the launches of the other lane
// that its footprint conflicts with (qmps_hazard.h) - before anything of it, the clearing memset of setup_accumulator included,
// touches memory.  The event pair of a timed launch stands on the launch's own lane, so it may span waves of a neighbour.
int energy_direct_d4(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t, bool on_lanes) {
  a.r_out = (flags & QMPS_FLAG_NO_ENV_OUT) ? nullptr : win_r(c);
  const bool accumulate = (flags & QMPS_FLAG_ACCUMULATE_COST) != 0;
  LaunchFootprint f;
  int lane = 0;
  if (on_lanes) {
    f.lo = c->window; f.hi = c->window + a.B;
    f.acc = accumulate ? acc_position(c, 0) : -1;
    f.acc_zero = accumulate ? acc_position(c, 2) : -1;      // (whether or not this launch finds it dirty)
    f.partials = !accumulate;
    if (int rc = lane_begin(c, f, &lane)) return rc;
  }
  Restore<hipStream_t> on_lane(c->launch_stream, c->lane(lane));
  if (int rc = cost_sink(c, a, accumulate, (a.B + 15) / 16, 16)) return rc;
  c->dominant = "energy_direct_d4_kernel";
#ifdef QMPS_WAVE_TIMELINE
  a.timeline = c->d_timeline;
#endif
  HIP_TRY(t.start());
  HIP_TRY(qmps::launch_energy_direct_d4(a, c->launch_stream, on_lanes));
  HIP_TRY(t.stop());
  if (on_lanes) {
    int64_t seq = 0;
    if (int rc = lane_end(c, f, lane, &seq)) return rc;
    if (accumulate) { c->acc_lane[c->acc_slot][c->acc_pos] = lane; c->acc_seq[c->acc_slot][c->acc_pos] = seq; }
  }
  return QMPS_OK;
}
int energy_direct_d4_serial(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t) { return energy_direct_d4(c, a, flags, t, false); }

// D = 16: power iteration on the matrix cores (one wave per evaluation) with the Krylov fall-back (QMPS_NO_KRYLOV: power iteration
// alone), then the energy pass
int energy_mfma_d16(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t) {
  c->dominant = "energy_mfma_d16_kernel<true>";
  if (flags & QMPS_FLAG_ACCUMULATE_COST)     // (otherwise no partial sums: qmps_cost_launch reduces E)
    if (int rc = setup_accumulator(c, a, a.B, a.B, 1)) return rc;
  const bool krylov = documented_switch("QMPS_NO_KRYLOV") == nullptr && a.max_iter > 64;
  HIP_TRY(t.start());
  if (int rc = power_with_krylov(c, a, krylov, qmps::launch_energy_mfma)) return rc;
  HIP_TRY(t.stop());
  return QMPS_OK;
}

// D = 4, plain power iteration (round 6): a 16-lane DPP row per evaluation (the map as a real 16 x 16 matrix in registers, a step =
// sixteen v_fmac_f64_dpp) in persistent waves that draw their evaluations from a counter - env_power_d4_kernel (qmps_direct.hip) - then
// the energies, the Cholesky test and the cost sums on the stored environments (energy_only_d4_kernel).  The lane-per-evaluation kernel
// of rounds 1-5 waited for the slowest of its 64 evaluations in every wave and for ONE evaluation per launch (QMPS_POWER_LANE=1 selects
// it: same iterates, same iteration counts).
int energy_power_row_d4(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t) {
  int* counter = c->d_queue + qmps_ctx::kPowerRowCounter;
  HIP_TRY(hipMemsetAsync(counter, 0, sizeof(int), c->stream));
  qmps::LaneArgs e = make_args(c, a.B, 1, 1.0, false);
  e.check_pd = 1;
  if (int rc = cost_sink(c, e, flags & QMPS_FLAG_ACCUMULATE_COST, (a.B + 15) / 16, 16)) return rc;
  int waves_per_simd = 5;          // (the kernel compiles to 108 VGPRs; __launch_bounds__(64, 4) allows 4 waves per SIMD)
  if (const char* w = tuning_knob("QMPS_POWER_WAVES")) waves_per_simd = atoi(w);
  c->dominant = "env_power_d4_kernel";
  HIP_TRY(t.start());
  HIP_TRY(qmps::launch_env_power_d4(a, counter, c->n_cus * 4 * waves_per_simd, c->stream));
  HIP_TRY(t.stop());
  HIP_TRY(qmps::launch_energy_only_d4(e, c->stream));
  return QMPS_OK;
}

// One lane per evaluation (D <= 4) or the block kernel (D = 8; D = 16 with QMPS_D16_BLOCK): power iteration and energies in one launch
int energy_power(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t) {
  const int solver = flags & 0xff;
  const bool accumulate = (flags & QMPS_FLAG_ACCUMULATE_COST) != 0;
  if (c->D == 8 && solver == QMPS_ENV_DIRECT) {
    // D = 8: the direct solve (one wave per evaluation) hands its result to the power iteration of the block kernel: its first step
    // is the acceptance test, its loop the fall-back.  Small batches (all launch latency: BASELINE configs[3] is 96 evaluations per
    // GPU) run both in ONE launch; large ones keep two kernels - the block kernel alone runs four waves per SIMD, the solve two.
    static const int64_t fuse_below = tuning_knob("QMPS_D8_FUSE_BELOW") ? atoll(tuning_knob("QMPS_D8_FUSE_BELOW")) : 4096;   // A/B knob
    if (a.B <= fuse_below) {
      a.direct = 1;
      a.r_in = nullptr;
    } else {
      HIP_TRY(qmps::launch_env_direct_d8(win_A(c), win_r(c), a.B, c->stream));
      a.r_in = win_r(c);
    }
  }
  c->dominant = c->D <= 4 ? "energy_lane_kernel<D,true>" : "energy_block_kernel<D,true>";
  if (c->D <= 4 || accumulate)     // (the block kernel leaves no partial sums: qmps_cost_launch reduces E)
    if (int rc = cost_sink(c, a, accumulate, c->D <= 4 ? (a.B + 63) / 64 : a.B, c->D <= 4 ? 64 : 1)) return rc;
  // D = 8 (round 5): the power loop behind a direct solve that was not accepted - an elimination without pivoting meets structural zeros
  // at special angles of the ansatz - is the only fall-back of the energy path whose cost grows with 1 / gap (D = 2, 4 square, D = 16
  // hands over): it gets the Krylov fall-back of D = 16.  QMPS_ENV_POWER stays the plain iteration (a-13: the classical statement of
  // PowerCircuit); QMPS_NO_KRYLOV switches it off.  On request only (QMPS_FLAG_KRYLOV_FALLBACK; the one-shot entry points set it): the
  // two extra launches - nearly always empty - cost 3.1 - 3.4 us of a 16 - 20 us step of resident tensors (B = 96 / 768, measured),
  // nothing next to the round trips of a one-shot call.
  // D = 16 under QMPS_D16_BLOCK: the same computation as energy_mfma_d16, so the hand-over is armed as it is there - whatever the solver
  // and without the flag (include/qmps_hip.h: "D = 16 always hands over").  It used to run the power iteration alone: status 1 at max_iter
  // where the matrix-core path returns status 0 (tests/test_gap_gpu.py).
  const bool wanted = c->D == 16 || (c->D == 8 && (flags & QMPS_FLAG_KRYLOV_FALLBACK) != 0 && solver != QMPS_ENV_POWER);
  const bool krylov = wanted && documented_switch("QMPS_NO_KRYLOV") == nullptr && a.max_iter > 64 && c->d_queue != nullptr && a.r_out != nullptr;
  HIP_TRY(t.start());
  if (int rc = power_with_krylov(c, a, krylov, qmps::launch_energy)) return rc;
  HIP_TRY(t.stop());
  return QMPS_OK;
}

// D = 2 hybrid: `handoff` plain steps, then the squaring tail in-lane (real 4 x 4 transfer matrix in registers); QMPS_ENV_DIRECT puts
// the 4 x 4 direct solve in front of it
int energy_squaring_d2(qmps_ctx* c, qmps::LaneArgs& a, int flags, KernelTimer& t) {
  a.handoff = c->handoff;
  a.hybrid = 1;
  a.direct = (flags & 0xff) == QMPS_ENV_DIRECT ? 1 : 0;
  a.skip = c->handoff == 0 ? c->skip_rounds : 0;
  if (int rc = cost_sink(c, a, flags & QMPS_FLAG_ACCUMULATE_COST, (a.B + 63) / 64, 64)) return rc;
  c->dominant = "energy_lane_kernel<2,true>";
  HIP_TRY(t.start());
  HIP_TRY(qmps::launch_energy(c->D, a, true, c->stream));
  HIP_TRY(t.stop());
  return QMPS_OK;
}

// D = 4 hybrid: (1) lane kernel: `handoff` plain steps, slow items -> worklist (skipped when handoff == 0: every item goes straight to
// the squaring kernel); (2) wave-per-item MFMA squaring over the worklist; (3) energy-only pass over the worklist.  No host round trip:
// the later kernels read the item count from HBM.  (QMPS_FLAG_ACCUMULATE_COST is refused on this path.)
int energy_squaring_d4(qmps_ctx* c, qmps::LaneArgs& a, int, KernelTimer& t) {
  const int64_t B = a.B;
  qmps::SquareArgs q;
  memset(&q, 0, sizeof(q));
  q.A = win_A(c); q.r_out = win_r(c); q.iters = win_iters(c); q.status = win_status(c);
  q.B = B; q.done = c->handoff; q.max_iter = a.max_iter; q.tol = a.tol;
  q.skip = c->handoff == 0 ? c->skip_rounds : 0;
  q.period = c->matvec_period;
  qmps::LaneArgs e = make_args(c, B, 1, 1.0, false);
  e.check_pd = 1;
  // the energy pass over every item runs two lanes per evaluation (with settled clocks the step is 0.9 % shorter than with the one-lane
  // pass: 0.1112 against 0.1122 ms at B = 65536; QMPS_LANE_IN_STEP keeps the one-lane pass)
  const bool pair = c->handoff == 0 && !c->no_pair && c->pair_in_step;
  if (c->handoff > 0) {
    HIP_TRY(hipMemsetAsync(c->d_work_count, 0, sizeof(int32_t), c->stream));
    a.handoff = c->handoff; a.hybrid = 1; a.work_count = c->d_work_count; a.work_idx = c->d_work_idx;
    c->dominant = "energy_lane_kernel<4,true>";
    HIP_TRY(t.start());
    HIP_TRY(qmps::launch_energy(c->D, a, true, c->stream));
    HIP_TRY(t.stop());
    q.r_in = win_r(c); q.work_count = c->d_work_count; q.work_idx = c->d_work_idx;
    e.idx_list = c->d_work_idx; e.idx_count = c->d_work_count;
  } else {
    q.r_in = c->have_guess && window_has_start(c, B) ? win_r(c) : nullptr;
    if (int rc = cost_sink(c, e, false, pair ? (B + 31) / 32 : (B + 63) / 64, 64)) return rc;   // (pair: one partial per 32 items)
  }
  // grid-stride workgroups of 4 waves: whole generations of the resident capacity (5 workgroups per CU), at most three
  // (measured at B = 65536 with settled clocks: 1280 / 2560 / 3840 / 5120 workgroups -> 0.0876 / 0.0870 / 0.0859 / 0.0875 ms;
  // 2048 and 3072, which end in a partial generation, 0.0900 and 0.0878)
  int grid = (int)((B + 15) / 16);
  const int generation = c->n_cus * 5;
  if (grid > generation) {
    grid = (grid / generation) * generation;
    if (grid > 3 * generation) grid = 3 * generation;
  }
  if (const char* g = tuning_knob("QMPS_SQ_GRID")) grid = atoi(g) < grid ? atoi(g) : grid;   // tuning knob
  if (grid < 1) grid = 1;
  if (c->handoff == 0) {
    c->dominant = "env_square_d4_kernel";
    HIP_TRY(t.start());
  }
  HIP_TRY(qmps::launch_square_tail(c->D, q, grid, c->stream));
  if (c->handoff == 0) HIP_TRY(t.stop());
  if (pair) HIP_TRY(qmps::launch_energy_pair_d4(e, c->stream));
  else HIP_TRY(qmps::launch_energy(c->D, e, false, c->stream));
  return QMPS_OK;
}

// solver: QMPS_ENV_DIRECT only at D = 4 (elsewhere already rewritten to QMPS_ENV_POWER_SQUARING).  The documented switches are
// read on every launch: the tests flip them between the launches of one context.
EnergyPathFn energy_path(const qmps_ctx* c, int solver, int max_iter) {
  if (solver == QMPS_ENV_DIRECT) return energy_direct_d4_serial;
  if (c->D == 16 && !documented_switch("QMPS_D16_BLOCK")) return energy_mfma_d16;
  const bool hybrid = solver == QMPS_ENV_POWER_SQUARING && c->D <= 4 && c->handoff < max_iter;
  if (hybrid) return c->D == 2 ? energy_squaring_d2 : energy_squaring_d4;
  if (c->D == 4 && solver == QMPS_ENV_POWER && c->d_queue != nullptr && documented_switch("QMPS_POWER_LANE") == nullptr)
    return energy_power_row_d4;
  return energy_power;
}

}  // namespace

int qmps_host::energy_launch(qmps_ctx* c, int64_t B, int max_iter, double tol, int flags, bool may_overlap) {
  if (int rc = bind_device(c)) return rc;
  // The fused D = 4 direct kernel alternates between the two lanes and orders itself by its footprint; every other path, a launch
  // inside a graph capture and a launch that stamps a wave timeline stay on the context stream, behind both lanes like any other call.
  const bool on_lanes = may_overlap && c->lanes > 1 && c->D == 4 && (flags & 0xff) == QMPS_ENV_DIRECT && !c->capturing && c->d_timeline == nullptr && B > 0;
  if (!on_lanes)
    if (int rc = join_lanes(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (int rc = check_resident(c, B)) return rc;
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "qmps_set_hamiltonian has not been called");
  if (max_iter < 1) return fail(QMPS_ERR_ARG, "max_iter must be >= 1");
  if (!(tol > 0.0)) return fail(QMPS_ERR_ARG, "tol must be > 0");
  const int solver = flags & 0xff;
  if (solver != QMPS_ENV_POWER && solver != QMPS_ENV_POWER_SQUARING && solver != QMPS_ENV_DIRECT)
    return fail(QMPS_ERR_ARG, "unknown environment solver %d", solver);
  if ((flags & ~0xff) & ~(QMPS_FLAG_NO_ENV_OUT | QMPS_FLAG_ACCUMULATE_COST | QMPS_FLAG_WARM_RESIDENT | QMPS_FLAG_KRYLOV_FALLBACK)) return fail(QMPS_ERR_ARG, "unknown flag bits 0x%x", flags & ~0xff);
  const bool warm_resident = (flags & QMPS_FLAG_WARM_RESIDENT) != 0;
  if (warm_resident && !c->env_start.any()) return fail(QMPS_ERR_STATE, "QMPS_FLAG_WARM_RESIDENT: no resident environments (run a launch that stores them, or qmps_set_env_guess)");
  const bool direct = solver == QMPS_ENV_DIRECT && c->D == 4;
  if ((flags & QMPS_FLAG_NO_ENV_OUT) && !direct) return fail(QMPS_ERR_ARG, "QMPS_FLAG_NO_ENV_OUT needs QMPS_ENV_DIRECT at D = 4");
  const bool accumulate = (flags & QMPS_FLAG_ACCUMULATE_COST) != 0;
  if (accumulate && c->D == 4 && !direct && solver == QMPS_ENV_POWER_SQUARING)
    return fail(QMPS_ERR_ARG, "QMPS_FLAG_ACCUMULATE_COST: at D = 4 use QMPS_ENV_DIRECT or QMPS_ENV_POWER");
  if (accumulate && c->acc_pending)
    return fail(QMPS_ERR_STATE, "the cost accumulated by the previous launch has not been consumed by qmps_cost_launch");
  if (accumulate && c->capturing) return fail(QMPS_ERR_STATE, "no cost accumulation inside a graph capture");
  // QMPS_ENV_DIRECT away from D = 4: D = 2 takes the lane kernel's squaring path with the 4 x 4 solve in front, D = 8 the block kernel
  // behind the direct solve, D = 16 iterates (documented)
  const EnergyPathFn run = energy_path(c, solver == QMPS_ENV_DIRECT && !direct ? QMPS_ENV_POWER_SQUARING : solver, max_iter);
  c->acc_pending = false;   // whatever an earlier launch accumulated no longer describes the resident energies
  c->have_overlap_x = false;   // d_r is about to hold environments, not overlap fixed points
  c->grad_warm_T = 0;
  const ResidentStates& s = c->states;
  const bool fused = direct && s.ansatz && fusable_ansatz(c, s.kind);   // the direct kernel builds the tensors itself
  if (!fused) {
    if (on_lanes && !s.has_tensors)      // the tensor build writes d_A on the context stream
      if (int rc = join_lanes(c)) return rc;
    if (int rc = ensure_tensors(c)) return rc;
  }
  qmps::LaneArgs a = make_args(c, B, max_iter, tol, true);
  // (a window none of whose slots was ever stored or guessed starts cold, as documented: its part of d_r holds whatever was there)
  if (warm_resident) a.r_in = window_has_start(c, B) ? win_r(c) : nullptr;
  if (fused) {
    const double* rows = s.borrowed() ? s.rows : c->d_params;
    a.ans_params = s.shifts > 0 ? rows : rows + (size_t)c->window * s.P;
    a.ans_P = s.P; a.ans_kind = s.kind; a.ans_nsh = s.shifts; a.ans_i = s.shift_index;
  }
  c->partials_B = -1;
  KernelTimer timer(c, periodic_timing(c));
  if (int rc = on_lanes ? energy_direct_d4(c, a, flags, timer, true) : run(c, a, flags, timer)) return rc;
  if (!c->capturing) c->launches++;
  // only the direct D = 4 path may store no environments (QMPS_FLAG_NO_ENV_OUT).  A warm launch that stores nothing leaves what it started
  // from in place: environments an earlier launch stored for these states stay what they were; guesses stay the start of the next solve,
  // but a launch has run over them and they are not its result - they can no longer be read back as environments (include/qmps_hip.h)
  const int64_t lo = c->window, hi = c->window + B;
  if (a.r_out != nullptr) {
    c->env.add(lo, hi);
    c->env_start.add(lo, hi);
    c->env_guessed.remove(lo, hi);
  } else if (a.r_in == nullptr) {
    c->env.remove(lo, hi);
    c->env_start.remove(lo, hi);
    c->env_guessed.remove(lo, hi);
  } else if (c->env_guessed.touches(lo, hi)) {
    c->env.remove(lo, hi);
    c->env_guessed.remove(lo, hi);
  }
  c->energies.add(lo, hi);
  c->counts.add(lo, hi);
  c->overlap_vals.remove(lo, hi);     // (rounds and statuses of an overlap launch over these slots are gone)
  c->overlap_x.remove(lo, hi);
  return QMPS_OK;
}

int qmps_energy_launch(qmps_ctx* c, int64_t B, int max_iter, double tol, int flags) try {
  return energy_launch(c, B, max_iter, tol, flags, true);
}
QMPS_API_CATCH

int qmps_energy_only_launch(qmps_ctx* c, int64_t B) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (int rc = check_resident(c, B)) return rc;
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "qmps_set_hamiltonian has not been called");
  if (!c->env.covers(c->window, c->window + B))
    return fail(QMPS_ERR_STATE, "no resident environment for the window [%lld, %lld): run qmps_energy_launch (storing them) or qmps_set_env_guess over it first", (long long)c->window, (long long)(c->window + B));
  if (int rc = ensure_tensors(c)) return rc;
  qmps::LaneArgs a = make_args(c, B, 1, 1.0, false);
  c->partials_B = -1;
  c->energies.add(c->window, c->window + B);
  if (B > 0 && !c->counts.covers(c->window, c->window + B)) {
    // nothing solved these evaluations since their states were set: the pass iterates nothing and tests nothing, and says so, instead
    // of leaving the counts and statuses of another launch beside its energies
    HIP_TRY(hipMemsetAsync(win_iters(c), 0, (size_t)B * sizeof(int32_t), c->stream));
    HIP_TRY(hipMemsetAsync(win_status(c), 0, (size_t)B * sizeof(int32_t), c->stream));
    c->counts.add(c->window, c->window + B);
    c->overlap_vals.remove(c->window, c->window + B);
  }
  if (c->D == 16 && !documented_switch("QMPS_D16_BLOCK"))
    HIP_TRY(qmps::launch_energy_mfma(c->D, a, false, c->stream));
  else if (c->D == 4 && tuning_knob("QMPS_ENERGY_PAIR") == nullptr)
    HIP_TRY(qmps::launch_energy_only_d4(a, c->stream));     // quad layout, 4+ waves per SIMD (round 1: two lanes per evaluation)
  else if (c->D == 4 && !c->no_pair)
    HIP_TRY(qmps::launch_energy_pair_d4(a, c->stream));
  else
    HIP_TRY(qmps::launch_energy(c->D, a, false, c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_sum_energies(qmps_ctx* c, int64_t B, double* cost) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (!cost) return fail(QMPS_ERR_ARG, "null cost");
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "no energies resident");
  c->partials_B = -1;   // d_partial is about to be overwritten by the generic two-pass reduction
  HIP_TRY(qmps::launch_sum(win_E(c), B, c->n_terms, c->d_partial, kSumBlocks, c->d_cost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_cost, c->d_cost, c->n_terms * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  memcpy(cost, c->h_cost, c->n_terms * sizeof(double));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_energies(qmps_ctx* c, int64_t B, double* E, int32_t* iters, int32_t* status) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (c->n_terms < 1) return fail(QMPS_ERR_STATE, "no energies resident");
  // what the window's slots hold must belong together: energies of the resident states, and - when asked for - the iteration counts
  // and statuses of the launch that computed them, not those an overlap launch wrote over them since
  // (an empty window asks for nothing)
  if (B > 0 && E && !c->energies.covers(c->window, c->window + B))
    return fail(QMPS_ERR_STATE, "no energies resident for the window [%lld, %lld): no energy launch has covered it since the states, or the number of terms, were set", (long long)c->window, (long long)(c->window + B));
  if (B > 0 && (iters || status) && !c->counts.covers(c->window, c->window + B))
    return fail(QMPS_ERR_STATE, "the iteration counts and statuses of the window [%lld, %lld) are not those of an energy launch (qmps_overlap_get / qmps_get_status read an overlap launch's)", (long long)c->window, (long long)(c->window + B));
  if (E) HIP_TRY(hipMemcpyAsync(E, win_E(c), (size_t)B * c->n_terms * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (iters) HIP_TRY(hipMemcpyAsync(iters, win_iters(c), (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (status) HIP_TRY(hipMemcpyAsync(status, win_status(c), (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_status(qmps_ctx* c, int64_t B, int32_t* status) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (!status) return fail(QMPS_ERR_ARG, "null status");
  if (B > 0 && !c->counts.covers(c->window, c->window + B) && !c->overlap_vals.covers(c->window, c->window + B))
    return fail(QMPS_ERR_STATE, "no launch, energy or overlap, has covered the window [%lld, %lld) since the states were set", (long long)c->window, (long long)(c->window + B));
  HIP_TRY(hipMemcpyAsync(status, win_status(c), (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_env(qmps_ctx* c, int64_t B, double* r) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (!r) return fail(QMPS_ERR_ARG, "null r");
  if (!c->env.covers(c->window, c->window + B)) return fail(QMPS_ERR_STATE, "no resident environment for the window [%lld, %lld)", (long long)c->window, (long long)(c->window + B));
  HIP_TRY(hipMemcpyAsync(r, win_r(c), (size_t)B * env_bytes(c), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_get_rdm(qmps_ctx* c, int64_t B, double* rho) try {
  if (int rc = bind(c)) return rc;
  if (int rc = check_window(c, B)) return rc;
  if (!rho) return fail(QMPS_ERR_ARG, "null rho");
  if (!c->env.covers(c->window, c->window + B)) return fail(QMPS_ERR_STATE, "no resident environment for the window [%lld, %lld)", (long long)c->window, (long long)(c->window + B));
  if (!c->d_rho) HIP_TRY(hipMalloc(&c->d_rho, (size_t)c->max_batch * 256));
  // recompute from the resident (A, r): the energy-only kernel writes rho when asked to
  c->want_rho = true;
  int rc = qmps_energy_only_launch(c, B);
  c->want_rho = false;
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(rho, (char*)c->d_rho + (size_t)c->window * 256, (size_t)B * 256, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return QMPS_OK;
}
QMPS_API_CATCH

int qmps_energy_batch(qmps_ctx* c, int64_t B, const double* states, int kind, const double* h, int n_terms,
                      const double* r0, int max_iter, double tol, double* E_out, int32_t* iters_out,
                      int32_t* status_out) try {
  if (!E_out) return fail(QMPS_ERR_ARG, "null E_out");
  if (int rc = qmps_set_states(c, B, states, kind)) return rc;
  if (int rc = qmps_set_hamiltonian(c, n_terms, h)) return rc;
  if (int rc = qmps_set_env_guess(c, B, r0)) return rc;
  if (int rc = energy_launch(c, B, max_iter, tol, c->default_solver | QMPS_FLAG_KRYLOV_FALLBACK, false)) return rc;
  return qmps_get_energies(c, B, E_out, iters_out, status_out);
}
QMPS_API_CATCH

int qmps_energy_batch_ansatz(qmps_ctx* c, int64_t B, int ansatz_kind, int n_params, const double* params, const double* h,
                             int n_terms, int max_iter, double tol, double* E_out, int32_t* iters_out, int32_t* status_out) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!E_out) return fail(QMPS_ERR_ARG, "null E_out");
  // the host buffers stay the caller's until this function returns: the copies in may stay in flight until the ONE
  // synchronisation of the read-back (a scalar objective call is all latency: three round trips -> one)
  int rc;
  {
    Restore<bool> deferred(c->defer_sync, true);
    rc = qmps_set_states_ansatz(c, B, ansatz_kind, n_params, params);
    if (!rc) rc = qmps_set_hamiltonian(c, n_terms, h);
    if (!rc) rc = energy_launch(c, B, max_iter, tol, c->default_solver | QMPS_FLAG_KRYLOV_FALLBACK | ((c->D == 4 && c->default_solver == QMPS_ENV_DIRECT) ? QMPS_FLAG_NO_ENV_OUT : 0), false);
  }
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  return qmps_get_energies(c, B, E_out, iters_out, status_out);
}
QMPS_API_CATCH

int qmps_energy_batch_su(qmps_ctx* c, int64_t B, const double* params, const double* h, int n_terms, int max_iter, double tol,
                         double* E_out, int32_t* iters_out, int32_t* status_out) try {
  if (!c) return fail(QMPS_ERR_ARG, "null context");
  if (!E_out) return fail(QMPS_ERR_ARG, "null E_out");
  int rc;
  {
    Restore<bool> deferred(c->defer_sync, true);
    rc = qmps_set_states_su(c, B, params);
    if (!rc) rc = qmps_set_hamiltonian(c, n_terms, h);
    if (!rc) rc = energy_launch(c, B, max_iter, tol, c->default_solver | QMPS_FLAG_KRYLOV_FALLBACK, false);
  }
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  return qmps_get_energies(c, B, E_out, iters_out, status_out);
}
QMPS_API_CATCH

int qmps_env_batch(qmps_ctx* c, int64_t B, const double* states, int kind, const double* r0, int max_iter, double tol,
                   double* r_out, int32_t* iters_out, int32_t* status_out) try {
  if (!r_out) return fail(QMPS_ERR_ARG, "null r_out");
  if (int rc = qmps_set_states(c, B, states, kind)) return rc;
  if (c->n_terms < 1) {
    // the solve kernel always evaluates at least one Hamiltonian term; use h = 0
    double zero[32];
    memset(zero, 0, sizeof(zero));
    if (int rc = qmps_set_hamiltonian(c, 1, zero)) return rc;
  }
  if (int rc = qmps_set_env_guess(c, B, r0)) return rc;
  if (int rc = energy_launch(c, B, max_iter, tol, c->default_solver | QMPS_FLAG_KRYLOV_FALLBACK, false)) return rc;
  if (int rc = qmps_get_energies(c, B, nullptr, iters_out, status_out)) return rc;
  return qmps_get_env(c, B, r_out);
}
QMPS_API_CATCH

namespace {
// the two-site unit cell (D = 2 only, qmps/ground_state.py:276), a one-shot call: results at the start of the buffers, like the
// qmps_set_* calls.  cell2_prepare checks the arguments and makes room for the unitary pairs (d_U, d_U2), the caller fills them,
// cell2_run launches and reads back.
int cell2_prepare(qmps_ctx* c, int64_t B, bool have_input, const char* null_input, const double* h, int n_terms, int max_iter, double tol,
                  const double* E_out) {
  if (int rc = bind(c)) return rc;
  if (int rc = check_B(c, B)) return rc;
  if (c->D != 2) return fail(QMPS_ERR_ARG, "the two-site unit cell path is D = 2 only (qmps/ground_state.py:276)");
  c->window = 0;
  if (!have_input && B > 0) return fail(QMPS_ERR_ARG, "%s", null_input);
  if (!E_out) return fail(QMPS_ERR_ARG, "null E_out");
  if (max_iter < 1 || !(tol > 0.0)) return fail(QMPS_ERR_ARG, "bad max_iter / tol");
  if (int rc = qmps_set_hamiltonian(c, n_terms, h)) return rc;
  const size_t ub = 2 * tensor_bytes(c);
  if (!c->d_U) HIP_TRY(hipMalloc(&c->d_U, (size_t)c->max_batch * ub));
  if (!c->d_U2) HIP_TRY(hipMalloc(&c->d_U2, (size_t)c->max_batch * ub));
  return QMPS_OK;
}
int cell2_run(qmps_ctx* c, int64_t B, int n_terms, int max_iter, double tol, double* E_out, int32_t* iters_out, int32_t* status_out) {
  qmps::Cell2Args a;
  a.U1 = c->d_U; a.U2 = c->d_U2; a.h = c->d_h; a.E = c->d_E; a.E12 = nullptr;
  a.iters = c->d_iters; a.status = c->d_status; a.B = B; a.n_terms = n_terms; a.max_iter = max_iter; a.tol = tol;
  c->partials_B = -1;
  HIP_TRY(qmps::launch_cell2(c->D, a, c->stream));
  c->states.hold_tensors(0);  // the resident single-site states (if any) are no longer what d_E refers to
  forget_results(c);
  c->energies.add(0, B);      // the unit cell's own energies, iteration counts and statuses, at the start of the buffers
  c->counts.add(0, B);
  return qmps_get_energies(c, B, E_out, iters_out, status_out);
}
}  // namespace

int qmps_cell2_energy_batch(qmps_ctx* c, int64_t B, const double* U1, const double* U2, const double* h, int n_terms,
                             int max_iter, double tol, double* E_out, int32_t* iters_out, int32_t* status_out) try {
  if (int rc = cell2_prepare(c, B, U1 && U2, "null unitaries", h, n_terms, max_iter, tol, E_out)) return rc;
  const size_t ub = 2 * tensor_bytes(c);
  HIP_TRY(hipMemcpyAsync(c->d_U, U1, (size_t)B * ub, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_U2, U2, (size_t)B * ub, hipMemcpyHostToDevice, c->stream));
  return cell2_run(c, B, n_terms, max_iter, tol, E_out, iters_out, status_out);
}
QMPS_API_CATCH

int qmps_cell2_energy_batch_su(qmps_ctx* c, int64_t B, const double* params, const double* h, int n_terms, int max_iter, double tol,
                               double* E_out, int32_t* iters_out, int32_t* status_out) try {
  if (int rc = cell2_prepare(c, B, params != nullptr, "null params", h, n_terms, max_iter, tol, E_out)) return rc;
  if (int rc = ensure_scratch(c, (size_t)B * 30 * sizeof(double) + 256)) return rc;
  double* d_p = (double*)c->d_scratch;
  HIP_TRY(hipMemcpyAsync(d_p, params, (size_t)B * 30 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // U1 = U4(p[:15]), U2 = U4(p[15:])  (qmps/ground_state.py:300-301), both built on the device
  HIP_TRY(qmps::launch_su_exp(4, d_p, B, 30, c->d_U, 0, c->stream));
  HIP_TRY(qmps::launch_su_exp(4, d_p + 15, B, 30, c->d_U2, 0, c->stream));
  return cell2_run(c, B, n_terms, max_iter, tol, E_out, iters_out, status_out);
}
QMPS_API_CATCH
