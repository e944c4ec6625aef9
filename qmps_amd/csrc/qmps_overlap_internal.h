// qmps_overlap_internal.h - helpers of the overlap entry points (qmps_capi_overlap.hip) that the evolve drivers (qmps_capi_evolve.hip,
// qmps_capi_roto.hip) build on: the kernel route of a call (OverlapRoute), the lazy buffers, one gradient evaluation enqueued.
// Host side, library-internal.
#pragma once
#include "qmps_ctx.h"

namespace qmps_host {

// Which kernels the overlap solves of a call run, and how.  overlap_route is the ONLY reader of the documented switches of the
// overlap side; every call that launches overlap kernels computes it once, at its top, and passes it down.
enum class OverlapFamily { LaneD2, SquareD4, Block, MfmaD16 };      // Block: D = 8, D = 4 under QMPS_OVERLAP_POWER, D = 16 under QMPS_D16_BLOCK
struct OverlapRoute {
  OverlapFamily family;
  bool mfma;                // the flag of launch_overlap_d: the squaring kernel at D = 4, the matrix-core kernels at D = 16 (D = 8 ignores it)
  bool squares;             // rounds are squarings of the matrix of the map: at most 60, and no warm start
  bool d16_switches_off;    // neither QMPS_D16_BLOCK nor QMPS_D16_ONE_WAVE, whatever D
  bool split_d16;           // D = 16 and d16_switches_off: work queue above 2 048 evaluations, pair launch, neighbour build inside it
  bool pair;                // the gradient's two solves go in one launch: D = 8, or split_d16
  bool krylov;              // the Krylov fall-back may be armed (arm_krylov)
  int no_deflation;         // OverlapArgs::no_deflation of every solve
  const char* name;         // c->dominant of a plain launch (qmps_kernel_time)
};
OverlapRoute overlap_route(const qmps_ctx* c);

int ensure_refs(qmps_ctx* c, int64_t n_ref);
int set_ww(qmps_ctx* c, const double* WW);
int ensure_overlap_outputs(qmps_ctx* c);
int ensure_gradient_buffers(qmps_ctx* c, int64_t T);      // what enqueue_gradient_kernels needs for T iterates
int ensure_mask_buffers(qmps_ctx* c);
int launch_overlap_kernels(qmps_ctx* c, const OverlapRoute& route, const qmps::OverlapArgs& a_in);
int flush_mask(qmps_ctx* c);

// The one-shot fields armed for "the next launch" (qmps_overlap_set_active's mask, the lock-step driver's warm-from-group and fork
// requests, per-trajectory tolerances) are spent on EVERY way out of the call that was to consume them - also when an earlier stage
// of that call fails: a later, unrelated launch must never inherit them.
struct DisarmOneShots {
  qmps_ctx* c;
  ~DisarmOneShots() { c->active_n = 0; c->mask_stash_n = 0; c->mask_host = nullptr; c->fork_after_copy = nullptr; c->warm_from_group = 0; c->grad_tol_in = nullptr; }
};

// Where a gradient evaluation of T iterates builds the tensors of their 2 P central-difference neighbours: inside the D = 16 pair
// launch, on the second stream beside the eigen-solves, or on the context stream in front of the probes
enum class NeighbourBuild { InPair, Beside, Inline };
NeighbourBuild neighbour_build(const qmps_ctx* c, const OverlapRoute& route, int64_t T, int kind, int P);

// One gradient evaluation of T iterates, ENQUEUED on the context stream and nothing else (see qmps_capi_overlap.hip)
struct GradPass {
  qmps::OverlapArgs a, l;
  qmps::OverlapGradArgs g;
  bool lazy_krylov = false;
};
int enqueue_gradient_kernels(qmps_ctx* c, const OverlapRoute& route, int64_t T, int kind, int P, const double* d_src, double h, int max_rounds, double tol, bool warm,
                             bool two_sided_f, const unsigned char* mask, bool allow_lazy_krylov, GradPass& gp, const double* tol_in = nullptr);

}  // namespace qmps_host
