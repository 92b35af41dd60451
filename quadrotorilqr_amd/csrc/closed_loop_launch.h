// closed_loop_launch.h -- what closed_loop.hip and closed_loop_scored.hip give the rest of the library: the launch of k_closed_loop
// (closed_loop_kernels.h) and of k_closed_loop_scored (closed_loop_scored_kernels.h) for one call of qilqr_closed_loop[_scored][_device],
// and the rule of what such calls refuse.  Declarations and host code only -- no device code enters the translation unit that includes
// this (ilqr_capi.hip through host/caller_arrays.h); hidden: not part of the C ABI.  The rule compiles under g++
// (tests/host_closed_loop_harness.cpp, tests/host_scored_flight_harness.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "call_parts.h"
#include "ranges.h"

namespace qilqr {

// ---- the refusals, from facts alone (no device, no handle): null when the call is admitted, else the reason.  ONE rule: the plain
// call is the scored call without a wrench, a desired trajectory or a score (closed_loop_refusal below).
struct ClosedLoopCall {
  const void *plan, *gains, *x0, *out_traj, *out_stats;  // the caller's arrays (host or device ones: only their addresses are looked at)
  long B, n, S, i0, i1;
  bool handle;    // there is a handle
  bool f32;       // ... in the mixed-precision mode
  bool modeled;   // ... with per-problem models set
  long models_B;  // ... for how many
  const void *out_score = nullptr;  // (the scored call's third output)
};
struct ClosedLoopScoredCall {
  ClosedLoopCall base;  // (base.out_score: the score array)
  const void *wrench, *desired;
  long n_w;
  long pobs_B;     // the handle's per-problem sphere table: for how many problems (0: none is set)
  long n_desired;  // ... its desired trajectory's knots
  long n_sched;    // ... its state-weight schedule's (0: none)
  long k0;         // ... its horizon start
};
// The order: the arguments the plain call has (so that each is refused by its own reason whatever the handle is), the scored call's
// arguments, the handle as the plain call looks at it, then the handle's tables and lengths.  Every test of the second and the fourth
// group is guarded by a pointer the plain call does not have.  length: the reason is one of length (QILQR_ERR_LENGTH_MISMATCH).
inline const char *closed_loop_scored_refusal(const ClosedLoopScoredCall &s, bool *length) {
  *length = false;
  const ClosedLoopCall &c = s.base;
  if (!c.plan || !c.gains || !c.x0) return "closed loop: null argument (plan, gains and x0 are needed)";
  if (!c.out_traj && !c.out_stats && !c.out_score) return "closed loop: no output (out_traj and out_stats are both null)";
  if (c.B <= 0 || c.n <= 0 || c.S <= 0) return "closed loop: B, n and S must be positive";
  if (c.i0 < 0 || c.i1 < c.i0 || c.i1 > c.n - 1) return "closed loop: the knots must satisfy 0 <= i0 <= i1 <= n - 1";
  if (off_16_bytes({c.plan, c.gains, c.x0, c.out_traj, c.out_stats})) return "closed loop: every array must be 16-byte aligned";
  // the samples run in parallel and every one reads the inputs: an output that overlaps an input (or another output) is a race
  const size_t samples = (size_t)c.B * (size_t)c.S, knots = (size_t)c.B * c.n;
  enum { PLAN, GAINS, X0, WRENCH, DESIRED, TRAJ, STATS, SCORE, RANGES };  // the inputs, then the outputs
  const struct { const void *p; size_t bytes; } r[RANGES] = {{c.plan, sizeof(double) * 18 * knots},
                                                             {c.gains, sizeof(double) * 52 * knots},
                                                             {c.x0, sizeof(double) * 13 * samples},
                                                             {s.wrench, sizeof(double) * 6 * samples * (size_t)(s.wrench ? s.n_w : 0)},
                                                             {s.desired, sizeof(double) * 18 * knots},
                                                             {c.out_traj, sizeof(double) * 18 * samples * c.n},
                                                             {c.out_stats, sizeof(double) * 4 * samples},
                                                             {c.out_score, sizeof(double) * 4 * samples}};
  auto overlap = [&r](int a, int b) { return ranges_overlap(r[a].p, r[a].bytes, r[b].p, r[b].bytes); };
  for (int o = TRAJ; o <= STATS; ++o)
    for (int k = PLAN; k <= X0; ++k)
      if (overlap(o, k)) return "closed loop: an output overlaps an input";
  if (overlap(TRAJ, STATS)) return "closed loop: the outputs overlap each other";
  if (s.wrench && s.n_w != 1 && s.n_w != c.n) return "closed loop: n_w must be 1 (one wrench per sample) or n (one per knot)";
  if (off_16_bytes({s.wrench, s.desired, c.out_score})) return "closed loop: wrench, desired and out_score must be 16-byte aligned";
  for (int k = PLAN; k < SCORE; ++k)
    if (overlap(SCORE, k)) return k < TRAJ ? "closed loop: the score overlaps an input" : "closed loop: the score overlaps another output";
  for (int o = TRAJ; o <= STATS; ++o)
    for (int k = WRENCH; k <= DESIRED; ++k)
      if (overlap(o, k)) return "closed loop: an output overlaps an input";
  if (!c.handle) return "closed loop: null handle";
  if (c.f32) return "closed loop: needs precision 0 (fp64)";
  if (c.modeled && c.models_B != c.B * c.S)
    return "closed loop: the per-problem models must have been set for B * S samples (model b S + j flies sample (b, j))";
  if (c.out_score) {
    if (s.pobs_B > 0 && s.pobs_B != c.B) return "closed loop: the per-problem obstacles were set for another B than this call's (the score reads row b of that table)";
    if (!s.desired && beyond_desired(c.i1, s.n_desired, s.k0)) {
      *length = true;
      return "closed loop: the scored knots reach beyond the handle's desired trajectory";
    }
    if (beyond_schedule(c.i1, s.n_sched, s.k0)) {
      *length = true;
      return "closed loop: the scored knots reach beyond the state-weight schedule";
    }
  }
  return nullptr;
}
inline const char *closed_loop_refusal(ClosedLoopCall c) {
  c.out_score = nullptr;
  bool length;
  return closed_loop_scored_refusal(ClosedLoopScoredCall{c, nullptr, nullptr, 0, 0, 0, 0, 0}, &length);
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "box_qp.h"
#include "se3_math.h"

namespace qilqr {

struct ClosedLoopLaunch {
  const double *d_plan;     // [B][n][18], device
  const double *d_gains;    // [B][n][52], device
  const double *d_x0;       // [B][S][13], device
  double *d_out_traj;       // [B][S][n][18], device, or null
  double *d_out_stats;      // [B][S][4], device, or null
  int B, n, S, i0, i1;
  int integrator;                // 0 explicit Euler, 1 Runge-Kutta
  const ControlLimits *limits;   // the handle's thrust limits, or null
  const double *d_models;        // the per-problem model records (batch_models.h) of these B * S samples, or null
};

// the form (closed_loop_kernels.h: closed_loop_shared_form, and the one place the diagnostics build overrides it) and the grid of a flight
// of B plans with S samples each; false: more blocks than a grid holds.  closed_loop.hip's, for both units.
__attribute__((visibility("hidden"))) bool closed_loop_form(int B, int S, bool *shared, dim3 *grid);

// enqueues the launch on `stream` and returns what the launch returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_closed_loop(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopLaunch &call);

// the kernels' first argument record of a call (closed_loop_kernels.h), for both units
struct ClosedLoopArgs;
__attribute__((visibility("hidden"))) ClosedLoopArgs closed_loop_args(const ClosedLoopLaunch &call);

// the scored call: the plain call's launch record and what the score and the wrench read (every pointer a device one).  A call with
// neither a wrench nor a score goes to launch_closed_loop.
struct ClosedLoopScoredLaunch {
  ClosedLoopLaunch base;
  const double *d_wrench;   // [B][S][n_w][6], or null
  int n_w;
  double *d_out_score;      // [B][S][4], or null: no score (then `score` is not read)
  ScoreOperands score;      // from the window's first knot (call_parts.h)
};
__attribute__((visibility("hidden"))) hipError_t launch_closed_loop_scored(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopScoredLaunch &call);

}  // namespace qilqr
#endif
