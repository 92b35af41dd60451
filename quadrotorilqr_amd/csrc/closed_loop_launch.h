// closed_loop_launch.h -- what closed_loop.hip and closed_loop_scored.hip give the rest of the library: the launch of k_closed_loop
// (closed_loop_kernels.h) for one call of qilqr_closed_loop[_device], that of k_closed_loop_scored (closed_loop_scored_kernels.h) for one
// of qilqr_closed_loop_scored[_device], and the rules of what such calls refuse.  Declarations and host code only -- no device code enters
// the translation unit that includes this (ilqr_capi.hip through host/api_calls.h); hidden: not part of the C ABI.  The rule compiles
// under g++ (tests/host_closed_loop_harness.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace qilqr {

// ---- the refusals, from facts alone (no device, no handle): null when the call is admitted, else the reason
struct ClosedLoopCall {
  const void *plan, *gains, *x0, *out_traj, *out_stats;  // the caller's arrays (host or device ones: only their addresses are looked at)
  long B, n, S, i0, i1;
  bool handle;    // there is a handle
  bool f32;       // ... in the mixed-precision mode
  bool modeled;   // ... with per-problem models set
  long models_B;  // ... for how many
  const void *out_score = nullptr;  // (the scored call's third output: only whether there is one is looked at here)
};
// The arguments first (so that each is refused by its own reason whatever the handle is), then the handle.
inline const char *closed_loop_argument_refusal(const ClosedLoopCall &c) {
  if (!c.plan || !c.gains || !c.x0) return "closed loop: null argument (plan, gains and x0 are needed)";
  if (!c.out_traj && !c.out_stats && !c.out_score) return "closed loop: no output (out_traj and out_stats are both null)";
  if (c.B <= 0 || c.n <= 0 || c.S <= 0) return "closed loop: B, n and S must be positive";
  if (c.i0 < 0 || c.i1 < c.i0 || c.i1 > c.n - 1) return "closed loop: the knots must satisfy 0 <= i0 <= i1 <= n - 1";
  if (((uintptr_t)c.plan | (uintptr_t)c.gains | (uintptr_t)c.x0 | (uintptr_t)c.out_traj | (uintptr_t)c.out_stats) & 15)
    return "closed loop: every array must be 16-byte aligned";
  // the samples run in parallel and every one reads the inputs: an output that overlaps an input (or the other output) is a race
  const size_t samples = (size_t)c.B * (size_t)c.S;
  const struct { const void *p; size_t bytes; } in[3] = {{c.plan, sizeof(double) * 18 * (size_t)c.B * c.n},
                                                         {c.gains, sizeof(double) * 52 * (size_t)c.B * c.n},
                                                         {c.x0, sizeof(double) * 13 * samples}},
                                                out[2] = {{c.out_traj, sizeof(double) * 18 * samples * c.n}, {c.out_stats, sizeof(double) * 4 * samples}};
  auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return x && y && x < y + nb && y < x + na;
  };
  for (int o = 0; o < 2; ++o)
    for (int k = 0; k < 3; ++k)
      if (overlap(out[o].p, out[o].bytes, in[k].p, in[k].bytes)) return "closed loop: an output overlaps an input";
  if (overlap(out[0].p, out[0].bytes, out[1].p, out[1].bytes)) return "closed loop: the outputs overlap each other";
  return nullptr;
}
inline const char *closed_loop_handle_refusal(const ClosedLoopCall &c) {
  if (!c.handle) return "closed loop: null handle";
  if (c.f32) return "closed loop: needs precision 0 (fp64)";
  if (c.modeled && c.models_B != c.B * c.S)
    return "closed loop: the per-problem models must have been set for B * S samples (model b S + j flies sample (b, j))";
  return nullptr;
}
inline const char *closed_loop_refusal(const ClosedLoopCall &c) {
  const char *why = closed_loop_argument_refusal(c);
  return why ? why : closed_loop_handle_refusal(c);
}

// ---- the scored call: closed_loop_refusal's facts and the new ones.  The order: the arguments the plain call has, the new arguments, the
// handle as the plain call looks at it, then the handle's tables and lengths.  length: the reason is one of length (QILQR_ERR_LENGTH_MISMATCH).
struct ClosedLoopScoredCall {
  ClosedLoopCall base;  // (base.out_score: the score array)
  const void *wrench, *desired;
  long n_w;
  long pobs_B;     // the handle's per-problem sphere table: for how many problems (0: none is set)
  long n_desired;  // ... its desired trajectory's knots
  long n_sched;    // ... its state-weight schedule's (0: none)
  long k0;         // ... its horizon start
};
inline const char *closed_loop_scored_refusal(const ClosedLoopScoredCall &s, bool *length) {
  *length = false;
  const ClosedLoopCall &c = s.base;
  const char *why = closed_loop_argument_refusal(c);
  if (why) return why;
  if (s.wrench && s.n_w != 1 && s.n_w != c.n) return "closed loop: n_w must be 1 (one wrench per sample) or n (one per knot)";
  if (((uintptr_t)s.wrench | (uintptr_t)s.desired | (uintptr_t)c.out_score) & 15) return "closed loop: wrench, desired and out_score must be 16-byte aligned";
  const size_t samples = (size_t)c.B * (size_t)c.S;
  const struct { const void *p; size_t bytes; } other[7] = {{c.plan, sizeof(double) * 18 * (size_t)c.B * c.n},
                                                            {c.gains, sizeof(double) * 52 * (size_t)c.B * c.n},
                                                            {c.x0, sizeof(double) * 13 * samples},
                                                            {s.wrench, sizeof(double) * 6 * samples * (size_t)(s.wrench ? s.n_w : 0)},
                                                            {s.desired, sizeof(double) * 18 * (size_t)c.B * c.n},
                                                            {c.out_traj, sizeof(double) * 18 * samples * c.n},
                                                            {c.out_stats, sizeof(double) * 4 * samples}};
  auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
    const char *x = (const char *)a, *y = (const char *)b;
    return x && y && x < y + nb && y < x + na;
  };
  const size_t score_bytes = sizeof(double) * 4 * samples;
  for (int k = 0; k < 7; ++k)
    if (overlap(c.out_score, score_bytes, other[k].p, other[k].bytes))
      return k < 5 ? "closed loop: the score overlaps an input" : "closed loop: the score overlaps another output";
  for (int o = 5; o < 7; ++o)
    for (int k = 3; k < 5; ++k)
      if (overlap(other[o].p, other[o].bytes, other[k].p, other[k].bytes)) return "closed loop: an output overlaps an input";
  if ((why = closed_loop_handle_refusal(c))) return why;
  if (c.out_score) {
    if (s.pobs_B > 0 && s.pobs_B != c.B) return "closed loop: the per-problem obstacles were set for another B than this call's (the score reads row b of that table)";
    if (!s.desired && c.i1 >= s.n_desired - s.k0) {
      *length = true;
      return "closed loop: the scored knots reach beyond the handle's desired trajectory";
    }
    if (s.n_sched > 0 && c.i1 >= s.n_sched - s.k0) {
      *length = true;
      return "closed loop: the scored knots reach beyond the state-weight schedule";
    }
  }
  return nullptr;
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

// enqueues the launch on `stream` and returns what the launch returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_closed_loop(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopLaunch &call);

// the scored call: the plain call's launch record and what the score and the wrench read (every pointer a device one).  A call with
// neither a wrench nor a score goes to launch_closed_loop.
struct ClosedLoopScoredLaunch {
  ClosedLoopLaunch base;
  const double *d_wrench;   // [B][S][n_w][6], or null
  int n_w;
  double *d_out_score;      // [B][S][4], or null: no score (then nothing below is read)
  const double *d_desired;  // the first desired knot of the window: per plan [B][n][18] (desired_step = n * 18), or the handle's (0)
  long desired_step;
  const double *d_q;        // the state weights of the window's first knot, 16-byte aligned: a schedule's (q_step = 144) or the handle's Q (0)
  int q_step;
  const double *d_shared;   // the handle's sphere tables
  int n_shared;
  const double *d_own;
  const int *d_own_counts;
  int own_K;
};
__attribute__((visibility("hidden"))) hipError_t launch_closed_loop_scored(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopScoredLaunch &call);

}  // namespace qilqr
#endif
