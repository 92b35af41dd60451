// mppi_launch.h -- what mppi.hip gives the rest of the library: the launches of k_mppi_flight and k_mppi_update (mppi_kernels.h) for
// qilqr_mppi_flight_device and qilqr_mppi_update_device, the rule of what those calls refuse, and the rule of their grids (the one
// statement of the update's block size, which mppi_adapt.hip and the host programs of tests/ use too).  Declarations
// and host code only -- no device code enters the translation unit that includes this (ilqr_capi.hip through host/caller_arrays.h);
// hidden: not part of the C ABI.  The rules compile under g++ (tests/host_mppi_harness.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "call_parts.h"
#include "ranges.h"

namespace qilqr {

// ---- the grids, from the counts alone
// k_mppi_flight: a block is one wavefront of 64 samples of one plan -- B cdiv(S, 64) blocks of 64 lanes; 0: more than a grid holds
inline long mppi_flight_blocks(long B, long S) {
  const long blocks = B * ((S + 63) / 64);
  return blocks > 0x7fffffffl ? 0 : blocks;
}
// k_mppi_update and k_mppi_adapt: one block per plan of the power of two >= S lanes, 64 at the least and 1024 at the most -- THE rule,
// for the launches and for the host programs of tests/; a lane carries cdiv(S, lanes) samples, 4 at S = 4096 (a lane without a sample
// folds nothing and adds +0 to the sums)
inline int mppi_update_lanes(long S) {
  int T = 64;
  while (T < S && T < 1024) T <<= 1;
  return T;
}
inline int mppi_update_threads(int S) { return mppi_update_lanes(S); }  // (the name mppi_kernels.h had for it: host programs written against that)
inline int mppi_samples_per_lane(long S) { return (int)((S + mppi_update_lanes(S) - 1) / mppi_update_lanes(S)); }
// go(std::integral_constant<int, mppi_update_lanes(S)>): the block size as the template argument of those kernels
template <typename Go>
auto with_update_lanes(long S, Go &&go) {
  switch (mppi_update_lanes(S)) {
    case 64: return go(std::integral_constant<int, 64>{});
    case 128: return go(std::integral_constant<int, 128>{});
    case 256: return go(std::integral_constant<int, 256>{});
    case 512: return go(std::integral_constant<int, 512>{});
    default: return go(std::integral_constant<int, 1024>{});
  }
}

// ---- the refusals, from facts alone (no device): null when the call is admitted, else the reason.  ONE rule for both calls; `update`
// says which.  THE ORDER:
//    1  a NULL rule, plan or score -- and, of the update, a NULL out_plan or info
//    2  B, n or S not positive, or n < 2 (a flight has a step)
//    3  S above QILQR_RISK_MAX_SAMPLES (4096)
//    4  a negative b0
//    5  a sigma that is NaN or negative
//    6  lambda not > 0, or NaN
//    7  a tau_s or a collision_cost that is negative or NaN
//    8  unknown flag bits, or reserved != 0
//    9  an array off a 16-byte boundary
//   10  an output overlapping an input: the flight's score, the update's out_plan (over plan, x0, desired -- and, the update's, score)
//   11  the update's info overlapping anything
//   12  a NULL handle
// and then the handle as the scored closed-loop flight looks at it: the mixed-precision mode, per-problem models or per-problem spheres
// set for another B, and -- a reason of length (QILQR_ERR_LENGTH_MISMATCH) -- knots beyond the handle's desired trajectory or schedule.
struct MppiCall {
  bool update;                                           // qilqr_mppi_update_device (else qilqr_mppi_flight_device)
  bool rule;                                             // there is a rule (the seven fields below are its)
  double sigma[4], tau_s, lambda, collision_cost;
  unsigned long flags, reserved;
  const void *plan, *x0, *desired, *score, *out_plan, *info;  // the device arrays (only their addresses are looked at)
  long B, n, S, b0;
  bool handle;     // there is a handle
  bool f32;        // ... in the mixed-precision mode
  bool modeled;    // ... with per-problem models set
  long models_B;   // ... for how many
  long pobs_B;     // its per-problem sphere table: for how many problems (0: none is set)
  long n_desired;  // its desired trajectory's knots
  long n_sched;    // its state-weight schedule's (0: none)
  long k0;         // its horizon start
};
inline const char *mppi_refusal(const MppiCall &c, bool *length) {
  *length = false;
  if (!c.rule || !c.plan || !c.score) return "mppi: null argument (the rule, d_plan and d_score are needed)";
  if (c.update && (!c.out_plan || !c.info)) return "mppi: null argument (d_out_plan and d_info are needed)";
  if (c.B <= 0 || c.n <= 0 || c.S <= 0) return "mppi: B, n and S must be positive";
  if (c.n < 2) return "mppi: n must be at least 2 (a flight has a step)";
  if (c.S > 4096) return "mppi: S must not exceed QILQR_RISK_MAX_SAMPLES (4096: one block weighs a plan's samples)";
  if (c.b0 < 0) return "mppi: b0 must not be negative";
  for (int a = 0; a < 4; ++a)
    if (!(c.sigma[a] >= 0.0)) return "mppi: every sigma must be a number and not negative";
  if (!(c.lambda > 0.0)) return "mppi: lambda must be positive";
  if (!(c.tau_s >= 0.0) || !(c.collision_cost >= 0.0)) return "mppi: tau_s and collision_cost must be numbers and not negative";
  if (c.flags & ~1ul) return "mppi: unknown flag bits (bit 0, QILQR_MPPI_FIRST_IS_NOMINAL, is the only one)";
  if (c.reserved != 0) return "mppi: the rule's reserved word must be 0";
  if (off_16_bytes({c.plan, c.x0, c.desired, c.score})) return "mppi: every array must be 16-byte aligned";
  if (c.update && off_16_bytes({c.out_plan, c.info})) return "mppi: every array must be 16-byte aligned";
  const size_t knots = sizeof(double) * 18 * (size_t)c.B * (size_t)c.n, states = sizeof(double) * 13 * (size_t)c.B,
               scores = sizeof(double) * 4 * (size_t)c.B * (size_t)c.S, infos = sizeof(double) * 8 * (size_t)c.B;
  const struct { const void *p; size_t bytes; } in[4] = {{c.plan, knots}, {c.x0, states}, {c.desired, knots}, {c.update ? c.score : nullptr, scores}};
  const void *out = c.update ? c.out_plan : c.score;
  const size_t out_bytes = c.update ? knots : scores;
  for (int k = 0; k < 4; ++k)
    if (ranges_overlap(out, out_bytes, in[k].p, in[k].bytes))
      return c.update ? "mppi: d_out_plan overlaps an input (the update does not work in place)" : "mppi: d_score overlaps an input";
  if (c.update) {
    for (int k = 0; k < 4; ++k)
      if (ranges_overlap(c.info, infos, in[k].p, in[k].bytes)) return "mppi: d_info overlaps an input";
    if (ranges_overlap(c.info, infos, c.out_plan, knots)) return "mppi: d_info overlaps d_out_plan";
  }
  if (!c.handle) return "mppi: null handle";
  if (c.f32) return "mppi: needs precision 0 (fp64)";
  if (c.modeled && c.models_B != c.B) return "mppi: the per-problem models must have been set for B plans (plan b flies with model b)";
  if (c.pobs_B > 0 && c.pobs_B != c.B) return "mppi: the per-problem obstacles were set for another B than this call's (the score reads row b of that table)";
  if (!c.desired && beyond_desired(c.n - 1, c.n_desired, c.k0)) {
    *length = true;
    return "mppi: the scored knots reach beyond the handle's desired trajectory";
  }
  if (beyond_schedule(c.n - 1, c.n_sched, c.k0)) {
    *length = true;
    return "mppi: the scored knots reach beyond the state-weight schedule";
  }
  return nullptr;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/quadrotor_ilqr.h"
#include "box_qp.h"
#include "se3_math.h"

namespace qilqr {

// one call's launch record; every pointer a device one.  The flight reads all but out_plan and info; the update all.
struct MppiLaunch {
  const double *d_plan;     // [B][n][18]
  const double *d_x0;       // [B][13], or null: words 1..13 of the plan's knot 0
  double *d_score;          // [B][S][4]: the flight's output, the update's input
  double *d_out_plan;       // [B][n][18] (update)
  double *d_info;           // [B][8] (update)
  int B, n, S, b0;
  uint64_t seed;
  qilqr_mppi_rule rule;          // the caller's
  int integrator;                // 0 explicit Euler, 1 Runge-Kutta
  const ControlLimits *limits;   // the handle's thrust limits, or null
  const double *d_models;        // the per-problem model records (batch_models.h) of these B plans, or null
  ScoreOperands score;           // from the plan's first knot (call_parts.h)
};

// each enqueues its launches on `stream` and returns what they returned; nothing is waited for.  The update is two launches:
// k_mppi_update, then k_mppi_flight with one sample, eps = 0 and the trajectory store on, over d_out_plan.
__attribute__((visibility("hidden"))) hipError_t launch_mppi_flight(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call);
__attribute__((visibility("hidden"))) hipError_t launch_mppi_update(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call);
// the second launch alone (mppi_adapt.hip enqueues it behind k_mppi_adapt): reads d_plan (knot 0, without d_x0), d_out_plan and writes it, and words 4 .. 7 of d_info
__attribute__((visibility("hidden"))) hipError_t launch_mppi_nominal_flight(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call);

}  // namespace qilqr
#endif
