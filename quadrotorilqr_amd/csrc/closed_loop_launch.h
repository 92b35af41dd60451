// closed_loop_launch.h -- what closed_loop.hip gives the rest of the library: the launch of k_closed_loop (closed_loop_kernels.h) for one
// call of qilqr_closed_loop[_device], and the rule of what such a call refuses.  Declarations and host code only -- no device code enters
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
};
// The arguments first (so that each is refused by its own reason whatever the handle is), then the handle.
inline const char *closed_loop_refusal(const ClosedLoopCall &c) {
  if (!c.plan || !c.gains || !c.x0) return "closed loop: null argument (plan, gains and x0 are needed)";
  if (!c.out_traj && !c.out_stats) return "closed loop: no output (out_traj and out_stats are both null)";
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
  if (!c.handle) return "closed loop: null handle";
  if (c.f32) return "closed loop: needs precision 0 (fp64)";
  if (c.modeled && c.models_B != c.B * c.S)
    return "closed loop: the per-problem models must have been set for B * S samples (model b S + j flies sample (b, j))";
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

}  // namespace qilqr
#endif
