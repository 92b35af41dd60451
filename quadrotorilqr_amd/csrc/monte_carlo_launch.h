// monte_carlo_launch.h -- what monte_carlo.hip gives the rest of the library: the launches of k_sample_gusts, k_sample_states and
// k_reduce_scores (monte_carlo_kernels.h) for qilqr_sample_gusts_device, qilqr_sample_states_device and qilqr_reduce_scores_device, and
// the rules of what those calls refuse.  Declarations and host code only -- no device code enters the translation unit that includes this
// (ilqr_capi.hip through host/caller_arrays.h); hidden: not part of the C ABI.  The rules compile under g++
// (tests/host_monte_carlo_harness.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ranges.h"

namespace qilqr {

// ---- the refusals, from facts alone (no device, no handle): null when the call is admitted, else the reason.  The arguments first, so
// that each is refused by its own reason whatever the handle is; the handle last.
namespace mc_rule {
inline const char *shape(long B, long S, long b0, long s0) {
  if (B <= 0 || S <= 0) return "B and S must be positive";
  if (b0 < 0 || s0 < 0) return "b0 and s0 must not be negative";
  return nullptr;
}
}  // namespace mc_rule

struct SampleGustsCall {
  bool handle, model;   // there is a handle; there is a model (the fields below are its)
  const void *wrench;   // the device array (only its address is looked at)
  long B, S, n_w, b0, s0;
  double mean[6], sigma[6], tau_force_s, tau_torque_s;
};
inline const char *sample_gusts_refusal(const SampleGustsCall &c) {
  if (!c.model || !c.wrench) return "sample gusts: null argument (the model and d_wrench are needed)";
  if (const char *why = mc_rule::shape(c.B, c.S, c.b0, c.s0)) return why;
  if (c.n_w <= 0) return "sample gusts: n_w must be positive";
  if (off_16_bytes({c.wrench})) return "sample gusts: d_wrench must be 16-byte aligned";
  for (int k = 0; k < 6; ++k) {
    if (!std::isfinite(c.mean[k])) return "sample gusts: the mean must be finite";
    if (!(c.sigma[k] >= 0.0) || !std::isfinite(c.sigma[k])) return "sample gusts: every sigma must be finite and not negative";
  }
  if (!(c.tau_force_s >= 0.0) || !std::isfinite(c.tau_force_s) || !(c.tau_torque_s >= 0.0) || !std::isfinite(c.tau_torque_s))
    return "sample gusts: the correlation times must be finite and not negative (0: white noise)";
  if (!c.handle) return "sample gusts: null handle";
  return nullptr;
}

struct SampleStatesCall {
  bool handle, sigma_given;
  const void *x_nom, *x0;  // the device arrays
  long B, S, b0, s0;
  unsigned long flags;
  double sigma[12];
};
inline const char *sample_states_refusal(const SampleStatesCall &c) {
  if (!c.x_nom || !c.sigma_given || !c.x0) return "sample states: null argument (d_x_nom, sigma12 and d_x0 are needed)";
  if (const char *why = mc_rule::shape(c.B, c.S, c.b0, c.s0)) return why;
  if (off_16_bytes({c.x_nom, c.x0})) return "sample states: d_x_nom and d_x0 must be 16-byte aligned";
  for (int k = 0; k < 12; ++k)
    if (!(c.sigma[k] >= 0.0) || !std::isfinite(c.sigma[k])) return "sample states: every sigma must be finite and not negative";
  if (c.flags & ~1ul) return "sample states: unknown flag bits (bit 0, the first sample is the nominal state, is the only one)";
  if (ranges_overlap(c.x0, sizeof(double) * 13 * (size_t)c.B * (size_t)c.S, c.x_nom, sizeof(double) * 13 * (size_t)c.B))
    return "sample states: d_x0 overlaps d_x_nom";
  if (!c.handle) return "sample states: null handle";
  return nullptr;
}

struct ReduceScoresCall {
  bool handle;
  const void *score, *summary;  // the device arrays
  long B, S;
};
inline const char *reduce_scores_refusal(const ReduceScoresCall &c) {
  if (!c.score || !c.summary) return "reduce scores: null argument (d_score and d_summary are needed)";
  if (c.B <= 0 || c.S <= 0) return "B and S must be positive";
  if (off_16_bytes({c.score, c.summary})) return "reduce scores: d_score and d_summary must be 16-byte aligned";
  if (ranges_overlap(c.summary, sizeof(double) * 8 * (size_t)c.B, c.score, sizeof(double) * 4 * (size_t)c.B * (size_t)c.S))
    return "reduce scores: d_summary overlaps d_score";
  if (!c.handle) return "reduce scores: null handle";
  return nullptr;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/quadrotor_ilqr.h"

namespace qilqr {

struct SampleGustsLaunch {
  double *d_wrench;  // [B][S][n_w][6], device
  int B, S, n_w, b0, s0;
  uint64_t seed;
  double dt;         // the handle's
  qilqr_gust_model model;  // the caller's
};
struct SampleStatesLaunch {
  const double *d_x_nom;  // [B][13], device
  double *d_x0;           // [B][S][13], device
  int B, S, b0, s0;
  uint32_t flags;
  uint64_t seed;
  double sigma[12];
};
struct ReduceScoresLaunch {
  const double *d_score;  // [B][S][4], device
  double *d_summary;      // [B][8], device
  int B, S;
};

// each enqueues its launch on `stream` and returns what the launch returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_sample_gusts(hipStream_t stream, const SampleGustsLaunch &call);
__attribute__((visibility("hidden"))) hipError_t launch_sample_states(hipStream_t stream, const SampleStatesLaunch &call);
__attribute__((visibility("hidden"))) hipError_t launch_reduce_scores(hipStream_t stream, const ReduceScoresLaunch &call);

}  // namespace qilqr
#endif
