// cov_launch.h -- what cov.hip gives the rest of the library: the launches of k_cov_build, k_cov_chain and k_cov_summary (cov_kernels.h) for
// qilqr_covariance_device, and the rule of what that call refuses.  Declarations and host code only -- no device code enters the
// translation unit that includes this (ilqr_capi.hip through host/caller_arrays.h); hidden: not part of the C ABI.  The rule compiles
// under g++ (tests/host_cov_harness.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ranges.h"

namespace qilqr {

constexpr int COV_IMAGE = 320;  // words of a knot's operand image in the handle's scratch (cov_kernels.h): five chunks of 64 lanes

// the call's constants, formed once on the host (cov_coeffs)
struct CovCoeffs {
  double s02[12];  // state_sigma^2
  double sg2[6];   // sigma_c^2
  double rho[6];   // the gust's one-step correlation (1: the wrench is held over the flight)
  double mean[6];
};
inline void cov_coeffs(const double state_sigma[12], const double mean[6], const double sigma[6], double tau_force_s, double tau_torque_s, bool held,
                       double dt, CovCoeffs &k) {
  for (int e = 0; e < 12; ++e) k.s02[e] = state_sigma[e] * state_sigma[e];
  for (int c = 0; c < 6; ++c) {
    const double tau = c < 3 ? tau_force_s : tau_torque_s;
    k.sg2[c] = sigma[c] * sigma[c];
    k.rho[c] = held ? 1.0 : (tau > 0.0 ? exp(-dt / tau) : 0.0);  // (gust_coeffs' rho, monte_carlo_kernels.h)
    k.mean[c] = mean[c];
  }
}

// ---- the refusals, from facts alone (no device): null when the call is admitted, else the reason.  THE ORDER:
//   1  a NULL rule or plan                      7  unknown flag bits, or reserved != 0
//   2  every output NULL                        8  an array off a 16-byte boundary
//   3  B or n not positive                      9  an output overlapping an input or another output
//   4  the knots out of range                  10  a NULL handle, then a mixed-precision one
//   5  a negative or non-finite sigma or tau   11  per-problem models, then per-problem spheres, set for another B
//   6  a non-finite mean
struct CovCall {
  bool rule;                   // there is a rule (the fields below are its)
  double state_sigma[12], mean[6], sigma[6], tau_force_s, tau_torque_s;
  unsigned long flags, reserved;
  const void *plan, *gains, *cov, *mean_out, *summary;  // the device arrays (only their addresses are looked at)
  long B, n, i0, i1;
  bool handle, f32, modeled;   // there is a handle; in the mixed-precision mode; with per-problem models
  long models_B, pobs_B;       // ... set for how many; its per-problem sphere table (0: none)
};
inline const char *cov_refusal(const CovCall &c) {
  if (!c.rule || !c.plan) return "covariance: null argument (the rule and d_plan are needed)";
  if (!c.cov && !c.mean_out && !c.summary) return "covariance: no output (d_cov, d_mean and d_summary are all null)";
  if (c.B <= 0 || c.n <= 0) return "covariance: B and n must be positive";
  if (c.i0 < 0 || c.i1 < c.i0 || c.i1 > c.n - 1) return "covariance: the knots must satisfy 0 <= i0 <= i1 <= n - 1";
  for (int k = 0; k < 12; ++k)
    if (!(c.state_sigma[k] >= 0.0) || !std::isfinite(c.state_sigma[k])) return "covariance: every sigma must be finite and not negative";
  for (int k = 0; k < 6; ++k)
    if (!(c.sigma[k] >= 0.0) || !std::isfinite(c.sigma[k])) return "covariance: every sigma must be finite and not negative";
  if (!(c.tau_force_s >= 0.0) || !std::isfinite(c.tau_force_s) || !(c.tau_torque_s >= 0.0) || !std::isfinite(c.tau_torque_s))
    return "covariance: the correlation times must be finite and not negative (0: white noise)";
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(c.mean[k])) return "covariance: the mean must be finite";
  if (c.flags & ~1ul) return "covariance: unknown flag bits (QILQR_COV_WRENCH_HELD is the only one)";
  if (c.reserved != 0) return "covariance: the rule's reserved word must be 0";
  if (off_16_bytes({c.plan, c.gains, c.cov, c.mean_out, c.summary})) return "covariance: every array must be 16-byte aligned";
  const size_t knots = (size_t)c.B * (size_t)c.n;
  enum { PLAN, GAINS, COV, MEAN, SUMMARY, RANGES };  // the inputs, then the outputs
  const struct { const void *p; size_t bytes; } r[RANGES] = {{c.plan, sizeof(double) * 18 * knots},
                                                             {c.gains, sizeof(double) * 52 * knots},
                                                             {c.cov, sizeof(double) * 144 * knots},
                                                             {c.mean_out, sizeof(double) * 12 * knots},
                                                             {c.summary, sizeof(double) * 8 * (size_t)c.B}};
  for (int o = COV; o <= SUMMARY; ++o)
    for (int k = PLAN; k <= GAINS; ++k)
      if (ranges_overlap(r[o].p, r[o].bytes, r[k].p, r[k].bytes)) return "covariance: an output overlaps an input";
  for (int o = COV; o <= SUMMARY; ++o)
    for (int k = o + 1; k <= SUMMARY; ++k)
      if (ranges_overlap(r[o].p, r[o].bytes, r[k].p, r[k].bytes)) return "covariance: the outputs overlap each other";
  if (!c.handle) return "covariance: null handle";
  if (c.f32) return "covariance: needs precision 0 (fp64)";
  if (c.modeled && c.models_B != c.B) return "covariance: the per-problem models were set for another B than this call's (plan b takes model b)";
  if (c.pobs_B > 0 && c.pobs_B != c.B) return "covariance: the per-problem obstacles were set for another B than this call's (the summary reads row b of that table)";
  return nullptr;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/quadrotor_ilqr.h"
#include "call_parts.h"
#include "se3_math.h"

namespace qilqr {

// one admitted call; every pointer a device one
struct CovLaunch {
  const double *d_plan;    // [B][n][18]
  const double *d_gains;   // [B][n][52], or null: the open loop
  double *d_image;         // [B][n][COV_IMAGE]: the handle's scratch (pads zero)
  double *d_cov;           // [B][n][144]: the caller's, or the handle's scratch when the caller gave none and asks for a summary; else null
  double *d_mean;          // [B][n][12]: likewise
  double *d_summary;       // [B][8], or null
  int B, n, i0, i1;
  int integrator;          // 0 explicit Euler, 1 Runge-Kutta
  const double *d_models;  // the per-problem model records (batch_models.h) of these B plans, or null
  qilqr_cov_rule rule;     // the caller's
  SphereTables spheres;    // the handle's (call_parts.h)
};
// enqueues the two or three launches on `stream` and returns what they returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_covariance(hipStream_t stream, const ModelConsts<double> &consts, const CovLaunch &call);

}  // namespace qilqr
#endif
