// risk_launch.h -- what risk.hip gives the rest of the library: the launches of k_risk_scores, k_select_plans and k_gather_plans
// (risk_kernels.h) for qilqr_risk_scores_device and qilqr_select_plans_device, and the rules of what those calls refuse.  Declarations and
// host code only -- no device code enters the translation unit that includes this (ilqr_capi.hip through host/caller_arrays.h); hidden:
// not part of the C ABI.  The rules compile under g++ (tests/host_risk_harness.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "ranges.h"

namespace qilqr {

// ---- the refusals, from facts alone (no device, no handle): null when the call is admitted, else the reason.  The arguments first, so
// that each is refused by its own reason whatever the handle is; the handle last.
struct RiskScoresCall {
  bool handle;
  const void *score, *risk;  // the device arrays (only their addresses are looked at)
  const double *levels;      // the host array (read once the counts are known to be in range)
  long B, S, column, n_levels;
};
inline const char *risk_scores_refusal(const RiskScoresCall &c) {
  if (!c.score || !c.levels || !c.risk) return "risk scores: null argument (d_score, levels and d_risk are needed)";
  if (c.B <= 0 || c.S <= 0) return "B and S must be positive";
  if (c.S > 4096) return "risk scores: S must not exceed QILQR_RISK_MAX_SAMPLES (4096: one block sorts a plan)";
  if (c.column != 0 && c.column != 1) return "risk scores: column must be QILQR_RISK_COST or QILQR_RISK_CLEARANCE";
  if (c.n_levels < 1 || c.n_levels > 8) return "risk scores: n_levels must be 1 ... QILQR_RISK_MAX_LEVELS (8)";
  for (long l = 0; l < c.n_levels; ++l)
    if (!(c.levels[l] >= 0.0 && c.levels[l] < 1.0)) return "risk scores: every level must lie in [0, 1)";
  if (off_16_bytes({c.score, c.risk})) return "risk scores: d_score and d_risk must be 16-byte aligned";
  if (ranges_overlap(c.risk, sizeof(double) * 4 * (size_t)c.B * (size_t)c.n_levels, c.score, sizeof(double) * 4 * (size_t)c.B * (size_t)c.S))
    return "risk scores: d_risk overlaps d_score";
  if (!c.handle) return "risk scores: null handle";
  return nullptr;
}

struct SelectPlansCall {
  bool handle, rule;  // there is a handle; there is a rule (the five fields below are its)
  long objective, level;
  double max_collision_fraction, max_diverged_fraction, min_clearance;
  const void *summary, *risk, *choice, *info;      // the device arrays
  const void *plan, *gains, *out_plan, *out_gains;  // the gather's: all or none
  long n_levels, V, C, n;
};
inline const char *select_plans_refusal(const SelectPlansCall &c) {
  if (!c.summary || !c.rule || !c.choice || !c.info) return "select plans: null argument (d_summary, the rule, d_choice and d_info are needed)";
  if (c.V <= 0 || c.C <= 0) return "select plans: V and C must be positive";
  if (c.objective < 0 || c.objective > 3) return "select plans: the objective must be 0 ... 3";
  const bool risky = c.objective >= 2;
  if (risky && (c.n_levels < 1 || c.n_levels > 8)) return "select plans: n_levels must be 1 ... QILQR_RISK_MAX_LEVELS (8)";
  if (risky && (c.level < 0 || c.level >= c.n_levels)) return "select plans: the level must be one of the risk array's n_levels";
  if (risky && !c.risk) return "select plans: objectives 2 and 3 need d_risk";
  if (std::isnan(c.max_collision_fraction) || std::isnan(c.max_diverged_fraction) || std::isnan(c.min_clearance))
    return "select plans: a threshold is NaN";
  if (off_16_bytes({c.summary, c.risk, c.choice, c.info, c.plan, c.gains, c.out_plan, c.out_gains})) return "select plans: every array must be 16-byte aligned";
  const int given = (c.plan != nullptr) + (c.gains != nullptr) + (c.out_plan != nullptr) + (c.out_gains != nullptr);
  if (given != 0 && given != 4) return "select plans: d_plan, d_gains, d_out_plan and d_out_gains are given all together or not at all";
  if (given == 4 && c.n <= 0) return "select plans: n must be positive";
  // every block reads only inputs and writes only outputs: an output that overlaps an input or another output is a race
  const size_t plans = (size_t)c.V * (size_t)c.C, V = (size_t)c.V, n = given == 4 ? (size_t)c.n : 0;
  const struct { const void *p; size_t bytes; } in[4] = {{c.summary, sizeof(double) * 8 * plans},
                                                         {risky ? c.risk : nullptr, sizeof(double) * 4 * plans * (size_t)(risky ? c.n_levels : 0)},
                                                         {c.plan, sizeof(double) * 18 * plans * n},
                                                         {c.gains, sizeof(double) * 52 * plans * n}},
                                                out[4] = {{c.choice, sizeof(int32_t) * V}, {c.info, sizeof(double) * 4 * V},
                                                          {c.out_plan, sizeof(double) * 18 * V * n}, {c.out_gains, sizeof(double) * 52 * V * n}};
  for (int o = 0; o < 4; ++o) {
    for (int i = 0; i < 4; ++i)
      if (ranges_overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return "select plans: an output overlaps an input";
    for (int p = 0; p < o; ++p)
      if (ranges_overlap(out[o].p, out[o].bytes, out[p].p, out[p].bytes)) return "select plans: two outputs overlap";
  }
  if (!c.handle) return "select plans: null handle";
  return nullptr;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/quadrotor_ilqr.h"

namespace qilqr {

struct RiskScoresLaunch {
  const double *d_score;  // [B][S][4], device
  double *d_risk;         // [B][n_levels][4], device
  int B, S, column, n_levels;
  const double *levels;   // [n_levels], host
};
struct SelectPlansLaunch {
  const double *d_summary, *d_risk;  // [C V][8], [C V][n_levels][4] or null, device
  int32_t *d_choice;                 // [V], device
  double *d_info;                    // [V][4], device
  int n_levels, V, C;
  qilqr_select_rule rule;            // the caller's
  const double *d_plan, *d_gains;    // the gather's (all null: no second launch)
  double *d_out_plan, *d_out_gains;
  int n;
};

// each enqueues its launches on `stream` and returns what they returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_risk_scores(hipStream_t stream, const RiskScoresLaunch &call);
__attribute__((visibility("hidden"))) hipError_t launch_select_plans(hipStream_t stream, const SelectPlansLaunch &call);

}  // namespace qilqr
#endif
