// risk.hip -- the translation unit of k_risk_scores, k_select_plans and k_gather_plans (risk_kernels.h), the device side of
// qilqr_risk_scores_device and qilqr_select_plans_device.  Its own unit for monte_carlo.hip's reason: the kernels work on the caller's
// arrays only, and the device code of the other units stays what it was.  Exports two hidden functions (risk_launch.h), which
// host/caller_arrays.h calls.
#include <hip/hip_runtime.h>

#include "risk_kernels.h"
#include "risk_launch.h"

namespace qilqr {

namespace {
template <int THREADS>
void risk_scores_go(hipStream_t stream, int B, const RiskScoresArgs &a) {
  hipLaunchKernelGGL(k_risk_scores<THREADS>, dim3((unsigned)B), dim3(THREADS), 12 * (size_t)a.P, stream, a);
}
}  // namespace

hipError_t launch_risk_scores(hipStream_t stream, const RiskScoresLaunch &call) {
  if (call.S > RISK_MAX_SAMPLES || call.n_levels > RISK_MAX_LEVELS) return hipErrorInvalidValue;
  RiskScoresArgs a{call.d_score, call.d_risk, call.S, risk_slots(call.S), call.column, call.n_levels, {}};
  for (int l = 0; l < call.n_levels; ++l) a.rank[l] = risk_rank(call.levels[l], call.S);
  switch (risk_threads(a.P)) {
    case 64: risk_scores_go<64>(stream, call.B, a); break;
    case 128: risk_scores_go<128>(stream, call.B, a); break;
    case 256: risk_scores_go<256>(stream, call.B, a); break;
    case 512: risk_scores_go<512>(stream, call.B, a); break;
    default: risk_scores_go<1024>(stream, call.B, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_select_plans(hipStream_t stream, const SelectPlansLaunch &call) {
  const SelectPlansArgs a{call.d_summary, call.d_risk, call.d_choice, call.d_info, call.n_levels, call.V, call.C,
                          SelectRule{call.rule.objective, call.rule.level, call.rule.max_collision_fraction, call.rule.max_diverged_fraction, call.rule.min_clearance}};
  hipLaunchKernelGGL(k_select_plans, dim3((unsigned)((call.V + 63) / 64)), dim3(64), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !call.d_out_plan) return e;
  const GatherPlansArgs g{call.d_choice, reinterpret_cast<const double2 *>(call.d_plan), reinterpret_cast<const double2 *>(call.d_gains),
                          reinterpret_cast<double2 *>(call.d_out_plan), reinterpret_cast<double2 *>(call.d_out_gains), call.V, call.C, call.n};
  const long pieces = (long)call.n * (GATHER_PLAN16 + GATHER_GAIN16), by = (pieces + GATHER_BLOCK - 1) / GATHER_BLOCK;
  hipLaunchKernelGGL(k_gather_plans, dim3((unsigned)call.V, (unsigned)(by > 65535 ? 65535 : by)), dim3(GATHER_BLOCK), 0, stream, g);
  return hipGetLastError();
}

}  // namespace qilqr
