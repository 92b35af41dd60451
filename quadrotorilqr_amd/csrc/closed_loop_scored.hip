// closed_loop_scored.hip -- the translation unit of k_closed_loop_scored (closed_loop_scored_kernels.h), the device side of
// qilqr_closed_loop_scored[_device].  A unit beside closed_loop.hip, whose sixteen kernels stay what they were: the 48 instantiations here
// are {wrench, score, both} x k_closed_loop's sixteen.  Exports one hidden function, launch_closed_loop_scored (closed_loop_launch.h), which
// host/caller_arrays.h calls; the form, the grid and the first argument record are closed_loop.hip's (closed_loop_form, closed_loop_args).
#include <hip/hip_runtime.h>

#include "closed_loop_scored_kernels.h"
#include "closed_loop_launch.h"
#include "launch_ext.h"

namespace qilqr {

namespace {
template <int INTEG, bool SHARED, bool WRENCH, bool SCORE>
hipError_t scored_go(hipStream_t stream, const ModelConsts<double> &c, const ClosedLoopArgs &a, const ClosedLoopScoreArgs &e, dim3 grid,
                     const ClosedLoopLaunch &call) {
  return with_extensions(call.limits, call.d_models, [&](auto... lim) {
    hipLaunchKernelGGL((k_closed_loop_scored<INTEG, SHARED, WRENCH, SCORE, decltype(lim)...>), grid, dim3(CL_BLOCK), 0, stream, c, a, e, lim...);
    return hipGetLastError();
  });
}
template <int INTEG, bool SHARED>
hipError_t scored_switch(hipStream_t stream, const ModelConsts<double> &c, const ClosedLoopArgs &a, const ClosedLoopScoreArgs &e, dim3 grid,
                         const ClosedLoopLaunch &call) {
  if (e.wrench && e.out_score) return scored_go<INTEG, SHARED, true, true>(stream, c, a, e, grid, call);
  if (e.wrench) return scored_go<INTEG, SHARED, true, false>(stream, c, a, e, grid, call);
  return scored_go<INTEG, SHARED, false, true>(stream, c, a, e, grid, call);
}
}  // namespace

hipError_t launch_closed_loop_scored(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopScoredLaunch &s) {
  const ClosedLoopLaunch &call = s.base;
  if (!s.d_wrench && !s.d_out_score) return launch_closed_loop(stream, consts, call);  // the existing instantiations: the parent's bits
  const ClosedLoopArgs a = closed_loop_args(call);
  const ClosedLoopScoreArgs e{s.d_wrench, s.n_w, s.score, s.d_out_score};
  bool shared;
  dim3 grid;
  if (!closed_loop_form(call.B, call.S, &shared, &grid)) return hipErrorInvalidValue;
  if (shared) return call.integrator == 1 ? scored_switch<1, true>(stream, consts, a, e, grid, call) : scored_switch<0, true>(stream, consts, a, e, grid, call);
  return call.integrator == 1 ? scored_switch<1, false>(stream, consts, a, e, grid, call) : scored_switch<0, false>(stream, consts, a, e, grid, call);
}

}  // namespace qilqr
