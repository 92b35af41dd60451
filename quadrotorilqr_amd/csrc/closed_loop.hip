// closed_loop.hip -- the translation unit of k_closed_loop (closed_loop_kernels.h), the device side of qilqr_closed_loop[_device].  Its own
// unit for shift.hip's reason: the call works on the caller's arrays only -- no workspace, no BatchState, no route -- and ilqr_capi.hip's
// device code stays what it was.  Exports launch_closed_loop, which host/caller_arrays.h
// reaches through launch_closed_loop_scored, and closed_loop_form and closed_loop_args, the form and grid and the first argument record of
// both closed-loop units (closed_loop_launch.h; hidden).
#include <hip/hip_runtime.h>

#include "closed_loop_kernels.h"
#include "closed_loop_launch.h"
#include "launch_ext.h"

namespace qilqr {

namespace {
#ifdef QILQR_DIAG
int g_force_form = -1;  // -1: the rule; 0 / 1: the flattened / the shared-operand form at every S (the threshold's measurement)
#endif
template <int INTEG, bool SHARED>
hipError_t closed_loop_go(hipStream_t stream, const ModelConsts<double> &c, const ClosedLoopArgs &a, dim3 grid, const ClosedLoopLaunch &call) {
  return with_extensions(call.limits, call.d_models, [&](auto... lim) {
    hipLaunchKernelGGL((k_closed_loop<INTEG, SHARED, decltype(lim)...>), grid, dim3(CL_BLOCK), 0, stream, c, a, lim...);
    return hipGetLastError();
  });
}
}  // namespace

bool closed_loop_form(int B, int S, bool *shared, dim3 *grid) {
  *shared = closed_loop_shared_form(S);
#ifdef QILQR_DIAG
  if (g_force_form >= 0) *shared = g_force_form != 0;
#endif
  const long per = (S + CL_BLOCK - 1) / CL_BLOCK;
  const long blocks = *shared ? (long)B * per : ((long)B * S + CL_BLOCK - 1) / CL_BLOCK;
  if (blocks > 0x7fffffffl) return false;
  *grid = dim3((unsigned)blocks);
  return true;
}

ClosedLoopArgs closed_loop_args(const ClosedLoopLaunch &call) {
  return ClosedLoopArgs{call.d_plan, call.d_gains, call.d_x0, call.d_out_traj, call.d_out_stats, call.B, call.n, call.S, call.i0, call.i1};
}

hipError_t launch_closed_loop(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopLaunch &call) {
  const ClosedLoopArgs a = closed_loop_args(call);
  bool shared;
  dim3 grid;
  if (!closed_loop_form(call.B, call.S, &shared, &grid)) return hipErrorInvalidValue;
  if (shared) return call.integrator == 1 ? closed_loop_go<1, true>(stream, consts, a, grid, call) : closed_loop_go<0, true>(stream, consts, a, grid, call);
  return call.integrator == 1 ? closed_loop_go<1, false>(stream, consts, a, grid, call) : closed_loop_go<0, false>(stream, consts, a, grid, call);
}

}  // namespace qilqr

#ifdef QILQR_DIAG
// (diagnostics build only: profiles/microbench/closed_loop.py times either form of both kernels at every S to find where they cross)
extern "C" int qilqr_debug_set_closed_loop_form(int32_t form) {
  qilqr::g_force_form = form < 0 ? -1 : (form != 0);
  return 0;
}
#endif
