// closed_loop.hip -- the translation unit of k_closed_loop (closed_loop_kernels.h), the device side of qilqr_closed_loop[_device].  Its own
// unit for shift.hip's reason: the call works on the caller's arrays only -- no workspace, no BatchState, no route -- and ilqr_capi.hip's
// device code stays what it was.  Exports one hidden function, launch_closed_loop (closed_loop_launch.h), which host/api_calls.h calls.
#include <hip/hip_runtime.h>

#include "closed_loop_kernels.h"
#include "closed_loop_launch.h"

namespace qilqr {

namespace {
#ifdef QILQR_DIAG
int g_force_form = -1;  // -1: the rule; 0 / 1: the flattened / the shared-operand form at every S (the threshold's measurement)
#endif
template <int INTEG, bool SHARED, typename... Lim>
hipError_t closed_loop_go(hipStream_t stream, const ModelConsts<double> &c, const ClosedLoopArgs &a, dim3 grid, Lim... lim) {
  hipLaunchKernelGGL((k_closed_loop<INTEG, SHARED, Lim...>), grid, dim3(CL_BLOCK), 0, stream, c, a, lim...);
  return hipGetLastError();
}
template <int INTEG, bool SHARED>
hipError_t closed_loop_ext(hipStream_t stream, const ModelConsts<double> &c, const ClosedLoopArgs &a, dim3 grid, const ClosedLoopLaunch &call) {
  const BatchModels bm{call.d_models};
  if (call.limits && call.d_models) return closed_loop_go<INTEG, SHARED>(stream, c, a, grid, *call.limits, bm);
  if (call.limits) return closed_loop_go<INTEG, SHARED>(stream, c, a, grid, *call.limits);
  if (call.d_models) return closed_loop_go<INTEG, SHARED>(stream, c, a, grid, bm);
  return closed_loop_go<INTEG, SHARED>(stream, c, a, grid);
}
}  // namespace

hipError_t launch_closed_loop(hipStream_t stream, const ModelConsts<double> &consts, const ClosedLoopLaunch &call) {
  const ClosedLoopArgs a{call.d_plan, call.d_gains, call.d_x0, call.d_out_traj, call.d_out_stats, call.B, call.n, call.S, call.i0, call.i1};
  bool shared = closed_loop_shared_form(call.S);
#ifdef QILQR_DIAG
  if (g_force_form >= 0) shared = g_force_form != 0;
#endif
  const long per = (call.S + CL_BLOCK - 1) / CL_BLOCK;
  const long blocks = shared ? (long)call.B * per : ((long)call.B * call.S + CL_BLOCK - 1) / CL_BLOCK;
  if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  if (shared) return call.integrator == 1 ? closed_loop_ext<1, true>(stream, consts, a, grid, call) : closed_loop_ext<0, true>(stream, consts, a, grid, call);
  return call.integrator == 1 ? closed_loop_ext<1, false>(stream, consts, a, grid, call) : closed_loop_ext<0, false>(stream, consts, a, grid, call);
}

}  // namespace qilqr

#ifdef QILQR_DIAG
// (diagnostics build only: profiles/microbench/closed_loop.py times either form at every S to find where they cross)
extern "C" int qilqr_debug_set_closed_loop_form(int32_t form) {
  qilqr::g_force_form = form < 0 ? -1 : (form != 0);
  return 0;
}
// (what closed_loop_scored.hip's launch reads, so that one switch forces both kernels' form)
extern "C" int qilqr_debug_closed_loop_form(void) { return qilqr::g_force_form; }
#endif
