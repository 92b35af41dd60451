// shift.hip -- the translation unit of k_shift (shift_kernels.h), the device side of qilqr_shift_batch[_device].  Its own unit because the
// shift works on the caller's arrays only: no workspace, no BatchState, no route -- and ilqr_capi.hip's device code stays what it was.
// Exports one hidden function, launch_shift (shift_launch.h), which host/api_calls.h calls.
#include <hip/hip_runtime.h>

#include "shift_kernels.h"
#include "shift_launch.h"

namespace qilqr {

namespace {
template <int INTEG, typename... Lim>
hipError_t shift_go(hipStream_t stream, const ModelConsts<double> &c, const ShiftArgs &a, dim3 grid, Lim... lim) {
  hipLaunchKernelGGL((k_shift<INTEG, Lim...>), grid, dim3(SHIFT_BLOCK), 0, stream, c, a, lim...);
  return hipGetLastError();
}
template <int INTEG>
hipError_t shift_ext(hipStream_t stream, const ModelConsts<double> &c, const ShiftArgs &a, dim3 grid, const ShiftLaunch &call) {
  const BatchModels bm{call.d_models};
  if (call.limits && call.d_models) return shift_go<INTEG>(stream, c, a, grid, *call.limits, bm);
  if (call.limits) return shift_go<INTEG>(stream, c, a, grid, *call.limits);
  if (call.d_models) return shift_go<INTEG>(stream, c, a, grid, bm);
  return shift_go<INTEG>(stream, c, a, grid);
}
}  // namespace

hipError_t launch_shift(hipStream_t stream, const ModelConsts<double> &consts, const ShiftLaunch &call) {
  ShiftArgs a{call.d_in, call.d_x0, call.d_out, call.B, call.n, call.steps, call.tail, 0};
  // (steps = 0 without x0 is a plain copy: no lane has a tail to roll or a knot 0 to anchor)
  a.tail_blocks = (call.steps > 0 || call.d_x0) ? (call.B + SHIFT_BLOCK - 1) / SHIFT_BLOCK : 0;
  const long copy_blocks = (shift_copy_pairs(a) + SHIFT_BLOCK - 1) / SHIFT_BLOCK;
  if (copy_blocks + a.tail_blocks > 0x7fffffffl) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(copy_blocks + a.tail_blocks));
  return call.integrator == 1 ? shift_ext<1>(stream, consts, a, grid, call) : shift_ext<0>(stream, consts, a, grid, call);
}

}  // namespace qilqr
