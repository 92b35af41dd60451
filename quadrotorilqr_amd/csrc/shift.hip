// shift.hip -- the translation unit of k_shift (shift_kernels.h), the device side of qilqr_shift_batch[_device].  Its own unit because the
// shift works on the caller's arrays only: no workspace, no BatchState, no route -- and ilqr_capi.hip's device code stays what it was.
// Exports one hidden function, launch_shift (shift_launch.h), which host/caller_arrays.h calls.
#include <hip/hip_runtime.h>

#include "shift_kernels.h"
#include "launch_ext.h"
#include "shift_launch.h"

namespace qilqr {

namespace {
template <int INTEG>
hipError_t shift_go(hipStream_t stream, const ModelConsts<double> &c, const ShiftArgs &a, dim3 grid, const ShiftLaunch &call) {
  return with_extensions(call.limits, call.d_models, [&](auto... lim) {
    hipLaunchKernelGGL((k_shift<INTEG, decltype(lim)...>), grid, dim3(SHIFT_BLOCK), 0, stream, c, a, lim...);
    return hipGetLastError();
  });
}
}  // namespace

hipError_t launch_shift(hipStream_t stream, const ModelConsts<double> &consts, const ShiftLaunch &call) {
  ShiftArgs a{call.d_in, call.d_x0, call.d_out, call.B, call.n, call.steps, call.tail, 0};
  // (steps = 0 without x0 is a plain copy: no lane has a tail to roll or a knot 0 to anchor)
  a.tail_blocks = (call.steps > 0 || call.d_x0) ? (call.B + SHIFT_BLOCK - 1) / SHIFT_BLOCK : 0;
  const long copy_blocks = (shift_copy_pairs(a) + SHIFT_BLOCK - 1) / SHIFT_BLOCK;
  if (copy_blocks + a.tail_blocks > 0x7fffffffl) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(copy_blocks + a.tail_blocks));
  return call.integrator == 1 ? shift_go<1>(stream, consts, a, grid, call) : shift_go<0>(stream, consts, a, grid, call);
}

}  // namespace qilqr
