// shift_launch.h -- the one function shift.hip gives the rest of the library: the launch of k_shift (shift_kernels.h) for one call of
// qilqr_shift_batch[_device].  Declarations only -- no device code enters the translation unit that includes this (ilqr_capi.hip through
// host/caller_arrays.h); hidden: not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include "box_qp.h"
#include "se3_math.h"

namespace qilqr {

struct ShiftLaunch {
  const double *d_in;      // [B][n][18], device
  const double *d_x0;      // [B][13], device, or null
  double *d_out;           // [B][n][18], device
  int B, n, steps, tail;
  int integrator;                // 0 explicit Euler, 1 Runge-Kutta
  const ControlLimits *limits;   // the handle's thrust limits, or null
  const double *d_models;        // the per-problem model records (batch_models.h) of these B problems, or null
};

// enqueues the launch on `stream` and returns what the launch returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_shift(hipStream_t stream, const ModelConsts<double> &consts, const ShiftLaunch &call);

}  // namespace qilqr
