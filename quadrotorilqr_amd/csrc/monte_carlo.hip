// monte_carlo.hip -- the translation unit of k_sample_gusts, k_sample_states and k_reduce_scores (monte_carlo_kernels.h), the device side
// of qilqr_sample_gusts_device, qilqr_sample_states_device and qilqr_reduce_scores_device.  Its own unit because the three work on the
// caller's arrays only -- no workspace, no model, no route -- and the device code of the other units stays what it was.  Exports three
// hidden functions (monte_carlo_launch.h), which host/caller_arrays.h calls.
#include <hip/hip_runtime.h>

#include "monte_carlo_kernels.h"
#include "monte_carlo_launch.h"

namespace qilqr {

hipError_t launch_sample_gusts(hipStream_t stream, const SampleGustsLaunch &call) {
  SampleGustsArgs a{call.d_wrench, call.B, call.S, call.n_w, (uint32_t)call.b0, (uint32_t)call.s0, call.seed, {}};
  gust_coeffs(call.model.mean, call.model.sigma, call.model.tau_force_s, call.model.tau_torque_s, call.dt, a.m);
  const long blocks = ((long)call.B * call.S + MC_GUST_FLIGHTS - 1) / MC_GUST_FLIGHTS;
  if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sample_gusts, dim3((unsigned)blocks), dim3(MC_GUST_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_sample_states(hipStream_t stream, const SampleStatesLaunch &call) {
  SampleStatesArgs a{call.d_x_nom, call.d_x0, call.B, call.S, (uint32_t)call.b0, (uint32_t)call.s0, call.flags, call.seed, {}};
  for (int k = 0; k < 12; ++k) a.sigma[k] = call.sigma[k];
  const long blocks = ((long)call.B * call.S + MC_STATE_BLOCK - 1) / MC_STATE_BLOCK;
  if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sample_states, dim3((unsigned)blocks), dim3(MC_STATE_BLOCK), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_reduce_scores(hipStream_t stream, const ReduceScoresLaunch &call) {
  hipLaunchKernelGGL(k_reduce_scores, dim3((unsigned)call.B), dim3(64), 0, stream, call.d_score, call.B, call.S, call.d_summary);
  return hipGetLastError();
}

}  // namespace qilqr
