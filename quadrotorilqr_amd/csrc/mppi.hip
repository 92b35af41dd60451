// mppi.hip -- the translation unit of k_mppi_flight and k_mppi_update (mppi_kernels.h), the device side of qilqr_mppi_flight_device and
// qilqr_mppi_update_device.  A unit beside closed_loop_scored.hip and monte_carlo.hip, whose kernels stay what they were: the eight
// instantiations of the flight are {Euler, Runge-Kutta} x the four of launch_ext.h, the update's five are its block sizes
// (with_update_lanes, mppi_launch.h).  Exports three
// hidden functions (mppi_launch.h): two that host/caller_arrays.h calls, and the nominal flight behind an update, which mppi_adapt.hip
// enqueues behind its own.
#include <hip/hip_runtime.h>

#include "mppi_kernels.h"
#include "mppi_launch.h"
#include "launch_ext.h"

namespace qilqr {

namespace {
template <int INTEG>
hipError_t flight_go(hipStream_t stream, const ModelConsts<double> &c, const MppiFlightArgs &a, dim3 grid, const MppiLaunch &call) {
  return with_extensions(call.limits, call.d_models, [&](auto... lim) {
    hipLaunchKernelGGL((k_mppi_flight<INTEG, decltype(lim)...>), grid, dim3(CL_BLOCK), 0, stream, c, a, lim...);
    return hipGetLastError();
  });
}

// the flight of S samples per plan that writes `score` (score_step words between plans); nominal: eps = 0, and sample 0's flight is
// stored over `traj`
hipError_t flight(hipStream_t stream, const ModelConsts<double> &c, const MppiLaunch &call, const double *plan, int S, double *score, long score_step,
                  bool nominal, double *traj) {
  const long blocks = mppi_flight_blocks(call.B, S);
  if (blocks <= 0) return hipErrorInvalidValue;
  MppiFlightArgs a = mppi_flight_args(call, plan, S, score, score_step, nominal, traj);
  mppi_coeffs(call.rule.sigma, call.rule.tau_s, c.dt, a.m);
  return call.integrator == 1 ? flight_go<1>(stream, c, a, dim3((unsigned)blocks), call) : flight_go<0>(stream, c, a, dim3((unsigned)blocks), call);
}
}  // namespace

hipError_t launch_mppi_flight(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call) {
  return flight(stream, consts, call, call.d_plan, call.S, call.d_score, 4l * call.S, false, nullptr);
}

hipError_t launch_mppi_update(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call) {
  if (call.S > MPPI_MAX_SAMPLES) return hipErrorInvalidValue;
  MppiCoeffs m;
  mppi_coeffs(call.rule.sigma, call.rule.tau_s, consts.dt, m);
  const MppiUpdateArgs a = mppi_update_args(call, m);
  with_update_lanes(call.S, [&](auto lanes) {
    hipLaunchKernelGGL(k_mppi_update<decltype(lanes)::value>, dim3((unsigned)call.B), dim3(decltype(lanes)::value), 0, stream, a);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_mppi_nominal_flight(stream, consts, call);
}

// the new plan's own flight: its states from x0 over d_out_plan, its score into words 4 .. 7 of d_info
hipError_t launch_mppi_nominal_flight(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call) {
  return flight(stream, consts, call, call.d_out_plan, 1, call.d_info + 4, MPPI_INFO, true, call.d_out_plan);
}

}  // namespace qilqr
