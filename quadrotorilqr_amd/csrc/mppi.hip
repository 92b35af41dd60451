// mppi.hip -- the translation unit of k_mppi_flight and k_mppi_update (mppi_kernels.h), the device side of qilqr_mppi_flight_device and
// qilqr_mppi_update_device.  A unit beside closed_loop_scored.hip and monte_carlo.hip, whose kernels stay what they were: the eight
// instantiations of the flight are {Euler, Runge-Kutta} x the four of launch_ext.h, the update's five are its block sizes.  Exports three
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
  mppi_coeffs(call.sigma, call.tau_s, c.dt, a.m);
  return call.integrator == 1 ? flight_go<1>(stream, c, a, dim3((unsigned)blocks), call) : flight_go<0>(stream, c, a, dim3((unsigned)blocks), call);
}

template <int THREADS>
void update_go(hipStream_t stream, int B, const MppiUpdateArgs &a) {
  hipLaunchKernelGGL(k_mppi_update<THREADS>, dim3((unsigned)B), dim3(THREADS), 0, stream, a);
}
}  // namespace

hipError_t launch_mppi_flight(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call) {
  return flight(stream, consts, call, call.d_plan, call.S, call.d_score, 4l * call.S, false, nullptr);
}

hipError_t launch_mppi_update(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call) {
  if (call.S > MPPI_MAX_SAMPLES) return hipErrorInvalidValue;
  MppiUpdateArgs a{};
  a.plan = call.d_plan;
  a.score = call.d_score;
  a.out_plan = call.d_out_plan;
  a.info = call.d_info;
  a.n = call.n;
  a.S = call.S;
  a.b0 = (uint32_t)call.b0;
  a.flags = call.flags;
  a.seed = call.seed;
  a.lambda = call.lambda;
  a.collision_cost = call.collision_cost;
  mppi_coeffs(call.sigma, call.tau_s, consts.dt, a.m);
  a.limited = call.limits ? 1 : 0;
  for (int r = 0; r < 4; ++r) {
    a.lim_lo[r] = call.limits ? call.limits->lo[r] : 0.0;
    a.lim_hi[r] = call.limits ? call.limits->hi[r] : 0.0;
  }
  switch (mppi_update_threads(call.S)) {
    case 64: update_go<64>(stream, call.B, a); break;
    case 128: update_go<128>(stream, call.B, a); break;
    case 256: update_go<256>(stream, call.B, a); break;
    case 512: update_go<512>(stream, call.B, a); break;
    default: update_go<1024>(stream, call.B, a); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_mppi_nominal_flight(stream, consts, call);
}

// the new plan's own flight: its states from x0 over d_out_plan, its score into words 4 .. 7 of d_info
hipError_t launch_mppi_nominal_flight(hipStream_t stream, const ModelConsts<double> &consts, const MppiLaunch &call) {
  return flight(stream, consts, call, call.d_out_plan, 1, call.d_info + 4, MPPI_INFO, true, call.d_out_plan);
}

}  // namespace qilqr
