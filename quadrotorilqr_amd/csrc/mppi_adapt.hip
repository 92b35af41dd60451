// mppi_adapt.hip -- the translation unit of k_mppi_flight_spread and k_mppi_adapt (mppi_adapt_kernels.h), the device side of
// qilqr_mppi_flight_spread_device and qilqr_mppi_adapt_device.  A unit beside mppi.hip, whose kernels stay what they were: the eight
// instantiations of the flight are {Euler, Runge-Kutta} x the four of launch_ext.h, the adaptation's five are its block sizes.  Exports
// two hidden functions (mppi_adapt_launch.h), which host/caller_arrays.h calls; the nominal flight behind the adaptation is mppi.hip's,
// and the common arguments and the block size are filled and chosen as there (mppi_flight_args, mppi_update_args, with_update_lanes).
#include <hip/hip_runtime.h>

#include "mppi_adapt_kernels.h"
#include "mppi_adapt_launch.h"
#include "launch_ext.h"

namespace qilqr {

namespace {
template <int INTEG>
hipError_t flight_go(hipStream_t stream, const ModelConsts<double> &c, const MppiFlightSpreadArgs &a, dim3 grid, const MppiLaunch &call) {
  return with_extensions(call.limits, call.d_models, [&](auto... lim) {
    hipLaunchKernelGGL((k_mppi_flight_spread<INTEG, decltype(lim)...>), grid, dim3(CL_BLOCK), 0, stream, c, a, lim...);
    return hipGetLastError();
  });
}
}  // namespace

hipError_t launch_mppi_flight_spread(hipStream_t stream, const ModelConsts<double> &consts, const MppiSpreadLaunch &call) {
  const MppiLaunch &m = call.base;
  const long blocks = mppi_flight_blocks(m.B, m.S);
  if (blocks <= 0) return hipErrorInvalidValue;
  MppiFlightSpreadArgs a{};
  a.f = mppi_flight_args(m, m.d_plan, m.S, m.d_score, 4l * m.S, false, nullptr);
  mppi_unit_coeffs(m.rule.tau_s, consts.dt, a.f.m);
  a.spread = call.d_spread;
  return m.integrator == 1 ? flight_go<1>(stream, consts, a, dim3((unsigned)blocks), m) : flight_go<0>(stream, consts, a, dim3((unsigned)blocks), m);
}

hipError_t launch_mppi_adapt(hipStream_t stream, const ModelConsts<double> &consts, const MppiSpreadLaunch &call) {
  const MppiLaunch &m = call.base;
  if (m.S > MPPI_MAX_SAMPLES) return hipErrorInvalidValue;
  MppiAdaptArgs a{};
  MppiCoeffs unit;
  mppi_unit_coeffs(m.rule.tau_s, consts.dt, unit);
  a.u = mppi_update_args(m, unit);
  a.spread = call.d_spread;
  a.out_spread = call.d_out_spread;
  mppi_adapt_coeffs(call.adapt.floor, call.adapt.cap, call.adapt.rate, a.k);
  with_update_lanes(m.S, [&](auto lanes) {
    hipLaunchKernelGGL(k_mppi_adapt<decltype(lanes)::value>, dim3((unsigned)m.B), dim3(decltype(lanes)::value), 0, stream, a);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the new plan's own flight: its states from x0 over d_out_plan, its score into words 4 .. 7 of d_info
  return launch_mppi_nominal_flight(stream, consts, m);
}

}  // namespace qilqr
