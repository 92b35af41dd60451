// cov.hip -- the translation unit of k_cov_build, k_cov_chain and k_cov_summary (cov_kernels.h), the device side of
// qilqr_covariance_device.  A unit of its own beside the flights': the four instantiations of k_cov_build are {Euler, Runge-Kutta} x
// {the handle's model, per-problem models}; the chain and the summary know neither.  Exports one hidden function (cov_launch.h), which
// host/caller_arrays.h calls.
#include <hip/hip_runtime.h>

#include "cov_kernels.h"
#include "cov_launch.h"

namespace qilqr {

namespace {
template <int INTEG>
hipError_t build_go(hipStream_t stream, const ModelConsts<double> &c, const CovBuildArgs &a, dim3 grid, const double *d_models) {
  if (d_models) hipLaunchKernelGGL((k_cov_build<INTEG, BatchModels>), grid, dim3(COV_BLOCK), 0, stream, c, a, BatchModels{d_models});
  else hipLaunchKernelGGL((k_cov_build<INTEG>), grid, dim3(COV_BLOCK), 0, stream, c, a);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_covariance(hipStream_t stream, const ModelConsts<double> &consts, const CovLaunch &call) {
  const long knots = (long)call.B * call.n, blocks = (knots + COV_BLOCK - 1) / COV_BLOCK;
  if (call.B <= 0 || call.n <= 0 || blocks > 0x7fffffffl || (call.d_summary && (!call.d_cov || !call.d_mean))) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (call.i0 < call.i1) {  // (a window of one knot has no step: nothing to build)
    const CovBuildArgs a{call.d_plan, call.d_gains, call.d_image, call.B, call.n, call.i0, call.i1};
    const dim3 grid((unsigned)blocks, call.integrator == 1 ? COV_RK4_PARTS : 2);
    e = call.integrator == 1 ? build_go<1>(stream, consts, a, grid, call.d_models) : build_go<0>(stream, consts, a, grid, call.d_models);
    if (e != hipSuccess) return e;
  }
  CovChainArgs ch{call.d_image, call.d_cov, call.d_mean, call.n, call.i0, call.i1, {}};
  const qilqr_gust_model &g = call.rule.gust;
  cov_coeffs(call.rule.state_sigma, g.mean, g.sigma, g.tau_force_s, g.tau_torque_s, (call.rule.flags & QILQR_COV_WRENCH_HELD) != 0, consts.dt, ch.k);
  hipLaunchKernelGGL(k_cov_chain, dim3((unsigned)call.B), dim3(COV_BLOCK), 0, stream, ch);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (call.d_summary) {
    const CovSummaryArgs s{call.d_plan, call.d_gains, call.d_cov, call.d_mean, call.d_summary, call.n, call.i0, call.i1, consts.dt, call.spheres};
    hipLaunchKernelGGL(k_cov_summary, dim3((unsigned)call.B), dim3(COV_BLOCK), 0, stream, s);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace qilqr
