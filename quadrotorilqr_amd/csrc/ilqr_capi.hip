// ilqr_capi.hip -- host side of libquadrotor_ilqr.so: the C ABI of include/quadrotor_ilqr.h
// over the HIP kernels of ilqr_kernels.h.  C++ because the reference's host side is C++
// (src/quadrotor_ilqr_binding.cc, src/ilqr.hh); no exceptions cross the ABI.  This is the one
// file the compiler is given: the host code lives in host/*.h, one header per concern, included
// below in the order they build on each other (as ilqr_kernels.h does for the device side).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#define QILQR_NO_SIZED_MACROS  // (this file DEFINES the legacy symbols the macros stand in front of)
#include "../../include/quadrotor_ilqr.h"
#include "host_model.h"
#include "ilqr_kernels.h"
#include "route.h"
#include "schedule.h"
#include "horizon.h"
#include "shift_launch.h"
#include "closed_loop_launch.h"
#include "monte_carlo_launch.h"
#include "risk_launch.h"
#include "mppi_launch.h"
#include "mppi_adapt_launch.h"
#include "cov_launch.h"
#include "fleet_launch.h"

using namespace qilqr;

// The host side by concern (one translation unit; this file was 2 800 lines):
#include "host/solver.h"        // the handle, errors, launch(), profiling slots, workspace, tiled up- and download
#include "host/launches.h"      // the route of a call, refusals, begin_batch and the launch_* helpers of every kernel family
#include "host/batch_solve.h"   // the round loops, the copy-back under the tail, sub-batch streams, the staged batch solve
#include "host/api_handle.h"    // create, destroy, options, profiles and the extension setters
#include "host/api_calls.h"     // qilqr_solve_batch, qilqr_solve, the stand-alone passes, pinned host memory
#include "host/caller_arrays.h" // the calls on the caller's own arrays: the shift, qilqr_backwards_pass_device, the closed-loop flights, the Monte-Carlo calls, risk and selection
#include "host/sharded.h"       // one batch over several devices: the RCCL binding, the gather, every qilqr_sharded_* entry point
#include "host/describe.h"      // qilqr_describe, qilqr_compaction_moves, the diagnostics builds' qilqr_debug_* entry points

extern "C" {

int qilqr_abi_version(void) { return QILQR_ABI_VERSION; }

const char *qilqr_last_error(void) { return g_last_error.c_str(); }

}  // extern "C"
