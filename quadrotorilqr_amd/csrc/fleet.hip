// fleet.hip -- the translation unit of k_fleet_fit, k_fleet_pairs, k_fleet_select and k_bob_set (fleet_kernels.h), the device side of
// qilqr_fleet_neighbours_device and qilqr_set_batch_obstacles_device.  A unit of its own for risk.hip's reason: the kernels work on the
// caller's arrays, the handle's scratch and its sphere table only, and the device code of the other units stays what it was.  Exports
// two hidden functions (fleet_launch.h), which host/caller_arrays.h calls.
#include <hip/hip_runtime.h>

#include "fleet_kernels.h"
#include "fleet_launch.h"

namespace qilqr {

hipError_t launch_fleet_neighbours(hipStream_t stream, const FleetLaunch &call) {
  const int B = call.B, n = call.n, V = call.V, K = call.K;
  if (B <= 0 || n <= 0 || V <= 0 || B % V || K < 1 || K > FLEET_MAX_NEIGHBOURS || !call.d_scratch) return hipErrorInvalidValue;
  const int C = fleet_chunks(V), P = fleet_chunk_size(V), tiles = (V + FLEET_TILE - 1) / FLEET_TILE;
  const long blocks = (long)tiles * C * (B / V);
  if (blocks > 0x7fffffffl) return hipErrorInvalidValue;
  const FleetScratch at = fleet_scratch(B, n, V, K);
  double *w = call.d_scratch;
  const unsigned ego_tiles = (unsigned)((B + FLEET_TILE - 1) / FLEET_TILE);

  hipLaunchKernelGGL(k_fleet_fit, dim3(ego_tiles), dim3(FLEET_TILE), 0, stream, FleetFitArgs{call.d_plan, w + at.pos, w + at.fit, B, n, V, fleet_row_words(V), call.dt});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;

  const FleetPairsArgs pairs{w + at.pd2, reinterpret_cast<int2 *>(w + at.prk), w + at.sd2, reinterpret_cast<int2 *>(w + at.srk), reinterpret_cast<int *>(w + at.sconf),
                             B, n, V, K, C, P, tiles, fleet_row_words(V), fleet_square(call.rule.conflict), call.rule.flags};
  hipLaunchKernelGGL(k_fleet_pairs, dim3((unsigned)blocks), dim3(FLEET_TILE), 0, stream, (const double *)(w + at.pos), pairs);
  if ((e = hipGetLastError()) != hipSuccess) return e;

  const FleetSelectArgs select{w + at.pd2, reinterpret_cast<const int2 *>(w + at.prk), w + at.sd2, reinterpret_cast<const int2 *>(w + at.srk),
                               reinterpret_cast<const int *>(w + at.sconf), w + at.fit, B, K, C,
                               FleetSelectRule{call.rule.radius, call.rule.weight, fleet_square(call.rule.range), fleet_square(call.rule.conflict), call.rule.flags},
                               call.d_summary, call.d_nbr, call.d_spheres, call.d_counts};
  hipLaunchKernelGGL(k_fleet_select, dim3(ego_tiles), dim3(FLEET_TILE), 0, stream, select);
  return hipGetLastError();
}

hipError_t launch_bob_set(hipStream_t stream, const BobSetLaunch &call) {
  if (call.B <= 0 || call.K < 1 || call.K > OB_MAX || !call.d_spheres || !call.d_tab || !call.d_tab_counts) return hipErrorInvalidValue;
  if (call.d_dropped) {
    const hipError_t e = hipMemsetAsync(call.d_dropped, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
  }
  const unsigned tiles = (unsigned)((call.B + OB_TILE - 1) / OB_TILE);
  hipLaunchKernelGGL(k_bob_set, dim3(tiles), dim3(OB_TILE), 0, stream, BobSetArgs{call.d_spheres, call.d_counts, call.d_tab, call.d_tab_counts, call.d_dropped, call.B, call.K});
  return hipGetLastError();
}

}  // namespace qilqr
