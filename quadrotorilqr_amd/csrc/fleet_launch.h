// fleet_launch.h -- what fleet.hip gives the rest of the library: the launches of k_fleet_fit, k_fleet_pairs and k_fleet_select for
// qilqr_fleet_neighbours_device and of k_bob_set for qilqr_set_batch_obstacles_device (fleet_kernels.h), the words of the handle's
// scratch a call needs, and the rules of what the two calls refuse.  Declarations and host code only -- no device code enters the
// translation unit that includes this (ilqr_capi.hip through host/caller_arrays.h); hidden: not part of the C ABI.  The rules compile
// under g++ (tests/host_fleet_harness.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "fleet_math.h"
#include "ranges.h"

namespace qilqr {

// ---- qilqr_fleet_neighbours_device's refusals, from facts alone (no device): null when the call is admitted, else the reason.  THE ORDER:
//   1  a NULL rule or plan                              5  a rule field out of its range, unknown flag bits, reserved != 0
//   2  every output NULL                                6  an array off a 16-byte boundary (d_counts: off 4 bytes)
//   3  B, n or V not positive, or V not dividing B      7  an output overlapping the plan or another output
//   4  K outside 1 ... QILQR_FLEET_MAX_NEIGHBOURS       8  a NULL handle, then a mixed-precision one
struct FleetCall {
  bool rule;                                // there is a rule (the fields below are its)
  double radius, weight, range, conflict;
  unsigned long flags, reserved;
  const void *plan, *summary, *nbr, *spheres, *counts;  // the device arrays (only their addresses are looked at)
  long B, n, V, K;
  bool handle, f32;                         // there is a handle; in the mixed-precision mode
};
inline const char *fleet_refusal(const FleetCall &c) {
  if (!c.rule || !c.plan) return "fleet neighbours: null argument (the rule and d_plan are needed)";
  if (!c.summary && !c.nbr && !c.spheres && !c.counts) return "fleet neighbours: no output (d_summary, d_nbr, d_spheres and d_counts are all null)";
  if (c.B <= 0 || c.n <= 0 || c.V <= 0) return "fleet neighbours: B, n and V must be positive";
  if (c.B % c.V != 0) return "fleet neighbours: V must divide B (rows b with equal b / V form a fleet)";
  if (c.K < 1 || c.K > FLEET_MAX_NEIGHBOURS) return "fleet neighbours: K must be 1 ... QILQR_FLEET_MAX_NEIGHBOURS";
  if (!(c.radius > 0.0) || !std::isfinite(c.radius)) return "fleet neighbours: the rule's radius must be finite and positive";
  if (!(c.weight >= 0.0) || !std::isfinite(c.weight)) return "fleet neighbours: the rule's weight must be finite and not negative";
  if (!(c.range > 0.0)) return "fleet neighbours: the rule's range must be positive (+inf: every listed partner)";
  if (!(c.conflict >= 0.0) || !std::isfinite(c.conflict)) return "fleet neighbours: the rule's conflict distance must be finite and not negative";
  if (c.flags & ~(unsigned long)(FLEET_COVER | FLEET_YIELD_TO_LOWER)) return "fleet neighbours: unknown flag bits (QILQR_FLEET_COVER and QILQR_FLEET_YIELD_TO_LOWER are the flags)";
  if (c.reserved != 0) return "fleet neighbours: the rule's reserved word must be 0";
  if (off_16_bytes({c.plan, c.summary, c.nbr, c.spheres}) || ((uintptr_t)c.counts & 3)) return "fleet neighbours: every array must be 16-byte aligned (d_counts: 4-byte)";
  enum { PLAN, SUMMARY, NBR, SPHERES, COUNTS, RANGES };  // the input, then the outputs
  const size_t B = (size_t)c.B, K = (size_t)c.K;
  const struct { const void *p; size_t bytes; } r[RANGES] = {{c.plan, sizeof(double) * 18 * B * (size_t)c.n},
                                                             {c.summary, sizeof(double) * FLEET_SUMMARY * B},
                                                             {c.nbr, sizeof(double) * FLEET_NBR * B * K},
                                                             {c.spheres, sizeof(double) * OB_BWORDS * B * K},
                                                             {c.counts, sizeof(int32_t) * B}};
  for (int o = SUMMARY; o <= COUNTS; ++o)
    if (ranges_overlap(r[o].p, r[o].bytes, r[PLAN].p, r[PLAN].bytes)) return "fleet neighbours: an output overlaps the plan";
  for (int o = SUMMARY; o <= COUNTS; ++o)
    for (int k = o + 1; k <= COUNTS; ++k)
      if (ranges_overlap(r[o].p, r[o].bytes, r[k].p, r[k].bytes)) return "fleet neighbours: the outputs overlap each other";
  if (!c.handle) return "fleet neighbours: null handle";
  if (c.f32) return "fleet neighbours: needs precision 0 (fp64)";
  return nullptr;
}

// ---- qilqr_set_batch_obstacles_device's refusals.  THE ORDER:
//   1  a NULL handle or table          3  K outside 1 ... QILQR_MAX_OBSTACLES          5  a mixed-precision handle
//   2  B not positive                  4  d_spheres off a 16-byte boundary, d_counts or d_dropped off a 4-byte one
// What the host setter refuses of the VALUES (a count outside 0 ... K, a bad row) cannot be looked at without a wait: k_bob_set applies
// bob_set_problem's rule to them instead.
struct BobSetCall {
  bool handle, f32;
  const void *spheres, *counts, *dropped;
  long B, K;
};
inline const char *bob_set_refusal(const BobSetCall &c) {
  if (!c.handle || !c.spheres) return "batch obstacles (device): null argument (the handle and d_spheres are needed)";
  if (c.B <= 0) return "batch obstacles (device): B must be positive (qilqr_set_batch_obstacles clears the table)";
  if (c.K < 1 || c.K > OB_MAX) return "batch obstacles (device): K must be 1 ... QILQR_MAX_OBSTACLES";
  if (off_16_bytes({c.spheres}) || (((uintptr_t)c.counts | (uintptr_t)c.dropped) & 3))
    return "batch obstacles (device): d_spheres must be 16-byte aligned, d_counts and d_dropped 4-byte";
  if (c.f32) return "batch obstacles need precision 0 (fp64): the mixed-precision kernels have no obstacle form";
  return nullptr;
}

// ---- the handle's scratch of a neighbours call, in doubles: the staged positions [fleet][knot][axis][fleet_row_words(V)], the fits
// [B][FLEET_FIT], and per partner chunk c the partial lists {d2 [c][K][B], (row, knot) [c][K][B]} and the partial FleetBest
// {d2 [c][B], (row, knot) [c][B], conflicts [c][B]}.  B = V = 8192, n = 100, K = 16: 7 049 920 words, 53.8 MiB.
struct FleetScratch {
  size_t pos, fit, pd2, prk, sd2, srk, sconf, words;  // where each part starts
};
inline FleetScratch fleet_scratch(long B, long n, long V, long K) {
  const size_t b = (size_t)B, c = (size_t)fleet_chunks((int)V), rows = b / (size_t)V * (size_t)n * 3;
  FleetScratch s{};
  s.pos = 0;
  s.fit = s.pos + rows * (size_t)fleet_row_words((int)V);
  s.pd2 = s.fit + b * FLEET_FIT;
  s.prk = s.pd2 + c * (size_t)K * b;
  s.sd2 = s.prk + c * (size_t)K * b;
  s.srk = s.sd2 + c * b;
  s.sconf = s.srk + c * b;
  s.words = s.sconf + (c * b + 1) / 2;
  return s;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "../../include/quadrotor_ilqr.h"

namespace qilqr {

// one admitted neighbours call; every pointer a device one
struct FleetLaunch {
  const double *d_plan;  // [B][n][18]
  double *d_scratch;     // fleet_scratch(B, n, V, K).words doubles: the handle's
  int B, n, V, K;
  double dt;             // the handle's
  qilqr_fleet_rule rule; // the caller's
  double *d_summary;     // [B][8], or null
  double *d_nbr;         // [B][K][4], or null
  double *d_spheres;     // [B][K][8], or null
  int32_t *d_counts;     // [B], or null
};
// enqueues the three launches on `stream` and returns what they returned; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_fleet_neighbours(hipStream_t stream, const FleetLaunch &call);

// one admitted setter call: the caller's rows into the handle's table and counts
struct BobSetLaunch {
  const double *d_spheres;  // [B][K][8]
  const int32_t *d_counts;  // [B], or null: all K
  int B, K;
  double *d_tab;            // bob_count(B, K) doubles
  int32_t *d_tab_counts;    // [B]
  int32_t *d_dropped;       // one word, or null
};
// zeroes *d_dropped (when given) and enqueues k_bob_set; nothing is waited for
__attribute__((visibility("hidden"))) hipError_t launch_bob_set(hipStream_t stream, const BobSetLaunch &call);

}  // namespace qilqr
#endif
