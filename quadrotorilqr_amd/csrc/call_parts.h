// call_parts.h -- what the calls on the caller's own arrays have in common beside the two questions of ranges.h, each stated once: the
// two length predicates of the rules that score against the handle (closed_loop_launch.h, mppi_launch.h), and what a score reads of the
// handle on the device (SphereTables, ScoreOperands).  The *Launch records and the kernels' argument records embed the latter two;
// host/caller_arrays.h fills each in one place (sphere_tables, score_operands).  Plain records, no HIP header; compiles under g++ (the
// tests' harnesses).
#pragma once

namespace qilqr {

// ---- host only: a call that scores knots up to `last` without a desired trajectory of its own reaches beyond the handle's n_desired
// knots from its horizon start k0; ... beyond its schedule of n_sched knots (0: none)
inline bool beyond_desired(long last, long n_desired, long k0) { return last >= n_desired - k0; }
inline bool beyond_schedule(long last, long n_sched, long k0) { return n_sched > 0 && last >= n_sched - k0; }

// ---- device side: every pointer a device one
// the handle's two sphere tables
struct SphereTables {
  const double *shared;    // the shared sphere table [n_shared][OB_WORDS], or null
  int n_shared;
  const double *own;       // the per-problem table (obstacles.h, bob_index), or null
  const int *own_counts;   // [B]
  int own_K;
};
// what a score reads beside the flight's own arrays
struct ScoreOperands {
  const double *desired;   // knot i of plan b is desired + b * desired_step + i * 18
  long desired_step;       // n * 18 (one per plan), or 0 (the handle's, from its horizon start)
  const double *q;         // knot i's state weights are q + i * q_step; 16-byte aligned
  int q_step;              // 144 (a schedule, from the horizon start), or 0 (the handle's Q)
  SphereTables spheres;
};

}  // namespace qilqr
