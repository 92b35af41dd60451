// schedule.h -- the check of a state-weight schedule (qilqr_set_state_weight_schedule): what the setter and the sharded setter refuse, and
// whether every matrix is bit-exactly symmetric (which backward kernel the handle then takes: route.h, RouteInputs::scheduled).  Host code
// only, no HIP: tests/test_schedule_cpu.py builds it with g++.
#pragma once

namespace qilqr {

constexpr int SCHED_WORDS = 144;  // a knot's Q: 12 x 12, row-major, tangent order
struct SchedCheck {
  const char *why = nullptr;        // what is wrong (null: nothing)
  long knot = -1;                   // ... and where: the first bad knot, row and column (-1: not about an entry)
  int row = -1, col = -1;
  bool symmetric = true;            // every Q_i == Q_i^T exactly (valid when nothing is wrong)
};
// Qs: n_knots x 144 doubles, or null with n_knots = 0 (clear).  Returns 0 when the schedule can be set (or cleared).
inline int sched_check(const double *Qs, long n_knots, SchedCheck *e) {
  *e = SchedCheck{};
  if (!Qs) {
    if (n_knots == 0) return 0;
    e->why = "Qs = NULL clears the schedule and goes with n_knots = 0";
    return 1;
  }
  if (n_knots < 1) {
    e->why = "n_knots must be at least 1 (Qs = NULL with n_knots = 0 clears the schedule)";
    return 1;
  }
  for (long i = 0; i < n_knots; ++i)
    for (int r = 0; r < 12; ++r)
      for (int c = 0; c < 12; ++c) {
        const double v = Qs[i * SCHED_WORDS + r * 12 + c];
        if (!(v - v == 0.0)) {  // NaN or an infinity
          e->why = "a non-finite entry";
          e->knot = i;
          e->row = r;
          e->col = c;
          return 1;
        }
        if (v != Qs[i * SCHED_WORDS + c * 12 + r]) e->symmetric = false;
      }
  return 0;
}

}  // namespace qilqr
