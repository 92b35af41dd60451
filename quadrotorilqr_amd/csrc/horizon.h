// horizon.h -- the index checks of the horizon start (qilqr_set_horizon_start): what the setter refuses, and which calls a handle with a
// start refuses for their length.  From the setter's call on, knot i of a call reads the handle's desired[k0 + i] and, wherever a
// state-weight schedule is read, Qs[k0 + i]: the window of a call of n knots is [k0, k0 + n) of both.  Host code only, no HIP:
// tests/test_shift_cpu.py builds it with g++.
#pragma once

namespace qilqr {

enum HorizonCheck { HZ_OK = 0, HZ_INVALID = 1, HZ_LENGTH_DESIRED = 2, HZ_LENGTH_SCHEDULE = 3 };

// the setter: 0 <= k0 < n_desired, and k0 < n_sched while a schedule is set (n_sched = 0: none).  k0 = 0 is what every handle starts with
// and is never refused (a handle without a desired trajectory has it too).
inline int horizon_start_check(long k0, long n_desired, long n_sched, const char **why) {
  *why = nullptr;
  if (k0 == 0) return HZ_OK;
  if (k0 < 0) {
    *why = "horizon start: k0 must not be negative";
    return HZ_INVALID;
  }
  if (k0 >= n_desired) {
    *why = "horizon start: k0 must be below the length of the handle's desired trajectory";
    return HZ_INVALID;
  }
  if (n_sched > 0 && k0 >= n_sched) {
    *why = "horizon start: k0 must be below the length of the state-weight schedule while one is set";
    return HZ_INVALID;
  }
  return HZ_OK;
}

// a call of n knots; which of the two lengths it exceeds is the return value.  shared_desired = no per-problem desired_batch is given (that
// array is already the caller's window); evaluates_cost = the call reads the schedule (every computing call but qilqr_forward_sim)
inline int horizon_window_check(long n, long k0, long n_desired, long n_sched, bool shared_desired, bool evaluates_cost, const char **why) {
  *why = nullptr;
  if (shared_desired && n > n_desired - k0) {
    *why = "trajectory longer than desired trajectory";
    return HZ_LENGTH_DESIRED;
  }
  if (evaluates_cost && n_sched > 0 && n > n_sched - k0) {
    *why = "trajectory longer than the state-weight schedule";
    return HZ_LENGTH_SCHEDULE;
  }
  return HZ_OK;
}

// a state-weight schedule of n_knots matrices set while a start is in force: the start stays inside it (the other half of the setter's rule)
inline int horizon_schedule_check(long k0, long n_knots, const char **why) {
  *why = nullptr;
  if (k0 < n_knots) return HZ_OK;
  *why = "state-weight schedule: shorter than the horizon start in force (lower the start first, or give a schedule that reaches beyond it)";
  return HZ_INVALID;
}

}  // namespace qilqr
