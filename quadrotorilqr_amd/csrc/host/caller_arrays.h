// host/caller_arrays.h -- the C ABI of the calls that work on the caller's own arrays and use no workspace, no BatchState and no route: the
// receding-horizon shift (k_shift: shift.hip), the backward pass over device arrays, the closed-loop flights of a plan (k_closed_loop and
// k_closed_loop_scored: closed_loop.hip, closed_loop_scored.hip), the ends of the Monte-Carlo loop (monte_carlo.hip) and the risk
// measures and the choice among candidate plans behind it (risk.hip), the sampling planner (mppi.hip, mppi_adapt.hip) and the linear
// covariance analysis of a plan's closed loop (cov.hip; its rule is cov_launch.h's, its scratch the handle's), and fleet deconfliction
// with the device-side setter of the per-problem sphere table (fleet.hip; the rules are fleet_launch.h's).  Each call has
// one refusal (from the rules of ranges.h and the seven *_launch.h), one enqueue, a device form that enqueues and returns (on_device), and
// -- the shift and the flight -- a host form that stages the arrays through one DeviceScratch (enqueue_and_drain).  What the calls read of
// the handle for a launch is read in one place each: sphere_tables, score_operands (the records are call_parts.h's).  Part of
// ilqr_capi.hip's translation unit.
#pragma once

namespace {
// The tail of a host form: the kernel is enqueued and, if that went well, the copies back are queued; the stream is drained whatever
// happened (the copies read and write the caller's arrays, the kernel the scratch: finished before either goes); then the enqueue's
// refusal is reported first and a HIP error, under the entry point's name, second.
template <typename Enqueue, typename CopyBack>
int enqueue_and_drain(qilqr_solver *s, const char *entry, Enqueue &&enqueue, CopyBack &&copy_back) {
  const int rc = enqueue();
  hipError_t e = rc == QILQR_OK ? copy_back() : hipSuccess;
  const hipError_t drained = hipStreamSynchronize(s->stream);
  if (rc) return rc;
  if (e == hipSuccess) e = drained;
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e));
  return QILQR_OK;
}

// A launch's outcome as a return code: a HIP failure is reported under the kernel's name.
int launched(const char *kernel, hipError_t e) {
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(e));
  return QILQR_OK;
}
// The tail of a device form, behind its refusal: the handle's device, then the enqueue (on the handle's stream; not waited for), which
// reports its own failure -- launched() for the launch, HIP_TRY for operands and scratch made on the way.
template <typename Enqueue>
int on_device(qilqr_solver *s, Enqueue &&enqueue) {
  HIP_TRY(hipSetDevice(s->device));
  return enqueue();
}

// ---- what a launch reads of the handle, each in one place (the records are call_parts.h's)
SphereTables sphere_tables(const qilqr_solver *s) {
  return SphereTables{s->n_obstacles > 0 ? s->d_obstacles : nullptr, s->n_obstacles, s->pobs_B > 0 ? s->d_pobs : nullptr,
                      s->pobs_B > 0 ? s->d_pobs_counts : nullptr, s->pobs_K};
}
// what a score reads: the desired trajectory (the caller's per plan, or the handle's from its horizon start), the state weights, the tables
int score_operands(qilqr_solver *s, const double *d_desired, int32_t n, ScoreOperands &o) {
  o.desired = d_desired ? d_desired : (const double *)s->d_desired + 18 * (size_t)s->k0;
  o.desired_step = d_desired ? 18l * n : 0;
  if (s->n_sched > 0) {
    o.q = s->d_qsched + (size_t)SCHED_WORDS * s->k0;
    o.q_step = SCHED_WORDS;
  } else {
    if (!s->d_cl_q) {  // (Q lies 8 bytes off a 16-byte boundary inside ModelConsts: a copy of its own, made once; the handle's Q never changes)
      HIP_TRY(hipMalloc((void **)&s->d_cl_q, sizeof(double) * 144));
      HIP_TRY(hipMemcpyAsync(s->d_cl_q, s->consts.Q, sizeof(double) * 144, hipMemcpyHostToDevice, s->stream));
    }
    o.q = s->d_cl_q;
    o.q_step = 0;
  }
  o.spheres = sphere_tables(s);
  return QILQR_OK;
}

// ---- the step between two solves of a receding horizon: k_shift (shift_kernels.h, compiled by shift.hip)
// what both forms refuse (the pointers are the caller's: host ones for qilqr_shift_batch, device ones for qilqr_shift_batch_device)
int shift_refuse(const qilqr_solver *s, const double *traj, const double *x0, int32_t B, int32_t n, int32_t steps, int32_t tail,
                 const double *out) {
  if (!s || !traj || !out) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || n <= 0) return fail(QILQR_ERR_INVALID_ARG, "B and n must be positive");
  if (steps < 0 || steps > n - 1)
    return fail(QILQR_ERR_INVALID_ARG, "shift: steps must be 0 ... n - 1 (" + std::to_string(steps) + " with n = " + std::to_string(n) + ")");
  if (tail != QILQR_TAIL_HOLD && tail != QILQR_TAIL_HOVER) return fail(QILQR_ERR_INVALID_ARG, "shift: tail must be QILQR_TAIL_HOLD or QILQR_TAIL_HOVER");
  if (s->f32) return fail(QILQR_ERR_INVALID_ARG, "shift: needs precision 0 (fp64)");
  if (s->modeled && B != s->models_B)
    return fail(QILQR_ERR_INVALID_ARG, "batch models were set for B = " + std::to_string(s->models_B) + " problems; this shift has B = " +
                                           std::to_string(B) + " (set them again, or clear them, for another batch)");
  if (off_16_bytes({traj, out, x0})) return fail(QILQR_ERR_INVALID_ARG, "shift: every array must be 16-byte aligned");
  // the copy is parallel and every block reads only the input: an output that overlaps an input is a race
  const size_t tb = sizeof(double) * 18 * (size_t)B * n, xb = sizeof(double) * QILQR_STATE * (size_t)B;
  if (ranges_overlap(traj, tb, out, tb)) return fail(QILQR_ERR_INVALID_ARG, "shift: the output overlaps the input (the shift does not work in place)");
  if (ranges_overlap(x0, xb, out, tb)) return fail(QILQR_ERR_INVALID_ARG, "shift: the output overlaps x0");
  return QILQR_OK;
}
int shift_enqueue(qilqr_solver *s, const double *d_traj, const double *d_x0, int32_t B, int32_t n, int32_t steps, int32_t tail, double *d_out) {
  const ShiftLaunch call{d_traj, d_x0, d_out, B, n, steps, tail, s->integrator, s->limited ? &s->limits : nullptr, s->modeled ? s->d_models : nullptr};
  return launched("k_shift", launch_shift(s->stream, s->consts, call));
}

// ---- the plan's feedback law flown from given states.  ONE flight: the plain call is the scored call without a wrench, a desired
// trajectory or a score, which launch_closed_loop_scored hands to k_closed_loop (closed_loop_kernels.h); with any of them the kernel is
// k_closed_loop_scored (closed_loop_scored_kernels.h).  `entry` and `kernel` are the names a HIP failure is reported under: the entry
// point's own.
struct FlightNames {
  const char *entry, *kernel;
};
constexpr FlightNames PLAIN_FLIGHT{"qilqr_closed_loop", "k_closed_loop"}, SCORED_FLIGHT{"qilqr_closed_loop_scored", "k_closed_loop_scored"};

// what both forms refuse (closed_loop_launch.h: closed_loop_scored_refusal; the pointers are the caller's, host or device ones)
int closed_loop_refuse(const qilqr_solver *s, const double *plan, const double *gains, const double *x0, const double *wrench, int32_t n_w,
                       const double *desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, const double *out_traj,
                       const double *out_stats, const double *out_score) {
  const ClosedLoopCall base{plan, gains, x0, out_traj, out_stats, B, n, S, i0, i1, s != nullptr, s && s->f32, s && s->modeled, s ? s->models_B : 0, out_score};
  const ClosedLoopScoredCall call{base, wrench, desired, n_w, s ? s->pobs_B : 0, s ? s->n_desired : 0, s ? s->n_sched : 0, s ? s->k0 : 0};
  bool length = false;
  const char *why = closed_loop_scored_refusal(call, &length);
  if (!why) return QILQR_OK;
  std::string text = why;
  if (length)
    return fail(QILQR_ERR_LENGTH_MISMATCH, text + " (i1 = " + std::to_string(i1) + ", horizon start " + std::to_string(s->k0) + ", desired trajectory of " +
                                               std::to_string(s->n_desired) + " knots" + (s->n_sched > 0 ? ", schedule of " + std::to_string(s->n_sched) : std::string()) + ")");
  if (s && s->modeled && !s->f32 && s->models_B != (long)B * S) text += ": they were set for " + std::to_string(s->models_B) + ", this call has B * S = " + std::to_string((long)B * S);
  return fail(QILQR_ERR_INVALID_ARG, text);
}
int closed_loop_enqueue(qilqr_solver *s, const char *kernel, const double *d_plan, const double *d_gains, const double *d_x0, const double *d_wrench,
                        int32_t n_w, const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, double *d_out_traj,
                        double *d_out_stats, double *d_out_score) {
  ClosedLoopScoredLaunch call{};
  call.base = ClosedLoopLaunch{d_plan, d_gains, d_x0, d_out_traj, d_out_stats, B, n, S, i0, i1, s->integrator, s->limited ? &s->limits : nullptr,
                              s->modeled ? s->d_models : nullptr};
  call.d_wrench = d_wrench;
  call.n_w = n_w;
  call.d_out_score = d_out_score;
  if (d_out_score)
    if (int rc = score_operands(s, d_desired, n, call.score)) return rc;
  return launched(kernel, launch_closed_loop_scored(s->stream, s->consts, call));
}

int closed_loop_device(qilqr_solver *s, const FlightNames &names, const double *d_plan, const double *d_gains, const double *d_x0, const double *d_wrench,
                       int32_t n_w, const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, double *d_out_traj,
                       double *d_out_stats, double *d_out_score) {
  int rc = closed_loop_refuse(s, d_plan, d_gains, d_x0, d_wrench, n_w, d_desired, B, n, S, i0, i1, d_out_traj, d_out_stats, d_out_score);
  if (rc) return rc;
  return on_device(s, [&] {
    return closed_loop_enqueue(s, names.kernel, d_plan, d_gains, d_x0, d_wrench, n_w, d_desired, B, n, S, i0, i1, d_out_traj, d_out_stats, d_out_score);
  });
}

int closed_loop_host(qilqr_solver *s, const FlightNames &names, const double *plan, const double *gains, const double *x0, const double *wrench,
                     int32_t n_w, const double *desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, double *out_traj, double *out_stats,
                     double *out_score) {
  int rc = closed_loop_refuse(s, plan, gains, x0, wrench, n_w, desired, B, n, S, i0, i1, out_traj, out_stats, out_score);
  if (rc) return rc;
  // as the initial trajectories are checked (manif's constructor check), naming the sample
  if ((rc = check_state_quaternions(x0, (long)B * S, S))) return rc;
  if (wrench)
    for (long r = 0; r < (long)B * S; ++r)
      for (long k = 0; k < n_w; ++k)
        for (int w = 0; w < QILQR_WRENCH; ++w)
          if (!std::isfinite(wrench[(r * n_w + k) * QILQR_WRENCH + w]))
            return fail(QILQR_ERR_INVALID_ARG, "wrench: a non-finite value at problem " + std::to_string(r / S) + ", sample " + std::to_string(r % S) + ", knot " +
                                                   std::to_string(k));
  HIP_TRY(hipSetDevice(s->device));
  DeviceScratch scratch;
  // (every count but x0's is even, and x0 goes last: each array starts on 16 bytes)
  const size_t samples = (size_t)B * S, pc = 18 * (size_t)B * n, gc = 52 * (size_t)B * n, xc = (size_t)QILQR_STATE * samples;
  const size_t tc = out_traj ? 18 * samples * n : 0, sc = out_stats ? QILQR_CL_STATS * samples : 0, oc = out_score ? QILQR_CL_SCORE * samples : 0;
  const size_t wc = wrench ? QILQR_WRENCH * samples * (size_t)n_w : 0, dc = desired ? pc : 0;
  HIP_TRY(hipMalloc((void **)&scratch.p, sizeof(double) * (pc + gc + tc + sc + oc + wc + dc + xc)));
  double *d_plan = scratch.p, *d_gains = d_plan + pc, *d_traj = d_gains + gc, *d_stats = d_traj + tc, *d_score = d_stats + sc, *d_wrench = d_score + oc,
         *d_desired = d_wrench + wc, *d_x0 = d_desired + dc;
  HIP_TRY(hipMemcpyAsync(d_plan, plan, sizeof(double) * pc, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_gains, gains, sizeof(double) * gc, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_x0, x0, sizeof(double) * xc, hipMemcpyHostToDevice, s->stream));
  if (wrench) HIP_TRY(hipMemcpyAsync(d_wrench, wrench, sizeof(double) * wc, hipMemcpyHostToDevice, s->stream));
  if (desired) HIP_TRY(hipMemcpyAsync(d_desired, desired, sizeof(double) * dc, hipMemcpyHostToDevice, s->stream));
  return enqueue_and_drain(
      s, names.entry,
      [&] {
        return closed_loop_enqueue(s, names.kernel, d_plan, d_gains, d_x0, wrench ? d_wrench : nullptr, n_w, desired ? d_desired : nullptr, B, n, S, i0, i1,
                                   out_traj ? d_traj : nullptr, out_stats ? d_stats : nullptr, out_score ? d_score : nullptr);
      },
      [&] {
        // knots i0 .. i1 of every sample, and nothing else of the caller's array: rows of (i1 - i0 + 1) knots at a pitch of n knots
        const size_t pitch = sizeof(double) * 18 * (size_t)n, off = 18 * (size_t)i0;
        hipError_t e = hipSuccess;
        if (out_traj)
          e = hipMemcpy2DAsync(out_traj + off, pitch, d_traj + off, pitch, sizeof(double) * 18 * (size_t)(i1 - i0 + 1), samples, hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess && out_stats) e = hipMemcpyAsync(out_stats, d_stats, sizeof(double) * sc, hipMemcpyDeviceToHost, s->stream);
        if (e == hipSuccess && out_score) e = hipMemcpyAsync(out_score, d_score, sizeof(double) * oc, hipMemcpyDeviceToHost, s->stream);
        return e;
      });
}
}  // namespace

extern "C" {
static_assert(QILQR_STATE == 13 && QILQR_TAIL_HOLD == 0 && QILQR_TAIL_HOVER == 1, "shift_kernels.h and the C header agree on the state words and the tails");
int qilqr_shift_batch_device(qilqr_solver *s, const double *d_traj, const double *d_x0, int32_t B, int32_t n, int32_t steps, int32_t tail,
                             double *d_out) {
  int rc = shift_refuse(s, d_traj, d_x0, B, n, steps, tail, d_out);
  if (rc) return rc;
  return on_device(s, [&] { return shift_enqueue(s, d_traj, d_x0, B, n, steps, tail, d_out); });
}

int qilqr_shift_batch(qilqr_solver *s, const double *traj, const double *x0, int32_t B, int32_t n, int32_t steps, int32_t tail, double *out) {
  int rc = shift_refuse(s, traj, x0, B, n, steps, tail, out);
  if (rc) return rc;
  // as the initial trajectories are checked (manif's constructor check), naming the problem
  if (x0 && (rc = check_state_quaternions(x0, B, 0))) return rc;
  HIP_TRY(hipSetDevice(s->device));
  DeviceScratch scratch;
  const size_t cnt = 18 * (size_t)B * n, xcnt = (size_t)QILQR_STATE * B;  // (cnt is even: input, output and x0 each start on 16 bytes)
  HIP_TRY(hipMalloc((void **)&scratch.p, sizeof(double) * (2 * cnt + xcnt)));
  double *d_in = scratch.p, *d_out = d_in + cnt, *d_x0 = x0 ? d_out + cnt : nullptr;
  HIP_TRY(hipMemcpyAsync(d_in, traj, sizeof(double) * cnt, hipMemcpyHostToDevice, s->stream));
  if (x0) HIP_TRY(hipMemcpyAsync(d_x0, x0, sizeof(double) * QILQR_STATE * (size_t)B, hipMemcpyHostToDevice, s->stream));
  return enqueue_and_drain(
      s, "qilqr_shift_batch", [&] { return shift_enqueue(s, d_in, d_x0, B, n, steps, tail, d_out); },
      [&] { return hipMemcpyAsync(out, d_out, sizeof(double) * cnt, hipMemcpyDeviceToHost, s->stream); });
}

// ---- gains about a plan that already sits on the device: qilqr_backwards_pass over plain device arrays -- the same linearise / k_init /
// launch_backward sequence through to_tiled / from_tiled, without the io scratch and the two copies over PCIe
int qilqr_backwards_pass_device(qilqr_solver *s, const double *d_traj, int32_t B, int32_t n, double *d_gains, double *d_terms) {
  if (!s || !d_traj || !d_gains) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  int rc = begin_batch(s, B, n, nullptr, E_PASS);
  if (rc) return rc;
  if ((rc = to_tiled(s, d_traj, s->st.traj[0], B, n, 18))) return rc;
  if ((rc = launch_linearize(s, B, n, 0, 0))) return rc;
  launch(s, K_OTHER, k_init, dim3(cdiv(B, 64)), dim3(64), s->params, s->st, (int)B, (int)n);
  if ((rc = launch_backward(s, B, n, 1))) return rc;
  if ((rc = from_tiled(s, d_gains, s->st.gains, s->st.gains, nullptr, 0, B, n, 52))) return rc;
  if (d_terms) HIP_TRY(hipMemcpyAsync(d_terms, s->st.terms, sizeof(double) * 2 * B, hipMemcpyDeviceToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipGetLastError());
  return device_error(s);
}

// ---- the closed-loop flights: the four entry points of closed_loop_device and closed_loop_host above
static_assert(QILQR_CL_STATS == 4, "closed_loop_kernels.h and the C header agree on the words of a sample's statistics");
static_assert(QILQR_CL_SCORE == 4 && QILQR_WRENCH == 6, "closed_loop_kernels.h and the C header agree on the words of a score and of a wrench");
int qilqr_closed_loop_device(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, int32_t B, int32_t n, int32_t S,
                             int32_t i0, int32_t i1, double *d_out_traj, double *d_out_stats) {
  return closed_loop_device(s, PLAIN_FLIGHT, d_plan, d_gains, d_x0, nullptr, 0, nullptr, B, n, S, i0, i1, d_out_traj, d_out_stats, nullptr);
}
int qilqr_closed_loop(qilqr_solver *s, const double *plan, const double *gains, const double *x0, int32_t B, int32_t n, int32_t S, int32_t i0,
                      int32_t i1, double *out_traj, double *out_stats) {
  return closed_loop_host(s, PLAIN_FLIGHT, plan, gains, x0, nullptr, 0, nullptr, B, n, S, i0, i1, out_traj, out_stats, nullptr);
}
int qilqr_closed_loop_scored_device(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, const double *d_wrench,
                                    int32_t n_w, const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1,
                                    double *d_out_traj, double *d_out_stats, double *d_out_score) {
  return closed_loop_device(s, SCORED_FLIGHT, d_plan, d_gains, d_x0, d_wrench, n_w, d_desired, B, n, S, i0, i1, d_out_traj, d_out_stats, d_out_score);
}
int qilqr_closed_loop_scored(qilqr_solver *s, const double *plan, const double *gains, const double *x0, const double *wrench, int32_t n_w,
                             const double *desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, double *out_traj, double *out_stats,
                             double *out_score) {
  return closed_loop_host(s, SCORED_FLIGHT, plan, gains, x0, wrench, n_w, desired, B, n, S, i0, i1, out_traj, out_stats, out_score);
}

// ---- the ends of the Monte-Carlo loop: k_sample_gusts, k_sample_states and k_reduce_scores (monte_carlo_kernels.h, compiled by
// monte_carlo.hip) on the caller's device arrays.  The handle gives its stream, its device and its dt; the rules are monte_carlo_launch.h's.
static_assert(QILQR_MC_SUMMARY == 8, "monte_carlo_kernels.h and the C header agree on the words of a plan's summary");
int qilqr_sample_gusts_device(qilqr_solver *s, const qilqr_gust_model *m, uint64_t seed, int32_t B, int32_t S, int32_t n_w, int32_t b0, int32_t s0,
                              double *d_wrench) {
  SampleGustsCall call{s != nullptr, m != nullptr, d_wrench, B, S, n_w, b0, s0, {}, {}, m ? m->tau_force_s : 0.0, m ? m->tau_torque_s : 0.0};
  for (int k = 0; k < 6; ++k) {
    call.mean[k] = m ? m->mean[k] : 0.0;
    call.sigma[k] = m ? m->sigma[k] : 0.0;
  }
  if (const char *why = sample_gusts_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  const SampleGustsLaunch go{d_wrench, B, S, n_w, b0, s0, seed, s->consts.dt, *m};
  return on_device(s, [&] { return launched("k_sample_gusts", launch_sample_gusts(s->stream, go)); });
}

int qilqr_sample_states_device(qilqr_solver *s, const double *d_x_nom, const double *sigma12, uint64_t seed, int32_t B, int32_t S, int32_t b0,
                               int32_t s0, uint32_t flags, double *d_x0) {
  SampleStatesCall call{s != nullptr, sigma12 != nullptr, d_x_nom, d_x0, B, S, b0, s0, flags, {}};
  for (int k = 0; k < 12; ++k) call.sigma[k] = sigma12 ? sigma12[k] : 0.0;
  if (const char *why = sample_states_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  SampleStatesLaunch go{d_x_nom, d_x0, B, S, b0, s0, flags, seed, {}};
  for (int k = 0; k < 12; ++k) go.sigma[k] = sigma12[k];
  return on_device(s, [&] { return launched("k_sample_states", launch_sample_states(s->stream, go)); });
}

int qilqr_reduce_scores_device(qilqr_solver *s, const double *d_score, int32_t B, int32_t S, double *d_summary) {
  const ReduceScoresCall call{s != nullptr, d_score, d_summary, B, S};
  if (const char *why = reduce_scores_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  return on_device(s, [&] { return launched("k_reduce_scores", launch_reduce_scores(s->stream, ReduceScoresLaunch{d_score, d_summary, B, S})); });
}
// ---- behind the reduction: tail measures per plan and the choice among a vehicle's candidates (k_risk_scores, k_select_plans and
// k_gather_plans: risk_kernels.h, compiled by risk.hip).  The handle gives its stream and its device; the rules are risk_launch.h's.
static_assert(QILQR_MC_RISK == 4 && QILQR_RISK_MAX_LEVELS == 8 && QILQR_RISK_MAX_SAMPLES == 4096 && QILQR_RISK_COST == 0 && QILQR_RISK_CLEARANCE == 1 &&
                  QILQR_SELECT_INFO == 4,
              "risk_kernels.h, risk_launch.h and the C header agree on the words of a level, the caps and the columns");
int qilqr_risk_scores_device(qilqr_solver *s, const double *d_score, int32_t B, int32_t S, int32_t column, const double *levels, int32_t n_levels,
                             double *d_risk) {
  const RiskScoresCall call{s != nullptr, d_score, d_risk, levels, B, S, column, n_levels};
  if (const char *why = risk_scores_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  const RiskScoresLaunch go{d_score, d_risk, B, S, column, n_levels, levels};
  return on_device(s, [&] { return launched("k_risk_scores", launch_risk_scores(s->stream, go)); });
}

int qilqr_select_plans_device(qilqr_solver *s, const double *d_summary, const double *d_risk, int32_t n_levels, const qilqr_select_rule *rule, int32_t V,
                              int32_t C, int32_t *d_choice, double *d_info, const double *d_plan, const double *d_gains, int32_t n, double *d_out_plan,
                              double *d_out_gains) {
  const SelectPlansCall call{s != nullptr, rule != nullptr, rule ? rule->objective : 0, rule ? rule->level : 0, rule ? rule->max_collision_fraction : 0.0,
                             rule ? rule->max_diverged_fraction : 0.0, rule ? rule->min_clearance : 0.0, d_summary, d_risk, d_choice, d_info, d_plan, d_gains,
                             d_out_plan, d_out_gains, n_levels, V, C, n};
  if (const char *why = select_plans_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  const bool risky = rule->objective >= 2;
  const SelectPlansLaunch go{d_summary, risky ? d_risk : nullptr, d_choice, d_info, risky ? n_levels : 0, V, C, *rule, d_plan, d_gains, d_out_plan, d_out_gains, n};
  return on_device(s, [&] { return launched("k_select_plans", launch_select_plans(s->stream, go)); });  // (one or two launches)
}
}  // extern "C"

// ---- the sampling planner: k_mppi_flight and k_mppi_update (mppi_kernels.h, compiled by mppi.hip) on the caller's device arrays.  ONE
// call: the flight is the update without d_out_plan and d_info.  The rule is mppi_launch.h's; the handle gives what it gives a scored flight.
namespace {
// the facts of a call for mppi_launch.h's rule
MppiCall mppi_call_of(const qilqr_solver *s, bool update, const qilqr_mppi_rule *rule, const double *d_plan, const double *d_x0, const double *d_desired,
                      const double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0, const double *d_out_plan, const double *d_info) {
  MppiCall call{};
  call.update = update;
  call.rule = rule != nullptr;
  if (rule) {
    for (int a = 0; a < 4; ++a) call.sigma[a] = rule->sigma[a];
    call.tau_s = rule->tau_s;
    call.lambda = rule->lambda;
    call.collision_cost = rule->collision_cost;
    call.flags = rule->flags;
    call.reserved = rule->reserved;
  }
  call.plan = d_plan; call.x0 = d_x0; call.desired = d_desired; call.score = d_score; call.out_plan = d_out_plan; call.info = d_info;
  call.B = B; call.n = n; call.S = S; call.b0 = b0;
  call.handle = s != nullptr;
  if (s) {
    call.f32 = s->f32; call.modeled = s->modeled; call.models_B = s->models_B; call.pobs_B = s->pobs_B;
    call.n_desired = s->n_desired; call.n_sched = s->n_sched; call.k0 = s->k0;
  }
  return call;
}
// the launch record of an admitted call
int mppi_launch_of(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0, const double *d_desired,
                   double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_out_plan, double *d_info, MppiLaunch &go) {
  go = MppiLaunch{d_plan, d_x0, d_score, d_out_plan, d_info, B, n, S, b0, seed, *rule, s->integrator, s->limited ? &s->limits : nullptr,
                  s->modeled ? s->d_models : nullptr, {}};
  return score_operands(s, d_desired, n, go.score);
}

int mppi_device(qilqr_solver *s, bool update, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0, const double *d_desired,
                double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_out_plan, double *d_info) {
  const MppiCall call = mppi_call_of(s, update, rule, d_plan, d_x0, d_desired, d_score, B, n, S, b0, d_out_plan, d_info);
  bool length = false;
  if (const char *why = mppi_refusal(call, &length)) return fail(length ? QILQR_ERR_LENGTH_MISMATCH : QILQR_ERR_INVALID_ARG, why);
  return on_device(s, [&] {
    MppiLaunch go{};
    if (int rc = mppi_launch_of(s, rule, seed, d_plan, d_x0, d_desired, d_score, B, n, S, b0, d_out_plan, d_info, go)) return rc;
    return launched(update ? "k_mppi_update" : "k_mppi_flight", update ? launch_mppi_update(s->stream, s->consts, go) : launch_mppi_flight(s->stream, s->consts, go));
  });
}

// the same two calls with the deviations per plan, knot and rotor (k_mppi_flight_spread and k_mppi_adapt: mppi_adapt_kernels.h, compiled
// by mppi_adapt.hip); the rule is mppi_adapt_launch.h's, which applies mppi_launch.h's first
int mppi_spread_device(qilqr_solver *s, bool adapting, const qilqr_mppi_rule *rule, const qilqr_mppi_adapt_rule *adapt, uint64_t seed, const double *d_plan,
                       const double *d_x0, const double *d_desired, const double *d_spread, double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0,
                       double *d_out_plan, double *d_out_spread, double *d_info) {
  MppiSpreadCall call{};
  call.base = mppi_call_of(s, adapting, rule, d_plan, d_x0, d_desired, d_score, B, n, S, b0, d_out_plan, d_info);
  call.adapt = adapt != nullptr;
  if (adapt) {
    for (int a = 0; a < 4; ++a) {
      call.floor[a] = adapt->floor[a];
      call.cap[a] = adapt->cap[a];
    }
    call.rate = adapt->rate;
    for (int k = 0; k < 3; ++k) call.reserved[k] = adapt->reserved[k];
  }
  call.spread = d_spread;
  call.out_spread = d_out_spread;
  bool length = false;
  if (const char *why = mppi_spread_refusal(call, &length)) return fail(length ? QILQR_ERR_LENGTH_MISMATCH : QILQR_ERR_INVALID_ARG, why);
  return on_device(s, [&] {
    MppiSpreadLaunch go{};
    if (int rc = mppi_launch_of(s, rule, seed, d_plan, d_x0, d_desired, d_score, B, n, S, b0, d_out_plan, d_info, go.base)) return rc;
    go.d_spread = d_spread;
    go.d_out_spread = d_out_spread;
    if (adapting) go.adapt = *adapt;
    return launched(adapting ? "k_mppi_adapt" : "k_mppi_flight_spread",
                    adapting ? launch_mppi_adapt(s->stream, s->consts, go) : launch_mppi_flight_spread(s->stream, s->consts, go));
  });
}
}  // namespace

extern "C" {
static_assert(QILQR_MPPI_INFO == 8 && QILQR_MPPI_FIRST_IS_NOMINAL == 1 && sizeof(qilqr_mppi_rule) == 64,
              "mppi_kernels.h, mppi_launch.h and the C header agree on the words of a plan's info, the flag and the rule");
int qilqr_mppi_flight_device(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0,
                             const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_score) {
  return mppi_device(s, false, rule, seed, d_plan, d_x0, d_desired, d_score, B, n, S, b0, nullptr, nullptr);
}
int qilqr_mppi_update_device(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0,
                             const double *d_desired, const double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_out_plan,
                             double *d_info) {
  return mppi_device(s, true, rule, seed, d_plan, d_x0, d_desired, const_cast<double *>(d_score), B, n, S, b0, d_out_plan, d_info);
}
static_assert(sizeof(qilqr_mppi_adapt_rule) == 96, "mppi_adapt_launch.h and the C header agree on the adapt rule");
int qilqr_mppi_flight_spread_device(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0,
                                    const double *d_desired, const double *d_spread, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_score) {
  return mppi_spread_device(s, false, rule, nullptr, seed, d_plan, d_x0, d_desired, d_spread, d_score, B, n, S, b0, nullptr, nullptr, nullptr);
}
int qilqr_mppi_adapt_device(qilqr_solver *s, const qilqr_mppi_rule *rule, const qilqr_mppi_adapt_rule *adapt, uint64_t seed, const double *d_plan,
                            const double *d_x0, const double *d_desired, const double *d_spread, const double *d_score, int32_t B, int32_t n, int32_t S,
                            int32_t b0, double *d_out_plan, double *d_out_spread, double *d_info) {
  return mppi_spread_device(s, true, rule, adapt, seed, d_plan, d_x0, d_desired, d_spread, const_cast<double *>(d_score), B, n, S, b0, d_out_plan,
                            d_out_spread, d_info);
}
}  // extern "C"

// ---- linear covariance analysis of a plan's closed loop: k_cov_build, k_cov_chain and k_cov_summary (cov_kernels.h, compiled by cov.hip)
// on the caller's device arrays.  The rule is cov_launch.h's; the handle gives its stream, its step, its models, its sphere tables and
// the scratch of the knots' operand images.
namespace {
// `words` doubles at *p (the handle's), grown when the call needs more: what runs on the stream may still read the old one
int cov_scratch(qilqr_solver *s, double **p, size_t *have, size_t words, bool zeroed) {
  if (*have >= words) return QILQR_OK;
  if (*p) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipFree(*p));
    *p = nullptr;
    *have = 0;
  }
  HIP_TRY(hipMalloc((void **)p, sizeof(double) * words));
  *have = words;
  // (the image's pads -- rows 12..15, wrench columns 6 and 7 -- are never written again: a knot's image is COV_IMAGE words wherever it lies)
  if (zeroed) HIP_TRY(hipMemsetAsync(*p, 0, sizeof(double) * words, s->stream));
  return QILQR_OK;
}
}  // namespace

extern "C" {
static_assert(QILQR_COV == 144 && QILQR_COV_SUMMARY == 8 && QILQR_COV_WRENCH_HELD == 1u && sizeof(qilqr_cov_rule) == 216,
              "cov_kernels.h, cov_launch.h and the C header agree on the words of a covariance, of a summary, the flag and the rule");
int qilqr_covariance_device(qilqr_solver *s, const qilqr_cov_rule *rule, const double *d_plan, const double *d_gains, int32_t B, int32_t n, int32_t i0,
                            int32_t i1, double *d_cov, double *d_mean, double *d_summary) {
  CovCall call{};
  call.rule = rule != nullptr;
  if (rule) {
    for (int k = 0; k < 12; ++k) call.state_sigma[k] = rule->state_sigma[k];
    for (int k = 0; k < 6; ++k) {
      call.mean[k] = rule->gust.mean[k];
      call.sigma[k] = rule->gust.sigma[k];
    }
    call.tau_force_s = rule->gust.tau_force_s;
    call.tau_torque_s = rule->gust.tau_torque_s;
    call.flags = rule->flags;
    call.reserved = rule->reserved;
  }
  call.plan = d_plan; call.gains = d_gains; call.cov = d_cov; call.mean_out = d_mean; call.summary = d_summary;
  call.B = B; call.n = n; call.i0 = i0; call.i1 = i1;
  call.handle = s != nullptr;
  if (s) {
    call.f32 = s->f32; call.modeled = s->modeled; call.models_B = s->models_B; call.pobs_B = s->pobs_B;
  }
  if (const char *why = cov_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  return on_device(s, [&] {
    const size_t knots = (size_t)B * (size_t)n;
    if (int rc = cov_scratch(s, &s->d_cov_image, &s->cov_image_words, knots * COV_IMAGE, true)) return rc;
    CovLaunch go{d_plan, d_gains, s->d_cov_image, d_cov, d_mean, d_summary, B, n, i0, i1, s->integrator, s->modeled ? s->d_models : nullptr, *rule, sphere_tables(s)};
    if (d_summary && (!d_cov || !d_mean)) {  // the summary reads Sigma_i and m_i where the chain left them
      if (int rc = cov_scratch(s, &s->d_cov_out, &s->cov_out_words, knots * (QILQR_COV + 12), false)) return rc;
      if (!d_cov) go.d_cov = s->d_cov_out;
      if (!d_mean) go.d_mean = s->d_cov_out + knots * QILQR_COV;
    }
    return launched("k_cov_chain", launch_covariance(s->stream, s->consts, go));
  });
}
}  // extern "C"

// ---- fleet deconfliction: k_fleet_fit, k_fleet_pairs and k_fleet_select on the caller's device plans, and k_bob_set from the caller's
// device table into the handle's (fleet_kernels.h, compiled by fleet.hip).  The rules are fleet_launch.h's; the handle gives its
// stream, its step, the neighbours call's scratch and the setter's table.
extern "C" {
static_assert(QILQR_FLEET_MAX_NEIGHBOURS == FLEET_MAX_NEIGHBOURS && QILQR_FLEET_NBR == FLEET_NBR && QILQR_FLEET_SUMMARY == FLEET_SUMMARY &&
                  QILQR_FLEET_COVER == FLEET_COVER && QILQR_FLEET_YIELD_TO_LOWER == FLEET_YIELD_TO_LOWER && sizeof(qilqr_fleet_rule) == 40,
              "fleet_math.h, fleet_launch.h and the C header agree on the cap, the words of an entry and of a summary, the flags and the rule");
int qilqr_fleet_neighbours_device(qilqr_solver *s, const qilqr_fleet_rule *rule, const double *d_plan, int32_t B, int32_t n, int32_t V, int32_t K,
                                  double *d_summary, double *d_nbr, double *d_spheres, int32_t *d_counts) {
  FleetCall call{};
  call.rule = rule != nullptr;
  if (rule) {
    call.radius = rule->radius; call.weight = rule->weight; call.range = rule->range; call.conflict = rule->conflict;
    call.flags = rule->flags;
    call.reserved = rule->reserved;
  }
  call.plan = d_plan; call.summary = d_summary; call.nbr = d_nbr; call.spheres = d_spheres; call.counts = d_counts;
  call.B = B; call.n = n; call.V = V; call.K = K;
  call.handle = s != nullptr;
  call.f32 = s && s->f32;
  if (const char *why = fleet_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  return on_device(s, [&] {
    if (int rc = cov_scratch(s, &s->d_fleet, &s->fleet_words, fleet_scratch(B, n, V, K).words, false)) return rc;
    const FleetLaunch go{d_plan, s->d_fleet, B, n, V, K, s->consts.dt, *rule, d_summary, d_nbr, d_spheres, d_counts};
    return launched("k_fleet_pairs", launch_fleet_neighbours(s->stream, go));
  });
}

int qilqr_set_batch_obstacles_device(qilqr_solver *s, const double *d_spheres, const int32_t *d_counts, int32_t B, int32_t K, int32_t *d_dropped) {
  const BobSetCall call{s != nullptr, s && s->f32, d_spheres, d_counts, d_dropped, B, K};
  if (const char *why = bob_set_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  return on_device(s, [&] {
    // the handle's table and counts, kept while they are large enough; what runs on the stream may still read the old ones
    const size_t words = (size_t)bob_count(B, K);
    if (s->pobs_cap < words || s->pobs_counts_cap < (size_t)B) {
      HIP_TRY(hipStreamSynchronize(s->stream));
      s->pobs_B = 0;  // (no table while the arrays are being replaced: a failure below leaves the handle without one)
      s->pobs_K = s->pobs_max = 0;
      s->pobs_moving = s->pobs_on_device = false;
      s->pobs_cap = s->pobs_counts_cap = 0;
      if (s->d_pobs) (void)hipFree(s->d_pobs);
      if (s->d_pobs_counts) (void)hipFree(s->d_pobs_counts);
      s->d_pobs = nullptr;
      s->d_pobs_counts = nullptr;
      HIP_TRY(hipMalloc((void **)&s->d_pobs, sizeof(double) * words));
      HIP_TRY(hipMalloc((void **)&s->d_pobs_counts, sizeof(int32_t) * (size_t)B));
      s->pobs_cap = words;
      s->pobs_counts_cap = (size_t)B;
    }
    const BobSetLaunch go{d_spheres, d_counts, B, K, s->d_pobs, s->d_pobs_counts, d_dropped};
    if (int rc = launched("k_bob_set", launch_bob_set(s->stream, go))) return rc;
    s->pobs_B = B;
    s->pobs_K = K;
    s->pobs_max = 0;
    s->pobs_moving = false;
    s->pobs_on_device = true;
    return (int)QILQR_OK;
  });
}
}  // extern "C"
