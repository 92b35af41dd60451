// host/describe.h -- a handle's choices in words (qilqr_describe), the compaction's move count, and the entry points that exist in
// the diagnostics builds only.  Part of ilqr_capi.hip's translation unit.
#pragma once

extern "C" {
// In words: which arithmetic and which kernels a batch solve of B problems on this handle uses (the choice between the
// reference's own forms and the symmetric-weight kernels is made by whether Q and R are bit-exactly symmetric, and was silent).
int qilqr_describe(qilqr_solver *s, int32_t B, char *buf, size_t cap) {
  if (!s || !buf || cap == 0 || B <= 0) return fail(QILQR_ERR_INVALID_ARG, "bad argument");
  // (the route of a device-resident batch solve with the handle's shared desired trajectory: nothing of the handle is touched)
  const Route r = plan_route(route_inputs(s), B, CallFacts{s->dev.sync_every});
  std::string t;
  const bool persistent = r.persistent;
  const BackwardKind kind = persistent ? BW_FOUR : r.backward;
  if (kind == BW_ONE && !r.symmetric)
    t += "arithmetic: the reference's own forms (ilqr.hh:126-133: Eigen's diagonally pivoted LDL^T, V_x = Q_x - K^T Q_uu k, V_xx = Q_xx - K^T Q_uu K, "
         "not symmetrised)";
  else
    t += "arithmetic: symmetric-weight forms (Q == Q^T and R == R^T exactly: unpivoted LDL^T, V_x = Q_x + K^T Q_u, V_xx = Q_xx + Q_xu K on a symmetric "
         "accumulator; force_general = 1 selects the reference's own forms)";
  t += s->integrator == 1 ? "; Runge-Kutta step (extension)" : "; explicit Euler step (the reference's)";
  if (s->limited) {
    char lim[256];
    std::snprintf(lim, sizeof lim, "; control limits [lo, hi] (extension): lo = {%g, %g, %g, %g}, hi = {%g, %g, %g, %g} N, box QP per knot",
                  s->limits.lo[0], s->limits.lo[1], s->limits.lo[2], s->limits.lo[3], s->limits.hi[0], s->limits.hi[1], s->limits.hi[2], s->limits.hi[3]);
    t += lim;
  }
  if (s->modeled)
    t += "; per-problem models (extension): " + std::to_string(s->models_B) + " problems, each with its own mass, g, inertia and moment arms" +
         (B != s->models_B ? " (a call of B = " + std::to_string(B) + " problems is refused)" : std::string());
  if (s->n_obstacles > 0) {
    t += "; obstacles (extension): " + std::to_string(s->n_obstacles) + " sphere(s) {center; radius, weight} =";
    for (int j = 0; j < s->n_obstacles; ++j) {
      const double *sp = s->obstacles.data() + (size_t)j * OB_WORDS;
      char one[160];
      std::snprintf(one, sizeof one, "%s {%g, %g, %g; %g, %g}", j ? "," : "", sp[0], sp[1], sp[2], sp[OB_RADIUS], sp[OB_WEIGHT]);
      t += one;
    }
    t += ", penalised in the knot cost by k_linearize (the rounds never take the kernels that linearise inside themselves)";
  }
  if (s->pobs_B > 0)
    t += "; batch obstacles (extension): per-problem spheres for B = " + std::to_string(s->pobs_B) + " problems, K = " + std::to_string(s->pobs_K) +
         (s->pobs_on_device ? std::string(", set on the device (qilqr_set_batch_obstacles_device: the counts and whether a sphere moves are not known here)")
                            : ", at most " + std::to_string(s->pobs_max) + " used per problem, " + (s->pobs_moving ? "some moving" : "none moving")) +
         ", penalised in the knot cost by k_linearize (the rounds never take the kernels that linearise inside themselves)" +
         (B != s->pobs_B ? " (a call of B = " + std::to_string(B) + " problems is refused)" : std::string());
  if (s->n_sched > 0)
    t += "; state-weight schedule (extension): n_knots = " + std::to_string(s->n_sched) + ", " +
         (s->sched_symmetric ? "every Q_i symmetric" : "not every Q_i symmetric") +
         ", knot i takes Qs[i] for Q in the cost half of k_linearize; the route of non-symmetric weights (dense records of kind 0, the "
         "one-wavefront backward kernel, three launches per round) whatever the handle's Q is";
  if (s->k0 != 0)
    t += "; horizon start (extension): knot i of a call reads desired[" + std::to_string(s->k0) + " + i] of the handle's desired trajectory" +
         (s->n_sched > 0 ? " and Qs[" + std::to_string(s->k0) + " + i] of the schedule" : std::string()) +
         " (a per-problem desired_batch and both sphere tables are the call's own)";
  t += s->f32 ? "; mixed precision (fp32 storage and lane-local arithmetic, fp64 recursion and cost sums)" : "; fp64";
  t += "; backward: ";
  t += persistent ? "k_solve4 (one launch per solve)" : kind == BW_FUSED ? "k_backward4, fused matrix + gradient wavefronts" : kind == BW_FOUR ? "k_backward4, six wavefronts"
       : kind == BW_TWO ? "k_backward2" : r.backward_ext.models ? std::string("k_backward_models<") + (r.symmetric ? "true>" : "false>") +
                                                        (r.backward_ext.limits ? " box form" : "") + ", one wavefront per trajectory"
       : r.backward_ext.limits ? "k_backward<true> box form, one wavefront per trajectory"
       : (r.symmetric ? "k_backward<true>, one wavefront per trajectory" : "k_backward<false>, one wavefront per trajectory (general kernel)");
  if (kind == BW_FOUR || backward_now(r, B) != kind)
    t += kind == BW_FOUR ? " (Q_uu factored by the gradient wavefront in launches with " + std::to_string(GFAC_MIN_LIVE) + " or more running trajectories, by the matrix wavefronts otherwise: the same bits)"
                         : " (six wavefronts, Q_uu factored by the gradient wavefront, while " + std::to_string(GFAC_MIN_LIVE) + " or more trajectories run: the same bits)";
  if (!persistent) {
    t += "; rollout: ";
    t += r.rollout == RO_LANE ? "k_rollout" : r.rollout == RO_16 ? "k_rollout16"
         : r.rollout == RO_THREE_THEN_16 ? "k_rollout3 for a trajectory's first " + std::to_string(ROLLOUT16_FROM) + " rollouts, k_rollout16 from there on" : "k_rollout3";
    const bool fused = r.combined && s->dev.sync_every > 1;
    const int parts = r.parts;
    const bool compact = r.compact;
    // the round's launch form by the predicates the rounds use: the combined launch on one stream where the compaction does not work between its halves
    if (fused && parts == 1 && !compact)
      t += r.round_kernel ? "; round: one launch (k_round), " + std::to_string(r.rounds_per_launch) + " rounds per launch, while no other batch solve of the process is in flight on the device"
                          : std::string("; round: k_backward_rollout + k_linearize");
    else if (compact && r.fuse_kinds)
      t += "; round: three launches while the compaction runs, then " +
           std::string(r.linearize_ext.obstacles ? "k_backward_rollout + k_linearize (obstacles)" : "k_round (the mixed mode: k_backward_rollout + k_linearize)") +
           " once the running trajectories fit " + std::to_string(std::min(parts, 3)) + " block(s) of four per CU";
    else if (compact && r.compaction != 1 && r.late_tail)
      t += "; round: three launches, then " +
           std::string(r.linearize_ext.obstacles ? "k_backward_rollout + k_linearize (the same bits; obstacles)" : "k_round (the same bits; the mixed mode: k_backward_rollout + k_linearize)") +
           " once the running trajectories fit " + std::to_string(std::min(parts, 3)) + " block(s) of four per CU"
           + (r.late_from > 0 ? " and the rollouts are k_rollout16's (round " + std::to_string(r.late_from) + " on)" : std::string());
    else
      t += "; round: three launches";
    t += "; sub-batch streams: " + std::to_string(parts);
    t += compact ? "; compaction of the running trajectories: on (device-resident calls)" : "; compaction: off";
  }
  std::snprintf(buf, cap, "%s", t.c_str());
  return QILQR_OK;
}

// trajectories k_compact_move moved in the last batch solve of this handle (0: compaction was off, or nothing finished early)
int qilqr_compaction_moves(qilqr_solver *s, int64_t *moves) {
  if (!s || !moves) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *moves = 0;
  for (long head : s->plan_heads) {
    int m = 0;
    HIP_TRY(hipMemcpy(&m, s->st.plan + head + 2, sizeof(int), hipMemcpyDeviceToHost));
    *moves += m;
  }
  return QILQR_OK;
}

#if defined(QILQR_STAMPS) || defined(QILQR_ROUND_STAMPS)
// diagnostic build only: per-trajectory section cycle sums of the last k_backward launch
int qilqr_debug_stamps(qilqr_solver *s, unsigned long long *out, int32_t B) {
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(out, s->st.stamps, sizeof(unsigned long long) * 8 * B, hipMemcpyDeviceToHost));
  return QILQR_OK;
}
#endif

#ifdef QILQR_DIAG
// diagnostics build only: from now on the step wavefronts of k_rollout16 withhold the velocity hand-off of knot `knot` (-1: none
// again), on the device the solver is bound to -- the other wavefront's bounded spin then runs out and the block is abandoned
// 1: the late finishers of the copy-back under the tail go through the compact block and the host's scatter although the caller's arrays map
// (the fallback's parity test; A/B of the two forms)
int qilqr_debug_set_staged_late(int32_t on) {
  g_force_staged_late = on ? 1 : 0;
  return QILQR_OK;
}
int qilqr_debug_set_rollout_stall(qilqr_solver *s, int32_t knot) {
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_r16_stall_knot), &knot, sizeof(int)));
  return QILQR_OK;
}
// the same for k_backward4's barrier-free form: the loader withholds the tags of record `rec` (-1: none again)
int qilqr_debug_set_backward_stall(qilqr_solver *s, int32_t rec) {
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bw4_stall_rec), &rec, sizeof(int)));
  return QILQR_OK;
}
// diagnostic build only (make diag; profiles/microbench/beside.py): the rollout kernel of the
// state a qilqr_forward_sim call left behind, `reps` times on the solver's stream, alone (beside = 0) or while a second
// stream runs k_linearize launches back to back (beside = 1).  us[0]: microseconds per rollout launch; us[1]: per
// linearisation launch.  Timing only: the linearisation reads the candidate while it is being written.
int qilqr_debug_rollout_beside_linearize(qilqr_solver *s, int32_t B, int32_t n, int32_t reps, int32_t beside, float *us) {
  if (beside && s->pobs_B > 0 && B != s->pobs_B)  // (k_linearize reads the per-problem spheres of rows 0 .. B - 1)
    return fail(QILQR_ERR_INVALID_ARG, "batch obstacles were set for B = " + std::to_string(s->pobs_B) + " problems");
  HIP_TRY(hipSetDevice(s->device));
  int rc;
  if ((rc = ensure_parts(s, 1))) return rc;
  hipEvent_t e[4];
  for (auto &x : e) HIP_TRY(hipEventCreate(&x));
  HIP_TRY(hipStreamSynchronize(s->stream));
  hipStream_t main_stream = s->stream, side = s->part_stream[0];
  const int nlin = 4 * reps;
  if (beside) {
    s->stream = side;
    HIP_TRY(hipEventRecord(e[2], side));
    for (int k = 0; k < nlin; ++k)
      if ((rc = launch_linearize(s, B, n, 1, 0, -1))) break;
    HIP_TRY(hipEventRecord(e[3], side));
    s->stream = main_stream;
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(e[0], main_stream));
  for (int k = 0; k < reps; ++k)
    if ((rc = launch_rollout(s, B, n, 0))) return rc;
  HIP_TRY(hipEventRecord(e[1], main_stream));
  HIP_TRY(hipStreamSynchronize(main_stream));
  HIP_TRY(hipStreamSynchronize(side));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
  us[0] = 1e3f * ms / reps;
  us[1] = 0.f;
  if (beside) {
    HIP_TRY(hipEventElapsedTime(&ms, e[2], e[3]));
    us[1] = 1e3f * ms / nlin;
  }
  for (auto &x : e) HIP_TRY(hipEventDestroy(x));
  return QILQR_OK;
}
#endif
}  // extern "C"
