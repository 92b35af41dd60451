// host/launches.h -- from a call to its kernels: what of the handle the route reads (route.h plans it), the calls a handle refuses,
// begin_batch, and one launch_* helper per kernel family.  Each helper reads the route planned for the call and names the instantiation;
// the arguments a family's kernels share are written once in it.  Part of ilqr_capi.hip's translation unit.
#pragma once

namespace {
// what of the handle the route reads (models = false: a call that ignores the per-problem models, qilqr_cost_trajectory)
RouteInputs route_inputs(const qilqr_solver *s, bool models = true) {
  return RouteInputs{s->symmetric, s->q_diag, layout_kind(s->layout), s->f32, s->integrator, s->limited, s->modeled && models,
                     s->n_obstacles > 0 || s->pobs_B > 0, s->dev, s->num_cus, hw_queues(), s->pobs_B > 0, s->n_sched > 0};
}
// the entry point a call comes through: a batch solve, qilqr_solve, a stand-alone pass, or qilqr_cost_trajectory (which ignores the models:
// the cost does not depend on the model, and a call of any B takes the handle's own route); E_SIM: qilqr_forward_sim, a pass that
// evaluates no cost (it ignores the per-problem spheres)
enum Entry { E_BATCH, E_SOLVE, E_PASS, E_COST, E_SIM };
// The calls a handle refuses for what its extensions cannot do (the setters check the values they are given)
int refuse(const qilqr_solver *s, long B, Entry call) {
  if (call == E_BATCH && s->dev.persistent == 1) {
    if (s->limited) return fail(QILQR_ERR_INVALID_ARG, "control limits: persistent = 1 (k_solve4) has no box form; take the rounds (persistent = 0)");
    if (s->modeled)
      return fail(QILQR_ERR_INVALID_ARG, "batch models: persistent = 1 (k_solve4) has one model for the batch; take the rounds (persistent = 0)");
    if (s->n_obstacles > 0)
      return fail(QILQR_ERR_INVALID_ARG, "obstacles: persistent = 1 (k_solve4) linearises without them; take the rounds (persistent = 0)");
    if (s->pobs_B > 0)
      return fail(QILQR_ERR_INVALID_ARG, "batch obstacles: persistent = 1 (k_solve4) linearises without them; take the rounds (persistent = 0)");
    if (s->n_sched > 0)
      return fail(QILQR_ERR_INVALID_ARG, "state-weight schedule: persistent = 1 (k_solve4) linearises with the handle's Q; take the rounds (persistent = 0)");
  }
  // per-problem spheres (qilqr_set_batch_obstacles): problem b reads row b, so every call that evaluates the cost is over the rows they were
  // set for (qilqr_solve: B = 1)
  if (call != E_SIM && s->pobs_B > 0 && B != s->pobs_B)
    return fail(QILQR_ERR_INVALID_ARG, "batch obstacles were set for B = " + std::to_string(s->pobs_B) + " problems; this call has B = " +
                                           std::to_string(B) + " (set them again, or clear them, for another batch)");
  if (call == E_SOLVE && s->modeled)
    return fail(QILQR_ERR_INVALID_ARG, "batch models are set: qilqr_solve solves one problem with the handle's model; use qilqr_solve_batch, or "
                                       "clear the models");
  // per-problem models (qilqr_set_batch_models): problem b reads record b, so every computing call is over the rows they were set for
  if (call != E_COST && s->modeled && B != s->models_B)
    return fail(QILQR_ERR_INVALID_ARG, "batch models were set for B = " + std::to_string(s->models_B) + " problems; this call has B = " +
                                           std::to_string(B) + " (set them again, or clear them, for another batch)");
  return QILQR_OK;
}
// ", horizon start k0" for the messages of a handle that has one
std::string horizon_text(const qilqr_solver *s) { return s->k0 ? ", horizon start " + std::to_string(s->k0) : std::string(); }
// bind the desired trajectory (shared, or per problem: plain device array, re-tiled here), plan the call's route and reset the buffer
// selectors
int begin_batch(qilqr_solver *s, long B, long n, const double *d_desired_batch, Entry call) {
  if (B <= 0 || n <= 0) return fail(QILQR_ERR_INVALID_ARG, "B and n must be positive");
  // the desired trajectory and the schedule are indexed by the absolute knot, from the horizon start on (horizon.h; a pass that evaluates
  // no cost does not read the schedule)
  const char *why = nullptr;
  const int window = horizon_window_check(n, s->k0, s->n_desired, s->n_sched, !d_desired_batch, call != E_SIM, &why);
  if (window == HZ_LENGTH_SCHEDULE)
    return fail(QILQR_ERR_LENGTH_MISMATCH, std::string(why) + " (" + std::to_string(n) + " knots, " + std::to_string(s->n_sched) + " matrices" +
                                               horizon_text(s) + ")");
  if (window != HZ_OK)
    return fail(QILQR_ERR_LENGTH_MISMATCH, why + (s->k0 ? " (" + std::to_string(s->n_desired) + " knots" + horizon_text(s) + ")" : std::string()));
  int rc = refuse(s, B, call);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  rc = ensure_workspace(s, B, n);
  if (rc) return rc;
  if (d_desired_batch) {
    if (!s->desired_tiled && (rc = dalloc_s(s, &s->desired_tiled, (size_t)tiled_count(s->cap_B, s->cap_n, 18)))) return rc;
    if ((rc = to_tiled(s, d_desired_batch, s->desired_tiled, B, n, 18))) return rc;
    s->st.desired = s->desired_tiled;
    s->st.desired_tiled = 1;
  } else {
    // the shared one from the horizon start on: plain [n_desired][18] rows (k0 < n_desired, or 0: the setter; fp64 whenever k0 != 0: the
    // setter refuses the mixed mode)
    s->st.desired = (const char *)s->d_desired + (size_t)s->k0 * 18 * (s->f32 ? sizeof(float) : sizeof(double));
    s->st.desired_tiled = 0;
  }
  // (null without a schedule: k_linearize then fills Q from the handle's constants; with one, plain [n_sched][144] from the horizon start on)
  // (k0 < n_sched while both are set: either setter refuses the other case)
  s->st.q_sched = s->n_sched > 0 ? s->d_qsched + (size_t)s->k0 * SCHED_WORDS : nullptr;
  s->st.n_sched = s->n_sched > 0 ? s->n_sched - s->k0 : 0;
  s->total_B = B;
  s->live_hint = 0;  // (nothing known yet: launch_backward takes the batch)
  const CallFacts facts{s->dev.sync_every, d_desired_batch != nullptr, s->st.cost_hist != nullptr, s->early_out != nullptr, 0.0 < s->params.max_iters};
  s->route = plan_route(route_inputs(s, call != E_COST), B, facts);
  s->st.layout.tiled = s->route.tiled ? 1 : 0;
  launch(s, K_OTHER, k_begin, dim3(cdiv(B, 256)), dim3(256), s->st, (int)B);
  return QILQR_OK;
}

inline const ModelConsts<double> &consts_of(const qilqr_solver *s, double) { return s->consts; }
inline const ModelConsts<float> &consts_of(const qilqr_solver *s, float) { return s->constsf; }
// one k_linearize launch; the extension argument (per-problem models, obstacles, or both) rides behind the common ones
template <typename S, int LK, int INTEG, bool TILED, typename... Ext>
int lin(qilqr_solver *s, long B, long n, int which, int need_flag, int round, Ext... ext) {
  const dim3 grid(cdiv(2 * ((B + 63) / 64) * 64 * n, QILQR_LIN_BLOCK));  // dynamics half + cost half
  launch(s, K_LINEARIZE, (k_linearize<S, LK, INTEG, TILED, Ext...>), grid, dim3(QILQR_LIN_BLOCK), consts_of(s, S()),
         (const ModelConsts<S> *)s->d_consts, s->st, (int)B, (int)n, which, need_flag, round, ext...);
  return QILQR_OK;
}
// the trailing argument of the form `ext` names (route.h, LIN_*), as a tuple of none or one: the one place that chooses among them
template <int EXT>
auto lin_ext_args(const qilqr_solver *s, int which) {
  const BatchModels bm{s->d_models};
  const Obstacles ob{s->d_obstacles, s->n_obstacles};
  // the per-problem spheres by the problem's row: a compacting batch solve moves trajectories between slots, and from its first candidate
  // linearisation on (which = 1: behind k_init, which writes the map) the row of a slot is st.orig's
  const ProblemObstacles po{ob, s->d_pobs, s->d_pobs_counts, s->pobs_K, (s->compact && which == 1) ? 1 : 0};
  if constexpr (EXT == LIN_PLAIN) return std::tuple<>();
  else if constexpr (EXT == LIN_MODELS) return std::make_tuple(bm);
  else if constexpr (EXT == LIN_OBSTACLES) return std::make_tuple(ob);
  else if constexpr (EXT == LIN_BOTH) return std::make_tuple(ModelsObstacles{bm, ob});
  // the per-problem spheres (with or without shared ones): the obstacle route's instantiations, in the form that carries both tables
  else if constexpr (EXT == (LIN_OBSTACLES | LIN_PROBLEM)) return std::make_tuple(po);
  else return std::make_tuple(ModelsProblemObstacles{bm, po});
}
// the launch of one key of the key space: instantiated where the rule admits the key (route.h, lin_instantiated), null in the table elsewhere
using LinLaunch = int (*)(qilqr_solver *, long, long, int, int, int);
template <int KEY>
int lin_keyed(qilqr_solver *s, long B, long n, int which, int need_flag, int round) {
  using S = std::conditional_t<(KEY >> 4) & 1, float, double>;
  return std::apply([&](auto... ext) { return lin<S, KEY & 3, (KEY >> 2) & 1, ((KEY >> 3) & 1) != 0>(s, B, n, which, need_flag, round, ext...); },
                    lin_ext_args<(KEY >> 5)>(s, which));
}
template <int KEY>
constexpr LinLaunch lin_launch() {
  if constexpr (lin_instantiated(KEY)) return &lin_keyed<KEY>;
  else return nullptr;
}
template <int... KEY>
LinLaunch lin_launch_of(int key, std::integer_sequence<int, KEY...>) {
  static constexpr LinLaunch table[] = {lin_launch<KEY>()...};  // (one indexed call: no chain of compares)
  return key >= 0 && key < (int)sizeof...(KEY) ? table[key] : nullptr;
}
int launch_linearize(qilqr_solver *s, long B, long n, int which, int need_flag, int round = -1) {
  const Route &r = s->route;
  const int ext = (r.linearize_ext.models ? LIN_MODELS : LIN_PLAIN) | (r.linearize_ext.obstacles ? LIN_OBSTACLES : LIN_PLAIN) |
                  (r.linearize_ext.problem_obstacles ? LIN_PROBLEM : LIN_PLAIN);
  // (the placement of the records, s->st.layout.tiled, was chosen with the call's backward kernel: Route::tiled)
  const int key = lin_key(r.lin_kind, r.integrator, s->st.layout.tiled != 0, r.f32, ext);
  const LinLaunch go = lin_launch_of(key, std::make_integer_sequence<int, LIN_KEYS>());
  return go ? go(s, B, n, which, need_flag, round) : fail(QILQR_ERR_INVALID_ARG, "k_linearize: no instantiation for this route");
}
int launch_backward(qilqr_solver *s, long B, long n, int force) {
  // one launch of the family: the kernel over its blocks, the common arguments, and the extension's behind them
  auto bw = [&](auto kernel, dim3 grid, dim3 block, auto... ext) {
    launch(s, K_BACKWARD, kernel, grid, block, s->consts, s->params, s->st, (int)B, (int)n, force, ext...);
  };
  const dim3 each((unsigned)B), fours(cdiv(B, 4));  // a block per trajectory, or per four
  const Route &r = s->route;
  // `live` = the trajectories known to be running on the device in this call (every sub-batch stream's last count; the batch while nothing is known)
  const long live = s->live_hint > 0 ? s->live_hint : std::max(B, s->total_B);
  const BackwardKind kind = backward_now(r, live);
  if (kind == BW_FUSED) {
    // four matrix-and-gradient wavefronts + one loader wavefront per four trajectories, no block barrier in the knot loop
    // (one register budget: the pipelined knot carries the previous knot's tail and does not fit 80 registers)
    if (s->f32) bw(k_backward4<float, 5, true, true>, fours, dim3(320));
    else bw(k_backward4<double, 5, true, true>, fours, dim3(320));
  } else if (kind == BW_FOUR) {
    // four matrix wavefronts + one gradient wavefront + one loader wavefront per four trajectories
    // (register budget by how many blocks the chip has to hold: see k_backward4)
    const bool many = r.many, gfac = gradient_factors(r, live);
    if (gfac && s->f32) bw(k_backward4<float, 6, false, false, true>, fours, dim3(384));
    else if (gfac) bw(k_backward4<double, 6, false, false, true>, fours, dim3(384));
    else if (s->f32 && many) bw(k_backward4<float, 6>, fours, dim3(384));
    else if (s->f32) bw(k_backward4<float, 5>, fours, dim3(384));
    else if (many) bw(k_backward4<double, 6>, fours, dim3(384));
    else bw(k_backward4<double, 5>, fours, dim3(384));
#ifdef QILQR_WITH_BACKWARD2
  } else if (kind == BW_TWO) {
    // two cooperating wavefronts per trajectory (matrix recursion / gradient recursion + operand streaming)
    if (s->f32) bw(k_backward2<float>, each, dim3(128));
    else bw(k_backward2<double>, each, dim3(128));
#endif
  } else if (r.backward_ext.models) {  // the per-problem models extension (fp64): the constant rows of J_u from each problem's record
    const BatchModels bm{s->d_models};
    if (r.backward_ext.limits)  // ... with the thrust limits: the box form
      bw(k_backward_models<true, ControlLimits>, each, dim3(64), bm, s->limits);
    else if (s->symmetric) bw(k_backward_models<true>, each, dim3(64), bm);
    else bw(k_backward_models<false>, each, dim3(64), bm);
  } else if (r.backward_ext.limits) {  // the thrust-limit extension: the box form (symmetric weights, fp64: qilqr_set_control_limits)
    bw(k_backward<true, double, ControlLimits>, each, dim3(64), s->limits);
  } else if (s->symmetric) {
    if (s->f32) bw(k_backward<true, float>, each, dim3(64));
    else bw(k_backward<true, double>, each, dim3(64));
  } else {
    if (s->f32) bw(k_backward<false, float>, each, dim3(64));
    else bw(k_backward<false, double>, each, dim3(64));
  }
  return QILQR_OK;
}
// ordinal: which rollout of its solve this is (rollout16_now); -1: the stand-alone entry points
int launch_rollout(qilqr_solver *s, long B, long n, int need_flag, long ordinal = -1) {
  // one launch of the family: the kernel over its blocks, the model constants it takes (fp64's, or the lane-local kernels' own in the mixed
  // mode), the common arguments, and the extension's behind them
  auto ro = [&](auto kernel, dim3 grid, dim3 block, const auto &consts, auto... ext) {
    launch(s, K_ROLLOUT, kernel, grid, block, consts, s->st, (int)B, (int)n, need_flag, ext...);
  };
  const dim3 lanes(cdiv(B, 64)), fours(cdiv(B, 4));  // a block per 64 trajectories (a lane each), or per four
  // (which rollout kernel, by how many trajectories share the chip: route.h, RolloutRule)
  const Route &r = s->route;
  const ExtArgs &x = r.rollout_ext;
  if (r.rollout == RO_LANE && x.models) {  // the per-problem models extension (either integrator, with or without limits)
    const BatchModels bm{s->d_models};
    if (x.limits && r.integrator == 1) ro(k_rollout<double, 1, ControlLimits, BatchModels>, lanes, dim3(64), s->consts, s->limits, bm);
    else if (x.limits) ro(k_rollout<double, 0, ControlLimits, BatchModels>, lanes, dim3(64), s->consts, s->limits, bm);
    else if (r.integrator == 1) ro(k_rollout<double, 1, BatchModels>, lanes, dim3(64), s->consts, bm);
    else ro(k_rollout<double, 0, BatchModels>, lanes, dim3(64), s->consts, bm);
  } else if (r.rollout == RO_LANE && x.limits) {  // the thrust-limit extension (either integrator): controls clamped
    if (r.integrator == 1) ro(k_rollout<double, 1, ControlLimits>, lanes, dim3(64), s->consts, s->limits);
    else ro(k_rollout<double, 0, ControlLimits>, lanes, dim3(64), s->consts, s->limits);
  } else if (r.rollout == RO_LANE && r.integrator == 1) {  // the Runge-Kutta extension: the lane-per-trajectory kernel only
    ro(k_rollout<double, 1>, lanes, dim3(64), s->consts);
  } else if (r.rollout == RO_LANE) {  // (single_wave_rollout = 1: until round 4 also the choice above 16384)
    if (s->f32) ro(k_rollout<float, 0>, lanes, dim3(64), s->constsf);
    else ro(k_rollout<double, 0>, lanes, dim3(64), s->consts);
  } else if (rollout16_now(r, ordinal)) {
    if (s->f32) ro(k_rollout16<float>, fours, dim3(192), s->consts);
    else ro(k_rollout16<double>, fours, dim3(192), s->consts);
  } else {
    if (s->f32) ro(k_rollout3<float>, lanes, dim3(192), s->constsf);
    else ro(k_rollout3<double>, lanes, dim3(192), s->consts);
  }
  return QILQR_OK;
}

// k_round (round_kernels.h): the combined launch and the linearisation of its candidates in one (Route::round_kernel).  The round's counts go
// into the counter set of its parity; the launch publishes the round before it.
int launch_round(qilqr_solver *s, long B, long n, long round, bool publish_prev, int rounds, bool six = false) {
  const ModelConsts<double> *cp = (const ModelConsts<double> *)s->d_consts;
  six = round_instance(RoundForm{rounds, six}).six;  // (the six-wavefront form is instantiated for launches of one and of four rounds)
  const dim3 grid(cdiv(B, 4)), block(six ? 384 : 320);
  BatchState st = s->st;
  int *base = s->st.counters;
  st.counters = base + (round & 1) * COUNT_WORDS;
  int *prev = base + ((round + 1) & 1) * COUNT_WORDS;
  const int prev_round = publish_prev ? (int)((round - 1) & 0x3fffffff) : -1;
  const int lk = round_lk(s->route);
#define QILQR_LAUNCH_ROUND(LK, R, SIX)                                                                                                          \
  case LK * 16 + R * 2 + SIX:                                                                                                                     \
    launch(s, K_BACKWARD, (k_round<LK, R, SIX>), grid, block, s->consts, cp, s->params, st, (int)B, (int)n, prev, prev_round);                    \
    ++s->round_launches[round_slot(LK, R, SIX)]; /* (qilqr_round_launches: the slot of the case's own template arguments) */                    \
    break
  switch (lk * 16 + rounds * 2 + (six ? 1 : 0)) {
    QILQR_LAUNCH_ROUND(3, 4, true); QILQR_LAUNCH_ROUND(2, 4, true); QILQR_LAUNCH_ROUND(1, 4, true);
    QILQR_LAUNCH_ROUND(3, 1, true); QILQR_LAUNCH_ROUND(2, 1, true); QILQR_LAUNCH_ROUND(1, 1, true);
    QILQR_LAUNCH_ROUND(3, 4, false); QILQR_LAUNCH_ROUND(2, 4, false); QILQR_LAUNCH_ROUND(1, 4, false);
    QILQR_LAUNCH_ROUND(3, 2, false); QILQR_LAUNCH_ROUND(2, 2, false); QILQR_LAUNCH_ROUND(1, 2, false);
    QILQR_LAUNCH_ROUND(3, 1, false); QILQR_LAUNCH_ROUND(2, 1, false); QILQR_LAUNCH_ROUND(1, 1, false);
    default: return fail(QILQR_ERR_INVALID_ARG, "k_round: no instantiation for this launch");
  }
#undef QILQR_LAUNCH_ROUND
  return QILQR_OK;
}
int launch_backward_rollout(qilqr_solver *s, long B, long n) {
  auto br = [&](auto kernel) { launch(s, K_BACKWARD, kernel, dim3(cdiv(B, 4)), dim3(320), s->consts, s->params, s->st, (int)B, (int)n); };
  if (s->f32) br(k_backward_rollout<float>);
  else br(k_backward_rollout<double>);
  return QILQR_OK;
}
int launch_accept(qilqr_solver *s, long B, long n, int ls_only) {
  launch(s, K_OTHER, k_accept, dim3(cdiv(B, 64)), dim3(64), s->params, s->st, (int)B, (int)n,
                     ls_only);
  return QILQR_OK;
}

// ---- compaction of the live trajectories (route.h: COMPACT_STOP, Route::compact, tail_fuse)
// Behind a round's compaction every running trajectory sits in a slot below the count of running trajectories, and the last count
// the host has read is an upper bound of that (counts only fall): the kernels that follow are launched over that many slots instead
// of the whole batch (in its tail a batch of 65536 otherwise pays 53 us per k_linearize launch for 100 000 blocks that find nothing
// to do).  Whole groups of 64: k_linearize and k_rollout3 hand out 64 consecutive slots per wavefront.
inline long slots_in_use(long bound, unsigned seen_active) {
  const long want = std::max<long>(64, ((long)seen_active + 63) / 64 * 64);
  return std::min(bound, want);
}
int launch_compact(qilqr_solver *s, long B, long n) {
  launch(s, K_OTHER, k_compact_plan, dim3(1), dim3(1024), s->st, (int)B);
  const unsigned grid = std::min<unsigned>(cdiv(B, 2) * 2, 4096u);  // (work items: COMPACT_SPLIT per pair; the kernel strides over them)
  const int with_records = s->params.mu_init > 0.0 ? 1 : 0;  // a restart runs the recursion on the current records again
  if (s->f32)
    launch(s, K_OTHER, k_compact_move<float>, dim3(grid), dim3(256), s->st, (int)B, (int)n, s->compact_out, with_records);
  else
    launch(s, K_OTHER, k_compact_move<double>, dim3(grid), dim3(256), s->st, (int)B, (int)n, s->compact_out, with_records);
  return QILQR_OK;
}

int gather(qilqr_solver *s, long B, long n, double *d_traj, double *d_cost, int *d_status, int *d_iters,
           int *d_bwd, int *d_fwd, const int *mask = nullptr, int want = 0, const int *row_of = nullptr) {
  if (s->f32)
    launch(s, K_OTHER, k_gather<float>, dim3((unsigned)cdiv(B, TILE), (unsigned)cdiv(n * 9 * TILE, 256)), dim3(256), s->st, (int)B, (int)n,
                       d_traj, d_cost, d_status, d_iters, d_bwd, d_fwd, mask, want, row_of);
  else
    launch(s, K_OTHER, k_gather<double>, dim3((unsigned)cdiv(B, TILE), (unsigned)cdiv(n * 9 * TILE, 256)), dim3(256), s->st, (int)B, (int)n,
                       d_traj, d_cost, d_status, d_iters, d_bwd, d_fwd, mask, want, row_of);
  return QILQR_OK;
}

// The persistent solve (solve4.h; Route::persistent): every trajectory from its first linearisation to its exit status in ONE launch.
#ifdef QILQR_WITH_SOLVE4
int launch_solve4(qilqr_solver *s, long B, long n) {
  const unsigned groups = cdiv(B, 4);
  const unsigned grid = std::min<unsigned>(groups, (unsigned)s->num_cus);  // one block per CU (256 VGPRs, 105 KB of LDS); the rest queue
#define QILQR_LAUNCH_S4(S, LK) \
  launch(s, K_SOLVE, k_solve4<S, LK>, dim3(grid), dim3(S4_THREADS), s->consts, (const ModelConsts<S> *)s->d_consts, s->params, s->st, (int)B, (int)n, 0u)
  switch (layout_kind(s->layout) + (s->route.f32 ? 3 : 0)) {
    case 0: QILQR_LAUNCH_S4(double, 0); break;
    case 1: QILQR_LAUNCH_S4(double, 1); break;
    case 2: QILQR_LAUNCH_S4(double, 2); break;
    case 3: QILQR_LAUNCH_S4(float, 0); break;
    case 4: QILQR_LAUNCH_S4(float, 1); break;
    default: QILQR_LAUNCH_S4(float, 2); break;
  }
#undef QILQR_LAUNCH_S4
  return QILQR_OK;
}
#else
int launch_solve4(qilqr_solver *, long, long) { return fail(QILQR_ERR_INVALID_ARG, "k_solve4 is in the diagnostics build"); }
#endif
}  // namespace
