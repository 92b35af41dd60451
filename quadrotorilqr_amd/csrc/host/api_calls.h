// host/api_calls.h -- the C ABI of the computing calls on one handle: the batch solves, qilqr_solve, the four stand-alone passes, the
// pinned host memory for their callers, the receding-horizon shift (whose kernel is shift.hip's), the backward pass over device arrays and the
// closed-loop flights of a plan (whose kernel is closed_loop.hip's).  Part of ilqr_capi.hip's translation unit.
#pragma once

extern "C" {
int qilqr_solve_batch_device(qilqr_solver *s, const double *d_init, const double *d_desired_batch, int32_t B,
                             int32_t n, double *d_out_traj, double *d_out_cost, int32_t *d_out_status,
                             int32_t *d_out_iters, int32_t *d_out_n_bwd, int32_t *d_out_n_fwd) {
  return solve_batch_device_impl(s, d_init, d_desired_batch, B, n, d_out_traj, d_out_cost, d_out_status, d_out_iters,
                                 d_out_n_bwd, d_out_n_fwd, /*drain=*/true);
}

// Order the solver's stream behind work of another stream: the solver's stream waits (on the device, no host
// stall) for `hip_event`, a hipEvent_t the caller recorded on the stream that produces the input buffers.
int qilqr_stream_wait_event(qilqr_solver *s, void *hip_event) {
  if (!s || !hip_event) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamWaitEvent(s->stream, (hipEvent_t)hip_event, 0));
  return QILQR_OK;
}

// host-buffer wrapper: solve_batch_staged, then the copies back -- behind the gather on the solver's stream, or, for a batch
// whose outputs are pinned, in two parts with the first under the tail rounds of the solve (EarlyOut)
namespace {
bool pinned_or_null(const void *p) {
  if (!p) return true;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (an ordinary malloc'ed pointer is reported as an error by some runtimes: not pinned, and not sticky)
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
}  // namespace
int qilqr_solve_batch(qilqr_solver *s, const double *init, const double *desired_batch, int32_t B, int32_t n,
                      double *out_traj, double *out_cost, int32_t *out_status, int32_t *out_iters,
                      int32_t *out_n_bwd, int32_t *out_n_fwd) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // the two-part copy-back pays when the trajectories are megabytes and the rounds run free on one stream; it needs pinned
  // outputs (a copy to pageable memory would hold this thread, which has rounds to enqueue)
  EarlyOut eo{out_traj, out_cost, out_status, out_iters, out_n_bwd, out_n_fwd};
  LateLayout late{};
  eo.layout = &late;
  const Route route = plan_route(route_inputs(s), B, CallFacts{s->dev.sync_every});
  const bool early = out_traj && B >= 256 && (size_t)B * n * 144 >= ((size_t)2 << 20) && s->dev.sync_every > 1 && route.parts == 1 &&
                     !route.persistent && 0.0 < s->params.max_iters && pinned_or_null(out_traj) && pinned_or_null(out_cost) &&
                     pinned_or_null(out_status) && pinned_or_null(out_iters) && pinned_or_null(out_n_bwd) && pinned_or_null(out_n_fwd);
  if (early) {
    eo.threshold = (unsigned)(B / 8);
    HIP_TRY(hipSetDevice(s->device));
    // (the staged form of the late part stays as the fallback for arrays that do not map; the diagnostics build can force it: A/B, its test)
    auto mapped = [](void *h, auto **v) -> bool {
      if (!h) return true;
      void *d = nullptr;
      if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        return false;
      }
      *v = (std::remove_reference_t<decltype(*v)>)d;
      return true;
    };
    eo.direct = !g_force_staged_late && mapped(out_traj, &eo.v_traj) && mapped(out_cost, &eo.v_cost) && mapped(out_status, &eo.v_status) &&
                mapped(out_iters, &eo.v_iters) && mapped(out_n_bwd, &eo.v_bwd) && mapped(out_n_fwd, &eo.v_fwd);
    int rc0 = ensure_early_buffers(s, B, n, eo.threshold);
    if (rc0) return rc0;
    s->early_out = &eo;
  }
  int rc = solve_batch_staged(s, init, desired_batch, B, n);
  s->early_out = nullptr;
  if (rc != QILQR_OK) {
    if (eo.fired) {  // nothing of a failed call keeps writing the caller's arrays
      (void)hipStreamSynchronize(s->early_stream);
      (void)hipStreamSynchronize(s->stream);
    }
    return rc;
  }
  const size_t tb = sizeof(double) * 18 * (size_t)B * n;
  const double *d_cost = s->stage_cost;
  const int *d_int = s->stage_int;
  hipError_t e = hipSuccess;
  if (eo.fired) {
    e = hipStreamSynchronize(s->early_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && !eo.direct) {
      const int count = *(const int *)(s->h_late + late.count);
      if (count < 0 || count > eo.late_cap) return fail(QILQR_ERR_HIP, "copy back: more late trajectories than were running");
      const int *idx = (const int *)(s->h_late + late.idx);
      const double *lt = (const double *)(s->h_late + late.traj), *lc = (const double *)(s->h_late + late.cost);
      const int *li = (const int *)(s->h_late + late.ints);
      const size_t row = (size_t)n * 18;
      for (int k = 0; k < count; ++k) {
        const int b = idx[k];
        std::memcpy(out_traj + (size_t)b * row, lt + (size_t)k * row, sizeof(double) * row);
        if (out_cost) out_cost[b] = lc[k];
        if (out_status) out_status[b] = li[k];
        if (out_iters) out_iters[b] = li[eo.late_cap + k];
        if (out_n_bwd) out_n_bwd[b] = li[2 * eo.late_cap + k];
        if (out_n_fwd) out_n_fwd[b] = li[3 * eo.late_cap + k];
      }
    }
  } else {
    if (out_traj) e = hipMemcpyAsync(out_traj, s->stage_traj, tb, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_cost) e = hipMemcpyAsync(out_cost, d_cost, sizeof(double) * B, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_status) e = hipMemcpyAsync(out_status, d_int, sizeof(int) * B, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_iters) e = hipMemcpyAsync(out_iters, d_int + B, sizeof(int) * B, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_n_bwd) e = hipMemcpyAsync(out_n_bwd, d_int + 2 * B, sizeof(int) * B, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_n_fwd) e = hipMemcpyAsync(out_n_fwd, d_int + 3 * B, sizeof(int) * B, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipGetLastError();
  }
  if (s->dev.profile) drain_events(s);
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("copy back: ") + hipGetErrorString(e));
  return device_error(s);
}

// pinned host memory for callers of the host-buffer entry points (direct DMA instead of HIP's pageable staging)
void *qilqr_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    g_last_error = "hipHostMalloc failed";
    return nullptr;
  }
  return p;
}
void qilqr_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int qilqr_solve(qilqr_solver *s, const double *init, int32_t n, double *out_traj, double *out_cost,
                int32_t *out_status, int32_t *out_iters, double *debug_cost, double *debug_trajs,
                int32_t debug_cap, int32_t *n_debug) {
  if (!s || !init || !out_traj) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  if (n <= 0) return fail(QILQR_ERR_INVALID_ARG, "empty trajectory");
  int rc;
  if ((rc = check_quaternions(init, n, "initial trajectory"))) return rc;
  if ((rc = begin_batch(s, 1, n, nullptr, E_SOLVE))) return rc;
  if ((rc = upload_tiled(s, init, s->st.traj[0], 1, n, 18))) return rc;
  const bool want_debug = s->options.populate_debug && debug_cap > 0 && (debug_cost || debug_trajs);
  if (want_debug) {
    // the ring lives in device memory (k_debug_capture appends to it behind every round's settle step); one download at the end
    const size_t want_t = debug_trajs ? (size_t)debug_cap * n * 18 : 0, want_c = (size_t)debug_cap;
    if (want_t > s->dbg_traj_cap) {
      if (s->dbg_trajs) (void)hipFree(s->dbg_trajs);
      s->dbg_trajs = nullptr;
      s->dbg_traj_cap = 0;
      HIP_TRY(hipMalloc((void **)&s->dbg_trajs, sizeof(double) * want_t));
      s->dbg_traj_cap = want_t;
    }
    if (want_c > s->dbg_cost_cap) {
      if (s->dbg_cost) (void)hipFree(s->dbg_cost);
      s->dbg_cost = nullptr;
      s->dbg_cost_cap = 0;
      HIP_TRY(hipMalloc((void **)&s->dbg_cost, sizeof(double) * want_c));
      s->dbg_cost_cap = want_c;
    }
    if (!s->dbg_seen) HIP_TRY(hipMalloc((void **)&s->dbg_seen, sizeof(int)));
    HIP_TRY(hipMemsetAsync(s->dbg_seen, 0, sizeof(int), s->stream));
    // the ring as k_round sees it: an idle wavefront of the launch captures behind every round's backward pass (debug_capture_wave), so the
    // launches keep their four rounds; rounds of separate launches are followed by k_debug_capture as before (`capture` below)
    s->st.dbg_trajs = debug_trajs ? s->dbg_trajs : nullptr;
    s->st.dbg_cost = s->dbg_cost;
    s->st.dbg_seen = s->dbg_seen;
    s->st.dbg_cap = (int)debug_cap;
  }
  struct DebugRingScope {  // (no other entry point sees the ring)
    qilqr_solver *s;
    ~DebugRingScope() { s->st.dbg_trajs = s->st.dbg_cost = nullptr; s->st.dbg_seen = nullptr; s->st.dbg_cap = 0; }
  } ring_scope{s};
  auto capture = [&]() -> int {
    // ilqr.hh:78-80: one entry per completed forward pass (accepted iteration)
    if (!want_debug || s->round_captured) return QILQR_OK;  // (a k_round launch has captured its own rounds)
    if (s->f32)
      launch(s, K_OTHER, k_debug_capture<float>, dim3(1), dim3(256), s->st, (int)n, debug_trajs ? s->dbg_trajs : nullptr, s->dbg_cost, s->dbg_seen, (int)debug_cap);
    else
      launch(s, K_OTHER, k_debug_capture<double>, dim3(1), dim3(256), s->st, (int)n, debug_trajs ? s->dbg_trajs : nullptr, s->dbg_cost, s->dbg_seen, (int)debug_cap);
    return QILQR_OK;
  };
  // (without debug entries nobody looks at the solve round by round: the launches may hold several rounds)
  if ((rc = run_solve(s, 1, n, s->dev.sync_every, capture, true, nullptr, /*double_ok=*/true))) return rc;
  int status = 0, iters = 0, seen = 0;
  double cost = 0;
  HIP_TRY(hipMemcpy(&status, s->st.status, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&iters, s->st.iters, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&cost, s->st.cost, sizeof(double), hipMemcpyDeviceToHost));
  if (want_debug) {
    HIP_TRY(hipMemcpy(&seen, s->dbg_seen, sizeof(int), hipMemcpyDeviceToHost));
    const int have = seen < debug_cap ? seen : debug_cap;
    if (have > 0 && debug_cost) HIP_TRY(hipMemcpy(debug_cost, s->dbg_cost, sizeof(double) * have, hipMemcpyDeviceToHost));
    if (have > 0 && debug_trajs) HIP_TRY(hipMemcpy(debug_trajs, s->dbg_trajs, sizeof(double) * (size_t)have * n * 18, hipMemcpyDeviceToHost));
  }
  if (s->dev.profile) drain_events(s);
  if (n_debug) *n_debug = want_debug ? (seen < debug_cap ? seen : debug_cap) : 0;
  if (status == QILQR_STATUS_LINE_SEARCH_FAILED)
    return fail(QILQR_ERR_LINE_SEARCH, "Reached maximum number of line search iterations, " +
                                           std::to_string(s->options.ls_max_iters) + "\n");
  if ((rc = download_tiled(s, out_traj, s->st.traj[0], s->st.traj[1], s->st.cur, 0, 1, n, 18))) return rc;
  if (out_cost) *out_cost = cost;
  if (out_status) *out_status = status;
  if (out_iters) *out_iters = iters;
  return QILQR_OK;
}

int qilqr_cost_trajectory(qilqr_solver *s, const double *traj, int32_t B, int32_t n, double *cost) {
  if (!s || !traj || !cost) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  int rc = begin_batch(s, B, n, nullptr, E_COST);
  if (rc) return rc;
  if ((rc = upload_tiled(s, traj, s->st.traj[0], B, n, 18))) return rc;
  if ((rc = launch_linearize(s, B, n, 0, 0))) return rc;
  launch(s, K_OTHER, k_init, dim3(cdiv(B, 64)), dim3(64), s->params, s->st, (int)B, (int)n);
  HIP_TRY(hipMemcpyAsync(cost, s->st.cost, sizeof(double) * B, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipGetLastError());
  return QILQR_OK;
}

int qilqr_backwards_pass(qilqr_solver *s, const double *traj, int32_t B, int32_t n, double *gains, double *terms) {
  if (!s || !traj || !gains || !terms) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  int rc = begin_batch(s, B, n, nullptr, E_PASS);
  if (rc) return rc;
  if ((rc = upload_tiled(s, traj, s->st.traj[0], B, n, 18))) return rc;
  if ((rc = launch_linearize(s, B, n, 0, 0))) return rc;
  launch(s, K_OTHER, k_init, dim3(cdiv(B, 64)), dim3(64), s->params, s->st, (int)B, (int)n);
  if ((rc = launch_backward(s, B, n, 1))) return rc;
  if ((rc = download_tiled(s, gains, s->st.gains, s->st.gains, nullptr, 0, B, n, 52))) return rc;
  HIP_TRY(hipMemcpyAsync(terms, s->st.terms, sizeof(double) * 2 * B, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipGetLastError());
  return device_error(s);
}

int qilqr_forward_sim(qilqr_solver *s, const double *traj, const double *gains, const double *alpha, int32_t B,
                      int32_t n, double *out_traj) {
  if (!s || !traj || !gains || !alpha || !out_traj) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  int rc = begin_batch(s, B, n, nullptr, E_SIM);
  if (rc) return rc;
  if ((rc = upload_tiled(s, traj, s->st.traj[0], B, n, 18))) return rc;
  if ((rc = upload_tiled(s, gains, s->st.gains, B, n, 52))) return rc;
  HIP_TRY(hipMemcpyAsync(s->st.alpha, alpha, sizeof(double) * B, hipMemcpyHostToDevice, s->stream));
  if ((rc = launch_rollout(s, B, n, 0))) return rc;
  if ((rc = download_tiled(s, out_traj, s->st.traj[1], s->st.traj[1], nullptr, 0, B, n, 18))) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipGetLastError());
  return device_error(s);
}

int qilqr_line_search(qilqr_solver *s, const double *traj, const double *cost, const double *gains,
                      const double *terms, int32_t B, int32_t n, double *out_traj, double *out_cost,
                      double *out_step, int32_t *out_status) {
  if (!s || !traj || !cost || !gains || !terms) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  int rc = begin_batch(s, B, n, nullptr, E_PASS);
  if (rc) return rc;
  struct Scratch {  // freed on every return path
    double *cost = nullptr, *terms = nullptr;
    ~Scratch() {
      if (cost) (void)hipFree(cost);
      if (terms) (void)hipFree(terms);
    }
  } scratch;
  HIP_TRY(hipMalloc((void **)&scratch.cost, sizeof(double) * B));
  HIP_TRY(hipMalloc((void **)&scratch.terms, sizeof(double) * 2 * B));
  double *const d_cost = scratch.cost, *const d_terms = scratch.terms;
  if ((rc = upload_tiled(s, traj, s->st.traj[0], B, n, 18))) return rc;
  if ((rc = upload_tiled(s, gains, s->st.gains, B, n, 52))) return rc;
  HIP_TRY(hipMemcpyAsync(d_cost, cost, sizeof(double) * B, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_terms, terms, sizeof(double) * 2 * B, hipMemcpyHostToDevice, s->stream));
  launch(s, K_OTHER, k_seed_search, dim3(cdiv(B, 64)), dim3(64), s->st, (int)B, d_cost, d_terms);
  if (s->params.ls_max_iters <= 0) {
    // ilqr.hh:178: the loop body never runs, the reference throws at once
    std::vector<int> st3(B, QILQR_STATUS_LINE_SEARCH_FAILED);
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (out_status) std::memcpy(out_status, st3.data(), sizeof(int) * B);
    return QILQR_OK;
  }
  for (int t = 0; t < s->params.ls_max_iters; ++t) {
    HIP_TRY(hipMemsetAsync(s->st.counters, 0, sizeof(int) * COUNT_WORDS, s->stream));
    if ((rc = launch_rollout(s, B, n, F_SEARCH))) return rc;
    if ((rc = launch_linearize(s, B, n, 1, F_SEARCH))) return rc;
    if ((rc = launch_accept(s, B, n, 1))) return rc;
    int n_active = 0;
    if ((rc = read_active(s, &n_active))) return rc;
    if (n_active == 0) break;
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  // results: accepted candidates are traj[cur] (cur flipped); failures keep the input
  std::vector<int> status(B);
  HIP_TRY(hipMemcpy(status.data(), s->st.status, sizeof(int) * B, hipMemcpyDeviceToHost));
  if (out_status) std::memcpy(out_status, status.data(), sizeof(int) * B);
  if (out_cost) HIP_TRY(hipMemcpy(out_cost, s->st.cost, sizeof(double) * B, hipMemcpyDeviceToHost));
  if (out_step) HIP_TRY(hipMemcpy(out_step, s->st.alpha, sizeof(double) * B, hipMemcpyDeviceToHost));
  if (out_traj && (rc = download_tiled(s, out_traj, s->st.traj[0], s->st.traj[1], s->st.cur, 0, B, n, 18))) return rc;
  HIP_TRY(hipGetLastError());
  return device_error(s);
}

// ---- the step between two solves of a receding horizon: k_shift (shift_kernels.h, compiled by shift.hip) on the caller's arrays
namespace {
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
  if (((uintptr_t)traj | (uintptr_t)out | (uintptr_t)x0) & 15) return fail(QILQR_ERR_INVALID_ARG, "shift: every array must be 16-byte aligned");
  // the copy is parallel and every block reads only the input: an output that overlaps an input is a race
  const char *i0 = (const char *)traj, *o0 = (const char *)out, *x = (const char *)x0;
  const size_t tb = sizeof(double) * 18 * (size_t)B * n, xb = sizeof(double) * QILQR_STATE * (size_t)B;
  if (i0 < o0 + tb && o0 < i0 + tb) return fail(QILQR_ERR_INVALID_ARG, "shift: the output overlaps the input (the shift does not work in place)");
  if (x && x < o0 + tb && o0 < x + xb) return fail(QILQR_ERR_INVALID_ARG, "shift: the output overlaps x0");
  return QILQR_OK;
}
int shift_enqueue(qilqr_solver *s, const double *d_traj, const double *d_x0, int32_t B, int32_t n, int32_t steps, int32_t tail, double *d_out) {
  const ShiftLaunch call{d_traj, d_x0, d_out, B, n, steps, tail, s->integrator, s->limited ? &s->limits : nullptr, s->modeled ? s->d_models : nullptr};
  const hipError_t e = launch_shift(s->stream, s->consts, call);
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("k_shift: ") + hipGetErrorString(e));
  return QILQR_OK;
}
}  // namespace

static_assert(QILQR_STATE == 13 && QILQR_TAIL_HOLD == 0 && QILQR_TAIL_HOVER == 1, "shift_kernels.h and the C header agree on the state words and the tails");
int qilqr_shift_batch_device(qilqr_solver *s, const double *d_traj, const double *d_x0, int32_t B, int32_t n, int32_t steps, int32_t tail,
                             double *d_out) {
  int rc = shift_refuse(s, d_traj, d_x0, B, n, steps, tail, d_out);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return shift_enqueue(s, d_traj, d_x0, B, n, steps, tail, d_out);  // (enqueued on the handle's stream; not waited for)
}

int qilqr_shift_batch(qilqr_solver *s, const double *traj, const double *x0, int32_t B, int32_t n, int32_t steps, int32_t tail, double *out) {
  int rc = shift_refuse(s, traj, x0, B, n, steps, tail, out);
  if (rc) return rc;
  if (x0)  // as the initial trajectories are checked (manif's constructor check), naming the problem
    for (long b = 0; b < B; ++b) {
      const double *q = x0 + b * QILQR_STATE + 3;
      const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      if (!(std::fabs(nn - 1.0) <= 1e-10)) return fail(QILQR_ERR_BAD_QUATERNION, "x0: quaternion not normalized at problem " + std::to_string(b));
    }
  HIP_TRY(hipSetDevice(s->device));
  struct Scratch {  // freed on every return path
    double *p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } scratch;
  const size_t cnt = 18 * (size_t)B * n, xcnt = (size_t)QILQR_STATE * B;  // (cnt is even: input, output and x0 each start on 16 bytes)
  HIP_TRY(hipMalloc((void **)&scratch.p, sizeof(double) * (2 * cnt + xcnt)));
  double *d_in = scratch.p, *d_out = d_in + cnt, *d_x0 = x0 ? d_out + cnt : nullptr;
  HIP_TRY(hipMemcpyAsync(d_in, traj, sizeof(double) * cnt, hipMemcpyHostToDevice, s->stream));
  if (x0) HIP_TRY(hipMemcpyAsync(d_x0, x0, sizeof(double) * QILQR_STATE * (size_t)B, hipMemcpyHostToDevice, s->stream));
  hipError_t e = hipSuccess;
  if ((rc = shift_enqueue(s, d_in, d_x0, B, n, steps, tail, d_out)) == QILQR_OK)
    e = hipMemcpyAsync(out, d_out, sizeof(double) * cnt, hipMemcpyDeviceToHost, s->stream);
  const hipError_t drained = hipStreamSynchronize(s->stream);  // (the copies read and write the caller's arrays, the kernel the scratch: finished before either goes)
  if (rc) return rc;
  if (e == hipSuccess) e = drained;
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("qilqr_shift_batch: ") + hipGetErrorString(e));
  return QILQR_OK;
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

// ---- the plan's feedback law flown from given states: k_closed_loop (closed_loop_kernels.h, compiled by closed_loop.hip) on the caller's arrays
namespace {
// what both forms refuse (closed_loop_launch.h: the rule, from facts alone; the pointers are the caller's, host or device ones)
int closed_loop_refuse(const qilqr_solver *s, const double *plan, const double *gains, const double *x0, int32_t B, int32_t n, int32_t S,
                       int32_t i0, int32_t i1, const double *out_traj, const double *out_stats) {
  const ClosedLoopCall call{plan, gains, x0, out_traj, out_stats, B, n, S, i0, i1, s != nullptr, s && s->f32, s && s->modeled, s ? s->models_B : 0};
  const char *why = closed_loop_refusal(call);
  if (!why) return QILQR_OK;
  std::string text = why;
  if (s && s->modeled && !s->f32 && s->models_B != (long)B * S)
    text += ": they were set for " + std::to_string(s->models_B) + ", this call has B * S = " + std::to_string((long)B * S);
  return fail(QILQR_ERR_INVALID_ARG, text);
}
int closed_loop_enqueue(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, int32_t B, int32_t n, int32_t S,
                        int32_t i0, int32_t i1, double *d_out_traj, double *d_out_stats) {
  const ClosedLoopLaunch call{d_plan, d_gains, d_x0, d_out_traj, d_out_stats, B, n, S, i0, i1, s->integrator, s->limited ? &s->limits : nullptr,
                              s->modeled ? s->d_models : nullptr};
  const hipError_t e = launch_closed_loop(s->stream, s->consts, call);
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("k_closed_loop: ") + hipGetErrorString(e));
  return QILQR_OK;
}
}  // namespace

static_assert(QILQR_CL_STATS == 4, "closed_loop_kernels.h and the C header agree on the words of a sample's statistics");
int qilqr_closed_loop_device(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, int32_t B, int32_t n, int32_t S,
                             int32_t i0, int32_t i1, double *d_out_traj, double *d_out_stats) {
  int rc = closed_loop_refuse(s, d_plan, d_gains, d_x0, B, n, S, i0, i1, d_out_traj, d_out_stats);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return closed_loop_enqueue(s, d_plan, d_gains, d_x0, B, n, S, i0, i1, d_out_traj, d_out_stats);  // (enqueued on the handle's stream; not waited for)
}

int qilqr_closed_loop(qilqr_solver *s, const double *plan, const double *gains, const double *x0, int32_t B, int32_t n, int32_t S, int32_t i0,
                      int32_t i1, double *out_traj, double *out_stats) {
  int rc = closed_loop_refuse(s, plan, gains, x0, B, n, S, i0, i1, out_traj, out_stats);
  if (rc) return rc;
  for (long r = 0; r < (long)B * S; ++r) {  // as the initial trajectories are checked (manif's constructor check), naming the sample
    const double *q = x0 + r * QILQR_STATE + 3;
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(std::fabs(nn - 1.0) <= 1e-10))
      return fail(QILQR_ERR_BAD_QUATERNION, "x0: quaternion not normalized at problem " + std::to_string(r / S) + ", sample " + std::to_string(r % S));
  }
  HIP_TRY(hipSetDevice(s->device));
  struct Scratch {  // freed on every return path
    double *p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } scratch;
  // (every count but x0's is even, and x0 goes last: each array starts on 16 bytes)
  const size_t samples = (size_t)B * S, pc = 18 * (size_t)B * n, gc = 52 * (size_t)B * n, xc = (size_t)QILQR_STATE * samples;
  const size_t tc = out_traj ? 18 * samples * n : 0, sc = out_stats ? QILQR_CL_STATS * samples : 0;
  HIP_TRY(hipMalloc((void **)&scratch.p, sizeof(double) * (pc + gc + tc + sc + xc)));
  double *d_plan = scratch.p, *d_gains = d_plan + pc, *d_traj = d_gains + gc, *d_stats = d_traj + tc, *d_x0 = d_stats + sc;
  HIP_TRY(hipMemcpyAsync(d_plan, plan, sizeof(double) * pc, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_gains, gains, sizeof(double) * gc, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipMemcpyAsync(d_x0, x0, sizeof(double) * xc, hipMemcpyHostToDevice, s->stream));
  hipError_t e = hipSuccess;
  if ((rc = closed_loop_enqueue(s, d_plan, d_gains, d_x0, B, n, S, i0, i1, out_traj ? d_traj : nullptr, out_stats ? d_stats : nullptr)) == QILQR_OK) {
    // knots i0 .. i1 of every sample, and nothing else of the caller's array: rows of (i1 - i0 + 1) knots at a pitch of n knots
    const size_t pitch = sizeof(double) * 18 * (size_t)n, off = 18 * (size_t)i0;
    if (out_traj)
      e = hipMemcpy2DAsync(out_traj + off, pitch, d_traj + off, pitch, sizeof(double) * 18 * (size_t)(i1 - i0 + 1), samples, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_stats) e = hipMemcpyAsync(out_stats, d_stats, sizeof(double) * sc, hipMemcpyDeviceToHost, s->stream);
  }
  const hipError_t drained = hipStreamSynchronize(s->stream);  // (the copies read and write the caller's arrays, the kernel the scratch: finished before either goes)
  if (rc) return rc;
  if (e == hipSuccess) e = drained;
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("qilqr_closed_loop: ") + hipGetErrorString(e));
  return QILQR_OK;
}

// ---- the scored flight: k_closed_loop_scored (closed_loop_scored_kernels.h, compiled by closed_loop_scored.hip) on the caller's arrays
namespace {
// what both forms refuse (closed_loop_launch.h: closed_loop_scored_refusal; the pointers are the caller's, host or device ones)
int closed_loop_scored_refuse(const qilqr_solver *s, const double *plan, const double *gains, const double *x0, const double *wrench, int32_t n_w,
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
int closed_loop_scored_enqueue(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, const double *d_wrench, int32_t n_w,
                               const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, double *d_out_traj, double *d_out_stats,
                               double *d_out_score) {
  ClosedLoopScoredLaunch call{};
  call.base = ClosedLoopLaunch{d_plan, d_gains, d_x0, d_out_traj, d_out_stats, B, n, S, i0, i1, s->integrator, s->limited ? &s->limits : nullptr,
                              s->modeled ? s->d_models : nullptr};
  call.d_wrench = d_wrench;
  call.n_w = n_w;
  call.d_out_score = d_out_score;
  if (d_out_score) {
    call.d_desired = d_desired ? d_desired : (const double *)s->d_desired + 18 * (size_t)s->k0;
    call.desired_step = d_desired ? 18l * n : 0;
    if (s->n_sched > 0) {
      call.d_q = s->d_qsched + (size_t)SCHED_WORDS * s->k0;
      call.q_step = SCHED_WORDS;
    } else {
      if (!s->d_cl_q) {  // (Q lies 8 bytes off a 16-byte boundary inside ModelConsts: a copy of its own, made once; the handle's Q never changes)
        HIP_TRY(hipMalloc((void **)&s->d_cl_q, sizeof(double) * 144));
        HIP_TRY(hipMemcpyAsync(s->d_cl_q, s->consts.Q, sizeof(double) * 144, hipMemcpyHostToDevice, s->stream));
      }
      call.d_q = s->d_cl_q;
      call.q_step = 0;
    }
    call.d_shared = s->n_obstacles > 0 ? s->d_obstacles : nullptr;
    call.n_shared = s->n_obstacles;
    call.d_own = s->pobs_B > 0 ? s->d_pobs : nullptr;
    call.d_own_counts = s->pobs_B > 0 ? s->d_pobs_counts : nullptr;
    call.own_K = s->pobs_K;
  }
  const hipError_t e = launch_closed_loop_scored(s->stream, s->consts, call);
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("k_closed_loop_scored: ") + hipGetErrorString(e));
  return QILQR_OK;
}
}  // namespace

static_assert(QILQR_CL_SCORE == 4 && QILQR_WRENCH == 6, "closed_loop_kernels.h and the C header agree on the words of a score and of a wrench");
int qilqr_closed_loop_scored_device(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, const double *d_wrench,
                                    int32_t n_w, const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1,
                                    double *d_out_traj, double *d_out_stats, double *d_out_score) {
  int rc = closed_loop_scored_refuse(s, d_plan, d_gains, d_x0, d_wrench, n_w, d_desired, B, n, S, i0, i1, d_out_traj, d_out_stats, d_out_score);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return closed_loop_scored_enqueue(s, d_plan, d_gains, d_x0, d_wrench, n_w, d_desired, B, n, S, i0, i1, d_out_traj, d_out_stats, d_out_score);  // (not waited for)
}

int qilqr_closed_loop_scored(qilqr_solver *s, const double *plan, const double *gains, const double *x0, const double *wrench, int32_t n_w,
                             const double *desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1, double *out_traj, double *out_stats,
                             double *out_score) {
  int rc = closed_loop_scored_refuse(s, plan, gains, x0, wrench, n_w, desired, B, n, S, i0, i1, out_traj, out_stats, out_score);
  if (rc) return rc;
  for (long r = 0; r < (long)B * S; ++r) {  // as qilqr_closed_loop checks them
    const double *q = x0 + r * QILQR_STATE + 3;
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(std::fabs(nn - 1.0) <= 1e-10))
      return fail(QILQR_ERR_BAD_QUATERNION, "x0: quaternion not normalized at problem " + std::to_string(r / S) + ", sample " + std::to_string(r % S));
  }
  if (wrench)
    for (long r = 0; r < (long)B * S; ++r)
      for (long k = 0; k < n_w; ++k)
        for (int w = 0; w < QILQR_WRENCH; ++w)
          if (!std::isfinite(wrench[(r * n_w + k) * QILQR_WRENCH + w]))
            return fail(QILQR_ERR_INVALID_ARG, "wrench: a non-finite value at problem " + std::to_string(r / S) + ", sample " + std::to_string(r % S) + ", knot " +
                                                   std::to_string(k));
  HIP_TRY(hipSetDevice(s->device));
  struct Scratch {  // freed on every return path
    double *p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } scratch;
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
  hipError_t e = hipSuccess;
  if ((rc = closed_loop_scored_enqueue(s, d_plan, d_gains, d_x0, wrench ? d_wrench : nullptr, n_w, desired ? d_desired : nullptr, B, n, S, i0, i1,
                                       out_traj ? d_traj : nullptr, out_stats ? d_stats : nullptr, out_score ? d_score : nullptr)) == QILQR_OK) {
    const size_t pitch = sizeof(double) * 18 * (size_t)n, off = 18 * (size_t)i0;
    if (out_traj)
      e = hipMemcpy2DAsync(out_traj + off, pitch, d_traj + off, pitch, sizeof(double) * 18 * (size_t)(i1 - i0 + 1), samples, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_stats) e = hipMemcpyAsync(out_stats, d_stats, sizeof(double) * sc, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && out_score) e = hipMemcpyAsync(out_score, d_score, sizeof(double) * oc, hipMemcpyDeviceToHost, s->stream);
  }
  const hipError_t drained = hipStreamSynchronize(s->stream);  // (the copies read and write the caller's arrays, the kernel the scratch: finished before either goes)
  if (rc) return rc;
  if (e == hipSuccess) e = drained;
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("qilqr_closed_loop_scored: ") + hipGetErrorString(e));
  return QILQR_OK;
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
  HIP_TRY(hipSetDevice(s->device));
  SampleGustsLaunch go{d_wrench, B, S, n_w, b0, s0, seed, s->consts.dt, {}, {}, m->tau_force_s, m->tau_torque_s};
  for (int k = 0; k < 6; ++k) {
    go.mean[k] = m->mean[k];
    go.sigma[k] = m->sigma[k];
  }
  const hipError_t e = launch_sample_gusts(s->stream, go);  // (enqueued on the handle's stream; not waited for)
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("k_sample_gusts: ") + hipGetErrorString(e));
  return QILQR_OK;
}

int qilqr_sample_states_device(qilqr_solver *s, const double *d_x_nom, const double *sigma12, uint64_t seed, int32_t B, int32_t S, int32_t b0,
                               int32_t s0, uint32_t flags, double *d_x0) {
  SampleStatesCall call{s != nullptr, sigma12 != nullptr, d_x_nom, d_x0, B, S, b0, s0, flags, {}};
  for (int k = 0; k < 12; ++k) call.sigma[k] = sigma12 ? sigma12[k] : 0.0;
  if (const char *why = sample_states_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  HIP_TRY(hipSetDevice(s->device));
  SampleStatesLaunch go{d_x_nom, d_x0, B, S, b0, s0, flags, seed, {}};
  for (int k = 0; k < 12; ++k) go.sigma[k] = sigma12[k];
  const hipError_t e = launch_sample_states(s->stream, go);  // (not waited for)
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("k_sample_states: ") + hipGetErrorString(e));
  return QILQR_OK;
}

int qilqr_reduce_scores_device(qilqr_solver *s, const double *d_score, int32_t B, int32_t S, double *d_summary) {
  const ReduceScoresCall call{s != nullptr, d_score, d_summary, B, S};
  if (const char *why = reduce_scores_refusal(call)) return fail(QILQR_ERR_INVALID_ARG, why);
  HIP_TRY(hipSetDevice(s->device));
  const hipError_t e = launch_reduce_scores(s->stream, ReduceScoresLaunch{d_score, d_summary, B, S});  // (not waited for)
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("k_reduce_scores: ") + hipGetErrorString(e));
  return QILQR_OK;
}
}  // extern "C"
