// host/api_calls.h -- the C ABI of the computing calls on one handle's workspace: the batch solves, qilqr_solve, the four stand-alone passes
// and the pinned host memory for their callers.  (The calls on the caller's own arrays are host/caller_arrays.h's.)  Part of ilqr_capi.hip's
// translation unit.
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
  DeviceScratch scratch_cost, scratch_terms;
  HIP_TRY(hipMalloc((void **)&scratch_cost.p, sizeof(double) * B));
  HIP_TRY(hipMalloc((void **)&scratch_terms.p, sizeof(double) * 2 * B));
  double *const d_cost = scratch_cost.p, *const d_terms = scratch_terms.p;
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
}  // extern "C"
