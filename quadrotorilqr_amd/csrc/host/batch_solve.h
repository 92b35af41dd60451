// host/batch_solve.h -- the host loops of a solve: the rounds on one stream (run_solve) with the copy-back of the finished trajectories
// under the tail, the rounds of sub-batches on their own streams (run_solve_parts), and the device-resident and the staged host-buffer
// batch solve built from them.  Part of ilqr_capi.hip's translation unit.
#pragma once

namespace {
// Batch solves in flight on a device, over all the handles of the process.  The combined kernel takes a whole CU per block of
// four trajectories (the rollout's register budget): alone on the chip that is +3 to +4 % of a solve, beside other solves'
// kernels it is in their way -- three handles in flight: 306 000-311 000 solves/s with it, 340 000 without.  A solve that
// finds another one in flight on its device therefore launches the two kernels apart (same bits either way).
// The choice is made again for every round a solve enqueues (a solve that is joined by another one changes over at its next round;
// the count covers the window in which a solve's host loop enqueues rounds -- the last `sync_every` rounds of a call that
// returns before its stream has drained are outside it).
constexpr int MAX_TRACKED_DEVICES = 64;  // (HIP ordinals of one process; a node has 8)
std::atomic<int> g_solves_in_flight[MAX_TRACKED_DEVICES];
struct InFlight {
  std::atomic<int> &n;
  explicit InFlight(int device) : n(g_solves_in_flight[(unsigned)device % MAX_TRACKED_DEVICES]) { n.fetch_add(1, std::memory_order_relaxed); }
  ~InFlight() { n.fetch_sub(1, std::memory_order_relaxed); }
  // (always: qilqr_device_config.fuse_in_flight = 1 keeps the combined launches beside other solves -- diagnostic)
  bool alone(bool always = false) const { return always || n.load(std::memory_order_relaxed) == 1; }
};

// The count of running trajectories that the launches of round `old` hand to the host (the word's high half is the round's tag): a bounded
// wait on `stream`, which never spins on a dead stream -- a drained or failed stream without the tag is an error.
int wait_for_count(const unsigned long long *word, hipStream_t stream, long old, unsigned long long *v) {
  const unsigned tag = (unsigned)((old & 0x3fffffff) + 1);
  for (long spins = 0;; ++spins) {
    *v = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if ((unsigned)(*v >> 32) == tag) return QILQR_OK;
    if ((spins & 1023) == 1023) {
      const hipError_t q = hipStreamQuery(stream);
      if (q != hipErrorNotReady) {
        *v = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        if ((unsigned)(*v >> 32) == tag) return QILQR_OK;
        return fail(QILQR_ERR_HIP, std::string("a round never reported its active count: ") + hipGetErrorString(q));
      }
    }
    __builtin_ia32_pause();
  }
}

int read_active(qilqr_solver *s, int *n_active) {
  HIP_TRY(hipMemcpyAsync(s->h_counters, s->st.counters + COUNT_BASE, sizeof(int) * COUNT_STRIPES, hipMemcpyDeviceToHost,
                         s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  int total = 0;
  for (int k = 0; k < COUNT_STRIPES; ++k) total += s->h_counters[k];
  *n_active = total;
  return QILQR_OK;
}

// ---- host-buffer batch solve: the copy-back under the tail of the solve.
// A batch takes as long as its slowest problem (configs[1]: 33 rounds for a mean of 12.5 iterations), and for the last third of
// the rounds nine trajectories in ten already have their exit status while the copy engines sit idle.  When the host sees
// the count of running trajectories fall to B / 8, it marks the finished ones between two rounds (k_mark_final, on the
// solver's stream), and a second stream gathers exactly those and copies the result arrays to the caller's (pinned) host
// buffers while the rounds of the others go on.  After the last round the late finishers -- at most B / 8 -- are gathered into
// a small compact block, copied, and put into their rows by the host.  The caller's arrays end up bit-identical to the
// one-piece copy.
int g_force_staged_late = 0;  // (diagnostics build: qilqr_debug_set_staged_late)
struct EarlyOut {
  double *h_traj, *h_cost;
  int32_t *h_status, *h_iters, *h_bwd, *h_fwd;
  // the same arrays as the DEVICE addresses them (pinned host memory is mapped: hipHostGetDevicePointer), when every one resolves: the late
  // finishers' rows are then written by k_gather straight into the caller's arrays over the link (round 6) -- no compact block, no second
  // copy, no scatter by the host
  bool direct = false;
  double *v_traj = nullptr, *v_cost = nullptr;
  int32_t *v_status = nullptr, *v_iters = nullptr, *v_bwd = nullptr, *v_fwd = nullptr;
  unsigned threshold = 0;  // fire when the active count is at or below this (and not zero)
  bool fired = false;
  int late_cap = 0;        // rows of the compact block: the active count seen when firing (the count only falls)
  struct LateLayout *layout = nullptr;
};
struct LateLayout {  // one block, device and host alike: [traj rows][cost][status | iters | n_bwd | n_fwd][idx][count]
  size_t traj, cost, ints, idx, count, bytes;
};
inline LateLayout late_layout(long rows, long n) {
  LateLayout L;
  L.traj = 0;
  L.cost = sizeof(double) * (size_t)rows * n * 18;
  L.ints = L.cost + sizeof(double) * rows;
  L.idx = L.ints + sizeof(int) * 4 * rows;
  L.count = L.idx + sizeof(int) * rows;
  L.bytes = L.count + sizeof(int) * 2;
  return L;
}
int ensure_early_buffers(qilqr_solver *s, long B, long n, long rows) {
  if (!s->early_stream) HIP_TRY(hipStreamCreateWithFlags(&s->early_stream, hipStreamNonBlocking));
  if (!s->early_evt) HIP_TRY(hipEventCreateWithFlags(&s->early_evt, hipEventDisableTiming));
  if (!s->early_done) HIP_TRY(hipEventCreateWithFlags(&s->early_done, hipEventDisableTiming));
  if ((size_t)B > s->early_cap) {
    if (s->d_early) (void)hipFree(s->d_early);
    s->d_early = nullptr;
    s->early_cap = 0;
    HIP_TRY(hipMalloc((void **)&s->d_early, sizeof(int) * 2 * (size_t)B));
    s->early_cap = (size_t)B;
  }
  const size_t want = late_layout(rows, n).bytes;
  if (want > s->late_bytes) {
    if (s->d_late) (void)hipFree(s->d_late);
    if (s->h_late) (void)hipHostFree(s->h_late);
    s->d_late = s->h_late = nullptr;
    s->late_bytes = 0;
    HIP_TRY(hipMalloc((void **)&s->d_late, want));
    HIP_TRY(hipHostMalloc((void **)&s->h_late, want, hipHostMallocDefault));
    s->late_bytes = want;
  }
  return QILQR_OK;
}

// called from the polling loop of run_solve when the count has fallen to the threshold
int fire_early_out(qilqr_solver *s, long B, long n, EarlyOut *eo, unsigned active) {
  eo->fired = true;
  eo->late_cap = (int)active;
  *eo->layout = late_layout((long)active, n);
  int *early = s->d_early, *late_count = (int *)(s->d_late + eo->layout->count);
  launch(s, K_OTHER, k_mark_final, dim3(cdiv(B, 256)), dim3(256), s->st, (int)B, early, late_count);
  HIP_TRY(hipEventRecord(s->early_evt, s->stream));
  HIP_TRY(hipStreamWaitEvent(s->early_stream, s->early_evt, 0));
  hipStream_t main_stream = s->stream;
  s->stream = s->early_stream;  // (launch() goes to s->stream)
  int *d_int = s->stage_int;
  const int rc = gather(s, B, n, eo->h_traj ? s->stage_traj : nullptr, eo->h_cost ? s->stage_cost : nullptr, eo->h_status ? d_int : nullptr,
                        eo->h_iters ? d_int + B : nullptr, eo->h_bwd ? d_int + 2 * B : nullptr, eo->h_fwd ? d_int + 3 * B : nullptr, early, 1,
                        nullptr);
  s->stream = main_stream;
  if (rc) return rc;
  hipStream_t es = s->early_stream;
  if (eo->h_traj) HIP_TRY(hipMemcpyAsync(eo->h_traj, s->stage_traj, sizeof(double) * 18 * (size_t)B * n, hipMemcpyDeviceToHost, es));
  if (eo->h_cost) HIP_TRY(hipMemcpyAsync(eo->h_cost, s->stage_cost, sizeof(double) * B, hipMemcpyDeviceToHost, es));
  if (eo->h_status) HIP_TRY(hipMemcpyAsync(eo->h_status, d_int, sizeof(int) * B, hipMemcpyDeviceToHost, es));
  if (eo->h_iters) HIP_TRY(hipMemcpyAsync(eo->h_iters, d_int + B, sizeof(int) * B, hipMemcpyDeviceToHost, es));
  if (eo->h_bwd) HIP_TRY(hipMemcpyAsync(eo->h_bwd, d_int + 2 * B, sizeof(int) * B, hipMemcpyDeviceToHost, es));
  if (eo->h_fwd) HIP_TRY(hipMemcpyAsync(eo->h_fwd, d_int + 3 * B, sizeof(int) * B, hipMemcpyDeviceToHost, es));
  HIP_TRY(hipEventRecord(s->early_done, es));
  return QILQR_OK;
}

// The outer loop of ILQR::solve (ilqr.hh:53-87) for trajectories already in st.traj[0].
// on_round is called behind every round's backward pass (and rollout), in both modes: debug capture enqueues its kernel there.
// drain = false: return as soon as the host knows that no trajectory is active; the caller enqueues
// its own work behind the rounds still in flight and waits for the stream itself.
// on_count (optional): called with the count of running trajectories each time the free-running loop learns one.
// double_ok: the caller does not look at the solve round by round (on_round does nothing): launches may hold two rounds
template <typename F>
int run_solve(qilqr_solver *s, long B, long n, int sync_every, F on_round, bool drain = true,
              const std::function<int(unsigned)> *on_count = nullptr, bool double_ok = false) {
  int rc;
  s->round_captured = false;
  if ((rc = launch_linearize(s, B, n, 0, 0))) return rc;
  {
    launch(s, K_OTHER, k_init, dim3(cdiv(B, 64)), dim3(64), s->params, s->st, (int)B, (int)n);
  }
  if (!(0.0 < s->params.max_iters)) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    return QILQR_OK;
  }
  // a trajectory needs at most max_iters backward passes and max_iters * ls_max_iters trials
  const double bound = (std::fmin(s->params.max_iters, 1e7) + 1.0) * ((double)std::max(s->params.ls_max_iters, 1) + 1.0) * (1.0 + max_restarts(s->params));
  const long max_rounds = (long)std::fmin(bound, 2e9);
  const int lag = (sync_every > 1) ? std::min(sync_every, 6) : 0;
  if (lag == 0) {
    // Synchronous rounds (debug capture): the host reads the count after every k_backward.
    for (long round = 0; round < max_rounds; ++round) {
      // k_backward first settles the candidate of the previous round (cost, Armijo, convergence) and
      // counts the trajectories still active; then rollout + linearise the next candidates
      if ((rc = launch_backward(s, B, n, 0))) return rc;
      int active = 0;
      if ((rc = read_active(s, &active))) return rc;
      if ((rc = on_round())) return rc;
      if (active == 0) break;
      if ((rc = launch_rollout(s, B, n, F_SEARCH, round))) return rc;
      if ((rc = launch_linearize(s, B, n, 1, F_SEARCH))) return rc;
    }
  } else {
    // Free-running rounds: three kernels per round and nothing else on the stream.  k_linearize hands
    // the count of still-active trajectories to the host through pinned memory, tagged with its round;
    // the host looks at the count `lag` rounds late, i.e. keeps the stream `lag` rounds ahead of the
    // device, so the GPU never waits for a host round trip.  Rounds enqueued past the end find nothing
    // to do.
    // the counter set of a round's parity (k_round publishes a round's count from the NEXT launch; the other kernels of a round
    // count and publish within it, in the same set)
    struct CounterSet {
      qilqr_solver *s;
      int *base;
      CounterSet(qilqr_solver *s_, long round, bool two) : s(s_), base(s_->st.counters) { if (two) s->st.counters = base + (round & 1) * COUNT_WORDS; }
      ~CounterSet() { s->st.counters = base; }
    };
    for (int k = 0; k < 8; ++k) s->h_active[k] = 0;
    const InFlight in_flight(s->device);
    const bool can_fuse = s->route.combined && !s->compact;  // (compaction works between the two halves)
    const TailFuse tf = tail_fuse(s->route, s->compact, 1);
    if (s->compact) s->plan_heads.push_back(0);
    unsigned seen_active = (unsigned)B;  // the last count the host has read (the count only falls)
    long used = B;                       // slots the round's kernels are launched over (slots_in_use)
    bool pending_publish = false;        // the round before was a k_round: the next launch publishes its count
    unsigned launched_rounds[8] = {1, 1, 1, 1, 1, 1, 1, 1};  // rounds in launch `round & 7` (its count is the sum of theirs)
    bool two_sets = false;               // a k_round has run in this solve: rounds count into the counter set of their parity
    bool tail_started = false;           // a compacted batch has changed over to the combined launch for the rest of the solve
    for (long round = 0; round < max_rounds; ++round) {
      const RoctxRange range(s, "round", round);
      // (one more compaction behind the last count above the threshold brings the slots in use under it)
      // (once the compaction has stopped for a batch that changes over to the combined launch it stays stopped: the launches may then hold
      // several rounds, and the sums of counts they report say nothing against the threshold)
      const bool compacting = s->compact && !tail_started && (seen_active > tf.stop || (tf.kinds && used > tf.slots));
      if (s->compact && tf.kinds && !compacting && used <= tf.slots && round >= tf.from) tail_started = true;
      s->live_hint = (long)seen_active;
      const bool fuse_now = (can_fuse || tail_started) && in_flight.alone(s->dev.fuse_in_flight == 1);
      // (until round 6 k_round linearised a block's candidates AFTER the rollout, 2.5 times slower than k_linearize with four candidates per
      // block and idle CUs beside it, and B = 64 ... 512 took k_backward_rollout + k_linearize in their first rounds; with the linearisation
      // behind the rollout -- round_follow -- k_round is ahead at every size: B = 64 + 2.1 %, 128 + 2.3 %, 256 + 3 %, 512 + 3.6 %)
      if (fuse_now && s->route.round_kernel) {
        // several rounds per launch where the rounds are this kernel for the rest of the solve (no compaction any more, whose
        // thresholds go by the count) and the caller does not look at a solve round by round (the single solve's debug capture)
        const RoundForm f = round_form(s->route, (can_fuse || tail_started) && double_ok, /*forced=*/true, seen_active, used);
        if ((rc = launch_round(s, used, n, round, pending_publish, f.rounds, f.six))) return rc;
        s->round_captured = true;
        launched_rounds[round & 7] = f.rounds;
        pending_publish = true;
        two_sets = true;
        if ((rc = on_round())) return rc;
        goto round_enqueued;
      }
      if (pending_publish) {  // the round before was a k_round: its count has no launch left to publish it
        launch(s, K_OTHER, k_publish_active, dim3(1), dim3(64), s->st.counters + ((round + 1) & 1) * COUNT_WORDS, s->st.host_active,
               (int)((round - 1) & 0x3fffffff));
        pending_publish = false;
      }
      launched_rounds[round & 7] = 1;
      s->round_captured = false;
      {
      const CounterSet counter_set(s, round, two_sets);
      if (fuse_now) {
        if ((rc = launch_backward_rollout(s, used, n))) return rc;
      } else {
        if ((rc = launch_backward(s, used, n, 0))) return rc;
        if (compacting) {
          if ((rc = launch_compact(s, used, n))) return rc;
          used = slots_in_use(used, seen_active);
        }
        if ((rc = launch_rollout(s, used, n, F_SEARCH, round))) return rc;
      }
      if ((rc = on_round())) return rc;  // (debug capture of the single solve: one more launch, nothing waited for)
      if ((rc = launch_linearize(s, used, n, 1, F_SEARCH, (int)(round & 0x3fffffff)))) return rc;
      }
    round_enqueued:
      // (following launches of several rounds ONE launch back instead of two -- four rounds that find nothing to do at the end of a solve
      // instead of eight -- measured no different: 4.71-4.73 ms either way)
      if (round >= lag) {
        const long old = round - lag;
        unsigned long long v;
        if ((rc = wait_for_count(&s->h_active[old & 7], s->stream, old, &v))) return rc;
        if ((unsigned)v == 0) break;
        // a launch of several rounds reports the SUM of their counts; counts only fall, so the mean over the launch's rounds is an upper
        // bound of the last round's -- of the count now
        const unsigned now_at_most = ((unsigned)v + launched_rounds[old & 7] - 1) / launched_rounds[old & 7];
        seen_active = now_at_most;
        // a block that gave up a hand-off (BatchState::host_error) voids the call: stop enqueuing rounds on void gains -- each
        // could burn a full bounded spin -- let what is in flight finish, and report
        if (__atomic_load_n(s->h_active + 8 * (1 + qilqr_solver::MAX_PARTS), __ATOMIC_ACQUIRE)) {
          (void)hipStreamSynchronize(s->stream);
          if (s->early_stream) (void)hipStreamSynchronize(s->early_stream);
          return device_error(s);
        }
        if (on_count && (rc = (*on_count)(now_at_most))) return rc;
        // (Round 3 tried following the device ONE round behind in the tail, where a round takes well over 100 us and the host
        // needs about 15 to enqueue the next: one round of three empty launches fewer after the last trajectory has finished --
        // 36 rounds instead of 37 -- and no measurable difference, 5.223 against 5.221 ms per solve.  `lag` stays fixed.)
      }
    }
  }
  if (drain) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    return device_error(s);
  }
  return QILQR_OK;
}

// ---- sub-batches on their own streams
// The three kernels of a round are bound by three different things (serial latency and the matrix pipe,
// serial latency at a handful of wavefronts, HBM writes), and one stream runs them one after the other.
// A batch is therefore cut into `parts` contiguous ranges of 64-trajectory tiles, each with its own
// stream, counters and host hand-off words, whose rounds run independently: while one part is in its
// rollout another is in its backward pass and a third writes its knot records.  Trajectories are
// independent, so the results are those of the single-stream solve.
struct Part {
  hipStream_t stream;
  BatchState st;  // the solver's workspace seen from the part's first trajectory
  long nb;        // trajectories in the part
  unsigned long long *h_active;
  bool done;
  unsigned seen_active;  // the last count of running trajectories the host has read
  long used;             // slots its kernels are launched over (slots_in_use)
  bool tail = false;          // the part has changed over to the combined launch for the rest of the solve (tail_fuse)
  bool round_kernel = false;  // ... and from there to k_round, several rounds per launch
  unsigned launched_rounds[8] = {1, 1, 1, 1, 1, 1, 1, 1};  // rounds in launch `round & 7` (its count is the sum of theirs)
};
// the workspace of trajectories [b0, b0 + nb), b0 a multiple of 64
BatchState slice_state(const qilqr_solver *s, long b0, long n, int part) {
  const BatchState &w = s->st;
  BatchState v = w;
  const size_t es = s->f32 ? sizeof(float) : sizeof(double);
  auto adv = [&](const void *p, long elems) { return (void *)((char *)p + (size_t)elems * es); };
  for (int k = 0; k < 2; ++k) {
    v.traj[k] = adv(w.traj[k], knot_base<true>(b0, n, 18));
    v.lin[k] = adv(w.lin[k], rec_base(w.layout, b0, n));  // (b0 is a multiple of 64: the same offset in either placement)
    v.knot_cost[k] = w.knot_cost[k] + cost_index(b0, 0, n);
  }
  v.gains = adv(w.gains, knot_base<true>(b0, n, 52));
  if (w.desired_tiled) v.desired = adv(w.desired, knot_base<true>(b0, n, 18));
  v.cur = w.cur + b0; v.cost = w.cost + b0; v.prev_cost = w.prev_cost + b0; v.terms = w.terms + 2 * b0;
  v.alpha = w.alpha + b0; v.mu = w.mu + b0; v.trial = w.trial + b0; v.flags = w.flags + b0; v.status = w.status + b0;
  v.iters = w.iters + b0; v.n_bwd = w.n_bwd + b0; v.n_fwd = w.n_fwd + b0;
  v.counters = s->d_part_counters + 2 * COUNT_WORDS * part;  // (two sets: k_init zeroes both, k_round alternates)
  v.host_active = s->d_active + 8 * (1 + part);
  if (w.cost_hist) v.cost_hist = w.cost_hist + b0 * w.hist_cap;
  v.dump = adv(w.dump, 4 * b0);
  v.orig = w.orig + b0;
  v.row0 = w.row0 + (int)b0;
  v.plan = w.plan + PLAN_HEAD * (part + 1) + 4 * b0;  // (part p's plan ends where part p + 1's begins)
  if (w.stamps) v.stamps = w.stamps + 8 * b0;
  return v;
}
// launch_* work on s->st / s->stream: point them at a part for the duration of a scope
struct PartScope {
  qilqr_solver *s;
  BatchState st0;
  hipStream_t stream0;
  PartScope(qilqr_solver *s_, const Part &p) : s(s_), st0(s_->st), stream0(s_->stream) {
    s->st = p.st;
    s->stream = p.stream;
  }
  ~PartScope() {
    s->st = st0;
    s->stream = stream0;
  }
};
// streams and completion events of the first nparts sub-batches, created on first use
int ensure_parts(qilqr_solver *s, int nparts) {
  for (int k = 0; k < nparts; ++k) {
    if (!s->part_stream[k]) HIP_TRY(hipStreamCreateWithFlags(&s->part_stream[k], hipStreamNonBlocking));
    if (!s->part_done[k]) HIP_TRY(hipEventCreateWithFlags(&s->part_done[k], hipEventDisableTiming));
  }
  return QILQR_OK;
}
// The outer loop of ILQR::solve for a batch cut into parts (free-running rounds only).  On return the
// main stream waits for every part; the caller enqueues its own work there.
int run_solve_parts(qilqr_solver *s, long B, long n, int nparts) {
  int rc;
  if ((rc = ensure_parts(s, nparts))) return rc;
  const long tiles = (B + 63) / 64;
  std::vector<Part> parts;
  for (int p = 0; p < nparts; ++p) {
    const long t0 = tiles * p / nparts, t1 = tiles * (p + 1) / nparts;
    const long b0 = t0 * 64, b1 = std::min(t1 * 64, B);
    Part part;
    part.stream = s->part_stream[p];
    part.st = slice_state(s, b0, n, p);
    part.nb = b1 - b0;
    part.h_active = s->h_active + 8 * (1 + p);
    part.done = false;
    part.seen_active = (unsigned)part.nb;
    part.used = part.nb;
    if (s->compact) s->plan_heads.push_back(part.st.plan - s->st.plan);
    for (int k = 0; k < 8; ++k) part.h_active[k] = 0;
    parts.push_back(part);
  }
  // the parts start when the main stream has tiled the inputs
  HIP_TRY(hipEventRecord(s->main_ready, s->stream));
  for (auto &part : parts) HIP_TRY(hipStreamWaitEvent(part.stream, s->main_ready, 0));
  for (auto &part : parts) {
    PartScope scope(s, part);
    if ((rc = launch_linearize(s, part.nb, n, 0, 0))) return rc;
    launch(s, K_OTHER, k_init, dim3(cdiv(part.nb, 64)), dim3(64), s->params, s->st, (int)part.nb, (int)n);
  }
  int remaining = nparts;
  if (0.0 < s->params.max_iters) {
    const double bound =
        (std::fmin(s->params.max_iters, 1e7) + 1.0) * ((double)std::max(s->params.ls_max_iters, 1) + 1.0) * (1.0 + max_restarts(s->params));
    const long max_rounds = (long)std::fmin(bound, 2e9);
    const int lag = std::max(1, std::min(s->dev.sync_every, 6));
    const InFlight in_flight(s->device);
    const TailFuse tf = tail_fuse(s->route, s->compact, nparts);
    for (long round = 0; round < max_rounds && remaining > 0; ++round) {
      long live_all = 0;  // (every part's last count: what shares the chip with this part's kernels)
      for (auto &part : parts) live_all += part.done ? 0 : (long)part.seen_active;
      s->live_hint = std::max<long>(live_all, 1);
      for (auto &part : parts) {
        if (part.done) continue;
        PartScope scope(s, part);
        const RoctxRange range(s, "round", round, (long)(&part - &parts[0]));
        // (compacting in EVERY round while it runs is right: waiting until 1/16, 1/8 or 1/4 of the slots in use are known holes measured -2 / -4 /
        // -5 % at B = 8192 and -9 / -9 / -12 % at 65536 -- profiles/r06_ab.txt)
        const bool compacting = s->compact && !part.tail && (part.seen_active > tf.stop || (tf.kinds && part.used > tf.slots));
        if (tf.kinds && !compacting && part.used <= tf.slots && round >= tf.from) part.tail = true;  // (counts and slots only fall)
        part.launched_rounds[round & 7] = 1;
        if (part.tail && (part.round_kernel || in_flight.alone(s->dev.fuse_in_flight == 1))) {
          // as in run_solve: k_round, four rounds per launch (fp64; the mixed mode keeps the combined launch and k_linearize).  One way only,
          // so the round before the first k_round has been published by its own k_linearize and every later one by the k_round behind it.
          if (s->route.round_kernel && QILQR_LATE_TAIL) {
            const RoundForm f = round_form(s->route, /*several=*/true, /*forced=*/false, part.seen_active, part.used);
            if ((rc = launch_round(s, part.used, n, round, part.round_kernel, f.rounds, f.six))) return rc;
            part.launched_rounds[round & 7] = (unsigned)f.rounds;
            part.round_kernel = true;
            continue;
          }
          if ((rc = launch_backward_rollout(s, part.used, n))) return rc;
          if ((rc = launch_linearize(s, part.used, n, 1, F_SEARCH, (int)(round & 0x3fffffff)))) return rc;
          continue;
        }
        if ((rc = launch_backward(s, part.used, n, 0))) return rc;
        if (compacting) {
          if ((rc = launch_compact(s, part.used, n))) return rc;
          part.used = slots_in_use(part.used, part.seen_active);
        }
        if ((rc = launch_rollout(s, part.used, n, F_SEARCH, round))) return rc;
        if ((rc = launch_linearize(s, part.used, n, 1, F_SEARCH, (int)(round & 0x3fffffff)))) return rc;
      }
      if (round < lag) continue;
      const long old = round - lag;
      for (auto &part : parts) {
        if (part.done) continue;
        unsigned long long v;
        if ((rc = wait_for_count(&part.h_active[old & 7], part.stream, old, &v))) return rc;
        // (a launch of several rounds reports the sum of their counts: the mean bounds the last round's)
        part.seen_active = ((unsigned)v + part.launched_rounds[old & 7] - 1) / part.launched_rounds[old & 7];
        if ((unsigned)v == 0) {
          part.done = true;
          --remaining;
        }
      }
      // a block that gave up a hand-off (BatchState::host_error) voids the call: stop enqueuing rounds on void gains -- each could burn a
      // full bounded spin in every block that gave up -- let what is in flight finish, and report (as run_solve does)
      if (__atomic_load_n(s->h_active + 8 * (1 + qilqr_solver::MAX_PARTS), __ATOMIC_ACQUIRE)) {
        for (auto &part : parts) (void)hipStreamSynchronize(part.stream);
        return device_error(s);
      }
    }
  }
  for (int p = 0; p < nparts; ++p) {
    HIP_TRY(hipEventRecord(s->part_done[p], parts[p].stream));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->part_done[p], 0));
  }
  return QILQR_OK;
}

// The batch solve on device-resident buffers.  drain = false: return with the gather enqueued, the caller puts
// its own copies behind it and waits for the stream itself.
int solve_batch_device_impl(qilqr_solver *s, const double *d_init, const double *d_desired_batch, int32_t B, int32_t n,
                            double *d_out_traj, double *d_out_cost, int32_t *d_out_status, int32_t *d_out_iters,
                            int32_t *d_out_n_bwd, int32_t *d_out_n_fwd, bool drain) {
  if (!s || !d_init) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  const RoctxRange range(s, "batch solve, trajectories:", (long)B);
  int rc = begin_batch(s, B, n, d_desired_batch, E_BATCH);
  if (rc) return rc;
  const bool persistent = s->route.persistent;
  if ((rc = to_tiled(s, d_init, s->st.traj[0], B, n, 18, persistent ? s->st.counters : nullptr))) return rc;
  const int nparts = s->route.parts;
  s->compact = s->route.compact;
  s->compact_out = CompactOut{d_out_traj, d_out_cost, d_out_status, d_out_iters, d_out_n_bwd, d_out_n_fwd};
  s->plan_heads.clear();
  struct CompactScope {  // (every return below leaves the flag off for the other entry points)
    qilqr_solver *s;
    ~CompactScope() { s->compact = false; }
  } compact_scope{s};
  if (persistent) {
    if ((rc = launch_solve4(s, B, n))) return rc;
  } else if (nparts > 1) {
    if ((rc = run_solve_parts(s, B, n, nparts))) return rc;
  } else {
    EarlyOut *eo = static_cast<EarlyOut *>(s->early_out);
    const std::function<int(unsigned)> hook = [&](unsigned active) -> int {
      if (eo->fired || active > eo->threshold) return QILQR_OK;
      return fire_early_out(s, B, n, eo, active);
    };
    if ((rc = run_solve(s, B, n, s->dev.sync_every, [] { return QILQR_OK; }, false, eo ? &hook : nullptr, /*double_ok=*/true))) return rc;
    if (eo && eo->fired && eo->direct) {
      // the late finishers' rows straight into the caller's (mapped, pinned) arrays, behind the early part's copies -- which cover every
      // row of those arrays, the late ones with stale data -- so that nothing overwrites them afterwards
      HIP_TRY(hipStreamWaitEvent(s->stream, s->early_done, 0));
      return gather(s, B, n, eo->v_traj, eo->v_cost, eo->v_status, eo->v_iters, eo->v_bwd, eo->v_fwd, s->d_early, 0, nullptr);
    }
    if (eo && eo->fired) {
      // the late finishers into the compact block, one copy to the pinned host block; qilqr_solve_batch puts them in place
      const LateLayout L = *eo->layout;
      int *early = s->d_early, *late_slot = early + s->early_cap, *late_idx = (int *)(s->d_late + L.idx), *late_count = (int *)(s->d_late + L.count);
      launch(s, K_OTHER, k_late_slots, dim3(cdiv(B, 256)), dim3(256), (int)B, (const int *)early, late_count, late_idx, late_slot, eo->late_cap);
      int *li = (int *)(s->d_late + L.ints);
      const long R = eo->late_cap;
      if ((rc = gather(s, B, n, eo->h_traj ? (double *)(s->d_late + L.traj) : nullptr, eo->h_cost ? (double *)(s->d_late + L.cost) : nullptr,
                       eo->h_status ? li : nullptr, eo->h_iters ? li + R : nullptr, eo->h_bwd ? li + 2 * R : nullptr,
                       eo->h_fwd ? li + 3 * R : nullptr, early, 0, late_slot)))
        return rc;
      HIP_TRY(hipMemcpyAsync(s->h_late, s->d_late, L.bytes, hipMemcpyDeviceToHost, s->stream));
      return QILQR_OK;  // (drain is false on this path: the caller waits for both streams)
    }
  }
  if ((rc = gather(s, B, n, d_out_traj, d_out_cost, d_out_status, d_out_iters, d_out_n_bwd, d_out_n_fwd, nullptr, 0,
                   s->compact ? s->st.orig : nullptr)))  // (with compaction: by the row a slot's trajectory came from)
    return rc;
  if (!drain) return QILQR_OK;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipGetLastError());
  if (s->dev.profile) drain_events(s);
  return device_error(s);
}

// The host-buffer batch solve up to, but not including, the copies back: checks, staging buffers (kept between calls, no
// hipMalloc / hipFree per call), H2D, the solve, the gather into s->stage_traj / stage_cost / stage_int -- everything
// enqueued on the solver's stream, nothing waited for.  The copies are plain hipMemcpyAsync: direct DMA when the caller's
// buffers are pinned (qilqr_host_alloc, or any hipHostMalloc / hipHostRegister'ed memory), HIP's own chunked staging when
// they are pageable.
int solve_batch_staged(qilqr_solver *s, const double *init, const double *desired_batch, int32_t B, int32_t n) {
  if (!s || !init) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || n <= 0) return fail(QILQR_ERR_INVALID_ARG, "B and n must be positive");
  const char *why = nullptr;  // (the desired trajectory's length from the horizon start on; begin_batch checks the schedule's)
  if (horizon_window_check(n, s->k0, s->n_desired, 0, !desired_batch, false, &why)) return fail(QILQR_ERR_LENGTH_MISMATCH, why);
  int rc;
  if ((rc = refuse(s, B, E_BATCH))) return rc;  // (before anything is enqueued)
  HIP_TRY(hipSetDevice(s->device));
  const size_t cnt = 18 * (size_t)B * n, tb = sizeof(double) * cnt;
  auto grow = [&](auto **p, size_t *cap, size_t want, size_t elem) -> hipError_t {
    if (want <= *cap) return hipSuccess;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc((void **)p, want * elem);
    if (e == hipSuccess) *cap = want;
    return e;
  };
  hipError_t e = grow(&s->stage_traj, &s->stage_traj_cap, cnt, sizeof(double));
  if (e == hipSuccess && desired_batch) e = grow(&s->stage_des, &s->stage_des_cap, cnt, sizeof(double));
  if (e == hipSuccess && (size_t)B > s->stage_B_cap) {
    if (s->stage_cost) (void)hipFree(s->stage_cost);
    if (s->stage_int) (void)hipFree(s->stage_int);
    s->stage_cost = nullptr;
    s->stage_int = nullptr;
    s->stage_B_cap = 0;
    e = hipMalloc((void **)&s->stage_cost, sizeof(double) * B);
    if (e == hipSuccess) e = hipMalloc((void **)&s->stage_int, sizeof(int) * 4 * B);
    if (e == hipSuccess) s->stage_B_cap = B;
  }
  // The uploads are enqueued first and the quaternion checks (manif's constructor check, SURVEY.md 8b: 0.1-0.2 ms of host
  // time for 1024 x 100 knots) run while the copy engine works; nothing that computes is enqueued before they have passed.
  if (e == hipSuccess) e = hipMemcpyAsync(s->stage_traj, init, tb, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess && desired_batch) e = hipMemcpyAsync(s->stage_des, desired_batch, tb, hipMemcpyHostToDevice, s->stream);
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("staging: ") + hipGetErrorString(e));
  if ((rc = check_quaternions(init, (long)B * n, "initial trajectory")) ||
      (desired_batch && (rc = check_quaternions(desired_batch, (long)B * n, "desired trajectory")))) {
    (void)hipStreamSynchronize(s->stream);  // the uploads read the caller's buffers: finished before the error returns
    return rc;
  }
  int *d_int = s->stage_int;
  return solve_batch_device_impl(s, s->stage_traj, desired_batch ? s->stage_des : nullptr, B, n, s->stage_traj, s->stage_cost, d_int,
                                 d_int + B, d_int + 2 * B, d_int + 3 * B, /*drain=*/false);
}
}  // namespace
