// host/solver.h -- the handle (qilqr_solver) and what every other host header stands on: the thread's last error, the one function every
// kernel launch goes through with its profiling slots and roctx ranges, the device workspace, the tiled up- and download of the host-buffer
// entry points, the scratch of one call, and the checks of a caller's trajectories and states.  Part of ilqr_capi.hip's translation unit (included from there, nowhere else).
#pragma once

namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail(QILQR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));         \
  } while (0)

// device memory of one call, freed on every return path (filled with HIP_TRY(hipMalloc((void **)&scratch.p, ...)))
struct DeviceScratch {
  double *p = nullptr;
  DeviceScratch() = default;
  DeviceScratch(const DeviceScratch &) = delete;
  DeviceScratch &operator=(const DeviceScratch &) = delete;
  ~DeviceScratch() {
    if (p) (void)hipFree(p);
  }
};

enum Kind { K_BACKWARD = 0, K_ROLLOUT = 1, K_LINEARIZE = 2, K_OTHER = 3, K_SOLVE = 4, K_KINDS = 5 };

struct EventPair {
  hipEvent_t a, b;
  int kind;
};

}  // namespace

struct qilqr_solver {
  int device = 0;
  hipStream_t stream = nullptr;
  ModelConsts<double> consts;
  SolveParams params;
  qilqr_options options;
  qilqr_device_config dev;
  int n_desired = 0;
  bool symmetric = false;  // Q == Q^T and R == R^T exactly: transpose-free backward kernel
  bool q_diag = false;     // Q exactly diagonal: the cost half of k_linearize scales rows instead of multiplying by Q (same bits)
  RecLayout layout;        // knot record layout chosen from the structure of Q
  void *d_desired = nullptr;    // shared desired trajectory, storage precision
  void *d_ctab = nullptr;       // constant operand table of k_backward, storage precision
  double *d_cl_q = nullptr;     // the handle's Q on a 16-byte boundary (qilqr_closed_loop_scored without a schedule), allocated at the first scored call
  double *d_cov_image = nullptr;  // qilqr_covariance_device's scratch: the knots' operand images (cov_launch.h: COV_IMAGE words each, pads zeroed once),
  size_t cov_image_words = 0;     // ... grown at the call that needs more
  double *d_cov_out = nullptr;    // ... and Sigma_i, m_i of a call that asks for the summary without one of them (156 words a knot)
  size_t cov_out_words = 0;
  void *d_consts = nullptr;     // the model constants in device memory (k_linearize reads them where it uses them)
  bool f32 = false;             // mixed-precision mode (qilqr_device_config.precision == 1)
  int integrator = 0;           // 0 explicit Euler (the reference), 1 the Runge-Kutta extension (qilqr_set_integrator)
  bool limited = false;         // per-rotor thrust limits set (qilqr_set_control_limits): the box route
  ControlLimits limits{};       // ... and their values
  bool modeled = false;         // per-problem models set (qilqr_set_batch_models): the general route, every call of exactly models_B problems
  long models_B = 0;            // ... for how many problems
  double *d_models = nullptr;   // ... their records in device memory, [models_B][PM_WORDS] (batch_models.h)
  int n_obstacles = 0;          // spherical obstacles in the cost (qilqr_set_obstacles): k_linearize adds them, k_round never runs
  double *d_obstacles = nullptr;   // ... the table in device memory, [OB_MAX][OB_WORDS] (obstacles.h), allocated at the first setter call
  std::vector<double> obstacles;   // ... and its host copy (qilqr_describe)
  long pobs_B = 0;                 // per-problem spheres (qilqr_set_batch_obstacles) for this many problems (0: none): every call of exactly pobs_B
  int pobs_K = 0, pobs_max = 0;    // ... K spheres per problem, the largest count
  bool pobs_moving = false;        // ... whether any used sphere has v != 0
  double *d_pobs = nullptr;        // ... the table in device memory, bob_count(pobs_B, pobs_K) doubles (obstacles.h, bob_index)
  int *d_pobs_counts = nullptr;    // ... and the counts, int32[pobs_B]
  // ... set by qilqr_set_batch_obstacles_device: pobs_max and pobs_moving are unknown to the host (qilqr_describe says so), and the two
  // arrays are kept between calls -- their capacities in doubles and in counts, 0 while the host setter's exact allocations stand
  bool pobs_on_device = false;
  size_t pobs_cap = 0, pobs_counts_cap = 0;
  double *d_fleet = nullptr;       // qilqr_fleet_neighbours_device's scratch (fleet_launch.h: fleet_scratch), grown at the call that needs more
  size_t fleet_words = 0;
  // the state-weight schedule (qilqr_set_state_weight_schedule): knot i of every problem takes Qs[i] for Q.  While it is set, `symmetric`,
  // `q_diag` and `layout` above are the schedule's (R and every Q_i symmetric; never diagonal; the dense kind 0) and the own_* fields keep
  // what qilqr_create derived from the handle's Q and R, for the clear
  int n_sched = 0;                 // ... its knots (0: none)
  bool sched_symmetric = false;    // ... every Q_i == Q_i^T exactly
  double *d_qsched = nullptr;      // ... the matrices in device memory, [n_sched][144]
  bool own_symmetric = false, own_q_diag = false, own_layout_sym = false, own_layout_ur0 = false;
  // the horizon start (qilqr_set_horizon_start, horizon.h): knot i of every call reads desired[k0 + i] of the shared desired trajectory and
  // Qs[k0 + i] of the schedule -- pointer arithmetic in begin_batch, no kernel knows of it
  int k0 = 0;
  ModelConsts<float> constsf;   // the model constants for the fp32 lane-local kernels
  // workspace
  long cap_B = 0, cap_n = 0;
  int hist_cap = 0;
  BatchState st{};
  std::vector<void *> allocs;
  int *h_counters = nullptr;  // pinned, 16 slots
  // pinned + mapped, 8 words per part written by k_linearize (BatchState::host_active): part 0 is the
  // whole batch on the main stream, parts 1..MAX_PARTS are sub-batches on their own streams
  unsigned long long *h_active = nullptr;
  unsigned long long *d_active = nullptr;  // the same memory as the device sees it
  static constexpr int MAX_PARTS = qilqr::MAX_PARTS;
  hipStream_t part_stream[MAX_PARTS] = {};
  hipEvent_t part_done[MAX_PARTS] = {};
  hipEvent_t main_ready = nullptr;
  int *d_part_counters = nullptr;  // [MAX_PARTS][2][COUNT_WORDS]
  long total_B = 0;                // trajectories in flight on the device in this call
  Route route;                     // the kernels this call takes (route.h): planned by begin_batch
  bool round_captured = false;     // the round just enqueued was a k_round launch (it fills the single solve's debug ring itself)
  long live_hint = 0;              // trajectories known to be running in this call right now (0: unknown, take the batch): launch_backward
  double *io_aos = nullptr;         // device scratch in the plain [B][n][W] layout (W <= 52), for host I/O (lazy)
  size_t io_cap = 0;                // its capacity in doubles
  void *desired_tiled = nullptr;    // per-problem desired trajectories, tiled (allocated on first use)
  // device staging of the host-buffer batch entry point (qilqr_solve_batch), kept between calls, grow-only
  double *stage_traj = nullptr, *stage_des = nullptr, *stage_cost = nullptr;
  int *stage_int = nullptr;
  size_t stage_traj_cap = 0, stage_des_cap = 0, stage_B_cap = 0;
  // copy-back of the finished trajectories under the tail rounds of a host-buffer batch solve (EarlyOut below)
  void *early_out = nullptr;              // EarlyOut *, set by qilqr_solve_batch for the duration of its solve
  hipStream_t early_stream = nullptr;
  hipEvent_t early_evt = nullptr;
  hipEvent_t early_done = nullptr;  // the early part's copies have landed (the late finishers' rows are written behind it)
  int *d_early = nullptr;                 // [2 B]: early[B] | late_slot[B]
  size_t early_cap = 0;                   // B it was allocated for
  char *d_late = nullptr, *h_late = nullptr;  // compact rows of the trajectories that finished late: device block, pinned host block
  size_t late_bytes = 0;
  // ILQRDebug ring of the single-problem solve (k_debug_capture), device memory, grow-only
  double *dbg_trajs = nullptr, *dbg_cost = nullptr;
  int *dbg_seen = nullptr;
  size_t dbg_traj_cap = 0, dbg_cost_cap = 0;
  // profiling
  std::vector<EventPair> events;
  size_t events_used = 0;
  double prof_ms[K_KINDS] = {0, 0, 0, 0, 0};
  unsigned prof_seen[K_KINDS] = {0, 0, 0, 0, 0};  // launches of each kind seen by the sampler
  int prof_n[K_KINDS] = {0, 0, 0, 0, 0};
  // k_round launches per instantiation since the last reset (launch_round counts, whatever dev.profile is; qilqr_round_launches)
  int32_t round_launches[QILQR_ROUND_KERNELS] = {};
  int num_cus = 256;  // compute units of the device (grid of the persistent solve)
  // compaction of the live trajectories (k_compact_plan / k_compact_move): on for the duration of a device-resident batch
  // solve that qualifies (compaction_for_call), with the caller's result arrays for the trajectories that leave early
  bool compact = false;
  qilqr::CompactOut compact_out{};
  std::vector<long> plan_heads;  // where the plans of the last batch solve's (sub-)batches start in st.plan (qilqr_debug_compaction_moves)
};

namespace {

// roctx ranges (SURVEY.md section 5 "Tracing / profiling"; qilqr_device_config.profile bit 16): the host thread marks the call, every round it
// enqueues and -- for a batch on sub-batch streams -- every part's share of a round, so that a `rocprofv3 --marker-trace --kernel-trace` of a
// large solve reads as rounds of named parts instead of four streams of anonymous launches (the ranges bracket the ENQUEUE on the host; the
// kernels they enqueue carry their correlation).  libroctx64 is bound at first use from beside the HIP runtime; absent, the ranges are nothing.
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    for (const char *name : {"libroctx64.so.4", "libroctx64.so", "librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so"}) {
      if (void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
        push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr;
        pop = nullptr;
      }
    }
  }
  static Roctx &get() {
    static Roctx r;
    return r;
  }
};
struct RoctxRange {
  bool on = false;
  RoctxRange(const qilqr_solver *s, const char *what, long a = -1, long b = -1);
  ~RoctxRange() {
    if (on) (void)Roctx::get().pop();
  }
};

RoctxRange::RoctxRange(const qilqr_solver *s, const char *what, long a, long b) {
  if (!(s->dev.profile & 0x10000) || !Roctx::get().push) return;
  char buf[96];
  if (a >= 0 && b >= 0) std::snprintf(buf, sizeof buf, "qilqr %s %ld part %ld", what, a, b);
  else if (a >= 0) std::snprintf(buf, sizeof buf, "qilqr %s %ld", what, a);
  else std::snprintf(buf, sizeof buf, "qilqr %s", what);
  (void)Roctx::get().push(buf);
  on = true;
}
// Slot for the start/stop events of one launch, or null when this kind of kernel is not being timed.
EventPair *timing_slot(qilqr_solver *s, int kind) {
  const int mode = s->dev.profile & 0xff, stride = (s->dev.profile >> 8) & 0xff;
  if (!mode) return nullptr;
  const unsigned seen = s->prof_seen[kind]++;  // every launch of the kind since the last reset
  if (kind != K_SOLVE) {  // (the one launch of a persistent solve is always timed)
    if (mode == 1 && kind != K_BACKWARD && kind != K_ROLLOUT) return nullptr;
    if (mode == 3 && kind != K_BACKWARD) return nullptr;
    if (mode == 4 && kind != K_ROLLOUT) return nullptr;
    // sampling: every stride-th launch of a kind carries events (a timed dispatch costs the stream ~6 us)
    if (stride > 1 && (seen % stride) != 0) return nullptr;
  }
  if (s->events_used == s->events.size()) {
    EventPair e;
    if (hipEventCreate(&e.a) != hipSuccess) return nullptr;
    if (hipEventCreate(&e.b) != hipSuccess) {
      (void)hipEventDestroy(e.a);
      return nullptr;
    }
    s->events.push_back(e);
  }
  EventPair *ep = &s->events[s->events_used++];
  ep->kind = kind;
  return ep;
}
// Every kernel goes through here.  A timed launch hands its start/stop events to the dispatch itself
// (hipExtLaunchKernelGGL): the timestamps are the kernel's own begin and end, and no extra barrier
// packet enters the stream, so profiling does not stretch the round it measures.
template <typename... P, typename... Args>
void launch(qilqr_solver *s, int kind, void (*kernel)(P...), dim3 grid, dim3 block, Args... args) {
  EventPair *ep = timing_slot(s, kind);
  hipExtLaunchKernelGGL(kernel, grid, block, 0, s->stream, ep ? ep->a : nullptr, ep ? ep->b : nullptr, 0,
                        static_cast<P>(args)...);  // arguments converted to the kernel's own parameter types
}

void drain_events(qilqr_solver *s) {
  for (size_t i = 0; i < s->events_used; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->events[i].a, s->events[i].b) == hipSuccess) {
      s->prof_ms[s->events[i].kind] += ms;
      s->prof_n[s->events[i].kind] += 1;
    }
  }
  s->events_used = 0;
}

// After a stream has drained: did a kernel give up (BatchState::host_error)?  k_rollout16 ends a block whose wavefronts lost
// a hand-off instead of spinning for ever; the trajectories of that block are then not what the solve should have produced.
int device_error(qilqr_solver *s) {
  unsigned long long *w = s->h_active + 8 * (1 + qilqr_solver::MAX_PARTS);
  const unsigned long long v = __atomic_load_n(w, __ATOMIC_ACQUIRE);
  if (!v) return QILQR_OK;
  __atomic_store_n(w, 0ull, __ATOMIC_RELEASE);
  if ((v >> 32) == 2)
    return fail(QILQR_ERR_HIP, "k_backward4: a hand-off between the wavefronts of block " + std::to_string((unsigned)v) +
                                   " never arrived (bounded spin ran out); its gains are void and the results of this call are invalid");
  return fail(QILQR_ERR_HIP, "k_rollout16: a hand-off between the wavefronts of block " + std::to_string((unsigned)v) +
                                 " never arrived (bounded spin ran out); its rollout was abandoned and the results of this call are invalid");
}

void free_workspace(qilqr_solver *s) {
  for (void *p : s->allocs) (void)hipFree(p);
  s->allocs.clear();
  s->cap_B = s->cap_n = 0;
  s->io_aos = nullptr;
  s->io_cap = 0;
  s->desired_tiled = nullptr;
}

template <typename T>
int dalloc(qilqr_solver *s, T **p, size_t count) {
  void *q = nullptr;
  hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
  if (e != hipSuccess) return fail(QILQR_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  s->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return QILQR_OK;
}

int dalloc_s(qilqr_solver *s, void **p, size_t count) {  // count elements of the storage type
  char *q = nullptr;
  int rc = dalloc(s, &q, count * (s->f32 ? sizeof(float) : sizeof(double)));
  *p = q;
  return rc;
}

// number of ILQRIterDebug entries a solve can produce: the loop of ilqr.hh:58 runs for i = 0 .. while i < max_iters
// with max_iters a double, i.e. ceil(max_iters) times
inline int debug_capacity(double max_iters) { return (int)std::fmin(std::fmax(std::ceil(max_iters), 0.0), 1e6); }

int ensure_workspace(qilqr_solver *s, long B, long n) {
  const int want_hist = s->options.populate_debug ? debug_capacity(s->params.max_iters) : 0;
  if (B <= s->cap_B && n <= s->cap_n && want_hist <= s->hist_cap) return QILQR_OK;
  // grow only: alternating (B, n) shapes settle on the larger of each instead of reallocating on every call
  const long cB = B > s->cap_B ? B : s->cap_B, cn = n > s->cap_n ? n : s->cap_n;
  free_workspace(s);
  BatchState &st = s->st;
  st.layout = s->layout;
  st.ctab = s->d_ctab;
  int rc;
  for (int k = 0; k < 2; ++k) {
    if ((rc = dalloc_s(s, &st.traj[k], (size_t)tiled_count(cB, cn, 18)))) return rc;
    if ((rc = dalloc_s(s, &st.lin[k], (size_t)rec_count(cB, cn, s->layout.stride)))) return rc;
    if ((rc = dalloc(s, &st.knot_cost[k], (size_t)tiled_count(cB, cn, 1)))) return rc;
  }
  if ((rc = dalloc_s(s, &st.gains, (size_t)tiled_count(cB, cn, 52)))) return rc;
  s->io_aos = nullptr;  // host-I/O scratch: allocated on first use (ensure_io), the device-resident solve needs none
  s->io_cap = 0;
  s->desired_tiled = nullptr;
  if ((rc = dalloc(s, &st.cur, cB))) return rc;
  if ((rc = dalloc(s, &st.cost, cB))) return rc;
  if ((rc = dalloc(s, &st.prev_cost, cB))) return rc;
  if ((rc = dalloc(s, &st.terms, 2 * cB))) return rc;
  if ((rc = dalloc(s, &st.alpha, cB))) return rc;
  if ((rc = dalloc(s, &st.mu, cB))) return rc;
  if ((rc = dalloc(s, &st.trial, cB))) return rc;
  if ((rc = dalloc(s, &st.flags, cB))) return rc;
  if ((rc = dalloc(s, &st.status, cB))) return rc;
  if ((rc = dalloc(s, &st.iters, cB))) return rc;
  if ((rc = dalloc(s, &st.n_bwd, cB))) return rc;
  if ((rc = dalloc(s, &st.n_fwd, cB))) return rc;
  if ((rc = dalloc(s, &st.counters, 2 * COUNT_WORDS))) return rc;  // (two sets: k_round alternates between them)
  if ((rc = dalloc_s(s, &st.dump, 4 * cB))) return rc;
  if ((rc = dalloc(s, &st.orig, cB))) return rc;
  if ((rc = dalloc(s, &st.plan, (size_t)PLAN_HEAD * (qilqr_solver::MAX_PARTS + 2) + 4 * (size_t)cB))) return rc;  // (a part: head, B holes, B live slots, B / 2 pairs x 4)
  st.row0 = 0;
#if defined(QILQR_STAMPS) || defined(QILQR_ROUND_STAMPS)
  if ((rc = dalloc(s, &st.stamps, 8 * cB))) return rc;
#else
  st.stamps = nullptr;
#endif
  st.cost_hist = nullptr;
  st.hist_cap = 0;
  if (want_hist > 0) {
    if ((rc = dalloc(s, &st.cost_hist, (size_t)cB * want_hist))) return rc;
    st.hist_cap = want_hist;
  }
  s->hist_cap = want_hist;
  s->cap_B = cB;
  s->cap_n = cn;
  return QILQR_OK;
}

// largest number of consecutive restarts lm_restart (kernels_common.h) can grant one iteration
inline double max_restarts(const SolveParams &p) {
  if (!(p.mu_init > 0.0) || !(p.mu_init <= p.mu_max)) return 0.0;
  return 1.0 + std::floor(std::log(p.mu_max / p.mu_init) / std::log(p.mu_factor));
}

// plain [B][n][W] fp64 (device) -> tiled, storage precision
// (zero_word: an int the same launch sets to zero -- the group queue of a persistent solve that follows)
int to_tiled(qilqr_solver *s, const double *d_plain, void *tiled, long B, long n, int W, int *zero_word = nullptr) {
  if (s->f32)
    launch(s, K_OTHER, k_retile<float>, dim3((unsigned)cdiv(B, TILE), (unsigned)cdiv(n * (W / 2) * TILE, 256)), dim3(256), d_plain, (double *)nullptr,
                       (float *)tiled, (float *)tiled, (const int *)nullptr, 0, (int)B, (int)n, W, 1, zero_word);
  else
    launch(s, K_OTHER, k_retile<double>, dim3((unsigned)cdiv(B, TILE), (unsigned)cdiv(n * (W / 2) * TILE, 256)), dim3(256), d_plain,
                       (double *)nullptr, (double *)tiled, (double *)tiled, (const int *)nullptr, 0, (int)B, (int)n, W, 1, zero_word);
  return QILQR_OK;
}
// tiled -> plain [B][n][W] fp64 (device); sel/flip choose between t0 and t1 per trajectory
int from_tiled(qilqr_solver *s, double *d_plain, void *t0, void *t1, const int *sel, int flip, long B, long n, int W) {
  if (s->f32)
    launch(s, K_OTHER, k_retile<float>, dim3((unsigned)cdiv(B, TILE), (unsigned)cdiv(n * (W / 2) * TILE, 256)), dim3(256), (const double *)nullptr,
                       d_plain, (float *)t0, (float *)t1, sel, flip, (int)B, (int)n, W, 0, (int *)nullptr);
  else
    launch(s, K_OTHER, k_retile<double>, dim3((unsigned)cdiv(B, TILE), (unsigned)cdiv(n * (W / 2) * TILE, 256)), dim3(256), (const double *)nullptr,
                       d_plain, (double *)t0, (double *)t1, sel, flip, (int)B, (int)n, W, 0, (int *)nullptr);
  return QILQR_OK;
}

// hardware queues HIP multiplexes this process's streams onto: GPU_MAX_HW_QUEUES as the runtime read it at start-up (default 4)
// Latched at the first qilqr_create_sized of the process, which calls it (the runtime reads the variable once, when it starts: a value
// put into the environment later -- os.environ after the first GPU call -- changes nothing in the runtime and must change nothing here)
int hw_queues() {
  static const int latched = [] {
    const char *e = std::getenv("GPU_MAX_HW_QUEUES");
    const int q = e ? std::atoi(e) : 4;
    return q > 0 ? q : 4;
  }();
  return latched;
}

// the plain-layout device scratch of the host-buffer entry points, sized to what the call needs
int ensure_io(qilqr_solver *s, size_t count) {
  if (count <= s->io_cap) return QILQR_OK;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->io_aos) {
    for (auto it = s->allocs.begin(); it != s->allocs.end(); ++it)
      if (*it == (void *)s->io_aos) {
        s->allocs.erase(it);
        break;
      }
    (void)hipFree(s->io_aos);
    s->io_aos = nullptr;
    s->io_cap = 0;
  }
  int rc = dalloc(s, &s->io_aos, count);
  if (rc) return rc;
  s->io_cap = count;
  return QILQR_OK;
}
// host plain array -> device tiled buffer through the io scratch
int upload_tiled(qilqr_solver *s, const double *h_plain, void *tiled, long B, long n, int W) {
  int rc0 = ensure_io(s, (size_t)B * n * W);
  if (rc0) return rc0;
  HIP_TRY(hipMemcpyAsync(s->io_aos, h_plain, sizeof(double) * (size_t)B * n * W, hipMemcpyHostToDevice, s->stream));
  return to_tiled(s, s->io_aos, tiled, B, n, W);
}
int download_tiled(qilqr_solver *s, double *h_plain, void *t0, void *t1, const int *sel, int flip, long B, long n,
                   int W) {
  int rc = ensure_io(s, (size_t)B * n * W);
  if (rc) return rc;
  if ((rc = from_tiled(s, s->io_aos, t0, t1, sel, flip, B, n, W))) return rc;
  HIP_TRY(hipMemcpyAsync(h_plain, s->io_aos, sizeof(double) * (size_t)B * n * W, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return QILQR_OK;
}

int check_quaternions(const double *traj, long count, const char *what) {
  // manif's SO3 constructor rejects quaternions that are not unit within 1e-10
  for (long i = 0; i < count; ++i) {
    const double *q = traj + i * 18 + 4;
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(std::fabs(nn - 1.0) <= 1e-10))
      return fail(QILQR_ERR_BAD_QUATERNION, std::string(what) + ": quaternion not normalized at knot " + std::to_string(i));
  }
  return QILQR_OK;
}
// the same check of states, rows of QILQR_STATE words (the x0 of the shift and of the flights): row r is sample r % S of problem r / S;
// S = 0: a row is a problem, and no sample is named
int check_state_quaternions(const double *x0, long rows, long S) {
  for (long r = 0; r < rows; ++r) {
    const double *q = x0 + r * QILQR_STATE + 3;
    const double nn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(std::fabs(nn - 1.0) <= 1e-10))
      return fail(QILQR_ERR_BAD_QUATERNION, "x0: quaternion not normalized at problem " + std::to_string(S ? r / S : r) +
                                                (S ? ", sample " + std::to_string(r % S) : std::string()));
  }
  return QILQR_OK;
}
}  // namespace
