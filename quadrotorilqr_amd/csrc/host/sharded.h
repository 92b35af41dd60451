// host/sharded.h -- the C ABI of one batch over several devices in one process: the RCCL binding, the sharded handle and its gather
// path, a shard's solve on its own host thread, and every qilqr_sharded_* entry point.  Part of ilqr_capi.hip's translation unit.
#pragma once

extern "C" {
// ---- one batch over several devices in one process (include/quadrotor_ilqr.h)
// RCCL is bound at run time (dlopen of librccl.so.1 when a sharded handle first needs a communicator), not as a link-time
// dependency: the library is 570 MB of code objects that a single-device caller never uses, and a host process that has
// PyTorch loaded already holds one under the same soname, which is then the one that is used.
extern "C++" {
namespace {
struct Rccl {
  void *lib = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string error, path;
  bool ok = false;
};
Rccl &rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    // Which librccl: the one that ships BESIDE the HIP runtime this process runs on (found from the address of a HIP entry
    // point).  A process can hold two ROCm installations -- PyTorch bundles its own libamdhip64 and librccl, this library is
    // linked against /opt/rocm's, and whichever libamdhip64 was loaded first serves both -- and an RCCL built for the other
    // runtime fails in ncclCommInitAll ("unhandled cuda error": measured, torch's librccl 7.0 on the 7.2 runtime).  Loaded
    // RTLD_LOCAL: a second copy beside one the host process already uses keeps its own state and exports nothing.
    std::vector<std::string> names;
    Dl_info where;
    if (dladdr((const void *)&hipGetDeviceCount, &where) && where.dli_fname) {
      const std::string path(where.dli_fname);
      const size_t slash = path.rfind('/');
      if (slash != std::string::npos) {
        names.push_back(path.substr(0, slash + 1) + "librccl.so.1");
        names.push_back(path.substr(0, slash + 1) + "librccl.so");
      }
    }
    names.push_back("librccl.so.1");
    names.push_back("librccl.so");
    for (const std::string &name : names) {
      r.lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (r.lib) {
        r.path = name;
        break;
      }
    }
    if (!r.lib) {
      const char *err = dlerror();
      r.error = std::string("librccl.so.1 cannot be loaded: ") + (err ? err : "?");
      return;
    }
#define QILQR_RCCL_SYM(field, sym)                                    \
  r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, #sym)); \
  if (!r.field) {                                                     \
    r.error = "librccl has no " #sym;                                 \
    return;                                                           \
  }
    QILQR_RCCL_SYM(GetVersion, ncclGetVersion)
    QILQR_RCCL_SYM(CommInitAll, ncclCommInitAll)
    QILQR_RCCL_SYM(CommDestroy, ncclCommDestroy)
    QILQR_RCCL_SYM(GroupStart, ncclGroupStart)
    QILQR_RCCL_SYM(GroupEnd, ncclGroupEnd)
    QILQR_RCCL_SYM(Send, ncclSend)
    QILQR_RCCL_SYM(Recv, ncclRecv)
    QILQR_RCCL_SYM(GetErrorString, ncclGetErrorString)
#undef QILQR_RCCL_SYM
    r.ok = true;
  });
  return r;
}
// the caller's current HIP device is put back on every return path (a torch host process has one)
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DeviceGuard() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};
}  // namespace
}  // extern "C++"

struct qilqr_sharded {
  std::vector<qilqr_solver *> solvers;
  std::vector<int> device;     // per shard: its HIP device
  std::vector<int> uniq;       // the distinct devices, in order of first appearance: rank k of the communicator is uniq[k]
  std::vector<int> rank_of;    // per shard: index of its device in uniq
  int transport = QILQR_TRANSPORT_AUTO;  // as requested
  int resolved = 0;                      // QILQR_TRANSPORT_RCCL or QILQR_TRANSPORT_PEER_COPY once the gather path exists
  std::vector<ncclComm_t> comms;         // per distinct device (RCCL transport)
  std::vector<hipStream_t> gstream;      // per distinct device: the stream the gather of that device's shards runs on
  std::vector<hipEvent_t> done;          // per shard: its solve (and gather kernel) have finished
  std::mutex gather_mutex;               // the shards' host threads enqueue their transfers one at a time (shared communicators / streams)
  std::string info;
  int32_t models_B = -1;                 // per-problem models set for this many problems (qilqr_sharded_set_batch_models), -1: none
  int32_t pobs_B = -1;                   // per-problem spheres set for this many problems (qilqr_sharded_set_batch_obstacles), -1: none
};

extern "C++" {
namespace {
void sharded_drop_gather_path(qilqr_sharded *h) {
  for (size_t k = 0; k < h->comms.size(); ++k)
    if (h->comms[k]) (void)rccl().CommDestroy(h->comms[k]);
  h->comms.clear();
  h->resolved = 0;
}
// communicators (RCCL) or nothing (peer copies), streams and events: built when the first gathered solve needs them
int sharded_ensure_gather_path(qilqr_sharded *h) {
  if (h->resolved) return QILQR_OK;
  const int nuniq = (int)h->uniq.size();
  if (h->gstream.empty()) {
    h->gstream.assign(nuniq, nullptr);
    for (int k = 0; k < nuniq; ++k) {
      HIP_TRY(hipSetDevice(h->uniq[k]));
      HIP_TRY(hipStreamCreateWithFlags(&h->gstream[k], hipStreamNonBlocking));
    }
    h->done.assign(h->solvers.size(), nullptr);
    for (size_t r = 0; r < h->solvers.size(); ++r) {
      HIP_TRY(hipSetDevice(h->device[r]));
      HIP_TRY(hipEventCreateWithFlags(&h->done[r], hipEventDisableTiming));
    }
  }
  // automatic: RCCL when the shards sit on more than one device (point-to-point over xGMI into the root's rows), plain device
  // copies when they all share one (nothing to communicate)
  int want = h->transport;
  if (want == QILQR_TRANSPORT_AUTO) want = nuniq > 1 ? QILQR_TRANSPORT_RCCL : QILQR_TRANSPORT_PEER_COPY;
  if (want == QILQR_TRANSPORT_RCCL) {
    Rccl &R = rccl();
    if (!R.ok) {
      if (h->transport == QILQR_TRANSPORT_RCCL) return fail(QILQR_ERR_HIP, "RCCL transport requested: " + R.error);
      want = QILQR_TRANSPORT_PEER_COPY;
      h->info = "peer copies (hipMemcpyPeerAsync): " + R.error;
    } else {
      h->comms.assign(nuniq, nullptr);
      const ncclResult_t st = R.CommInitAll(h->comms.data(), nuniq, h->uniq.data());
      if (st != ncclSuccess) {
        h->comms.clear();
        const std::string why = std::string("ncclCommInitAll: ") + R.GetErrorString(st);
        if (h->transport == QILQR_TRANSPORT_RCCL) return fail(QILQR_ERR_HIP, "RCCL transport requested: " + why);
        want = QILQR_TRANSPORT_PEER_COPY;
        h->info = "peer copies (hipMemcpyPeerAsync): " + why;
      } else {
        int ver = 0;
        (void)R.GetVersion(&ver);
        h->info = "rccl: ncclSend / ncclRecv, " + std::to_string(nuniq) + " rank" + (nuniq > 1 ? "s" : "") + " in one process (version code " +
                  std::to_string(ver) + ", " + R.path + ")";
      }
    }
  }
  if (want == QILQR_TRANSPORT_PEER_COPY && h->info.rfind("peer copies", 0) != 0) h->info = "peer copies (hipMemcpyPeerAsync)";
  h->resolved = want;
  return QILQR_OK;
}

// One shard's solve on the calling thread.  host_out: copy back into the caller's host arrays (qilqr_solve_batch); otherwise
// leave the results in the solver's staging buffers and record done[r] behind them (qilqr_solve_batch_sharded_device).
struct ShardCall {
  const double *init, *desired;
  int32_t B, n;
  double *out_traj, *out_cost;
  int32_t *out_status, *out_iters, *out_n_bwd, *out_n_fwd;
  bool host_out;
  int32_t root = -1;  // !host_out: the out_* arrays are device arrays on devices[root]; every shard sends its rows there itself
};
// One transfer of the gather: `count` elements of array `array` (0 traj, 1 cost, 2 status, 3 iters, 4 n_bwd, 5 n_fwd) from
// element src_off of shard `shard`'s staging buffer (rank src_rank of the communicator = the shard's device) to element dst_off
// of the root's array (rank dst_rank).  The whole schedule is a function of (B, n, shards, root, which arrays, ranks) alone --
// qilqr_gather_schedule below exposes it so that a test can check it for eight distinct devices without any.
struct GatherPiece {
  int32_t shard, array, src_rank, dst_rank;
  int64_t src_off, dst_off, count;
};
inline void gather_schedule_of_shard(int32_t B, int32_t n, int32_t k, int32_t r, int32_t root, const int *rank_of, unsigned arrays,
                                     std::vector<GatherPiece> *out) {
  int32_t b0 = 0, cnt = 0;
  (void)qilqr_shard_range(B, k, r, &b0, &cnt);
  if (cnt == 0) return;
  const int64_t row = (int64_t)n * 18;
  if (arrays & 1u) out->push_back({r, 0, rank_of[r], rank_of[root], 0, (int64_t)b0 * row, (int64_t)cnt * row});
  if (arrays & 2u) out->push_back({r, 1, rank_of[r], rank_of[root], 0, (int64_t)b0, (int64_t)cnt});
  for (int q = 0; q < 4; ++q)  // the four int32 arrays sit one behind the other in the shard's staging block: [4][cnt]
    if (arrays & (4u << q)) out->push_back({r, 2 + q, rank_of[r], rank_of[root], (int64_t)q * cnt, (int64_t)b0, (int64_t)cnt});
}
// enqueue shard r's transfers behind its solve (called from the shard's own host thread as soon as the solve is enqueued and
// its completion event recorded: the rows travel while slower shards still solve).  RCCL: ONE group per shard -- a send on the
// shard's communicator and a receive on the root's for each piece; communicators and gather streams are shared between
// shards (every shard receives on the root's), so the enqueue is serialised by the handle's mutex.
int enqueue_shard_gather(qilqr_sharded *h, const ShardCall &c, int32_t r);
void run_shard(qilqr_sharded *h, const ShardCall &c, int32_t r, int *rc_out, std::string *msg_out) {
  const int32_t k = (int32_t)h->solvers.size();
  int32_t b0 = 0, cnt = 0;
  (void)qilqr_shard_range(c.B, k, r, &b0, &cnt);
  if (cnt == 0) return;  // fewer problems than shards
  const size_t to = (size_t)b0 * c.n * 18;
  int rc;
  if (c.host_out) {
    rc = qilqr_solve_batch(h->solvers[r], c.init + to, c.desired ? c.desired + to : nullptr, cnt, c.n,
                           c.out_traj ? c.out_traj + to : nullptr, c.out_cost ? c.out_cost + b0 : nullptr,
                           c.out_status ? c.out_status + b0 : nullptr, c.out_iters ? c.out_iters + b0 : nullptr,
                           c.out_n_bwd ? c.out_n_bwd + b0 : nullptr, c.out_n_fwd ? c.out_n_fwd + b0 : nullptr);
  } else {
    rc = solve_batch_staged(h->solvers[r], c.init + to, c.desired ? c.desired + to : nullptr, cnt, c.n);
    if (rc == QILQR_OK && hipEventRecord(h->done[r], h->solvers[r]->stream) != hipSuccess) rc = fail(QILQR_ERR_HIP, "hipEventRecord");
    if (rc == QILQR_OK && c.root >= 0) rc = enqueue_shard_gather(h, c, r);
  }
  *rc_out = rc;
  if (rc != QILQR_OK) *msg_out = g_last_error;  // (thread-local: carried back to the caller)
}
// every shard on a host thread of its own (HIP's current device is per thread), shard 0 on the caller's
int run_all_shards(qilqr_sharded *h, const ShardCall &c) {
  const int32_t k = (int32_t)h->solvers.size();
  std::vector<int> rcs(k, QILQR_OK);
  std::vector<std::string> msgs(k);
  std::vector<std::thread> threads;
  bool spawn_failed = false;
  try {
    threads.reserve(k);
    for (int32_t r = 1; r < k; ++r) threads.emplace_back(run_shard, h, std::cref(c), r, &rcs[r], &msgs[r]);
  } catch (...) {
    spawn_failed = true;  // (std::system_error: no thread could be started; the shards that have one still run)
  }
  const int32_t started = 1 + (int32_t)threads.size();
  run_shard(h, c, 0, &rcs[0], &msgs[0]);
  for (std::thread &t : threads) t.join();
  if (spawn_failed)  // the shards without a thread run here, one after the other
    for (int32_t r = started; r < k; ++r) run_shard(h, c, r, &rcs[r], &msgs[r]);
  for (int32_t r = 0; r < k; ++r)
    if (rcs[r] != QILQR_OK)
      return fail(rcs[r], "shard " + std::to_string(r) + " (device " + std::to_string(h->device[r]) + "): " + msgs[r]);
  return QILQR_OK;
}
// The sharded setters' one procedure: set(solver, begin, count) hands every shard its rows [begin, begin + count) of a batch of B, and on
// the first failure clear(solver) takes the extension off every shard -- none is left half set -- and the failing shard's message is raised
// again.  checked: what the setter's check of the whole batch returned, where a failure of it clears the shards as well.
template <typename Set, typename Clear>
int sharded_set(qilqr_sharded *h, int32_t B, Set set, Clear clear, int checked = QILQR_OK) {
  DeviceGuard guard;
  const int32_t k = (int32_t)h->solvers.size();
  int rc = checked;
  for (int32_t r = 0; r < k && !rc; ++r) {
    int32_t b0 = 0, cnt = 0;
    (void)qilqr_shard_range(B, k, r, &b0, &cnt);
    rc = set(h->solvers[r], b0, cnt);
  }
  if (!rc) return QILQR_OK;
  const std::string msg = g_last_error;
  for (qilqr_solver *q : h->solvers) (void)clear(q);
  return fail(rc, msg);
}
}  // namespace
}  // extern "C++"

int qilqr_shard_range(int32_t B, int32_t n_shards, int32_t r, int32_t *begin, int32_t *count) {
  if (B < 0 || n_shards <= 0 || r < 0 || r >= n_shards || !begin || !count) return fail(QILQR_ERR_INVALID_ARG, "bad shard arguments");
  const int32_t q = B / n_shards, rem = B % n_shards;
  *begin = r * q + (r < rem ? r : rem);
  *count = q + (r < rem ? 1 : 0);
  return QILQR_OK;
}

int qilqr_sharded_create(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                         int32_t n_desired, double dt_s, const qilqr_options *options, const qilqr_device_config *dev,
                         const int32_t *devices, int32_t n_devices, qilqr_sharded **out) {
  return qilqr_sharded_create_sized(model, Q, R, desired, n_desired, dt_s, options, dev, QILQR_DEVICE_CONFIG_BYTES_ABI5, devices, n_devices, out);
}

int qilqr_sharded_create_sized(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                               int32_t n_desired, double dt_s, const qilqr_options *options, const qilqr_device_config *dev,
                               size_t dev_bytes, const int32_t *devices, int32_t n_devices, qilqr_sharded **out) {
  if (!out || !devices || n_devices <= 0 || n_devices > 64) return fail(QILQR_ERR_INVALID_ARG, "bad device list");
  DeviceGuard guard;
  qilqr_sharded *h = nullptr;
  try {
    h = new qilqr_sharded();
    for (int32_t r = 0; r < n_devices; ++r) {
      qilqr_device_config dc;
      if (!read_device_config(dev, dev_bytes, &dc)) {
        qilqr_sharded_destroy(h);
        return fail(QILQR_ERR_INVALID_ARG, "dev_bytes is not the size of a qilqr_device_config");
      }
      dc.device = devices[r];
      qilqr_solver *s = nullptr;
      const int rc = qilqr_create_sized(model, Q, R, desired, n_desired, dt_s, options, &dc, sizeof(dc), &s);
      if (rc != QILQR_OK) {
        const std::string msg = "shard " + std::to_string(r) + " (device " + std::to_string(devices[r]) + "): " + g_last_error;
        qilqr_sharded_destroy(h);
        return fail(rc, msg);
      }
      h->solvers.push_back(s);
      h->device.push_back(devices[r]);
      int idx = -1;
      for (size_t u = 0; u < h->uniq.size(); ++u)
        if (h->uniq[u] == devices[r]) idx = (int)u;
      if (idx < 0) {
        idx = (int)h->uniq.size();
        h->uniq.push_back(devices[r]);
      }
      h->rank_of.push_back(idx);
    }
  } catch (...) {  // std::bad_alloc and friends do not cross the C ABI
    if (h) qilqr_sharded_destroy(h);
    return fail(QILQR_ERR_INVALID_ARG, "qilqr_sharded_create: out of host memory");
  }
  *out = h;
  return QILQR_OK;
}

int qilqr_sharded_create_mask_sized(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                                    int32_t n_desired, double dt_s, const qilqr_options *options,
                                    const qilqr_device_config *dev, size_t dev_bytes, uint64_t device_mask, qilqr_sharded **out) {
  int32_t devices[64];
  int32_t k = 0;
  for (int32_t d = 0; d < 64; ++d)
    if (device_mask & (1ull << d)) devices[k++] = d;
  if (k == 0) return fail(QILQR_ERR_INVALID_ARG, "empty device mask");
  return qilqr_sharded_create_sized(model, Q, R, desired, n_desired, dt_s, options, dev, dev_bytes, devices, k, out);
}
// (the raw symbol, for binaries built before ABI version 7: the 32 bytes of ABI version 5 -- fields behind them, `compaction` of version 6
// included, keep their defaults: the header says so)
int qilqr_sharded_create_mask(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                              int32_t n_desired, double dt_s, const qilqr_options *options,
                              const qilqr_device_config *dev, uint64_t device_mask, qilqr_sharded **out) {
  return qilqr_sharded_create_mask_sized(model, Q, R, desired, n_desired, dt_s, options, dev, QILQR_DEVICE_CONFIG_BYTES_ABI5, device_mask, out);
}

void qilqr_sharded_destroy(qilqr_sharded *h) {
  if (!h) return;
  DeviceGuard guard;
  for (qilqr_solver *s : h->solvers) qilqr_destroy(s);
  sharded_drop_gather_path(h);
  for (size_t k = 0; k < h->gstream.size(); ++k)
    if (h->gstream[k]) {
      (void)hipSetDevice(h->uniq[k]);
      (void)hipStreamDestroy(h->gstream[k]);
    }
  for (size_t r = 0; r < h->done.size(); ++r)
    if (h->done[r]) {
      (void)hipSetDevice(h->device[r]);
      (void)hipEventDestroy(h->done[r]);
    }
  delete h;
}

int32_t qilqr_sharded_count(const qilqr_sharded *h) { return h ? (int32_t)h->solvers.size() : 0; }

qilqr_solver *qilqr_sharded_solver(qilqr_sharded *h, int32_t r) {
  return (h && r >= 0 && r < (int32_t)h->solvers.size()) ? h->solvers[r] : nullptr;
}

int qilqr_solve_batch_sharded(qilqr_sharded *h, const double *init, const double *desired_batch, int32_t B, int32_t n,
                              double *out_traj, double *out_cost, int32_t *out_status, int32_t *out_iters,
                              int32_t *out_n_bwd, int32_t *out_n_fwd) {
  if (!h || h->solvers.empty() || !init) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || n <= 0) return fail(QILQR_ERR_INVALID_ARG, "B and n must be positive");
  if (h->models_B >= 0 && B != h->models_B)  // (a shard with no rows of the models' batch has none set: checked here, for the whole batch)
    return fail(QILQR_ERR_INVALID_ARG, "batch models were set for B = " + std::to_string(h->models_B) + " problems; this call has B = " + std::to_string(B));
  if (h->pobs_B >= 0 && B != h->pobs_B)  // (likewise for the per-problem spheres)
    return fail(QILQR_ERR_INVALID_ARG, "batch obstacles were set for B = " + std::to_string(h->pobs_B) + " problems; this call has B = " + std::to_string(B));
  DeviceGuard guard;
  try {
    const ShardCall c{init, desired_batch, B, n, out_traj, out_cost, out_status, out_iters, out_n_bwd, out_n_fwd, true};
    return run_all_shards(h, c);
  } catch (...) {
    return fail(QILQR_ERR_INVALID_ARG, "qilqr_solve_batch_sharded: out of host memory");
  }
}

int qilqr_sharded_set_batch_models(qilqr_sharded *h, const qilqr_model *models, int32_t B) {
  if (!h || h->solvers.empty()) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // checked for the whole batch first, so that an error names the batch's index (every shard has the same dt, Q and R)
  std::vector<double> tab;
  int rc = check_batch_models(h->solvers[0], models, B, &tab);
  if (rc) return rc;
  h->models_B = -1;
  rc = sharded_set(h, B, [&](qilqr_solver *s, int32_t b0, int32_t cnt) { return qilqr_set_batch_models(s, cnt ? models + b0 : nullptr, cnt); },
                   [](qilqr_solver *s) { return qilqr_set_batch_models(s, nullptr, 0); });
  if (!rc && models) h->models_B = B;
  return rc;
}

int qilqr_sharded_set_obstacles(qilqr_sharded *h, const double *spheres, int32_t count) {
  if (!h || h->solvers.empty()) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  const int rc = check_obstacles(h->solvers[0], spheres, count);  // (checked once, before any shard changes)
  if (rc) return rc;
  // (every shard the whole table)
  return sharded_set(h, 0, [&](qilqr_solver *s, int32_t, int32_t) { return qilqr_set_obstacles(s, spheres, count); },
                     [](qilqr_solver *s) { return qilqr_set_obstacles(s, nullptr, 0); });
}

int qilqr_sharded_set_batch_obstacles(qilqr_sharded *h, const double *spheres, const int32_t *counts, int32_t B, int32_t K) {
  if (!h || h->solvers.empty()) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // (the whole batch is checked before any shard is set, so the index in an error is the batch's; any failure leaves every shard cleared)
  const int checked = check_batch_obstacles(h->solvers[0], spheres, counts, B, K);
  h->pobs_B = -1;
  const auto clear = [](qilqr_solver *s) { return qilqr_set_batch_obstacles(s, nullptr, nullptr, 0, 0); };
  const auto set = [&](qilqr_solver *s, int32_t b0, int32_t cnt) {
    return cnt ? qilqr_set_batch_obstacles(s, spheres + (size_t)b0 * K * OB_BWORDS, counts ? counts + b0 : nullptr, cnt, K) : clear(s);
  };
  const int rc = sharded_set(h, B, set, clear, checked);
  if (!rc && B > 0) h->pobs_B = B;
  return rc;
}

int qilqr_sharded_set_state_weight_schedule(qilqr_sharded *h, const double *Qs, int32_t n_knots) {
  if (!h || h->solvers.empty()) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // (checked once, before any shard changes; every shard the whole schedule; any failure leaves every shard cleared)
  bool qsym = true;
  const int checked = check_state_weight_schedule(h->solvers[0], Qs, n_knots, &qsym);
  return sharded_set(h, 0, [&](qilqr_solver *s, int32_t, int32_t) { return qilqr_set_state_weight_schedule(s, Qs, n_knots); },
                     [](qilqr_solver *s) { return qilqr_set_state_weight_schedule(s, nullptr, 0); }, checked);
}

int qilqr_sharded_set_horizon_start(qilqr_sharded *h, int32_t k0) {
  if (!h || h->solvers.empty()) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // (checked once, before any shard changes: every shard has the same desired trajectory and schedule.  All or none: a refused start
  // leaves every shard at the start it had, as the single handle's setter does)
  const int checked = check_horizon_start(h->solvers[0], k0);
  if (checked) return checked;
  std::vector<int> had;
  for (const qilqr_solver *s : h->solvers) had.push_back(s->k0);
  return sharded_set(h, 0, [&](qilqr_solver *s, int32_t, int32_t) { return qilqr_set_horizon_start(s, k0); },
                     [&](qilqr_solver *s) {
                       for (size_t r = 0; r < h->solvers.size(); ++r)
                         if (h->solvers[r] == s) s->k0 = had[r];
                       return QILQR_OK;
                     });
}

int qilqr_sharded_set_transport(qilqr_sharded *h, int32_t transport) {
  if (!h) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  if (transport != QILQR_TRANSPORT_AUTO && transport != QILQR_TRANSPORT_RCCL && transport != QILQR_TRANSPORT_PEER_COPY)
    return fail(QILQR_ERR_INVALID_ARG, "transport must be QILQR_TRANSPORT_AUTO, _RCCL or _PEER_COPY");
  DeviceGuard guard;
  if (transport != h->transport) sharded_drop_gather_path(h);
  h->transport = transport;
  h->info.clear();
  return sharded_ensure_gather_path(h);
}

const char *qilqr_sharded_transport(qilqr_sharded *h) {
  if (!h) return "";
  DeviceGuard guard;
  if (!h->resolved && sharded_ensure_gather_path(h) != QILQR_OK) return "";
  return h->info.c_str();
}

// The C counterpart of quadrotorilqr_amd/sharding.gather_to_root: every shard's results go from the staging buffers of its
// solver straight into ITS rows of the root device's arrays -- ragged (shards differ by one problem when the count does not
// divide B), no padding, nothing concatenated afterwards.  RCCL transport: one ncclSend on the shard's device and one
// ncclRecv on the root's per array, all inside one group (a single host thread drives every communicator of the process);
// a shard on the root's own device is a send and a receive on the same communicator.  Peer-copy transport:
// hipMemcpyPeerAsync.  Either way the transfer of a shard starts when that shard's solve has finished (stream-ordered
// behind its `done` event), not when the slowest has.
extern "C++" {
namespace {
int enqueue_shard_gather(qilqr_sharded *h, const ShardCall &c, int32_t r) {
  const int32_t k = (int32_t)h->solvers.size();
  const unsigned arrays = (c.out_traj ? 1u : 0u) | (c.out_cost ? 2u : 0u) | (c.out_status ? 4u : 0u) | (c.out_iters ? 8u : 0u) |
                          (c.out_n_bwd ? 16u : 0u) | (c.out_n_fwd ? 32u : 0u);
  std::vector<GatherPiece> sched;
  gather_schedule_of_shard(c.B, c.n, k, r, c.root, h->rank_of.data(), arrays, &sched);
  if (sched.empty()) return QILQR_OK;
  qilqr_solver *s = h->solvers[r];
  const int rr = h->rank_of[c.root], root_dev = h->device[c.root];
  hipStream_t gs = h->gstream[h->rank_of[r]], rs = h->gstream[rr];
  void *dst_base[6] = {c.out_traj, c.out_cost, c.out_status, c.out_iters, c.out_n_bwd, c.out_n_fwd};
  const void *src_base[6] = {s->stage_traj, s->stage_cost, s->stage_int, s->stage_int, s->stage_int, s->stage_int};
  if (h->resolved == QILQR_TRANSPORT_RCCL) {
    // A communicator executes its operations in the order they were issued, and every shard's receives are operations of the ROOT's
    // communicator: issued when the solves are enqueued, the group of a slow shard would hold back the receives of every faster shard
    // issued behind it.  The shard's host thread therefore waits for its own solve first and issues its group then: the
    // groups reach the root's communicator in the order the shards finish.  (Peer copies run on a stream per source device and need no
    // such care.)
    HIP_TRY(hipSetDevice(h->device[r]));
    HIP_TRY(hipEventSynchronize(h->done[r]));
  }
  std::lock_guard<std::mutex> lock(h->gather_mutex);
  HIP_TRY(hipSetDevice(h->device[r]));
  HIP_TRY(hipStreamWaitEvent(gs, h->done[r], 0));
  if (h->resolved == QILQR_TRANSPORT_RCCL) {
    // the receives run on the root's gather stream: it must not start them before this shard's rows exist either
    if (rs != gs) {
      HIP_TRY(hipSetDevice(root_dev));
      HIP_TRY(hipStreamWaitEvent(rs, h->done[r], 0));
      HIP_TRY(hipSetDevice(h->device[r]));
    }
    Rccl &R = rccl();
    ncclResult_t st = R.GroupStart();
    for (const GatherPiece &pc : sched) {
      if (st != ncclSuccess) break;
      const size_t es = pc.array < 2 ? sizeof(double) : sizeof(int32_t);
      const ncclDataType_t ty = pc.array < 2 ? ncclDouble : ncclInt32;
      st = R.Send((const char *)src_base[pc.array] + es * pc.src_off, (size_t)pc.count, ty, pc.dst_rank, h->comms[pc.src_rank], gs);
      if (st == ncclSuccess) st = R.Recv((char *)dst_base[pc.array] + es * pc.dst_off, (size_t)pc.count, ty, pc.src_rank, h->comms[pc.dst_rank], rs);
    }
    const ncclResult_t st_end = R.GroupEnd();
    if (st == ncclSuccess) st = st_end;
    if (st != ncclSuccess) return fail(QILQR_ERR_HIP, std::string("RCCL gather: ") + R.GetErrorString(st));
  } else {
    for (const GatherPiece &pc : sched) {
      const size_t es = pc.array < 2 ? sizeof(double) : sizeof(int32_t);
      HIP_TRY(hipMemcpyPeerAsync((char *)dst_base[pc.array] + es * pc.dst_off, root_dev, (const char *)src_base[pc.array] + es * pc.src_off,
                                 h->device[r], es * (size_t)pc.count, gs));
    }
  }
  return QILQR_OK;
}
}  // namespace
}  // extern "C++"

// The transfers qilqr_solve_batch_sharded_device issues, without issuing them (no device is touched): for a batch of B problems of
// n knots over n_shards shards whose devices are `devices` (ordinals; equal ordinals share a communicator rank, numbered in order
// of first appearance), root shard `root`, arrays = bit mask (1 traj, 2 cost, 4 status, 8 iters, 16 n_bwd, 32 n_fwd).  out:
// 7 x int64 per transfer = {shard, array, src_rank, dst_rank, src_off, dst_off, count} in the order they are enqueued per shard
// (shard by shard here; at run time every shard's group goes out when that shard's solve has).  Returns the number of transfers
// (out may be NULL or shorter: cap entries are written).
int qilqr_gather_schedule(int32_t B, int32_t n, const int32_t *devices, int32_t n_shards, int32_t root, uint32_t arrays, int64_t *out,
                          int32_t cap) {
  if (B <= 0 || n <= 0 || n_shards <= 0 || !devices || root < 0 || root >= n_shards) return fail(QILQR_ERR_INVALID_ARG, "bad argument"), -1;
  try {
    std::vector<int> uniq, rank_of(n_shards);
    for (int32_t r = 0; r < n_shards; ++r) {
      size_t u = 0;
      while (u < uniq.size() && uniq[u] != devices[r]) ++u;
      if (u == uniq.size()) uniq.push_back(devices[r]);
      rank_of[r] = (int)u;
    }
    std::vector<GatherPiece> sched;
    for (int32_t r = 0; r < n_shards; ++r) gather_schedule_of_shard(B, n, n_shards, r, root, rank_of.data(), arrays, &sched);
    for (size_t i = 0; i < sched.size() && out && (int32_t)i < cap; ++i) {
      const GatherPiece &pc = sched[i];
      const int64_t row[7] = {pc.shard, pc.array, pc.src_rank, pc.dst_rank, pc.src_off, pc.dst_off, pc.count};
      for (int q = 0; q < 7; ++q) out[7 * i + q] = row[q];
    }
    return (int)sched.size();
  } catch (...) {
    return fail(QILQR_ERR_INVALID_ARG, "out of host memory"), -1;
  }
}

int qilqr_solve_batch_sharded_device(qilqr_sharded *h, const double *init, const double *desired_batch, int32_t B, int32_t n,
                                     int32_t root, double *d_out_traj, double *d_out_cost, int32_t *d_out_status,
                                     int32_t *d_out_iters, int32_t *d_out_n_bwd, int32_t *d_out_n_fwd, double *gather_ms) {
  if (!h || h->solvers.empty() || !init) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || n <= 0) return fail(QILQR_ERR_INVALID_ARG, "B and n must be positive");
  if (h->models_B >= 0 && B != h->models_B)
    return fail(QILQR_ERR_INVALID_ARG, "batch models were set for B = " + std::to_string(h->models_B) + " problems; this call has B = " + std::to_string(B));
  if (h->pobs_B >= 0 && B != h->pobs_B)
    return fail(QILQR_ERR_INVALID_ARG, "batch obstacles were set for B = " + std::to_string(h->pobs_B) + " problems; this call has B = " + std::to_string(B));
  const int32_t k = (int32_t)h->solvers.size();
  if (root < 0 || root >= k) return fail(QILQR_ERR_INVALID_ARG, "root must be a shard index");
  DeviceGuard guard;
  try {
    int rc = sharded_ensure_gather_path(h);
    if (rc) return rc;
    ShardCall c{init, desired_batch, B, n, d_out_traj, d_out_cost, d_out_status, d_out_iters, d_out_n_bwd, d_out_n_fwd, false};
    c.root = root;
    auto settle_everything = [&]() {  // nothing of a failed call stays in flight: solver streams AND gather streams
      for (qilqr_solver *s : h->solvers) {
        (void)hipSetDevice(s->device);
        (void)hipStreamSynchronize(s->stream);
        if (s->early_stream) (void)hipStreamSynchronize(s->early_stream);
      }
      for (size_t u = 0; u < h->uniq.size(); ++u) {
        (void)hipSetDevice(h->uniq[u]);
        (void)hipStreamSynchronize(h->gstream[u]);
      }
    };
    if ((rc = run_all_shards(h, c))) {  // (every shard has enqueued its own transfers behind its solve: enqueue_shard_gather)
      settle_everything();
      return rc;
    }
    std::vector<std::vector<int>> pieces(k);  // (only whether a shard has rows)
    for (int32_t r = 0; r < k; ++r) {
      int32_t b0 = 0, cnt = 0;
      (void)qilqr_shard_range(B, k, r, &b0, &cnt);
      if (cnt > 0) pieces[r].push_back(1);
    }
    // exposed gather time: from the moment the SLOWEST solve has finished to the moment the root holds every row (the faster
    // shards' rows have been travelling since their own solves finished)
    auto sync_or_settle = [&](hipError_t e, const char *what) -> int {
      if (e == hipSuccess) return QILQR_OK;
      settle_everything();
      return fail(QILQR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    for (int32_t r = 0; r < k; ++r)
      if (!pieces[r].empty()) {
        if ((rc = sync_or_settle(hipSetDevice(h->device[r]), "hipSetDevice"))) return rc;
        if ((rc = sync_or_settle(hipEventSynchronize(h->done[r]), "hipEventSynchronize"))) return rc;
      }
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t u = 0; u < h->uniq.size(); ++u) {
      if ((rc = sync_or_settle(hipSetDevice(h->uniq[u]), "hipSetDevice"))) return rc;
      if ((rc = sync_or_settle(hipStreamSynchronize(h->gstream[u]), "hipStreamSynchronize (gather)"))) return rc;
    }
    if (gather_ms) *gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (qilqr_solver *s : h->solvers)
      if (s->dev.profile) drain_events(s);
    for (int32_t r = 0; r < k; ++r)
      if ((rc = device_error(h->solvers[r]))) return fail(rc, "shard " + std::to_string(r) + " (device " + std::to_string(h->device[r]) + "): " + g_last_error);
    return QILQR_OK;
  } catch (...) {
    return fail(QILQR_ERR_INVALID_ARG, "qilqr_solve_batch_sharded_device: out of host memory");
  }
}
}  // extern "C"
