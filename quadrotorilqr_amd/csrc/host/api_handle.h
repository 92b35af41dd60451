// host/api_handle.h -- the C ABI of a handle: create and destroy, options, profiles, regularisation, and the setters of the extensions
// (integrator, control limits, per-problem models, obstacles, the state-weight schedule, the horizon start) with the checks of what they are given.  Part of ilqr_capi.hip's
// translation unit.
#pragma once

extern "C" {
// the caller's structure (dev_bytes of it: the fields of the header it was compiled with) over the defaults
static bool read_device_config(const qilqr_device_config *dev, size_t dev_bytes, qilqr_device_config *dc) {
  *dc = qilqr_device_config{};
  dc->sync_every = 2;
  if (!dev) return true;
  if (dev_bytes < sizeof(int32_t) || dev_bytes % sizeof(int32_t) != 0) return false;
  std::memcpy(dc, dev, std::min(dev_bytes, sizeof(qilqr_device_config)));  // (a caller NEWER than the library: its extra fields are not known here)
  return true;
}

int qilqr_create(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                 int32_t n_desired, double dt_s, const qilqr_options *options,
                 const qilqr_device_config *dev, qilqr_solver **out) {
  // the symbol binaries built before ABI version 7 call: it reads the fields every such header had
  return qilqr_create_sized(model, Q, R, desired, n_desired, dt_s, options, dev, QILQR_DEVICE_CONFIG_BYTES_ABI5, out);
}

int qilqr_create_sized(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                       int32_t n_desired, double dt_s, const qilqr_options *options,
                       const qilqr_device_config *dev, size_t dev_bytes, qilqr_solver **out) {
  if (!model || !Q || !R || !options || !out || n_desired < 0 || (n_desired > 0 && !desired))
    return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // QuadrotorModel ctor, quadrotor_model.cc:6-25
  ModelConsts<double> mc;
  if (!make_model_consts(model->mass_kg, model->inertia, model->arm_length_m, model->torque_to_thrust_ratio_m,
                         model->g_mpss, Q, R, dt_s, &mc))
    return fail(QILQR_ERR_BAD_INERTIA, "Inertia matrix is not positive definite!");
  if (n_desired > 0) {
    int rc = check_quaternions(desired, n_desired, "desired trajectory");
    if (rc) return rc;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(QILQR_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
  qilqr_device_config dc;
  if (!read_device_config(dev, dev_bytes, &dc)) return fail(QILQR_ERR_INVALID_ARG, "dev_bytes is not the size of a qilqr_device_config");
  (void)hw_queues();  // latched here, with the process's first solver
  if (dc.device < 0 || dc.device >= ndev) return fail(QILQR_ERR_INVALID_ARG, "bad device ordinal");
  if (dc.round_launch < 0 || dc.round_launch > 2) return fail(QILQR_ERR_INVALID_ARG, "round_launch is 0 (automatic), 1 (three launches per round) or 2 (two)");
  if (!(dc.rounds_per_launch == 0 || dc.rounds_per_launch == 1 || dc.rounds_per_launch == 2 || dc.rounds_per_launch == 4))
    return fail(QILQR_ERR_INVALID_ARG, "rounds_per_launch is 0 (automatic), 1, 2 or 4");
  if (dc.sync_every < 1) dc.sync_every = 1;
#ifndef QILQR_WITH_SOLVE4
  if (dc.persistent == 1)
    return fail(QILQR_ERR_INVALID_ARG, "persistent = 1 (k_solve4, the one-launch solve) is in the diagnostics build: make -C quadrotorilqr_amd/csrc diag");
#endif
  if (dc.compaction < -1 || dc.compaction > 1) return fail(QILQR_ERR_INVALID_ARG, "compaction is -1 (never), 0 (automatic) or 1 (whenever possible)");
  if (dc.force_general == 6)
    return fail(QILQR_ERR_INVALID_ARG, "force_general = 6 (the fused k_backward4 with a block barrier per knot) was retired in round 4: 5 is the fused form");
#ifndef QILQR_WITH_BACKWARD2
  if (dc.force_general == 3)
    return fail(QILQR_ERR_INVALID_ARG, "force_general = 3 (k_backward2) is in the diagnostics build: make -C quadrotorilqr_amd/csrc diag");
#endif

  qilqr_solver *s = new qilqr_solver();
  s->device = dc.device;
  s->dev = dc;
  s->options = *options;
  s->params = SolveParams{options->step_update, options->desired_reduction_frac, options->rtol, options->atol,
                          options->max_iters, options->ls_max_iters, 0.0, 1.0, 0.0};
  s->consts = mc;
  s->f32 = (dc.precision == 1);
  convert_consts(mc, s->constsf);
  s->symmetric = true;
  for (int i = 0; i < 12; ++i)
    for (int k = 0; k < i; ++k) s->symmetric = s->symmetric && (Q[i * 12 + k] == Q[k * 12 + i]);
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < i; ++k) s->symmetric = s->symmetric && (R[i * 4 + k] == R[k * 4 + i]);
  if (dc.force_general == 1) s->symmetric = false;
  {
    bool qsym = true, ur0 = true;
    for (int i = 0; i < 12; ++i)
      for (int k = 0; k < 12; ++k) {
        qsym = qsym && (Q[i * 12 + k] == Q[k * 12 + i]);
        if (i < 6 && k >= 6) ur0 = ur0 && (Q[i * 12 + k] == 0.0);
      }
    s->layout = make_layout(qsym && dc.force_general != 1, ur0);
    bool diag = true;
    for (int i = 0; i < 12; ++i)
      for (int k = 0; k < 12; ++k)
        if (i != k) diag = diag && (Q[i * 12 + k] == 0.0);
    s->q_diag = diag && dc.dense_weights == 0;  // (qilqr_device_config.dense_weights: A/B and the bit-identity test)
  }
  // (what a cleared state-weight schedule restores)
  s->own_symmetric = s->symmetric;
  s->own_q_diag = s->q_diag;
  s->own_layout_sym = s->layout.sym != 0;
  s->own_layout_ur0 = s->layout.ur_zero != 0;
  s->n_desired = n_desired;

  hipError_t e = hipSetDevice(s->device);
  if (e == hipSuccess) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) == hipSuccess && cus > 0) s->num_cus = cus;
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  const size_t es = s->f32 ? sizeof(float) : sizeof(double);
  if (e == hipSuccess) e = hipMalloc(&s->d_desired, es * 18 * (n_desired > 0 ? n_desired : 1));
  if (e == hipSuccess && n_desired > 0) {
    if (s->f32) {
      std::vector<float> tmp((size_t)18 * n_desired);
      for (size_t i = 0; i < tmp.size(); ++i) tmp[i] = (float)desired[i];
      e = hipMemcpy(s->d_desired, tmp.data(), es * tmp.size(), hipMemcpyHostToDevice);
    } else {
      e = hipMemcpy(s->d_desired, desired, es * 18 * n_desired, hipMemcpyHostToDevice);
    }
  }
  if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_counters, sizeof(int) * COUNT_WORDS, hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc((void **)&s->h_active, sizeof(unsigned long long) * (8 * (1 + qilqr_solver::MAX_PARTS) + 1),
                      hipHostMallocMapped | hipHostMallocCoherent);  // (+ 1: the error word, BatchState::host_error)
  if (e == hipSuccess) {
    for (int k = 0; k < 8 * (1 + qilqr_solver::MAX_PARTS) + 1; ++k) s->h_active[k] = 0;
    e = hipHostGetDevicePointer((void **)&s->d_active, s->h_active, 0);
    s->st.host_active = s->d_active;
    s->st.host_error = s->d_active + 8 * (1 + qilqr_solver::MAX_PARTS);
  }
  if (e == hipSuccess) e = hipMalloc((void **)&s->d_part_counters, sizeof(int) * 2 * COUNT_WORDS * qilqr_solver::MAX_PARTS);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->main_ready, hipEventDisableTiming);
  // (the streams and events of sub-batches are created when a solve first uses them: ensure_parts)
  if (e == hipSuccess) e = hipMalloc(&s->d_consts, s->f32 ? sizeof(ModelConsts<float>) : sizeof(ModelConsts<double>));
  if (e == hipSuccess)
    e = s->f32 ? hipMemcpy(s->d_consts, &s->constsf, sizeof(ModelConsts<float>), hipMemcpyHostToDevice)
               : hipMemcpy(s->d_consts, &s->consts, sizeof(ModelConsts<double>), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&s->d_ctab, es * CTAB_SIZE);
  if (e == hipSuccess) {
    double tab[CTAB_SIZE];
    float tabf[CTAB_SIZE];
    build_ctab(s->consts.Bu, s->consts.Q, tab);
    for (int i = 0; i < CTAB_SIZE; ++i) tabf[i] = (float)tab[i];
    e = hipMemcpy(s->d_ctab, s->f32 ? (const void *)tabf : (const void *)tab, es * CTAB_SIZE, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    const int rc = fail(QILQR_ERR_HIP, std::string("qilqr_create: ") + hipGetErrorString(e));
    qilqr_destroy(s);
    return rc;
  }
  *out = s;
  return QILQR_OK;
}

void qilqr_destroy(qilqr_solver *s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  free_workspace(s);
  for (auto &e : s->events) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  if (s->early_stream) (void)hipStreamDestroy(s->early_stream);
  if (s->early_evt) (void)hipEventDestroy(s->early_evt);
  if (s->early_done) (void)hipEventDestroy(s->early_done);
  if (s->d_early) (void)hipFree(s->d_early);
  if (s->d_late) (void)hipFree(s->d_late);
  if (s->h_late) (void)hipHostFree(s->h_late);
  if (s->dbg_trajs) (void)hipFree(s->dbg_trajs);
  if (s->dbg_cost) (void)hipFree(s->dbg_cost);
  if (s->dbg_seen) (void)hipFree(s->dbg_seen);
  if (s->stage_traj) (void)hipFree(s->stage_traj);
  if (s->stage_des) (void)hipFree(s->stage_des);
  if (s->stage_cost) (void)hipFree(s->stage_cost);
  if (s->stage_int) (void)hipFree(s->stage_int);
  if (s->d_desired) (void)hipFree(s->d_desired);
  if (s->d_ctab) (void)hipFree(s->d_ctab);
  if (s->d_models) (void)hipFree(s->d_models);
  if (s->d_obstacles) (void)hipFree(s->d_obstacles);
  if (s->d_pobs) (void)hipFree(s->d_pobs);
  if (s->d_pobs_counts) (void)hipFree(s->d_pobs_counts);
  if (s->d_qsched) (void)hipFree(s->d_qsched);
  if (s->d_cl_q) (void)hipFree(s->d_cl_q);
  if (s->d_cov_image) (void)hipFree(s->d_cov_image);
  if (s->d_cov_out) (void)hipFree(s->d_cov_out);
  if (s->d_fleet) (void)hipFree(s->d_fleet);
  if (s->d_consts) (void)hipFree(s->d_consts);
  if (s->h_counters) (void)hipHostFree(s->h_counters);
  if (s->h_active) (void)hipHostFree(s->h_active);
  if (s->d_part_counters) (void)hipFree(s->d_part_counters);
  if (s->main_ready) (void)hipEventDestroy(s->main_ready);
  for (int k = 0; k < qilqr_solver::MAX_PARTS; ++k) {
    if (s->part_done[k]) (void)hipEventDestroy(s->part_done[k]);
    if (s->part_stream[k]) (void)hipStreamDestroy(s->part_stream[k]);
  }
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

int qilqr_device(const qilqr_solver *s) { return s ? s->device : -1; }
void *qilqr_stream(const qilqr_solver *s) { return s ? (void *)s->stream : nullptr; }

int qilqr_cost_history(qilqr_solver *s, int32_t B, double *hist, int32_t cap, int32_t *out_cap) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  if (out_cap) *out_cap = s->hist_cap;
  if (!hist) return QILQR_OK;
  if (!s->options.populate_debug || !s->st.cost_hist || s->hist_cap <= 0)
    return fail(QILQR_ERR_INVALID_ARG, "cost history needs options.populate_debug");
  if (B <= 0 || B > s->cap_B || cap < s->hist_cap) return fail(QILQR_ERR_INVALID_ARG, "bad B or cap");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::vector<double> tmp((size_t)B * s->hist_cap);
  std::vector<int> iters(B);
  HIP_TRY(hipMemcpy(tmp.data(), s->st.cost_hist, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(iters.data(), s->st.iters, sizeof(int) * B, hipMemcpyDeviceToHost));
  for (long b = 0; b < B; ++b)
    for (int k = 0; k < cap; ++k)
      hist[b * cap + k] = (k < iters[b] && k < s->hist_cap) ? tmp[b * s->hist_cap + k] : std::nan("");
  return QILQR_OK;
}

int qilqr_profile_reset(qilqr_solver *s) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->events_used = 0;
  for (int k = 0; k < K_KINDS; ++k) {
    s->prof_ms[k] = 0;
    s->prof_n[k] = 0;
    s->prof_seen[k] = 0;
  }
  for (int k = 0; k < QILQR_ROUND_KERNELS; ++k) s->round_launches[k] = 0;
  return QILQR_OK;
}

int qilqr_round_launches(qilqr_solver *s, int32_t counts[QILQR_ROUND_KERNELS]) {
  if (!s || !counts) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  // (counted on the host where the launch is enqueued: nothing to wait for)
  for (int k = 0; k < QILQR_ROUND_KERNELS; ++k) counts[k] = s->round_launches[k];
  return QILQR_OK;
}

int qilqr_profile_mode(qilqr_solver *s, int32_t mode) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  if (mode < 0 || (mode & 0xff) > 4 || (mode >> 16)) return fail(QILQR_ERR_INVALID_ARG, "profile mode must be 0..4 (+ stride << 8)");
  int rc = qilqr_profile_reset(s);
  if (rc) return rc;
  s->dev.profile = mode;
  return QILQR_OK;
}

int qilqr_set_regularisation(qilqr_solver *s, double mu_init, double mu_factor, double mu_max) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  if (!(mu_init >= 0.0) || !std::isfinite(mu_init)) return fail(QILQR_ERR_INVALID_ARG, "mu_init must be finite and >= 0");
  if (mu_init > 0.0) {
    if (!(mu_factor > 1.0) || !std::isfinite(mu_factor)) return fail(QILQR_ERR_INVALID_ARG, "mu_factor must be finite and > 1");
    if (!(mu_max >= mu_init) || !std::isfinite(mu_max)) return fail(QILQR_ERR_INVALID_ARG, "mu_max must be finite and >= mu_init");
    // the restarts of one iteration must fit the round bound of run_solve
    if (std::log(mu_max / mu_init) / std::log(mu_factor) > 1000.0)
      return fail(QILQR_ERR_INVALID_ARG, "more than 1000 restarts between mu_init and mu_max");
  } else {
    mu_factor = 1.0;
    mu_max = 0.0;
  }
  s->params.mu_init = mu_init;
  s->params.mu_factor = mu_factor;
  s->params.mu_max = mu_max;
  return QILQR_OK;
}

int qilqr_set_integrator(qilqr_solver *s, int32_t integrator) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  if (integrator != 0 && integrator != 1) return fail(QILQR_ERR_INVALID_ARG, "integrator must be 0 (explicit Euler) or 1 (Runge-Kutta)");
  if (integrator == 1 && s->f32) return fail(QILQR_ERR_INVALID_ARG, "the Runge-Kutta extension needs precision 0 (fp64)");
  if (integrator == s->integrator) return QILQR_OK;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // the knot records change shape (dense M instead of the Euler step's six blocks): the workspace is rebuilt on the next call
  free_workspace(s);
  s->integrator = integrator;
  s->layout = make_layout(s->layout.sym != 0, s->layout.ur_zero != 0, integrator == 1);
  return QILQR_OK;
}

int qilqr_set_control_limits(qilqr_solver *s, const double *lo, const double *hi) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  if ((lo == nullptr) != (hi == nullptr)) return fail(QILQR_ERR_INVALID_ARG, "control limits: lo and hi are both given or both NULL");
  if (lo) {
    for (int a = 0; a < 4; ++a)
      if (std::isnan(lo[a]) || std::isnan(hi[a]) || !(lo[a] < hi[a]))
        return fail(QILQR_ERR_INVALID_ARG, "control limits: rotor " + std::to_string(a) + " needs lo < hi and no NaN");
    if (s->f32) return fail(QILQR_ERR_INVALID_ARG, "control limits need precision 0 (fp64)");
    if (!s->symmetric)
      return fail(QILQR_ERR_INVALID_ARG, "control limits need exactly symmetric Q and R (and force_general != 1; with a state-weight schedule, every Q_i): the box form is the symmetric recursion");
    // the QP needs a strictly convex Q_uu = 2 R + J_u^T V_xx J_u: R positive definite (Cholesky of 2 R)
    double L[16] = {0};
    bool pd = true;
    for (int i = 0; i < 4 && pd; ++i)
      for (int k = 0; k <= i && pd; ++k) {
        double v = 2.0 * s->consts.R[i * 4 + k];
        for (int m = 0; m < k; ++m) v -= L[i * 4 + m] * L[k * 4 + m];
        if (i == k) {
          pd = v > 0.0;
          L[i * 4 + i] = pd ? std::sqrt(v) : 0.0;
        } else {
          L[i * 4 + k] = v / L[k * 4 + k];
        }
      }
    if (!pd) return fail(QILQR_ERR_INVALID_ARG, "control limits need R positive definite (the box QP of every knot must be strictly convex)");
  }
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // (nothing of the workspace depends on the limits: the record placement is chosen per call, begin_batch -> Route::tiled)
  s->limited = lo != nullptr;
  if (lo)
    for (int a = 0; a < 4; ++a) {
      s->limits.lo[a] = lo[a];
      s->limits.hi[a] = hi[a];
    }
  else
    s->limits = ControlLimits{};
  return QILQR_OK;
}

namespace {
// qilqr_set_batch_models' checks of what it is given, and the records (empty: clear), shared with the sharded setter; the index is the batch's
int check_batch_models(const qilqr_solver *s, const qilqr_model *models, int32_t B, std::vector<double> *tab) {
  if (B < 0 || (models == nullptr) != (B == 0))
    return fail(QILQR_ERR_INVALID_ARG, "batch models: B > 0 models, or models = NULL and B = 0 to clear them");
  tab->clear();
  if (models) {
    if (s->f32) return fail(QILQR_ERR_INVALID_ARG, "batch models need precision 0 (fp64): the mixed-precision kernels have one model");
    // every model gets qilqr_create's checks (make_model_consts), with the handle's dt, Q and R: the records hold the bits of such a handle
    tab->resize((size_t)B * PM_WORDS);
    const long bad = make_model_table(models, (long)B, s->consts.Q, s->consts.R, s->consts.dt, tab->data());
    if (bad >= 0)
      return fail(QILQR_ERR_BAD_INERTIA, "Inertia matrix is not positive definite! (batch models: problem " + std::to_string(bad) + ")");
  }
  return QILQR_OK;
}
}  // namespace

int qilqr_set_batch_models(qilqr_solver *s, const qilqr_model *models, int32_t B) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  std::vector<double> tab;
  int rc = check_batch_models(s, models, B, &tab);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  // (nothing of the workspace depends on the models: the record placement is chosen per call, begin_batch -> Route::tiled)
  s->modeled = false;
  s->models_B = 0;
  if (s->d_models) (void)hipFree(s->d_models);
  s->d_models = nullptr;
  if (models) {
    HIP_TRY(hipMalloc((void **)&s->d_models, sizeof(double) * tab.size()));
    HIP_TRY(hipMemcpy(s->d_models, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    s->modeled = true;
    s->models_B = B;
  }
  return QILQR_OK;
}

namespace {
// qilqr_set_obstacles' checks of a table, shared with the sharded setter
int check_obstacles(const qilqr_solver *s, const double *spheres, int32_t count) {
  if (count < 0 || count > QILQR_MAX_OBSTACLES || (spheres == nullptr) != (count == 0))
    return fail(QILQR_ERR_INVALID_ARG, "obstacles: 1 ... " + std::to_string(QILQR_MAX_OBSTACLES) +
                                           " spheres {cx, cy, cz, radius, weight}, or spheres = NULL and count = 0 to clear them");
  for (int32_t j = 0; j < count; ++j) {
    const double *sp = spheres + (size_t)j * OB_WORDS;
    for (int k = 0; k < OB_WORDS; ++k)
      if (!std::isfinite(sp[k])) return fail(QILQR_ERR_INVALID_ARG, "obstacles: sphere " + std::to_string(j) + " has a non-finite value");
    if (!(sp[OB_RADIUS] > 0.0)) return fail(QILQR_ERR_INVALID_ARG, "obstacles: sphere " + std::to_string(j) + " has radius <= 0");
    if (!(sp[OB_WEIGHT] >= 0.0)) return fail(QILQR_ERR_INVALID_ARG, "obstacles: sphere " + std::to_string(j) + " has weight < 0");
  }
  if (count > 0 && s->f32)
    return fail(QILQR_ERR_INVALID_ARG, "obstacles need precision 0 (fp64): the mixed-precision kernels have no obstacle form");
  return QILQR_OK;
}
}  // namespace

static_assert(OB_MAX == QILQR_MAX_OBSTACLES, "obstacles.h and the C header agree on the table size");
int qilqr_set_obstacles(qilqr_solver *s, const double *spheres, int32_t count) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  int rc = check_obstacles(s, spheres, count);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));  // (no launch of this handle still reads the table)
  s->n_obstacles = 0;
  s->obstacles.assign(spheres, spheres + (size_t)count * OB_WORDS);
  if (count > 0) {
    if (!s->d_obstacles) HIP_TRY(hipMalloc((void **)&s->d_obstacles, sizeof(double) * OB_MAX * OB_WORDS));
    HIP_TRY(hipMemcpy(s->d_obstacles, spheres, sizeof(double) * (size_t)count * OB_WORDS, hipMemcpyHostToDevice));
    s->n_obstacles = count;
  }
  return QILQR_OK;
}

namespace {
// qilqr_set_batch_obstacles' checks of a table (obstacles.h, bob_check), shared with the sharded setter; the index is the batch's
int check_batch_obstacles(const qilqr_solver *s, const double *spheres, const int32_t *counts, int32_t B, int32_t K) {
  BobCheck e;
  if (bob_check(spheres, counts, B, K, QILQR_MAX_OBSTACLES, &e)) {
    std::string at;
    if (e.b >= 0) at = " (problem " + std::to_string(e.b) + (e.j >= 0 ? ", sphere " + std::to_string(e.j) : std::string()) + ")";
    return fail(QILQR_ERR_INVALID_ARG, std::string("batch obstacles: ") + e.why + at);
  }
  if (B > 0 && s->f32)
    return fail(QILQR_ERR_INVALID_ARG, "batch obstacles need precision 0 (fp64): the mixed-precision kernels have no obstacle form");
  return QILQR_OK;
}
}  // namespace

static_assert(OB_BWORDS == QILQR_OBSTACLE_WORDS, "obstacles.h and the C header agree on a per-problem sphere's words");
int qilqr_set_batch_obstacles(qilqr_solver *s, const double *spheres, const int32_t *counts, int32_t B, int32_t K) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  int rc = check_batch_obstacles(s, spheres, counts, B, K);
  if (rc) return rc;
  // the device layout and the counts on the host (the caller's rows re-laid once, here)
  std::vector<double> tab;
  std::vector<int32_t> cnt;
  int kmax = 0;
  bool moving = false;
  if (B > 0) {
    tab.resize((size_t)bob_count(B, K));
    bob_relayout(spheres, B, K, tab.data());
    cnt.resize((size_t)B);
    for (int32_t b = 0; b < B; ++b) {
      cnt[b] = counts ? counts[b] : K;
      kmax = std::max(kmax, (int)cnt[b]);
      for (int32_t j = 0; j < cnt[b]; ++j)
        for (int w = OB_BV; w < OB_BV + 3; ++w) moving = moving || spheres[((size_t)b * K + j) * OB_BWORDS + w] != 0.0;
    }
  }
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));  // (no launch of this handle still reads the table)
  s->pobs_B = 0;
  s->pobs_K = s->pobs_max = 0;
  s->pobs_moving = false;
  s->pobs_on_device = false;  // (the arrays below are this call's exact allocations: the device setter's capacities start again)
  s->pobs_cap = s->pobs_counts_cap = 0;
  if (s->d_pobs) (void)hipFree(s->d_pobs);
  if (s->d_pobs_counts) (void)hipFree(s->d_pobs_counts);
  s->d_pobs = nullptr;
  s->d_pobs_counts = nullptr;
  if (B > 0) {
    HIP_TRY(hipMalloc((void **)&s->d_pobs, sizeof(double) * tab.size()));
    HIP_TRY(hipMalloc((void **)&s->d_pobs_counts, sizeof(int32_t) * cnt.size()));
    HIP_TRY(hipMemcpy(s->d_pobs, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->d_pobs_counts, cnt.data(), sizeof(int32_t) * cnt.size(), hipMemcpyHostToDevice));
    s->pobs_B = B;
    s->pobs_K = K;
    s->pobs_max = kmax;
    s->pobs_moving = moving;
  }
  return QILQR_OK;
}

namespace {
// qilqr_set_state_weight_schedule's checks of what it is given (schedule.h, sched_check) and of the handle, shared with the sharded setter;
// *symmetric: every Q_i == Q_i^T exactly
int check_state_weight_schedule(const qilqr_solver *s, const double *Qs, int32_t n_knots, bool *symmetric) {
  SchedCheck e;
  if (sched_check(Qs, n_knots, &e)) {
    std::string at;
    if (e.knot >= 0) at = " (knot " + std::to_string(e.knot) + ", row " + std::to_string(e.row) + ", column " + std::to_string(e.col) + ")";
    return fail(QILQR_ERR_INVALID_ARG, std::string("state-weight schedule: ") + e.why + at);
  }
  *symmetric = e.symmetric;
  if (!Qs) {
    // (limits can be set on a handle whose own Q is not symmetric while a symmetric schedule stands in for it)
    if (s->limited && !s->own_symmetric)
      return fail(QILQR_ERR_INVALID_ARG, "state-weight schedule: control limits are set and the handle's own Q and R are not exactly symmetric: "
                                         "clear the limits before the schedule");
    return QILQR_OK;
  }
  if (s->f32)
    return fail(QILQR_ERR_INVALID_ARG, "state-weight schedule: needs precision 0 (fp64): the mixed-precision kernels have one Q");
  const char *why = nullptr;  // (qilqr_set_horizon_start keeps k0 < n_knots from its side)
  if (horizon_schedule_check(s->k0, n_knots, &why))
    return fail(QILQR_ERR_INVALID_ARG, std::string(why) + " (n_knots = " + std::to_string(n_knots) + ", horizon start " + std::to_string(s->k0) + ")");
  if (s->limited && !e.symmetric)
    return fail(QILQR_ERR_INVALID_ARG, "state-weight schedule: control limits are set and a Q_i is not exactly symmetric: the box form is the "
                                       "symmetric recursion");
  return QILQR_OK;
}
}  // namespace

int qilqr_set_state_weight_schedule(qilqr_solver *s, const double *Qs, int32_t n_knots) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  bool qsym = true;
  int rc = check_state_weight_schedule(s, Qs, n_knots, &qsym);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));  // (no launch of this handle still reads the table)
  // the records change shape with the schedule (the dense kind 0 while it is set, the kind of the handle's Q otherwise): the workspace is
  // rebuilt on the next call, as for qilqr_set_integrator
  const bool had = s->n_sched > 0;
  if (had || Qs) free_workspace(s);
  s->n_sched = 0;
  s->sched_symmetric = false;
  s->st.q_sched = nullptr;
  s->st.n_sched = 0;
  if (s->d_qsched) (void)hipFree(s->d_qsched);
  s->d_qsched = nullptr;
  s->symmetric = s->own_symmetric;
  s->q_diag = s->own_q_diag;
  s->layout = make_layout(s->own_layout_sym, s->own_layout_ur0, s->integrator == 1);
  if (Qs) {
    const size_t words = (size_t)n_knots * SCHED_WORDS;
    HIP_TRY(hipMalloc((void **)&s->d_qsched, sizeof(double) * words));
    const hipError_t up = hipMemcpy(s->d_qsched, Qs, sizeof(double) * words, hipMemcpyHostToDevice);
    if (up != hipSuccess) {  // (the handle stays cleared: no table is left behind for a later call to read)
      (void)hipFree(s->d_qsched);
      s->d_qsched = nullptr;
      return fail(QILQR_ERR_HIP, std::string("qilqr_set_state_weight_schedule: hipMemcpy: ") + hipGetErrorString(up));
    }
    bool rsym = true;
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < i; ++k) rsym = rsym && (s->consts.R[i * 4 + k] == s->consts.R[k * 4 + i]);
    s->n_sched = n_knots;
    s->sched_symmetric = qsym;
    s->symmetric = qsym && rsym && s->dev.force_general != 1;
    s->q_diag = false;
    s->layout = make_layout(false, false, s->integrator == 1);
  }
  return QILQR_OK;
}

namespace {
// qilqr_set_horizon_start's checks (horizon.h, horizon_start_check) and of the handle, shared with the sharded setter
int check_horizon_start(const qilqr_solver *s, int32_t k0) {
  const char *why = nullptr;
  if (horizon_start_check(k0, s->n_desired, s->n_sched, &why))
    return fail(QILQR_ERR_INVALID_ARG, std::string(why) + " (k0 = " + std::to_string(k0) + ", desired trajectory of " + std::to_string(s->n_desired) +
                                           " knots" + (s->n_sched > 0 ? ", schedule of " + std::to_string(s->n_sched) : std::string()) + ")");
  // (the fp32 shared desired trajectory has 72-byte rows: an odd start would move the row base off 16 bytes)
  if (k0 != 0 && s->f32) return fail(QILQR_ERR_INVALID_ARG, "horizon start: needs precision 0 (fp64)");
  return QILQR_OK;
}
}  // namespace

int qilqr_set_horizon_start(qilqr_solver *s, int32_t k0) {
  if (!s) return fail(QILQR_ERR_INVALID_ARG, "null solver");
  const int rc = check_horizon_start(s, k0);
  if (rc) return rc;
  // (begin_batch reads it when the next call starts; launches in flight have their pointers already: nothing to wait for)
  s->k0 = k0;
  return QILQR_OK;
}

int qilqr_profile_get(qilqr_solver *s, qilqr_profile *out) {
  if (!s || !out) return fail(QILQR_ERR_INVALID_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  drain_events(s);
  out->backward_ms = s->prof_ms[K_BACKWARD];
  out->backward_launches = s->prof_n[K_BACKWARD];
  out->rollout_ms = s->prof_ms[K_ROLLOUT];
  out->rollout_launches = s->prof_n[K_ROLLOUT];
  out->linearize_ms = s->prof_ms[K_LINEARIZE];
  out->linearize_launches = s->prof_n[K_LINEARIZE];
  out->other_ms = s->prof_ms[K_OTHER];
  out->other_launches = s->prof_n[K_OTHER];
  out->backward_seen = (int32_t)s->prof_seen[K_BACKWARD];
  out->rollout_seen = (int32_t)s->prof_seen[K_ROLLOUT];
  out->linearize_seen = (int32_t)s->prof_seen[K_LINEARIZE];
  out->other_seen = (int32_t)s->prof_seen[K_OTHER];
  out->solve_ms = s->prof_ms[K_SOLVE];
  out->solve_launches = s->prof_n[K_SOLVE];
  out->solve_seen = (int32_t)s->prof_seen[K_SOLVE];
  return QILQR_OK;
}
}  // extern "C"
