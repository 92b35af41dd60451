// host_mppi_common.h -- what the two host programs of the sampling planner share (tests only): tests/host_mppi_harness.cpp and
// tests/host_mppi_adapt_harness.cpp.  The case file's reader, one sample's record and flight, the butterfly, the head of the update spelled
// out over arrays (lanes' minima, weights, eta, q, the info words -- the host's side of the head of k_mppi_update and k_mppi_adapt) and the parser of
// the refusal's common words.  Each program keeps its own fold of the per-knot moments and its own output layout.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"
#include "../quadrotorilqr_amd/csrc/mppi_kernels.h"
#include "../quadrotorilqr_amd/csrc/mppi_launch.h"

namespace qilqr {

struct MppiCase {
  int B, n, S, integ, own_K, n_shared, b0;
  bool limited;
  uint32_t flags;
  uint64_t seed;
  double lambda, collision_cost;
  MppiCoeffs m;  // the program's to fill: the rule's, or the unit recursion's
  const double *tab, *plan, *x0, *desired, *q, *shared, *own, *counts, *lo, *hi, *score;
  long desired_step, q_step;
};

// a case file in memory: the words a case points into, the model, and what of the header is not the case's
struct MppiCaseFile {
  std::vector<double> in, tab;
  ModelConsts<double> c;
  double dt, tau_s, sigma[4];
  const double *tail;  // the words behind host_mppi_harness's layout
};

// IN of host_mppi_harness.cpp, followed by B n tail_per_knot + tail_fixed words (file.tail); 0, or the program's exit code
inline int mppi_read_case(const char *in_path, bool needs_score, size_t tail_per_knot, size_t tail_fixed, MppiCase &k, MppiCaseFile &file) {
  FILE *f = std::fopen(in_path, "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> &in = file.in;
  in.resize((size_t)bytes / sizeof(double));
  const bool whole = std::fread(in.data(), sizeof(double), in.size(), f) == in.size();
  std::fclose(f);
  if (!whole) return 2;
  if (in.size() < 28) return 3;
  k.B = (int)in[0]; k.n = (int)in[1]; k.S = (int)in[2]; k.integ = (int)in[3];
  k.limited = in[4] != 0.0;
  const bool modeled = in[5] != 0.0;
  const double dt = file.dt = in[6];
  const bool has_x0 = in[7] != 0.0, has_desired = in[8] != 0.0;
  const int n_sched = (int)in[9], k0 = (int)in[10], n_des = (int)in[11];
  k.n_shared = (int)in[12]; k.own_K = (int)in[13]; k.b0 = (int)in[14];
  k.flags = (uint32_t)in[15];
  k.seed = (uint64_t)in[16] | ((uint64_t)in[17] << 32);
  file.tau_s = in[18];
  k.lambda = in[19]; k.collision_cost = in[20];
  for (int a = 0; a < 4; ++a) file.sigma[a] = in[21 + a];
  const bool has_score = in[25] != 0.0;
  if (k.B <= 0 || k.n < 2 || k.S <= 0 || k.S > MPPI_MAX_SAMPLES || k.n_shared > OB_MAX || k.own_K > OB_MAX || (needs_score && !has_score)) return 3;
  if ((!has_desired && k0 + k.n - 1 >= n_des) || (n_sched > 0 && k0 + k.n - 1 >= n_sched)) return 3;
  static_assert(sizeof(qilqr_model) == 13 * sizeof(double), "qilqr_model is 13 doubles");
  const size_t B = (size_t)k.B, n = (size_t)k.n, S = (size_t)k.S;
  const size_t want = 28 + 13 + 144 + 16 + 8 + (modeled ? B * 13 : 0) + B * n * 18 + (has_x0 ? B * 13 : 0) + (has_desired ? B * n * 18 : 0) +
                      (size_t)n_des * 18 + (size_t)n_sched * 144 + (size_t)k.n_shared * 5 + B * k.own_K * 8 + (k.own_K ? B : 0) + (has_score ? B * S * 4 : 0) +
                      B * n * tail_per_knot + tail_fixed;
  if (in.size() != want) return 3;
  const double *p = in.data() + 28;
  qilqr_model model;
  std::memcpy(&model, p, sizeof model);
  p += 13;
  const double *Q = p, *R = p + 144;
  k.lo = p + 160; k.hi = p + 164;
  p += 168;
  if (!make_model_consts(model.mass_kg, model.inertia, model.arm_length_m, model.torque_to_thrust_ratio_m, model.g_mpss, Q, R, dt, &file.c)) return 4;
  if (modeled) {
    std::vector<qilqr_model> models(B);
    std::memcpy(models.data(), p, B * sizeof(qilqr_model));
    p += B * 13;
    file.tab.resize(B * PM_WORDS);
    if (make_model_table(models.data(), (long)B, Q, R, dt, file.tab.data()) != -1) return 4;
  }
  k.tab = modeled ? file.tab.data() : nullptr;
  k.plan = p; p += B * n * 18;
  k.x0 = has_x0 ? p : nullptr; p += has_x0 ? B * 13 : 0;
  const double *per_plan = has_desired ? p : nullptr; p += has_desired ? B * n * 18 : 0;
  const double *handle_desired = p; p += (size_t)n_des * 18;
  const double *sched = n_sched ? p : nullptr; p += (size_t)n_sched * 144;
  k.shared = k.n_shared ? p : nullptr; p += (size_t)k.n_shared * 5;
  k.own = k.own_K ? p : nullptr; p += B * k.own_K * 8;
  k.counts = k.own_K ? p : nullptr; p += k.own_K ? B : 0;
  k.score = has_score ? p : nullptr; p += has_score ? B * S * 4 : 0;
  file.tail = p;
  k.desired = per_plan ? per_plan : handle_desired + 18 * (size_t)k0;
  k.desired_step = per_plan ? 18l * k.n : 0;
  k.q = sched ? sched + 144 * (size_t)k0 : Q;
  k.q_step = sched ? 144 : 0;
  return 0;
}
inline int mppi_write_out(const char *out_path, const std::vector<double> &out) {
  FILE *f = std::fopen(out_path, "wb");
  if (!f) return 2;
  const bool whole = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  std::fclose(f);
  return whole ? 0 : 2;
}

// plan b's model, and the record of its sample j
inline ModelConsts<double> mppi_host_model(const ModelConsts<double> &c, const MppiCase &k, int b) {
  return k.tab ? problem_model(c, BatchModels{k.tab}, (long)b) : c;
}
inline MppiSample mppi_host_sample(const MppiCase &k, int b, int j, bool nominal, double *score, double *traj) {
  MppiSample s;
  s.x0 = k.x0 ? k.x0 + (long)b * 13 : k.plan + (long)b * k.n * 18 + 1;
  s.n = k.n;
  s.seed = k.seed;
  s.plan = (uint32_t)(k.b0 + b);
  s.sample = (uint32_t)j;
  s.nominal = nominal || mppi_is_nominal(k.flags, j);
  // (the per-problem spheres in the caller's layout: a row of K spheres of OB_BWORDS consecutive words)
  s.spheres = ClSpheres{k.shared, k.n_shared, k.own ? k.own + (long)b * k.own_K * OB_BWORDS : nullptr, k.own ? (int)k.counts[b] : 0, 1, OB_BWORDS};
  s.score = score;
  s.traj = traj;
  return s;
}
// mppi_sample by the case's integrator and limits
template <typename Fetch>
void mppi_host_fly(const ModelConsts<double> &mdl, const MppiCase &k, Fetch &fetch, const MppiSample &s) {
  if (k.integ == 1 && k.limited) mppi_sample<1, true>(mdl, k.m, fetch, s, k.lo, k.hi);
  else if (k.integ == 1) mppi_sample<1, false>(mdl, k.m, fetch, s);
  else if (k.limited) mppi_sample<0, true>(mdl, k.m, fetch, s, k.lo, k.hi);
  else mppi_sample<0, false>(mdl, k.m, fetch, s);
}

// the butterfly 32, 16, 8, 4, 2, 1 inside every wavefront of v[0 .. T): v[l] <- combine(v[l], v[l ^ off]), all lanes at once
template <typename V, typename Combine>
void butterfly(std::vector<V> &v, Combine combine) {
  for (int off = 32; off >= 1; off >>= 1) {
    std::vector<V> from(v);
    for (size_t l = 0; l < v.size(); ++l) v[l] = combine(from[l], from[l ^ (size_t)off]);
  }
}
inline double add(double a, double b) { return a + b; }

// The head of the update of plan b by T = mppi_update_lanes(S) lanes, one after the other: time and states copied to op (the plan's rows
// of out_plan), J_min, the weights, eta and q, and words 0 .. 3 of info (the plan's eight)
struct MppiHostHead {
  bool any;
  double eta;
  std::vector<double> weights;
};
inline MppiHostHead mppi_host_head(const MppiCase &k, int b, double *op, double *info) {
  const int S = k.S, n = k.n, T = mppi_update_lanes(S), W = T / 64;
  const double *plan = k.plan + (long)b * n * 18, *mine = k.score + 4 * (long)b * S;
  for (int i = 0; i < n; ++i)
    for (int w = 0; w < 14; ++w) op[i * 18 + w] = plan[i * 18 + w];
  std::vector<MppiMin> lanes(T);
  for (int t = 0; t < T; ++t) lanes[t] = mppi_lane_min(mine, S, t, T, k.collision_cost);
  butterfly(lanes, [](const MppiMin &a, const MppiMin &b2) { return mppi_min_combine(a, b2); });
  MppiMin f = lanes[0];
  for (int w = 1; w < W; ++w) f = mppi_min_combine(f, lanes[64 * w]);
  MppiHostHead h{f.j >= 0, 0.0, std::vector<double>(S)};
  for (int j = 0; j < S; ++j) h.weights[j] = h.any ? mppi_weight(mppi_key(mine + 4 * (long)j, k.collision_cost), f.key, k.lambda) : 0.0;
  std::vector<double> le(T), lq(T), we(W), wq(W);
  for (int t = 0; t < T; ++t) mppi_lane_weights(h.weights.data(), S, t, T, le[t], lq[t]);
  butterfly(le, add);
  butterfly(lq, add);
  for (int w = 0; w < W; ++w) { we[w] = le[64 * w]; wq[w] = lq[64 * w]; }
  h.eta = mppi_waves_in_order(we.data(), W, 1);
  mppi_info_words(f, h.eta, mppi_waves_in_order(wq.data(), W, 1), info);
  return h;
}

// the 29 words of host_mppi_harness's refuse
inline void mppi_parse_call(char **a, MppiCall &c) {
  auto ptr = [](const char *s) { return (const void *)(uintptr_t)std::strtoull(s, nullptr, 10); };
  auto num = [](const char *s) { return std::strtod(s, nullptr); };
  c.update = std::atoi(a[0]) != 0;
  c.rule = std::atoi(a[1]) != 0;
  for (int r = 0; r < 4; ++r) c.sigma[r] = num(a[2 + r]);
  c.tau_s = num(a[6]); c.lambda = num(a[7]); c.collision_cost = num(a[8]);
  c.flags = std::strtoul(a[9], nullptr, 10); c.reserved = std::strtoul(a[10], nullptr, 10);
  c.plan = ptr(a[11]); c.x0 = ptr(a[12]); c.desired = ptr(a[13]); c.score = ptr(a[14]); c.out_plan = ptr(a[15]); c.info = ptr(a[16]);
  c.B = std::atol(a[17]); c.n = std::atol(a[18]); c.S = std::atol(a[19]); c.b0 = std::atol(a[20]);
  c.handle = std::atoi(a[21]) != 0; c.f32 = std::atoi(a[22]) != 0; c.modeled = std::atoi(a[23]) != 0;
  c.models_B = std::atol(a[24]); c.pobs_B = std::atol(a[25]); c.n_desired = std::atol(a[26]); c.n_sched = std::atol(a[27]); c.k0 = std::atol(a[28]);
}

}  // namespace qilqr
