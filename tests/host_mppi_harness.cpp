// host_mppi_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the per-lane routines
// of the sampling planner (quadrotorilqr_amd/csrc/mppi_kernels.h: mppi_eps_row, mppi_sample, the folds and combinations of the update) and
// the rule of what its calls refuse (mppi_launch.h: mppi_refusal) compiled with g++, for tests/test_mppi_cpu.py and tests/test_gpu_mppi.py.
// The update runs the block's lanes one after the other: every lane's fold is the library's text, the butterfly 32 .. 1 and the
// wavefronts in index order are spelled out here over arrays where the kernel has shuffles and LDS.
//
//   host_mppi_harness fly IN OUT      OUT: score (B S 4) | eps as drawn (B S n 4)
//   host_mppi_harness update IN OUT   OUT: out_plan (B n 18) | info (B 8); IN carries the scores
//       IN, a file of doubles: a header of 28 words
//           B n S integrator limited modeled dt has_x0 has_desired n_sched k0 n_des n_shared own_K b0 flags seed_lo seed_hi tau_s lambda
//           collision_cost sigma[4] has_score 0 0
//       | qilqr_model (13) | Q (144) | R (16) | lo (4) | hi (4) | models (B x 13, only when modeled) | plan (B n 18) | x0 (B 13, only when
//       has_x0) | desired per plan (B n 18, only when has_desired) | the handle's desired trajectory (n_des 18) | the schedule (n_sched 144) |
//       shared spheres (n_shared 5) | per-problem spheres (B own_K 8) | their counts (B, only when own_K) | score (B S 4, only when has_score)
//       The handle's facts are applied as the library applies them: desired[k0 + i] and Qs[k0 + i] for knot i, row b of the per-problem
//       table, model b for plan b.
//   host_mppi_harness refuse update rule sigma0 sigma1 sigma2 sigma3 tau_s lambda collision_cost flags reserved plan x0 desired score out_plan
//                            info B n S b0 handle f32 modeled models_B pobs_B n_desired n_sched k0
//       (addresses and integers in decimal, the doubles as strtod reads them) prints the reason, or "ok"; a reason of length is prefixed
//       with "length: "
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"
#include "../quadrotorilqr_amd/csrc/mppi_kernels.h"
#include "../quadrotorilqr_amd/csrc/mppi_launch.h"

using namespace qilqr;

namespace {

struct Case {
  int B, n, S, integ, own_K, n_shared, b0;
  bool limited;
  uint32_t flags;
  uint64_t seed;
  double lambda, collision_cost;
  MppiCoeffs m;
  const double *tab, *plan, *x0, *desired, *q, *shared, *own, *counts, *lo, *hi, *score;
  long desired_step, q_step;
};

// one sample of plan b over `plan` (the case's, or the update's new one)
void fly_one(const ModelConsts<double> &c, const Case &k, int b, int j, bool nominal, const double *plan, double *score, double *traj) {
  const ModelConsts<double> mdl = k.tab ? problem_model(c, BatchModels{k.tab}, (long)b) : c;
  MppiFlatFetch fetch{plan, k.desired + (long)b * k.desired_step, k.q, k.q_step};
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
  if (k.integ == 1 && k.limited) mppi_sample<1, true>(mdl, k.m, fetch, s, k.lo, k.hi);
  else if (k.integ == 1) mppi_sample<1, false>(mdl, k.m, fetch, s);
  else if (k.limited) mppi_sample<0, true>(mdl, k.m, fetch, s, k.lo, k.hi);
  else mppi_sample<0, false>(mdl, k.m, fetch, s);
}

void run_fly(const ModelConsts<double> &c, const Case &k, std::vector<double> &out) {
  const size_t samples = (size_t)k.B * k.S;
  out.assign(samples * 4 + samples * k.n * 4, std::nan(""));
  double *score = out.data(), *eps = score + samples * 4;
  for (int b = 0; b < k.B; ++b)
    for (int j = 0; j < k.S; ++j) {
      const size_t row = (size_t)b * k.S + j;
      fly_one(c, k, b, j, false, k.plan + (long)b * k.n * 18, score + row * 4, nullptr);
      double g[4] = {0.0, 0.0, 0.0, 0.0};
      for (int i = 0; i < k.n; ++i) {
        mppi_eps_row(k.m, k.seed, (uint32_t)(k.b0 + b), (uint32_t)j, (uint32_t)i, mppi_is_nominal(k.flags, j), g);
        for (int a = 0; a < 4; ++a) eps[(row * k.n + i) * 4 + a] = g[a];
      }
    }
}

// the butterfly 32, 16, 8, 4, 2, 1 inside every wavefront of v[0 .. T): v[l] <- combine(v[l], v[l ^ off]), all lanes at once
template <typename V, typename Combine>
void butterfly(std::vector<V> &v, Combine combine) {
  for (int off = 32; off >= 1; off >>= 1) {
    std::vector<V> from(v);
    for (size_t l = 0; l < v.size(); ++l) v[l] = combine(from[l], from[l ^ (size_t)off]);
  }
}

void run_update(const ModelConsts<double> &c, const Case &k, std::vector<double> &out) {
  const int S = k.S, n = k.n, T = mppi_update_threads(S), W = T / 64;
  out.assign((size_t)k.B * n * 18 + (size_t)k.B * 8, std::nan(""));
  double *out_plan = out.data(), *info = out_plan + (size_t)k.B * n * 18;
  auto add = [](double a, double b) { return a + b; };
  for (int b = 0; b < k.B; ++b) {
    const double *plan = k.plan + (long)b * n * 18, *mine = k.score + 4 * (long)b * S;
    double *op = out_plan + (long)b * n * 18;
    for (int i = 0; i < n; ++i)
      for (int w = 0; w < 14; ++w) op[i * 18 + w] = plan[i * 18 + w];
    std::vector<MppiMin> lanes(T);
    for (int t = 0; t < T; ++t) lanes[t] = mppi_lane_min(mine, S, t, T, k.collision_cost);
    butterfly(lanes, [](const MppiMin &a, const MppiMin &b2) { return mppi_min_combine(a, b2); });
    MppiMin f = lanes[0];
    for (int w = 1; w < W; ++w) f = mppi_min_combine(f, lanes[64 * w]);
    const bool any = f.j >= 0;
    std::vector<double> weights(S);
    for (int j = 0; j < S; ++j) weights[j] = any ? mppi_weight(mppi_key(mine + 4 * (long)j, k.collision_cost), f.key, k.lambda) : 0.0;
    std::vector<double> le(T), lq(T), we(W), wq(W);
    for (int t = 0; t < T; ++t) mppi_lane_weights(weights.data(), S, t, T, le[t], lq[t]);
    butterfly(le, add);
    butterfly(lq, add);
    for (int w = 0; w < W; ++w) { we[w] = le[64 * w]; wq[w] = lq[64 * w]; }
    const double eta = mppi_waves_in_order(we.data(), W, 1), q = mppi_waves_in_order(wq.data(), W, 1);
    mppi_info_words(f, eta, q, info + 8 * (long)b);
    std::vector<double> g((size_t)S * 4, 0.0), part((size_t)W * 4);
    std::vector<double> acc[4];
    for (int i = 0; i < n; ++i) {
      for (int r = 0; r < 4; ++r) acc[r].assign(T, 0.0);
      for (int t = 0; t < T; ++t) {
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = t; j < S; j += T) {
          mppi_eps_row(k.m, k.seed, (uint32_t)(k.b0 + b), (uint32_t)j, (uint32_t)i, mppi_is_nominal(k.flags, j), &g[(size_t)j * 4]);
          mppi_fold_term(weights[j], &g[(size_t)j * 4], a4);
        }
        for (int r = 0; r < 4; ++r) acc[r][t] = a4[r];
      }
      for (int r = 0; r < 4; ++r) {
        butterfly(acc[r], add);
        for (int w = 0; w < W; ++w) part[(size_t)w * 4 + r] = acc[r][64 * w];
      }
      for (int r = 0; r < 4; ++r) {
        const double d = mppi_waves_in_order(&part[r], W, 4);
        op[i * 18 + 14 + r] = mppi_new_control(plan[i * 18 + 14 + r], d, eta, any, k.limited, k.limited ? k.lo[r] : 0.0, k.limited ? k.hi[r] : 0.0);
      }
    }
    // the new plan's own flight: its states over out_plan, its score into words 4 .. 7 of info
    fly_one(c, k, b, 0, true, op, info + 8 * (long)b + 4, op);
  }
}

int run_case(const char *mode, const char *in_path, const char *out_path) {
  FILE *f = std::fopen(in_path, "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double));
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
  std::fclose(f);
  if (in.size() < 28) return 3;
  Case k{};
  k.B = (int)in[0]; k.n = (int)in[1]; k.S = (int)in[2]; k.integ = (int)in[3];
  k.limited = in[4] != 0.0;
  const bool modeled = in[5] != 0.0;
  const double dt = in[6];
  const bool has_x0 = in[7] != 0.0, has_desired = in[8] != 0.0;
  const int n_sched = (int)in[9], k0 = (int)in[10], n_des = (int)in[11];
  k.n_shared = (int)in[12]; k.own_K = (int)in[13]; k.b0 = (int)in[14];
  k.flags = (uint32_t)in[15];
  k.seed = (uint64_t)in[16] | ((uint64_t)in[17] << 32);
  const double tau_s = in[18];
  k.lambda = in[19]; k.collision_cost = in[20];
  const double sigma[4] = {in[21], in[22], in[23], in[24]};
  const bool has_score = in[25] != 0.0, update = !std::strcmp(mode, "update");
  if (k.B <= 0 || k.n < 2 || k.S <= 0 || k.S > MPPI_MAX_SAMPLES || k.n_shared > OB_MAX || k.own_K > OB_MAX || (update && !has_score)) return 3;
  if ((!has_desired && k0 + k.n - 1 >= n_des) || (n_sched > 0 && k0 + k.n - 1 >= n_sched)) return 3;
  static_assert(sizeof(qilqr_model) == 13 * sizeof(double), "qilqr_model is 13 doubles");
  static_assert(sizeof(qilqr_mppi_rule) == 64, "qilqr_mppi_rule is 64 bytes");
  const size_t B = (size_t)k.B, n = (size_t)k.n, S = (size_t)k.S;
  const size_t want = 28 + 13 + 144 + 16 + 8 + (modeled ? B * 13 : 0) + B * n * 18 + (has_x0 ? B * 13 : 0) + (has_desired ? B * n * 18 : 0) +
                      (size_t)n_des * 18 + (size_t)n_sched * 144 + (size_t)k.n_shared * 5 + B * k.own_K * 8 + (k.own_K ? B : 0) + (has_score ? B * S * 4 : 0);
  if (in.size() != want) return 3;
  const double *p = in.data() + 28;
  qilqr_model model;
  std::memcpy(&model, p, sizeof model);
  p += 13;
  const double *Q = p, *R = p + 144;
  k.lo = p + 160; k.hi = p + 164;
  p += 168;
  ModelConsts<double> c;
  if (!make_model_consts(model.mass_kg, model.inertia, model.arm_length_m, model.torque_to_thrust_ratio_m, model.g_mpss, Q, R, dt, &c)) return 4;
  std::vector<double> tab;
  if (modeled) {
    std::vector<qilqr_model> models(B);
    std::memcpy(models.data(), p, B * sizeof(qilqr_model));
    p += B * 13;
    tab.resize(B * PM_WORDS);
    if (make_model_table(models.data(), (long)B, Q, R, dt, tab.data()) != -1) return 4;
  }
  k.tab = modeled ? tab.data() : nullptr;
  k.plan = p; p += B * n * 18;
  k.x0 = has_x0 ? p : nullptr; p += has_x0 ? B * 13 : 0;
  const double *per_plan = has_desired ? p : nullptr; p += has_desired ? B * n * 18 : 0;
  const double *handle_desired = p; p += (size_t)n_des * 18;
  const double *sched = n_sched ? p : nullptr; p += (size_t)n_sched * 144;
  k.shared = k.n_shared ? p : nullptr; p += (size_t)k.n_shared * 5;
  k.own = k.own_K ? p : nullptr; p += B * k.own_K * 8;
  k.counts = k.own_K ? p : nullptr; p += k.own_K ? B : 0;
  k.score = has_score ? p : nullptr;
  k.desired = per_plan ? per_plan : handle_desired + 18 * (size_t)k0;
  k.desired_step = per_plan ? 18l * k.n : 0;
  k.q = sched ? sched + 144 * (size_t)k0 : Q;
  k.q_step = sched ? 144 : 0;
  mppi_coeffs(sigma, tau_s, dt, k.m);
  std::vector<double> out;
  if (update) run_update(c, k, out);
  else run_fly(c, k, out);
  f = std::fopen(out_path, "wb");
  if (!f) return 2;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}

int run_refuse(char **a) {
  auto ptr = [](const char *s) { return (const void *)(uintptr_t)std::strtoull(s, nullptr, 10); };
  auto num = [](const char *s) { return std::strtod(s, nullptr); };
  MppiCall c{};
  c.update = std::atoi(a[0]) != 0;
  c.rule = std::atoi(a[1]) != 0;
  for (int r = 0; r < 4; ++r) c.sigma[r] = num(a[2 + r]);
  c.tau_s = num(a[6]); c.lambda = num(a[7]); c.collision_cost = num(a[8]);
  c.flags = std::strtoul(a[9], nullptr, 10); c.reserved = std::strtoul(a[10], nullptr, 10);
  c.plan = ptr(a[11]); c.x0 = ptr(a[12]); c.desired = ptr(a[13]); c.score = ptr(a[14]); c.out_plan = ptr(a[15]); c.info = ptr(a[16]);
  c.B = std::atol(a[17]); c.n = std::atol(a[18]); c.S = std::atol(a[19]); c.b0 = std::atol(a[20]);
  c.handle = std::atoi(a[21]) != 0; c.f32 = std::atoi(a[22]) != 0; c.modeled = std::atoi(a[23]) != 0;
  c.models_B = std::atol(a[24]); c.pobs_B = std::atol(a[25]); c.n_desired = std::atol(a[26]); c.n_sched = std::atol(a[27]); c.k0 = std::atol(a[28]);
  bool length = false;
  const char *why = mppi_refusal(c, &length);
  std::printf("%s%s\n", length ? "length: " : "", why ? why : "ok");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && (!std::strcmp(argv[1], "fly") || !std::strcmp(argv[1], "update"))) return run_case(argv[1], argv[2], argv[3]);
  if (argc == 31 && !std::strcmp(argv[1], "refuse")) return run_refuse(argv + 2);
  if (argc == 3 && !std::strcmp(argv[1], "grid")) {
    const long S = std::atol(argv[2]);
    std::printf("%ld %d %d %d\n", mppi_flight_blocks(1, S), mppi_update_lanes(S), mppi_samples_per_lane(S), mppi_update_threads((int)S));
    return 0;
  }
  std::fprintf(stderr, "usage: %s fly IN OUT | update IN OUT | grid S | refuse update rule sigma0 sigma1 sigma2 sigma3 tau_s lambda collision_cost flags "
                       "reserved plan x0 desired score out_plan info B n S b0 handle f32 modeled models_B pobs_B n_desired n_sched k0\n", argv[0]);
  return 1;
}
