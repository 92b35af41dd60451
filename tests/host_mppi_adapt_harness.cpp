// host_mppi_adapt_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the per-lane
// routines of the planner's adapted spread (quadrotorilqr_amd/csrc/mppi_adapt_kernels.h: mppi_spread_eps, mppi_sample over a fetch with a
// spread, the folds of the two moments, mppi_weighted_var, mppi_blend_spread) and the rule of what its calls refuse
// (mppi_adapt_launch.h: mppi_spread_refusal) compiled with g++, for tests/test_mppi_adapt_cpu.py and tests/test_gpu_mppi_adapt.py.
// As tests/host_mppi_harness.cpp, the adaptation runs the block's lanes one after the other: every lane's fold is the library's text,
// the butterfly 32 .. 1 and the wavefronts in index order are spelled out here.
//
//   host_mppi_adapt_harness fly IN OUT     OUT: score (B S 4) | eps as flown (B S n 4)
//   host_mppi_adapt_harness adapt IN OUT   OUT: out_plan (B n 18) | info (B 8) | out_spread (B n 4) | the weighted variances (B n 4)
//       IN: the file of tests/host_mppi_harness.cpp (its header's sigma is not read), followed by
//           spread (B n 4) | floor (4) | cap (4) | rate
//   host_mppi_adapt_harness refuse <the 29 words of host_mppi_harness's refuse> adapt floor0 cap0 rate reserved spread out_spread
//       (floor0 / cap0: of rotor 0, the others are 0.1 and 1; reserved: word 1) prints the reason, or "ok"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"
#include "../quadrotorilqr_amd/csrc/mppi_adapt_kernels.h"
#include "../quadrotorilqr_amd/csrc/mppi_adapt_launch.h"

using namespace qilqr;

namespace {

struct Case {
  int B, n, S, integ, own_K, n_shared, b0;
  bool limited;
  uint32_t flags;
  uint64_t seed;
  double lambda, collision_cost;
  MppiCoeffs m;  // the unit recursion's
  MppiAdaptCoeffs k;
  const double *tab, *plan, *x0, *desired, *q, *shared, *own, *counts, *lo, *hi, *score, *spread;
  long desired_step, q_step;
};

// one sample of plan b over `plan`; spread: plan b's rows, or null for the nominal flight of a new plan (mppi.hip's)
void fly_one(const ModelConsts<double> &c, const Case &k, int b, int j, bool nominal, const double *plan, double *score, double *traj) {
  const ModelConsts<double> mdl = k.tab ? problem_model(c, BatchModels{k.tab}, (long)b) : c;
  MppiFlatSpreadFetch fetch{{plan, k.desired + (long)b * k.desired_step, k.q, k.q_step}, k.spread + 4 * (long)b * k.n};
  MppiSample s;
  s.x0 = k.x0 ? k.x0 + (long)b * 13 : k.plan + (long)b * k.n * 18 + 1;
  s.n = k.n;
  s.seed = k.seed;
  s.plan = (uint32_t)(k.b0 + b);
  s.sample = (uint32_t)j;
  s.nominal = nominal || mppi_is_nominal(k.flags, j);
  s.spheres = ClSpheres{k.shared, k.n_shared, k.own ? k.own + (long)b * k.own_K * OB_BWORDS : nullptr, k.own ? (int)k.counts[b] : 0, 1, OB_BWORDS};
  s.score = score;
  s.traj = traj;
  if (nominal) {  // the library's second launch is k_mppi_flight: no spread is read
    MppiFlatFetch plain = fetch;
    if (k.integ == 1 && k.limited) mppi_sample<1, true>(mdl, k.m, plain, s, k.lo, k.hi);
    else if (k.integ == 1) mppi_sample<1, false>(mdl, k.m, plain, s);
    else if (k.limited) mppi_sample<0, true>(mdl, k.m, plain, s, k.lo, k.hi);
    else mppi_sample<0, false>(mdl, k.m, plain, s);
    return;
  }
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
        const bool nominal = mppi_is_nominal(k.flags, j);
        mppi_eps_row(k.m, k.seed, (uint32_t)(k.b0 + b), (uint32_t)j, (uint32_t)i, nominal, g);
        mppi_spread_eps(k.spread + 4 * ((long)b * k.n + i), g, nominal, &eps[(row * k.n + i) * 4]);
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

void run_adapt(const ModelConsts<double> &c, const Case &k, std::vector<double> &out) {
  const int S = k.S, n = k.n, T = mppi_update_threads(S), W = T / 64;
  const size_t knots = (size_t)k.B * n;
  out.assign(knots * 18 + (size_t)k.B * 8 + knots * 4 + knots * 4, std::nan(""));
  double *out_plan = out.data(), *info = out_plan + knots * 18, *out_spread = info + (size_t)k.B * 8, *out_var = out_spread + knots * 4;
  auto add = [](double a, double b) { return a + b; };
  for (int b = 0; b < k.B; ++b) {
    const double *plan = k.plan + (long)b * n * 18, *mine = k.score + 4 * (long)b * S, *spread = k.spread + 4 * (long)b * n;
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
    std::vector<double> g((size_t)S * 4, 0.0), part((size_t)W * 4), part2((size_t)W * 4);
    std::vector<double> acc[4], acc2[4];
    for (int i = 0; i < n; ++i) {
      for (int r = 0; r < 4; ++r) { acc[r].assign(T, 0.0); acc2[r].assign(T, 0.0); }
      for (int t = 0; t < T; ++t) {
        double a4[4] = {0.0, 0.0, 0.0, 0.0}, b4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = t; j < S; j += T) {
          const bool nominal = mppi_is_nominal(k.flags, j);
          mppi_eps_row(k.m, k.seed, (uint32_t)(k.b0 + b), (uint32_t)j, (uint32_t)i, nominal, &g[(size_t)j * 4]);
          double e[4];
          mppi_spread_eps(spread + 4 * (long)i, &g[(size_t)j * 4], nominal, e);
          mppi_fold_moments(weights[j], e, a4, b4);
        }
        for (int r = 0; r < 4; ++r) { acc[r][t] = a4[r]; acc2[r][t] = b4[r]; }
      }
      for (int r = 0; r < 4; ++r) {
        butterfly(acc[r], add);
        butterfly(acc2[r], add);
        for (int w = 0; w < W; ++w) { part[(size_t)w * 4 + r] = acc[r][64 * w]; part2[(size_t)w * 4 + r] = acc2[r][64 * w]; }
      }
      for (int r = 0; r < 4; ++r) {
        const double d = mppi_waves_in_order(&part[r], W, 4), d2 = mppi_waves_in_order(&part2[r], W, 4);
        op[i * 18 + 14 + r] = mppi_new_control(plan[i * 18 + 14 + r], d, eta, any, k.limited, k.limited ? k.lo[r] : 0.0, k.limited ? k.hi[r] : 0.0);
        const double var = any ? mppi_weighted_var(d, d2, eta) : 0.0;
        const size_t ws = ((size_t)b * n + i) * 4 + r;
        out_var[ws] = var;
        out_spread[ws] = mppi_blend_spread(spread[4 * i + r], var, any, k.k.one_minus_rate, k.k.rate, k.k.floor[r], k.k.cap[r]);
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
  const bool has_score = in[25] != 0.0, adapt = !std::strcmp(mode, "adapt");
  if (k.B <= 0 || k.n < 2 || k.S <= 0 || k.S > MPPI_MAX_SAMPLES || k.n_shared > OB_MAX || k.own_K > OB_MAX || (adapt && !has_score)) return 3;
  if ((!has_desired && k0 + k.n - 1 >= n_des) || (n_sched > 0 && k0 + k.n - 1 >= n_sched)) return 3;
  static_assert(sizeof(qilqr_model) == 13 * sizeof(double), "qilqr_model is 13 doubles");
  static_assert(sizeof(qilqr_mppi_adapt_rule) == 96, "qilqr_mppi_adapt_rule is 96 bytes");
  const size_t B = (size_t)k.B, n = (size_t)k.n, S = (size_t)k.S;
  const size_t want = 28 + 13 + 144 + 16 + 8 + (modeled ? B * 13 : 0) + B * n * 18 + (has_x0 ? B * 13 : 0) + (has_desired ? B * n * 18 : 0) +
                      (size_t)n_des * 18 + (size_t)n_sched * 144 + (size_t)k.n_shared * 5 + B * k.own_K * 8 + (k.own_K ? B : 0) + (has_score ? B * S * 4 : 0) +
                      B * n * 4 + 9;
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
  k.score = has_score ? p : nullptr; p += has_score ? B * S * 4 : 0;
  k.spread = p; p += B * n * 4;
  mppi_adapt_coeffs(p, p + 4, p[8], k.k);
  k.desired = per_plan ? per_plan : handle_desired + 18 * (size_t)k0;
  k.desired_step = per_plan ? 18l * k.n : 0;
  k.q = sched ? sched + 144 * (size_t)k0 : Q;
  k.q_step = sched ? 144 : 0;
  mppi_unit_coeffs(tau_s, dt, k.m);
  std::vector<double> out;
  if (adapt) run_adapt(c, k, out);
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
  MppiSpreadCall sc{};
  MppiCall &c = sc.base;
  c.update = std::atoi(a[0]) != 0;
  c.rule = std::atoi(a[1]) != 0;
  for (int r = 0; r < 4; ++r) c.sigma[r] = num(a[2 + r]);
  c.tau_s = num(a[6]); c.lambda = num(a[7]); c.collision_cost = num(a[8]);
  c.flags = std::strtoul(a[9], nullptr, 10); c.reserved = std::strtoul(a[10], nullptr, 10);
  c.plan = ptr(a[11]); c.x0 = ptr(a[12]); c.desired = ptr(a[13]); c.score = ptr(a[14]); c.out_plan = ptr(a[15]); c.info = ptr(a[16]);
  c.B = std::atol(a[17]); c.n = std::atol(a[18]); c.S = std::atol(a[19]); c.b0 = std::atol(a[20]);
  c.handle = std::atoi(a[21]) != 0; c.f32 = std::atoi(a[22]) != 0; c.modeled = std::atoi(a[23]) != 0;
  c.models_B = std::atol(a[24]); c.pobs_B = std::atol(a[25]); c.n_desired = std::atol(a[26]); c.n_sched = std::atol(a[27]); c.k0 = std::atol(a[28]);
  sc.adapt = std::atoi(a[29]) != 0;
  for (int r = 0; r < 4; ++r) { sc.floor[r] = 0.1; sc.cap[r] = 1.0; }
  sc.floor[0] = num(a[30]); sc.cap[0] = num(a[31]); sc.rate = num(a[32]);
  sc.reserved[0] = sc.reserved[2] = 0.0;
  sc.reserved[1] = num(a[33]);
  sc.spread = ptr(a[34]); sc.out_spread = ptr(a[35]);
  bool length = false;
  const char *why = mppi_spread_refusal(sc, &length);
  std::printf("%s%s\n", length ? "length: " : "", why ? why : "ok");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && (!std::strcmp(argv[1], "fly") || !std::strcmp(argv[1], "adapt"))) return run_case(argv[1], argv[2], argv[3]);
  if (argc == 38 && !std::strcmp(argv[1], "refuse")) return run_refuse(argv + 2);
  std::fprintf(stderr, "usage: %s fly IN OUT | adapt IN OUT | refuse <29 words of host_mppi_harness's refuse> adapt floor0 cap0 rate reserved spread out_spread\n",
               argv[0]);
  return 1;
}
