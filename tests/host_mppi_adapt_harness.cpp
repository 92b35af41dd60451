// host_mppi_adapt_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the per-lane
// routines of the planner's adapted spread (quadrotorilqr_amd/csrc/mppi_adapt_kernels.h: mppi_spread_eps, mppi_sample over a fetch with a
// spread, the folds of the two moments, mppi_weighted_var, mppi_blend_spread) and the rule of what its calls refuse
// (mppi_adapt_launch.h: mppi_spread_refusal) compiled with g++, for tests/test_mppi_adapt_cpu.py and tests/test_gpu_mppi_adapt.py.
// As tests/host_mppi_harness.cpp, the adaptation runs the block's lanes one after the other: every lane's fold is the library's text,
// the butterfly 32 .. 1 and the wavefronts in index order are spelled out -- the update's head, the butterfly and the reader of IN in
// tests/host_mppi_common.h, shared with that program; the fold of the two moments here.
//
//   host_mppi_adapt_harness fly IN OUT     OUT: score (B S 4) | eps as flown (B S n 4)
//   host_mppi_adapt_harness adapt IN OUT   OUT: out_plan (B n 18) | info (B 8) | out_spread (B n 4) | the weighted variances (B n 4)
//       IN: the file of tests/host_mppi_harness.cpp (its header's sigma is not read), followed by
//           spread (B n 4) | floor (4) | cap (4) | rate
//   host_mppi_adapt_harness refuse <the 29 words of host_mppi_harness's refuse> adapt floor0 cap0 rate reserved spread out_spread
//       (floor0 / cap0: of rotor 0, the others are 0.1 and 1; reserved: word 1) prints the reason, or "ok"
#include "host_mppi_common.h"
#include "../quadrotorilqr_amd/csrc/mppi_adapt_kernels.h"
#include "../quadrotorilqr_amd/csrc/mppi_adapt_launch.h"

using namespace qilqr;

namespace {

struct Case : MppiCase {  // (m: the unit recursion's)
  MppiAdaptCoeffs k;
  const double *spread;
};

// one sample of plan b over `plan`, with plan b's rows of the spread; nominal: the flight of a new plan (mppi.hip's)
void fly_one(const ModelConsts<double> &c, const Case &k, int b, int j, bool nominal, const double *plan, double *score, double *traj) {
  const ModelConsts<double> mdl = mppi_host_model(c, k, b);
  const MppiSample s = mppi_host_sample(k, b, j, nominal, score, traj);
  MppiFlatSpreadFetch fetch{{plan, k.desired + (long)b * k.desired_step, k.q, k.q_step}, k.spread + 4 * (long)b * k.n};
  if (nominal) {  // the library's second launch is k_mppi_flight: no spread is read
    MppiFlatFetch plain = fetch;
    mppi_host_fly(mdl, k, plain, s);
  } else {
    mppi_host_fly(mdl, k, fetch, s);
  }
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

void run_adapt(const ModelConsts<double> &c, const Case &k, std::vector<double> &out) {
  const int S = k.S, n = k.n, T = mppi_update_lanes(S), W = T / 64;
  const size_t knots = (size_t)k.B * n;
  out.assign(knots * 18 + (size_t)k.B * 8 + knots * 4 + knots * 4, std::nan(""));
  double *out_plan = out.data(), *info = out_plan + knots * 18, *out_spread = info + (size_t)k.B * 8, *out_var = out_spread + knots * 4;
  for (int b = 0; b < k.B; ++b) {
    const double *plan = k.plan + (long)b * n * 18, *spread = k.spread + 4 * (long)b * n;
    double *op = out_plan + (long)b * n * 18;
    const MppiHostHead h = mppi_host_head(k, b, op, info + 8 * (long)b);
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
          mppi_fold_moments(h.weights[j], e, a4, b4);
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
        op[i * 18 + 14 + r] = mppi_new_control(plan[i * 18 + 14 + r], d, h.eta, h.any, k.limited, k.limited ? k.lo[r] : 0.0, k.limited ? k.hi[r] : 0.0);
        const double var = h.any ? mppi_weighted_var(d, d2, h.eta) : 0.0;
        const size_t ws = ((size_t)b * n + i) * 4 + r;
        out_var[ws] = var;
        out_spread[ws] = mppi_blend_spread(spread[4 * i + r], var, h.any, k.k.one_minus_rate, k.k.rate, k.k.floor[r], k.k.cap[r]);
      }
    }
    // the new plan's own flight: its states over out_plan, its score into words 4 .. 7 of info
    fly_one(c, k, b, 0, true, op, info + 8 * (long)b + 4, op);
  }
}

int run_case(const char *mode, const char *in_path, const char *out_path) {
  static_assert(sizeof(qilqr_mppi_adapt_rule) == 96, "qilqr_mppi_adapt_rule is 96 bytes");
  const bool adapt = !std::strcmp(mode, "adapt");
  Case k{};
  MppiCaseFile file;
  if (const int bad = mppi_read_case(in_path, adapt, 4, 9, k, file)) return bad;
  const double *p = file.tail;
  k.spread = p; p += (size_t)k.B * k.n * 4;
  mppi_adapt_coeffs(p, p + 4, p[8], k.k);
  mppi_unit_coeffs(file.tau_s, file.dt, k.m);
  std::vector<double> out;
  if (adapt) run_adapt(file.c, k, out);
  else run_fly(file.c, k, out);
  return mppi_write_out(out_path, out);
}

int run_refuse(char **a) {
  auto ptr = [](const char *s) { return (const void *)(uintptr_t)std::strtoull(s, nullptr, 10); };
  auto num = [](const char *s) { return std::strtod(s, nullptr); };
  MppiSpreadCall sc{};
  mppi_parse_call(a, sc.base);
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
