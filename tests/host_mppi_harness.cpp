// host_mppi_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the per-lane routines
// of the sampling planner (quadrotorilqr_amd/csrc/mppi_kernels.h: mppi_eps_row, mppi_sample, the folds and combinations of the update) and
// the rule of what its calls refuse (mppi_launch.h: mppi_refusal) compiled with g++, for tests/test_mppi_cpu.py and tests/test_gpu_mppi.py.
// The update runs the block's lanes one after the other: every lane's fold is the library's text, the butterfly 32 .. 1 and the
// wavefronts in index order are spelled out over arrays where the kernel has shuffles and LDS -- the update's head, the butterfly and the
// reader of IN in tests/host_mppi_common.h, which tests/host_mppi_adapt_harness.cpp shares; the fold of the weighted perturbations here.
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
#include "host_mppi_common.h"

using namespace qilqr;

namespace {

// one sample of plan b over `plan` (the case's, or the update's new one)
void fly_one(const ModelConsts<double> &c, const MppiCase &k, int b, int j, bool nominal, const double *plan, double *score, double *traj) {
  MppiFlatFetch fetch{plan, k.desired + (long)b * k.desired_step, k.q, k.q_step};
  mppi_host_fly(mppi_host_model(c, k, b), k, fetch, mppi_host_sample(k, b, j, nominal, score, traj));
}

void run_fly(const ModelConsts<double> &c, const MppiCase &k, std::vector<double> &out) {
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

void run_update(const ModelConsts<double> &c, const MppiCase &k, std::vector<double> &out) {
  const int S = k.S, n = k.n, T = mppi_update_lanes(S), W = T / 64;
  out.assign((size_t)k.B * n * 18 + (size_t)k.B * 8, std::nan(""));
  double *out_plan = out.data(), *info = out_plan + (size_t)k.B * n * 18;
  for (int b = 0; b < k.B; ++b) {
    const double *plan = k.plan + (long)b * n * 18;
    double *op = out_plan + (long)b * n * 18;
    const MppiHostHead h = mppi_host_head(k, b, op, info + 8 * (long)b);
    std::vector<double> g((size_t)S * 4, 0.0), part((size_t)W * 4);
    std::vector<double> acc[4];
    for (int i = 0; i < n; ++i) {
      for (int r = 0; r < 4; ++r) acc[r].assign(T, 0.0);
      for (int t = 0; t < T; ++t) {
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = t; j < S; j += T) {
          mppi_eps_row(k.m, k.seed, (uint32_t)(k.b0 + b), (uint32_t)j, (uint32_t)i, mppi_is_nominal(k.flags, j), &g[(size_t)j * 4]);
          mppi_fold_term(h.weights[j], &g[(size_t)j * 4], a4);
        }
        for (int r = 0; r < 4; ++r) acc[r][t] = a4[r];
      }
      for (int r = 0; r < 4; ++r) {
        butterfly(acc[r], add);
        for (int w = 0; w < W; ++w) part[(size_t)w * 4 + r] = acc[r][64 * w];
      }
      for (int r = 0; r < 4; ++r) {
        const double d = mppi_waves_in_order(&part[r], W, 4);
        op[i * 18 + 14 + r] = mppi_new_control(plan[i * 18 + 14 + r], d, h.eta, h.any, k.limited, k.limited ? k.lo[r] : 0.0, k.limited ? k.hi[r] : 0.0);
      }
    }
    // the new plan's own flight: its states over out_plan, its score into words 4 .. 7 of info
    fly_one(c, k, b, 0, true, op, info + 8 * (long)b + 4, op);
  }
}

int run_case(const char *mode, const char *in_path, const char *out_path) {
  static_assert(sizeof(qilqr_mppi_rule) == 64, "qilqr_mppi_rule is 64 bytes");
  const bool update = !std::strcmp(mode, "update");
  MppiCase k{};
  MppiCaseFile file;
  if (const int bad = mppi_read_case(in_path, update, 0, 0, k, file)) return bad;
  mppi_coeffs(file.sigma, file.tau_s, file.dt, k.m);
  std::vector<double> out;
  if (update) run_update(file.c, k, out);
  else run_fly(file.c, k, out);
  return mppi_write_out(out_path, out);
}

int run_refuse(char **a) {
  MppiCall c{};
  mppi_parse_call(a, c);
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
    // (the last word: the block size that the launches hand the kernels as their template argument)
    std::printf("%ld %d %d %d\n", mppi_flight_blocks(1, S), mppi_update_lanes(S), mppi_samples_per_lane(S),
                with_update_lanes(S, [](auto lanes) { return (int)decltype(lanes)::value; }));
    return 0;
  }
  std::fprintf(stderr, "usage: %s fly IN OUT | update IN OUT | grid S | refuse update rule sigma0 sigma1 sigma2 sigma3 tau_s lambda collision_cost flags "
                       "reserved plan x0 desired score out_plan info B n S b0 handle f32 modeled models_B pobs_B n_desired n_sched k0\n", argv[0]);
  return 1;
}
