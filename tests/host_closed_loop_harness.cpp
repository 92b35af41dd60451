// host_closed_loop_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the per-sample
// routine of the closed-loop flight (quadrotorilqr_amd/csrc/closed_loop_kernels.h: closed_loop_sample over ClFlatFetch) and the rule of
// what a call refuses (closed_loop_launch.h: closed_loop_refusal) compiled with g++, for tests/test_closed_loop_cpu.py.
//
//   host_closed_loop_harness fly IN OUT
//       IN, a file of doubles: B n S i0 i1 integrator limited modeled dt | qilqr_model (13) | Q (144) | R (16) | lo (4) | hi (4) |
//       models (B S x 13, only when modeled) | plan (B n 18) | gains (B n 52) | x0 (B S 13)
//       OUT, a file of doubles: traj (B S n 18; knots outside i0 .. i1 keep the NaN they are prefilled with) | stats (B S 4) |
//       rollout (B n 18): rollout_problem<false> of every plan from its own knot 0 with alpha = 0, the handle's model, the same integrator
//       and limits -- what S = 1, x0 = plan[:, 0, 1:14], i0 = 0, i1 = n - 1 must reproduce bit for bit
//   host_closed_loop_harness refuse plan gains x0 out_traj out_stats B n S i0 i1 handle f32 modeled models_B
//       (addresses and numbers in decimal) prints the reason, or "ok"
//   host_closed_loop_harness form S...
//       prints, for every S, "shared" or "flattened": closed_loop_shared_form(S), the rule of the kernel's two forms
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"
#include "../quadrotorilqr_amd/csrc/closed_loop_kernels.h"
#include "../quadrotorilqr_amd/csrc/closed_loop_launch.h"

using namespace qilqr;

namespace {

template <int INTEG, bool LIM>
void fly(const ModelConsts<double> &c, const double *tab, const double *plan, const double *gains, const double *x0, int B, int n, int S, int i0,
         int i1, const double *lo, const double *hi, double *traj, double *stats, double *rollout) {
  for (int b = 0; b < B; ++b) {
    const double *pb = plan + (long)b * n * 18, *gb = gains + (long)b * n * 52;
    for (int j = 0; j < S; ++j) {
      const long row = (long)b * S + j;
      const ModelConsts<double> m = tab ? problem_model(c, BatchModels{tab}, row) : c;
      ClFlatFetch fetch{pb, gb};
      closed_loop_sample<INTEG, LIM>(m, fetch, x0 + row * CL_STATE, i0, i1, traj + row * n * 18, stats + row * CL_STATS, lo, hi);
    }
    rollout_problem<false, double, INTEG, LIM>(c, pb, gb, 0.0, rollout + (long)b * n * 18, n, lo, hi);
  }
}

int run_fly(const char *in_path, const char *out_path) {
  FILE *f = std::fopen(in_path, "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double));
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
  std::fclose(f);
  if (in.size() < 9) return 3;
  const int B = (int)in[0], n = (int)in[1], S = (int)in[2], i0 = (int)in[3], i1 = (int)in[4], integ = (int)in[5];
  const bool limited = in[6] != 0.0, modeled = in[7] != 0.0;
  const double dt = in[8];
  if (B <= 0 || n <= 0 || S <= 0 || i0 < 0 || i1 < i0 || i1 > n - 1) return 3;
  static_assert(sizeof(qilqr_model) == 13 * sizeof(double), "qilqr_model is 13 doubles");
  const size_t samples = (size_t)B * S;
  const size_t want = 9 + 13 + 144 + 16 + 8 + (modeled ? samples * 13 : 0) + (size_t)B * n * 70 + samples * 13;
  if (in.size() != want) return 3;
  const double *p = in.data() + 9;
  qilqr_model model;
  std::memcpy(&model, p, sizeof model);
  p += 13;
  const double *Q = p, *R = p + 144, *lo = p + 160, *hi = p + 164;
  p += 168;
  ModelConsts<double> c;
  if (!make_model_consts(model.mass_kg, model.inertia, model.arm_length_m, model.torque_to_thrust_ratio_m, model.g_mpss, Q, R, dt, &c)) return 4;
  std::vector<double> tab;
  if (modeled) {
    std::vector<qilqr_model> models(samples);
    std::memcpy(models.data(), p, samples * sizeof(qilqr_model));
    p += samples * 13;
    tab.resize(samples * PM_WORDS);
    if (make_model_table(models.data(), (long)samples, Q, R, dt, tab.data()) != -1) return 4;
  }
  const double *plan = p, *gains = plan + (size_t)B * n * 18, *x0 = gains + (size_t)B * n * 52;
  std::vector<double> out(samples * n * 18 + samples * 4 + (size_t)B * n * 18, std::nan(""));
  double *traj = out.data(), *stats = traj + samples * n * 18, *rollout = stats + samples * 4;
  const double *t = modeled ? tab.data() : nullptr;
  if (integ == 1 && limited) fly<1, true>(c, t, plan, gains, x0, B, n, S, i0, i1, lo, hi, traj, stats, rollout);
  else if (integ == 1) fly<1, false>(c, t, plan, gains, x0, B, n, S, i0, i1, nullptr, nullptr, traj, stats, rollout);
  else if (limited) fly<0, true>(c, t, plan, gains, x0, B, n, S, i0, i1, lo, hi, traj, stats, rollout);
  else fly<0, false>(c, t, plan, gains, x0, B, n, S, i0, i1, nullptr, nullptr, traj, stats, rollout);
  f = std::fopen(out_path, "wb");
  if (!f) return 2;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}

int run_refuse(char **a) {
  auto ptr = [](const char *s) { return (const void *)(uintptr_t)std::strtoull(s, nullptr, 10); };
  const ClosedLoopCall call{ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(a[4]), std::atol(a[5]), std::atol(a[6]), std::atol(a[7]),
                            std::atol(a[8]), std::atol(a[9]), std::atoi(a[10]) != 0, std::atoi(a[11]) != 0, std::atoi(a[12]) != 0,
                            std::atol(a[13])};
  const char *why = closed_loop_refusal(call);
  std::puts(why ? why : "ok");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "fly")) return run_fly(argv[2], argv[3]);
  if (argc == 16 && !std::strcmp(argv[1], "refuse")) return run_refuse(argv + 2);
  if (argc >= 3 && !std::strcmp(argv[1], "form")) {
    for (int k = 2; k < argc; ++k) std::puts(closed_loop_shared_form(std::atoi(argv[k])) ? "shared" : "flattened");
    return 0;
  }
  std::fprintf(stderr, "usage: %s fly IN OUT | refuse plan gains x0 out_traj out_stats B n S i0 i1 handle f32 modeled models_B | form S...\n", argv[0]);
  return 1;
}
