// host_scored_flight_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the per-sample
// routine of the scored closed-loop flight (quadrotorilqr_amd/csrc/closed_loop_kernels.h: closed_loop_sample with its WRENCH and SCORE
// switches over ClFlatScoreFetch) and the rule of what a scored call refuses (closed_loop_launch.h: closed_loop_scored_refusal) compiled
// with g++, for tests/test_scored_flight_cpu.py.
//
//   host_scored_flight_harness fly IN OUT
//       IN, a file of doubles: a header of 20 words
//           B n S i0 i1 integrator limited modeled dt n_w has_desired n_sched k0 n_des n_shared own_K scored 0 0 0
//       | qilqr_model (13) | Q (144) | R (16) | lo (4) | hi (4) | models (B S x 13, only when modeled) | plan (B n 18) | gains (B n 52) |
//       x0 (B S 13) | wrench (B S n_w 6; n_w = 0: none) | desired per plan (B n 18, only when has_desired) | the handle's desired
//       trajectory (n_des 18) | the schedule (n_sched 144) | shared spheres (n_shared 5) | per-problem spheres (B own_K 8) | their counts (B)
//       OUT, a file of doubles: traj (B S n 18; knots outside i0 .. i1 keep the NaN they are prefilled with) | stats (B S 4) |
//       score (B S 4; NaN when not scored)
//       The handle's facts are applied as the library applies them: desired[k0 + i] and Qs[k0 + i] for knot i, row b of the per-problem table.
//   host_scored_flight_harness refuse plan gains x0 out_traj out_stats B n S i0 i1 handle f32 modeled models_B out_score wrench desired
//                                     n_w pobs_B n_desired n_sched k0
//       (addresses and numbers in decimal) prints the reason, or "ok"; a reason of length is prefixed with "length: "
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

struct Case {
  int B, n, S, i0, i1, n_w, own_K, n_shared;
  const double *tab, *plan, *gains, *x0, *wrench, *desired, *q, *shared, *own, *counts, *lo, *hi;
  long desired_step, q_step;
  double *traj, *stats, *score;
};

template <int INTEG, bool LIM, bool WRENCH, bool SCORE>
void fly(const ModelConsts<double> &c, const Case &k) {
  for (int b = 0; b < k.B; ++b) {
    const double *pb = k.plan + (long)b * k.n * 18, *gb = k.gains + (long)b * k.n * 52;
    for (int j = 0; j < k.S; ++j) {
      const long row = (long)b * k.S + j;
      const ModelConsts<double> m = k.tab ? problem_model(c, BatchModels{k.tab}, row) : c;
      ClSampleExtras ex;
      ex.wrench = WRENCH ? k.wrench + row * k.n_w * CL_WRENCH : nullptr;
      ex.wrench_step = k.n_w == 1 ? 0 : CL_WRENCH;
      ex.score = SCORE ? k.score + row * CL_SCORE : nullptr;
      // (the per-problem spheres in the caller's layout: a row of K spheres of OB_BWORDS consecutive words)
      ex.spheres = ClSpheres{k.shared, k.n_shared, k.own ? k.own + (long)b * k.own_K * OB_BWORDS : nullptr, k.own ? (int)k.counts[b] : 0, 1, OB_BWORDS};
      double *traj = k.traj + row * k.n * 18, *stats = k.stats + row * CL_STATS;
      if (WRENCH || SCORE) {
        ClFlatScoreFetch fetch{ClFlatFetch{pb, gb}, SCORE ? k.desired + (long)b * k.desired_step : nullptr, k.q, k.q_step};
        closed_loop_sample<INTEG, LIM, ClFlatScoreFetch, WRENCH, SCORE>(m, fetch, k.x0 + row * CL_STATE, k.i0, k.i1, traj, stats, k.lo, k.hi, &ex);
      } else {
        ClFlatFetch fetch{pb, gb};
        closed_loop_sample<INTEG, LIM>(m, fetch, k.x0 + row * CL_STATE, k.i0, k.i1, traj, stats, k.lo, k.hi);
      }
    }
  }
}
template <int INTEG, bool LIM>
void fly_switch(const ModelConsts<double> &c, const Case &k, bool wrench, bool score) {
  if (wrench && score) fly<INTEG, LIM, true, true>(c, k);
  else if (wrench) fly<INTEG, LIM, true, false>(c, k);
  else if (score) fly<INTEG, LIM, false, true>(c, k);
  else fly<INTEG, LIM, false, false>(c, k);
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
  if (in.size() < 20) return 3;
  const int B = (int)in[0], n = (int)in[1], S = (int)in[2], i0 = (int)in[3], i1 = (int)in[4], integ = (int)in[5];
  const bool limited = in[6] != 0.0, modeled = in[7] != 0.0;
  const double dt = in[8];
  const int n_w = (int)in[9];
  const bool has_desired = in[10] != 0.0;
  const int n_sched = (int)in[11], k0 = (int)in[12], n_des = (int)in[13], n_shared = (int)in[14], own_K = (int)in[15];
  const bool scored = in[16] != 0.0;
  if (B <= 0 || n <= 0 || S <= 0 || i0 < 0 || i1 < i0 || i1 > n - 1 || (n_w != 0 && n_w != 1 && n_w != n)) return 3;
  if (scored && ((!has_desired && k0 + i1 >= n_des) || (n_sched > 0 && k0 + i1 >= n_sched))) return 3;
  static_assert(sizeof(qilqr_model) == 13 * sizeof(double), "qilqr_model is 13 doubles");
  const size_t samples = (size_t)B * S;
  const size_t want = 20 + 13 + 144 + 16 + 8 + (modeled ? samples * 13 : 0) + (size_t)B * n * 70 + samples * 13 + samples * n_w * 6 +
                      (has_desired ? (size_t)B * n * 18 : 0) + (size_t)n_des * 18 + (size_t)n_sched * 144 + (size_t)n_shared * 5 + (size_t)B * own_K * 8 +
                      (own_K ? B : 0);
  if (in.size() != want) return 3;
  const double *p = in.data() + 20;
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
  Case k{};
  k.B = B; k.n = n; k.S = S; k.i0 = i0; k.i1 = i1; k.n_w = n_w; k.own_K = own_K; k.n_shared = n_shared;
  k.tab = modeled ? tab.data() : nullptr;
  k.plan = p; p += (size_t)B * n * 18;
  k.gains = p; p += (size_t)B * n * 52;
  k.x0 = p; p += samples * 13;
  k.wrench = n_w ? p : nullptr; p += samples * n_w * 6;
  const double *per_plan = has_desired ? p : nullptr; p += has_desired ? (size_t)B * n * 18 : 0;
  const double *handle_desired = p; p += (size_t)n_des * 18;
  const double *sched = n_sched ? p : nullptr; p += (size_t)n_sched * 144;
  k.shared = n_shared ? p : nullptr; p += (size_t)n_shared * 5;
  k.own = own_K ? p : nullptr; p += (size_t)B * own_K * 8;
  k.counts = own_K ? p : nullptr;
  k.desired = per_plan ? per_plan : handle_desired + 18 * (size_t)k0;
  k.desired_step = per_plan ? 18l * n : 0;
  k.q = sched ? sched + 144 * (size_t)k0 : Q;
  k.q_step = sched ? 144 : 0;
  k.lo = limited ? lo : nullptr;
  k.hi = limited ? hi : nullptr;
  std::vector<double> out(samples * n * 18 + samples * 4 + samples * 4, std::nan(""));
  k.traj = out.data(); k.stats = k.traj + samples * n * 18; k.score = k.stats + samples * 4;
  const bool wr = k.wrench != nullptr;
  if (integ == 1 && limited) fly_switch<1, true>(c, k, wr, scored);
  else if (integ == 1) fly_switch<1, false>(c, k, wr, scored);
  else if (limited) fly_switch<0, true>(c, k, wr, scored);
  else fly_switch<0, false>(c, k, wr, scored);
  f = std::fopen(out_path, "wb");
  if (!f) return 2;
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}

int run_refuse(char **a) {
  auto ptr = [](const char *s) { return (const void *)(uintptr_t)std::strtoull(s, nullptr, 10); };
  const ClosedLoopCall base{ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(a[4]), std::atol(a[5]), std::atol(a[6]), std::atol(a[7]),
                            std::atol(a[8]), std::atol(a[9]), std::atoi(a[10]) != 0, std::atoi(a[11]) != 0, std::atoi(a[12]) != 0,
                            std::atol(a[13]), ptr(a[14])};
  const ClosedLoopScoredCall call{base, ptr(a[15]), ptr(a[16]), std::atol(a[17]), std::atol(a[18]), std::atol(a[19]), std::atol(a[20]), std::atol(a[21])};
  bool length = false;
  const char *why = closed_loop_scored_refusal(call, &length);
  std::printf("%s%s\n", length ? "length: " : "", why ? why : "ok");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "fly")) return run_fly(argv[2], argv[3]);
  if (argc == 24 && !std::strcmp(argv[1], "refuse")) return run_refuse(argv + 2);
  std::fprintf(stderr, "usage: %s fly IN OUT | refuse plan gains x0 out_traj out_stats B n S i0 i1 handle f32 modeled models_B out_score wrench desired "
                       "n_w pobs_B n_desired n_sched k0\n", argv[0]);
  return 1;
}
