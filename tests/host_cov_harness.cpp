// host_cov_harness.cpp -- CPU test harness (tests only, never part of the product library), a stand-alone program: the routines of the
// linear covariance analysis that compile for the host (quadrotorilqr_amd/csrc/cov_kernels.h: the knots' F and G, the recursion in plain
// loops, a knot's measures and the plan's summary) and the rule of what the call refuses (cov_launch.h: cov_refusal) compiled with g++,
// for tests/test_covariance_cpu.py and tests/test_gpu_covariance.py.
//
//   host_cov_harness run IN OUT
//       IN, a file of doubles: B n i0 i1 integrator modeled has_gains held dt n_shared own_K | qilqr_model (13) | Q (144) | R (16) |
//       state_sigma (12) | mean (6) | sigma (6) | tau_force_s tau_torque_s | models (B x 13, only when modeled) | plan (B n 18) |
//       gains (B n 52, only with has_gains) | shared (n_shared x 5) | own (B own_K 8) counts (B) (only with own_K > 0)
//       OUT, a file of doubles: cov (B n 144) | mean (B n 12) | summary (B 8) | cross (B n 72: C_i) | F (B n 144) | G (B n 72); knots
//       outside the window (for F and G: outside i0 .. i1 - 1) keep the NaN they are prefilled with
//   host_cov_harness step IN OUT
//       IN: integrator dt rows | qilqr_model (13) | rows x {x (13), u (4), w (6)};  OUT: rows x 13, the flight's own disturbed step
//       (closed_loop_kernels.h: cl_disturbed_acceleration / se3_rplus_fast, or cl_rk4_step_wrench) from x under u and the wrench w
//   host_cov_harness refuse rule sigma0 gsigma0 tau mean0 flags reserved plan gains cov mean summary B n i0 i1 handle f32 modeled models_B pobs_B
//       (addresses and numbers in decimal; "nan" and "inf" are numbers) prints the reason, or "ok"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/host_model.h"
#include "../quadrotorilqr_amd/csrc/cov_kernels.h"
#include "../quadrotorilqr_amd/csrc/cov_launch.h"

using namespace qilqr;

namespace {

bool read_doubles(const char *path, std::vector<double> &in) {
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  in.resize((size_t)bytes / sizeof(double));
  const bool ok = std::fread(in.data(), sizeof(double), in.size(), f) == in.size();
  std::fclose(f);
  return ok;
}
bool write_doubles(const char *path, const std::vector<double> &out) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  std::fclose(f);
  return ok;
}

// dense F (144) and G (72) of one knot through the routines the kernel calls
void knot_matrices(int integ, const ModelConsts<double> &c, const double *pt, const double *K, double *F, double *G) {
  if (integ == 1) {
    for (int part = 0; part < COV_RK4_PARTS; ++part)
      cov_rk4_part(c, pt, K, part, [&](bool g, int r, int col, double v) { (g ? G[r * 6 + col] : F[r * 12 + col]) = v; });
  } else {
    cov_euler_closed_loop_jacobian(c, pt, K, [&](int r, int col, double v) { F[r * 12 + col] = v; });
    cov_euler_wrench_jacobian(c, pt, [&](int r, int col, double v) { G[r * 6 + col] = v; });
  }
}

int run(const char *in_path, const char *out_path) {
  std::vector<double> in;
  if (!read_doubles(in_path, in)) return 2;
  if (in.size() < 11) return 3;
  const int B = (int)in[0], n = (int)in[1], i0 = (int)in[2], i1 = (int)in[3], integ = (int)in[4];
  const bool modeled = in[5] != 0.0, has_gains = in[6] != 0.0, held = in[7] != 0.0;
  const double dt = in[8];
  const int n_shared = (int)in[9], own_K = (int)in[10];
  if (B <= 0 || n <= 0 || i0 < 0 || i1 < i0 || i1 > n - 1 || n_shared < 0 || n_shared > OB_MAX || own_K < 0 || own_K > OB_MAX) return 3;
  const size_t knots = (size_t)B * n;
  const size_t want = 11 + 13 + 144 + 16 + 12 + 6 + 6 + 2 + (modeled ? (size_t)B * 13 : 0) + knots * 18 + (has_gains ? knots * 52 : 0) + (size_t)n_shared * 5 +
                      (own_K > 0 ? (size_t)B * own_K * 8 + B : 0);
  if (in.size() != want) return 3;
  const double *p = in.data() + 11;
  qilqr_model model;
  static_assert(sizeof(qilqr_model) == 13 * sizeof(double), "qilqr_model is 13 doubles");
  std::memcpy(&model, p, sizeof model);
  p += 13;
  const double *Q = p, *R = p + 144, *state_sigma = p + 160, *mean = p + 172, *sigma = p + 178;
  const double tau_f = p[184], tau_t = p[185];
  p += 186;
  ModelConsts<double> c;
  if (!make_model_consts(model.mass_kg, model.inertia, model.arm_length_m, model.torque_to_thrust_ratio_m, model.g_mpss, Q, R, dt, &c)) return 4;
  std::vector<double> tab;
  if (modeled) {
    std::vector<qilqr_model> models((size_t)B);
    std::memcpy(models.data(), p, (size_t)B * sizeof(qilqr_model));
    p += (size_t)B * 13;
    tab.resize((size_t)B * PM_WORDS);
    if (make_model_table(models.data(), (long)B, Q, R, dt, tab.data()) != -1) return 4;
  }
  const double *plan = p;
  p += knots * 18;
  const double *gains = has_gains ? p : nullptr;
  if (has_gains) p += knots * 52;
  const double *shared = p;
  p += (size_t)n_shared * 5;
  const double *own = own_K > 0 ? p : nullptr, *counts = own_K > 0 ? p + (size_t)B * own_K * 8 : nullptr;
  CovCoeffs k;
  cov_coeffs(state_sigma, mean, sigma, tau_f, tau_t, held, dt, k);
  std::vector<double> out(knots * (144 + 12 + 72 + 144 + 72) + (size_t)B * 8, std::nan(""));
  double *cov = out.data(), *mn = cov + knots * 144, *summary = mn + knots * 12, *cross = summary + (size_t)B * 8, *F = cross + knots * 72, *G = F + knots * 144;
  for (int b = 0; b < B; ++b) {
    const ModelConsts<double> m = modeled ? problem_model(c, BatchModels{tab.data()}, (long)b) : c;
    const size_t k0 = (size_t)b * n;
    for (int i = i0; i < i1; ++i) knot_matrices(integ, m, plan + (k0 + i) * 18, gains ? gains + (k0 + i) * 52 + 4 : nullptr, F + (k0 + i) * 144, G + (k0 + i) * 72);
    cov_chain_reference(F + k0 * 144, G + k0 * 72, k, i0, i1, cov + k0 * 144, mn + k0 * 12, cross + k0 * 72);
    const int n_own = own ? (int)counts[b] : 0;
    if (n_own < 0 || n_own > own_K) return 3;
    const ClSpheres sp{shared, n_shared, own ? own + (size_t)b * own_K * 8 : nullptr, n_own, 1, OB_BWORDS};
    CovPlanSummary s;
    for (int i = i0; i <= i1; ++i)
      s.take(cov_knot_measures(cov + (k0 + i) * 144, mn + (k0 + i) * 12, plan + (k0 + i) * 18, gains ? gains + (k0 + i) * 52 + 4 : nullptr, sp, (double)i * dt), i, i1);
    s.words(summary + (size_t)b * 8);
  }
  return write_doubles(out_path, out) ? 0 : 2;
}

int step(const char *in_path, const char *out_path) {
  std::vector<double> in;
  if (!read_doubles(in_path, in)) return 2;
  if (in.size() < 16) return 3;
  const int integ = (int)in[0], rows = (int)in[2];
  const double dt = in[1];
  if (rows <= 0 || in.size() != 16 + (size_t)rows * 23) return 3;
  qilqr_model model;
  std::memcpy(&model, in.data() + 3, sizeof model);
  double Q[144] = {0.0}, R[16] = {0.0};
  for (int e = 0; e < 12; ++e) Q[e * 13] = 1.0;
  for (int e = 0; e < 4; ++e) R[e * 5] = 1.0;
  ModelConsts<double> c;
  if (!make_model_consts(model.mass_kg, model.inertia, model.arm_length_m, model.torque_to_thrust_ratio_m, model.g_mpss, Q, R, dt, &c)) return 4;
  std::vector<double> out((size_t)rows * 13);
  RolloutSeries<double> sr;
  sr.load();
  for (int r = 0; r < rows; ++r) {
    const double *x = in.data() + 16 + (size_t)r * 23, *u = x + 13, *w = u + 4;
    double t[3] = {x[0], x[1], x[2]}, q[4] = {x[4], x[5], x[6], x[3]}, v[6];
    for (int a = 0; a < 6; ++a) v[a] = x[7 + a];
    if (integ == 1) {
      cl_rk4_step_wrench(c, t, q, v, u, w);
    } else {  // (closed_loop_sample's Euler step under a wrench, statement for statement)
      double acc[6], tau[6];
      cl_disturbed_acceleration<true>(c, q, v, u, w, acc);
      for (int a = 0; a < 6; ++a) tau[a] = c.dt * v[a];
      se3_rplus_fast(t, q, tau, sr);
      for (int a = 0; a < 6; ++a) v[a] = v[a] + c.dt * acc[a];
    }
    double *o = out.data() + (size_t)r * 13;
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = q[3]; o[4] = q[0]; o[5] = q[1]; o[6] = q[2];
    for (int a = 0; a < 6; ++a) o[7 + a] = v[a];
  }
  return write_doubles(out_path, out) ? 0 : 2;
}

int refuse(char **a) {
  auto ptr = [](const char *s) { return (const void *)(uintptr_t)std::strtoull(s, nullptr, 10); };
  CovCall c{};
  c.rule = std::atoi(a[0]) != 0;
  for (int k = 0; k < 12; ++k) c.state_sigma[k] = 1e-3;
  for (int k = 0; k < 6; ++k) c.sigma[k] = 1e-2;
  c.state_sigma[0] = std::atof(a[1]);
  c.sigma[0] = std::atof(a[2]);
  c.tau_force_s = 0.0;
  c.tau_torque_s = std::atof(a[3]);
  c.mean[0] = std::atof(a[4]);
  c.flags = std::strtoul(a[5], nullptr, 10);
  c.reserved = std::strtoul(a[6], nullptr, 10);
  c.plan = ptr(a[7]); c.gains = ptr(a[8]); c.cov = ptr(a[9]); c.mean_out = ptr(a[10]); c.summary = ptr(a[11]);
  c.B = std::atol(a[12]); c.n = std::atol(a[13]); c.i0 = std::atol(a[14]); c.i1 = std::atol(a[15]);
  c.handle = std::atoi(a[16]) != 0; c.f32 = std::atoi(a[17]) != 0; c.modeled = std::atoi(a[18]) != 0;
  c.models_B = std::atol(a[19]); c.pobs_B = std::atol(a[20]);
  const char *why = cov_refusal(c);
  std::puts(why ? why : "ok");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 4 && !std::strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "step")) return step(argv[2], argv[3]);
  if (argc == 23 && !std::strcmp(argv[1], "refuse")) return refuse(argv + 2);
  std::fprintf(stderr, "usage: %s run IN OUT | step IN OUT | refuse <21 facts>\n", argv[0]);
  return 1;
}
