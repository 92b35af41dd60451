// host_monte_carlo_harness.cpp -- the Monte-Carlo kernels' arithmetic on the host: philox.h, the per-lane routines of
// monte_carlo_kernels.h and the rules of monte_carlo_launch.h, compiled with g++ into a stand-alone program (tests/test_monte_carlo_cpu.py
// builds and runs it, once under the address and undefined-behaviour sanitizers).  The loops here are the kernels' loops: a lane per
// (flight, pair) that walks the rows in order, a lane per (plan, sample), and 64 lanes per plan combined by the butterfly 32 .. 1.
//
//   philox c0 c1 c2 c3 k0 k1             (hex) -> the four output words, hex
//   words seed plan sample row stream pair     -> the four words of that draw, hex
//   normals w0 w1 w2 w3                  (hex) -> z0 z1 as hexadecimal floating point
//   draws in.bin out.bin        in:  {seed lo, seed hi, N, N x {plan, sample, row, stream, pair}}   out: N x {w0, w1, w2, w3, z0, z1}
//   gusts in.bin out.bin        in:  {B, S, n_w, b0, s0, seed lo, seed hi, dt, tau_f, tau_t, mean[6], sigma[6]} as doubles
//                               out: wrench[B][S][n_w][6]
//   states in.bin out.bin       in:  {B, S, b0, s0, seed lo, seed hi, flags, 0, sigma[12], x_nom[B][13]}     out: x0[B][S][13]
//   reduce in.bin out.bin       in:  {B, S, score[B][S][4]}                                                    out: summary[B][8]
//   refuse gusts|states|reduce ...       the facts of a call (see run_refuse) -> "ok" or the reason
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/philox.h"
#include "../quadrotorilqr_amd/csrc/monte_carlo_kernels.h"
#include "../quadrotorilqr_amd/csrc/monte_carlo_launch.h"

using namespace qilqr;

static_assert(QILQR_MC_SUMMARY == MC_SUMMARY, "the header and the kernels agree on the words of a summary");

static std::vector<double> read_all(const char *path) {
  FILE *f = std::fopen(path, "rb");
  if (!f) { std::perror(path); std::exit(2); }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> v((size_t)bytes / sizeof(double));
  if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
  std::fclose(f);
  return v;
}
static int write_all(const char *path, const std::vector<double> &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f) { std::perror(path); return 2; }
  const bool ok = std::fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok ? 0 : 2;
}
static uint64_t seed_of(double lo, double hi) { return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32); }
static void need(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "bad input: %s\n", what); std::exit(2); }
}

static int run_draws(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() >= 3 && (long)in.size() == 3 + 5 * (long)in[2], "draws takes a head of 3 words and 5 per draw");
  const long N = (long)in[2];
  const uint64_t seed = seed_of(in[0], in[1]);
  std::vector<double> out((size_t)(6 * N));
  for (long k = 0; k < N; ++k) {
    const double *d = &in[(size_t)(3 + 5 * k)];
    uint32_t w[4];
    mc_words(seed, (uint32_t)d[0], (uint32_t)d[1], (uint32_t)d[2], (uint32_t)d[3], (uint32_t)d[4], w);
    for (int a = 0; a < 4; ++a) out[(size_t)(6 * k + a)] = (double)w[a];
    mc_normals(w, out[(size_t)(6 * k + 4)], out[(size_t)(6 * k + 5)]);
  }
  return write_all(out_path, out);
}

static int run_gusts(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() == 22, "gusts takes 22 words");
  const long B = (long)in[0], S = (long)in[1], n_w = (long)in[2];
  const uint32_t b0 = (uint32_t)in[3], s0 = (uint32_t)in[4];
  const uint64_t seed = seed_of(in[5], in[6]);
  GustCoeffs m;
  gust_coeffs(&in[10], &in[16], in[8], in[9], in[7], m);
  std::vector<double> out((size_t)(B * S * n_w * 6));
  for (long f = 0; f < B * S; ++f)  // k_sample_gusts' lanes: a pair of one flight, its rows in order
    for (int pair = 0; pair < 3; ++pair) {
      double g[2] = {0.0, 0.0};
      for (long i = 0; i < n_w; ++i) {
        double w[2];
        gust_row(m, seed, b0 + (uint32_t)(f / S), s0 + (uint32_t)(f % S), (uint32_t)i, pair, g, w);
        out[(size_t)((f * n_w + i) * 6 + 2 * pair)] = w[0];
        out[(size_t)((f * n_w + i) * 6 + 2 * pair + 1)] = w[1];
      }
    }
  return write_all(out_path, out);
}

static int run_states(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() >= 20, "states takes a head of 20 words");
  const long B = (long)in[0], S = (long)in[1];
  const uint32_t b0 = (uint32_t)in[2], s0 = (uint32_t)in[3], flags = (uint32_t)in[6];
  const uint64_t seed = seed_of(in[4], in[5]);
  need((long)in.size() == 20 + 13 * B, "states takes x_nom[B][13] behind the head");
  std::vector<double> out((size_t)(B * S * 13));
  for (long r = 0; r < B * S; ++r)  // k_sample_states' lanes
    sample_state(&in[20 + 13 * (r / S)], &in[8], seed, b0 + (uint32_t)(r / S), s0 + (uint32_t)(r % S), flags, &out[(size_t)(13 * r)]);
  return write_all(out_path, out);
}

static int run_reduce(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() >= 2, "reduce takes B and S");
  const long B = (long)in[0], S = (long)in[1];
  need((long)in.size() == 2 + 4 * B * S, "reduce takes score[B][S][4] behind B and S");
  std::vector<double> out((size_t)(B * MC_SUMMARY));
  for (long b = 0; b < B; ++b) {  // k_reduce_scores' wavefront: 64 lanes, each lane's fold, the butterfly, the mean, and again
    const double *mine = &in[2] + 4 * b * S;
    McFold f[64], g[64];
    for (int lane = 0; lane < 64; ++lane) f[lane] = mc_fold_lane(mine, (int)S, lane);
    for (int off = 32; off >= 1; off >>= 1) {
      for (int lane = 0; lane < 64; ++lane) g[lane] = mc_fold_combine(f[lane], f[lane ^ off]);
      for (int lane = 0; lane < 64; ++lane) f[lane] = g[lane];
    }
    for (int lane = 1; lane < 64; ++lane) need(!std::memcmp(&f[lane].sum, &f[0].sum, sizeof(double)) && f[lane].i_max == f[0].i_max && f[lane].i_min == f[0].i_min, "the butterfly leaves every lane the same");
    const double mean = f[0].n_finite > 0 ? f[0].sum / (double)f[0].n_finite : 0.0;
    double ss[64], st[64];
    for (int lane = 0; lane < 64; ++lane) ss[lane] = mc_fold_deviations(mine, (int)S, lane, mean);
    for (int off = 32; off >= 1; off >>= 1) {
      for (int lane = 0; lane < 64; ++lane) st[lane] = ss[lane] + ss[lane ^ off];
      for (int lane = 0; lane < 64; ++lane) ss[lane] = st[lane];
    }
    mc_summary(f[0], ss[0], (int)S, &out[(size_t)(b * MC_SUMMARY)]);
  }
  return write_all(out_path, out);
}

// refuse gusts  handle model wrench B S n_w b0 s0 tau_f tau_t mean[6] sigma[6]     (22 values)
// refuse states handle sigma_given x_nom x0 B S b0 s0 flags sigma[12]              (21 values)
// refuse reduce handle score summary B S                                           (5 values)
static int run_refuse(int n, char **v) {
  auto L = [&](int k) { return std::strtol(v[k], nullptr, 0); };
  auto P = [&](int k) { return (const void *)(uintptr_t)std::strtoull(v[k], nullptr, 0); };
  auto D = [&](int k) { return std::strtod(v[k], nullptr); };
  const char *why = "?";
  if (!std::strcmp(v[0], "gusts") && n == 23) {
    SampleGustsCall c{L(1) != 0, L(2) != 0, P(3), L(4), L(5), L(6), L(7), L(8), {}, {}, D(9), D(10)};
    for (int k = 0; k < 6; ++k) { c.mean[k] = D(11 + k); c.sigma[k] = D(17 + k); }
    why = sample_gusts_refusal(c);
  } else if (!std::strcmp(v[0], "states") && n == 22) {
    SampleStatesCall c{L(1) != 0, L(2) != 0, P(3), P(4), L(5), L(6), L(7), L(8), std::strtoul(v[9], nullptr, 0), {}};
    for (int k = 0; k < 12; ++k) c.sigma[k] = D(10 + k);
    why = sample_states_refusal(c);
  } else if (!std::strcmp(v[0], "reduce") && n == 6) {
    const ReduceScoresCall c{L(1) != 0, P(2), P(3), L(4), L(5)};
    why = reduce_scores_refusal(c);
  } else {
    std::fprintf(stderr, "refuse: which call, and how many facts?\n");
    return 2;
  }
  std::printf("%s\n", why ? why : "ok");
  return 0;
}

int main(int argc, char **argv) {
  auto H = [&](int k) { return (uint32_t)std::strtoul(argv[k], nullptr, 16); };
  if (argc == 8 && !std::strcmp(argv[1], "philox")) {
    uint32_t c[4] = {H(2), H(3), H(4), H(5)};
    philox4x32_10(c, H(6), H(7));
    std::printf("%08x %08x %08x %08x\n", c[0], c[1], c[2], c[3]);
    return 0;
  }
  if (argc == 8 && !std::strcmp(argv[1], "words")) {
    uint32_t w[4];
    mc_words(std::strtoull(argv[2], nullptr, 0), (uint32_t)std::strtoul(argv[3], nullptr, 0), (uint32_t)std::strtoul(argv[4], nullptr, 0),
             (uint32_t)std::strtoul(argv[5], nullptr, 0), (uint32_t)std::strtoul(argv[6], nullptr, 0), (uint32_t)std::strtoul(argv[7], nullptr, 0), w);
    std::printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    return 0;
  }
  if (argc == 6 && !std::strcmp(argv[1], "normals")) {
    const uint32_t w[4] = {H(2), H(3), H(4), H(5)};
    double z0, z1;
    mc_normals(w, z0, z1);
    std::printf("%a %a\n", z0, z1);
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "draws")) return run_draws(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "gusts")) return run_gusts(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "states")) return run_states(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "reduce")) return run_reduce(argv[2], argv[3]);
  if (argc >= 3 && !std::strcmp(argv[1], "refuse")) return run_refuse(argc - 2, argv + 2);
  std::fprintf(stderr, "usage: %s philox|words|normals|gusts|states|reduce|refuse ...\n", argv[0]);
  return 2;
}
