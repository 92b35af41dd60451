// host_risk_harness.cpp -- the risk and selection kernels' decisions on the host: the per-lane routines of risk_kernels.h and the rules
// of risk_launch.h, compiled with g++ into a stand-alone program (tests/test_risk_cpu.py builds and runs it, once under the address and
// undefined-behaviour sanitizers).  The loops here are the kernels' loops: every stage of the network over its P / 2 comparators
// (risk_comparator is the kernel's schedule, risk_exchange its comparator), 64 lanes per level combined by the butterfly 32 .. 1, a
// lane per vehicle.
//
//   sort in.bin out.bin     in:  {N, then N x {S, key[S]}}                      out: N x idx[P], P = the power of two >= S
//   rank S level ...                                                            -> the rank of each level, one line
//   risk in.bin out.bin     in:  {B, S, column, L, level[L], score[B][S][4]}    out: risk[B][L][4]
//   select in.bin out.bin   in:  {V, C, L, objective, level, max collision, max diverged, min clearance, risk given,
//                                 summary[C V][8], risk[C V][L][4] if given}    out: {choice[V], info[V][4]}
//   refuse risk|select ...  the facts of a call (see run_refuse) -> "ok" or the reason
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/risk_kernels.h"
#include "../quadrotorilqr_amd/csrc/risk_launch.h"

using namespace qilqr;

static_assert(QILQR_MC_RISK == RISK_WORDS && QILQR_RISK_MAX_LEVELS == RISK_MAX_LEVELS && QILQR_RISK_MAX_SAMPLES == RISK_MAX_SAMPLES &&
                  QILQR_RISK_COST == RISK_COST && QILQR_RISK_CLEARANCE == RISK_CLEARANCE && QILQR_SELECT_INFO == SELECT_INFO,
              "the header and the kernels agree on the words, the caps and the columns");
static_assert(sizeof(qilqr_select_rule) == sizeof(SelectRule) && sizeof(SelectRule) == 32, "the header's rule is the kernels'");

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
static void need(bool ok, const char *what) {
  if (!ok) { std::fprintf(stderr, "bad input: %s\n", what); std::exit(2); }
}

// k_risk_scores' block up to the last barrier: the slots filled from the plan's score rows, then every stage over its comparators
static void sort_plan(const double *score, int S, int column, std::vector<double> &keys, std::vector<int> &idx) {
  const int P = risk_slots(S);
  keys.assign((size_t)P, 0.0);
  idx.assign((size_t)P, 0);
  for (int p = 0; p < P; ++p) {
    keys[(size_t)p] = p < S ? risk_key(score + 4 * (long)p, column) : INFINITY;
    idx[(size_t)p] = p;
  }
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1)
      for (int c = 0; c < P / 2; ++c) {
        const RiskPair pr = risk_comparator(k, j, c);
        need(pr.lo >= 0 && pr.lo < pr.hi && pr.hi < P && pr.hi == pr.lo + j, "a comparator stays inside the slots");
        risk_exchange(keys.data(), idx.data(), pr);
      }
}

static int run_sort(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() >= 1, "sort takes N and N arrays");
  const long N = (long)in[0];
  std::vector<double> out, keys;
  std::vector<int> idx;
  size_t at = 1;
  for (long a = 0; a < N; ++a) {
    need(at < in.size(), "sort: an array is missing");
    const int S = (int)in[at++];
    need(S >= 1 && S <= RISK_MAX_SAMPLES && at + (size_t)S <= in.size(), "sort: S is 1 ... 4096 and its keys follow");
    std::vector<double> score((size_t)(4 * S), 0.0);
    for (int j = 0; j < S; ++j) score[(size_t)(4 * j)] = in[at + (size_t)j];
    at += (size_t)S;
    sort_plan(score.data(), S, RISK_COST, keys, idx);
    for (int v : idx) out.push_back((double)v);
  }
  need(at == in.size(), "sort: words behind the last array");
  return write_all(out_path, out);
}

static int run_risk(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() >= 4, "risk takes B, S, column and L");
  const long B = (long)in[0], S = (long)in[1], column = (long)in[2], L = (long)in[3];
  need(S >= 1 && S <= RISK_MAX_SAMPLES && L >= 1 && L <= RISK_MAX_LEVELS && (column == 0 || column == 1), "risk: S, L or the column out of range");
  need((long)in.size() == 4 + L + 4 * B * S, "risk takes level[L] and score[B][S][4] behind the head");
  std::vector<double> out((size_t)(B * L * RISK_WORDS)), keys;
  std::vector<int> idx;
  for (long b = 0; b < B; ++b) {
    sort_plan(&in[(size_t)(4 + L)] + 4 * b * S, (int)S, (int)column, keys, idx);
    for (long l = 0; l < L; ++l) {  // wavefront 0: 64 lanes' shares and the butterfly
      const int k = risk_rank(in[(size_t)(4 + l)], (int)S);
      double sum[64], nxt[64];
      for (int lane = 0; lane < 64; ++lane) sum[lane] = risk_tail_lane(keys.data(), (int)S, k, lane);
      for (int off = 32; off >= 1; off >>= 1) {
        for (int lane = 0; lane < 64; ++lane) nxt[lane] = sum[lane] + sum[lane ^ off];
        for (int lane = 0; lane < 64; ++lane) sum[lane] = nxt[lane];
      }
      for (int lane = 1; lane < 64; ++lane) need(!std::memcmp(&sum[lane], &sum[0], sizeof(double)), "the butterfly leaves every lane the same");
      risk_words(keys[(size_t)k], sum[0], idx[(size_t)k], (int)S - k, (int)column, &out[(size_t)((b * L + l) * RISK_WORDS)]);
    }
  }
  return write_all(out_path, out);
}

static int run_select(const char *in_path, const char *out_path) {
  const std::vector<double> in = read_all(in_path);
  need(in.size() >= 9, "select takes a head of 9 words");
  const long V = (long)in[0], C = (long)in[1], L = (long)in[2];
  const SelectRule rule{(int32_t)in[3], (int32_t)in[4], in[5], in[6], in[7]};
  const bool risk_given = in[8] != 0.0;
  need(V >= 1 && C >= 1 && (long)in.size() == 9 + 8 * V * C + (risk_given ? 4 * V * C * L : 0), "select takes summary[C V][8] and risk[C V][L][4] behind the head");
  const double *summary = &in[9], *risk = risk_given ? summary + 8 * V * C : nullptr;
  std::vector<double> out((size_t)(V * (1 + SELECT_INFO)));
  for (long v = 0; v < V; ++v)  // k_select_plans' lanes
    out[(size_t)v] = (double)select_vehicle(rule, summary, risk, (int)L, (int)V, (int)C, (int)v, &out[(size_t)(V + SELECT_INFO * v)]);
  return write_all(out_path, out);
}

// refuse risk   handle score risk levels_given B S column n_levels level[8]                                            (16 values)
// refuse select handle rule objective level max_collision max_diverged min_clearance summary risk choice info plan gains out_plan
//               out_gains n_levels V C n                                                                                (19 values)
static int run_refuse(int n, char **v) {
  auto L = [&](int k) { return std::strtol(v[k], nullptr, 0); };
  auto P = [&](int k) { return (const void *)(uintptr_t)std::strtoull(v[k], nullptr, 0); };
  auto D = [&](int k) { return std::strtod(v[k], nullptr); };
  const char *why = "?";
  if (!std::strcmp(v[0], "risk") && n == 17) {
    double levels[8];
    for (int k = 0; k < 8; ++k) levels[k] = D(9 + k);
    const RiskScoresCall c{L(1) != 0, P(2), P(3), L(4) ? levels : nullptr, L(5), L(6), L(7), L(8)};
    why = risk_scores_refusal(c);
  } else if (!std::strcmp(v[0], "select") && n == 20) {
    const SelectPlansCall c{L(1) != 0, L(2) != 0, L(3), L(4), D(5), D(6), D(7), P(8), P(9), P(10), P(11), P(12), P(13), P(14), P(15), L(16), L(17), L(18), L(19)};
    why = select_plans_refusal(c);
  } else {
    std::fprintf(stderr, "refuse: which call, and how many facts?\n");
    return 2;
  }
  std::printf("%s\n", why ? why : "ok");
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "rank")) {
    const int S = (int)std::strtol(argv[2], nullptr, 0);
    for (int k = 3; k < argc; ++k) std::printf("%d%c", risk_rank(std::strtod(argv[k], nullptr), S), k + 1 < argc ? ' ' : '\n');
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "sort")) return run_sort(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "risk")) return run_risk(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "select")) return run_select(argv[2], argv[3]);
  if (argc >= 3 && !std::strcmp(argv[1], "refuse")) return run_refuse(argc - 2, argv + 2);
  std::fprintf(stderr, "usage: %s sort|rank|risk|select|refuse ...\n", argv[0]);
  return 2;
}
