// Fleet deconfliction on the host: the routines of quadrotorilqr_amd/csrc/fleet_math.h that the kernels of fleet.hip call -- the pair's
// distance, the order, the list, the fit, the selection, the row rule of the device-side sphere setter -- and the two rules of
// fleet_launch.h, compiled with g++ into a stand-alone program.  The partners of an ego are cut into chunks of a size given on the
// command line, each chunk's list is formed on its own and the lists are merged, as k_fleet_pairs and k_fleet_select do it.
//   run IN OUT          IN: B n V K chunk dt radius weight range conflict flags, then plan[B][n][18] (all doubles)
//                       OUT: summary[B][8] nbr[B][K][4] spheres[B][K][8] counts[B] fit[B][8]
//   bob IN OUT          IN: B K has_counts, spheres[B][K][8], counts[B]
//                       OUT: the table by bob_set_problem [bob_count], counts[B], dropped, the table by bob_relayout [bob_count]
//   refuse ...          fleet_refusal of the facts given (tests/test_fleet_cpu.py: ORDER)        refuse_bob ...   bob_set_refusal
//   sizeof              sizeof(qilqr_fleet_rule)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/quadrotor_ilqr.h"
#include "../quadrotorilqr_amd/csrc/fleet_launch.h"

using namespace qilqr;

static std::vector<double> read_all(const char *path) {
  FILE *f = std::fopen(path, "rb");
  if (!f) std::exit(2);
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> v((size_t)bytes / sizeof(double));
  if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
  return v;
}
static void write_all(const char *path, const std::vector<double> &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f || std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(2);
  std::fclose(f);
}
static double num(const char *s) { return std::strtod(s, nullptr); }  // ("nan", "inf" and "-inf" included)

static int run(const char *in, const char *out) {
  const std::vector<double> w = read_all(in);
  const int B = (int)w[0], n = (int)w[1], V = (int)w[2], K = (int)w[3], chunk = (int)w[4];
  const double dt = w[5];
  const FleetSelectRule rule{w[6], w[7], fleet_square(w[8]), fleet_square(w[9]), (unsigned)w[10]};
  const double *plan = w.data() + 11;
  std::vector<double> fits((size_t)B * FLEET_FIT);
  for (int b = 0; b < B; ++b) fleet_fit(plan + (size_t)b * n * 18 + 1, 18, n, dt, fits.data() + (size_t)b * FLEET_FIT);
  const int C = (V + chunk - 1) / chunk;
  std::vector<double> summary((size_t)B * FLEET_SUMMARY), nbr((size_t)B * K * FLEET_NBR), spheres((size_t)B * K * OB_BWORDS), counts((size_t)B);
  std::vector<double> pd2((size_t)C * K), md2((size_t)K);
  std::vector<int> prow((size_t)C * K), pknot((size_t)C * K), mrow((size_t)K), mknot((size_t)K);
  std::vector<FleetBest> pbest((size_t)C);
  for (int b = 0; b < B; ++b) {
    const int g = b / V, ev = b % V;
    const double *pa = plan + (size_t)b * n * 18 + 1;
    // a chunk's list and FleetBest: what one wavefront of k_fleet_pairs leaves for this ego
    for (int c = 0; c < C; ++c) {
      const FleetList list{pd2.data() + (size_t)c * K, prow.data() + (size_t)c * K, pknot.data() + (size_t)c * K, 1, K};
      fleet_list_clear(list);
      double wd2 = fleet_inf();
      int wrow = FLEET_NO_ROW;
      FleetBest best = fleet_best_none();
      for (int pv = c * chunk; pv < V && pv < (c + 1) * chunk; ++pv) {
        if (pv == ev) continue;
        const int row = g * V + pv;
        const double *pb = plan + (size_t)row * n * 18 + 1;
        double m = fleet_inf();
        int mk = -1;
        for (int i = 0; i < n; ++i) fleet_pair_step(fleet_d2(pa[i * 18], pa[i * 18 + 1], pa[i * 18 + 2], pb[i * 18], pb[i * 18 + 1], pb[i * 18 + 2]), i, m, mk);
        fleet_best_pair(best, m, row, mk, rule.conflict2);
        if (!(rule.flags & FLEET_YIELD_TO_LOWER) || pv < ev) fleet_list_offer(list, wd2, wrow, m, row, mk);
      }
      pbest[(size_t)c] = best;
    }
    // the merge: k_fleet_select
    const FleetList list{md2.data(), mrow.data(), mknot.data(), 1, K};
    fleet_list_clear(list);
    double wd2 = fleet_inf();
    int wrow = FLEET_NO_ROW;
    FleetBest best = fleet_best_none();
    for (int c = 0; c < C; ++c) {
      for (int k = 0; k < K; ++k) {
        if (prow[(size_t)c * K + k] == FLEET_NO_ROW) break;
        fleet_list_offer(list, wd2, wrow, pd2[(size_t)c * K + k], prow[(size_t)c * K + k], pknot[(size_t)c * K + k]);
      }
      fleet_best_merge(best, pbest[(size_t)c]);
    }
    int32_t count = 0;
    fleet_select_write(list, best, fits.data(), rule, nbr.data() + (size_t)b * K * FLEET_NBR, spheres.data() + (size_t)b * K * OB_BWORDS, &count,
                       summary.data() + (size_t)b * FLEET_SUMMARY);
    counts[(size_t)b] = count;
  }
  std::vector<double> o;
  for (const auto *v : {&summary, &nbr, &spheres, &counts, &fits}) o.insert(o.end(), v->begin(), v->end());
  write_all(out, o);
  return 0;
}

static int bob(const char *in, const char *out) {
  const std::vector<double> w = read_all(in);
  const int B = (int)w[0], K = (int)w[1];
  const bool has_counts = w[2] != 0.0;
  const double *spheres = w.data() + 3, *counts = spheres + (size_t)B * K * OB_BWORDS;
  const long words = bob_count(B, K), rows = (B + OB_TILE - 1) / OB_TILE * OB_TILE;
  std::vector<double> tab((size_t)words, -1.0), kept((size_t)B), relaid((size_t)words);
  int dropped = 0;
  for (long row = 0; row < rows; ++row) {  // (a lane of k_bob_set each; the last tile's padding rows included)
    if (row < B) kept[(size_t)row] = bob_set_problem(spheres + (size_t)row * K * OB_BWORDS, has_counts ? (int)counts[row] : K, K, tab.data(), row, &dropped);
    else bob_set_problem(nullptr, 0, K, tab.data(), row, &dropped);
  }
  bob_relayout(spheres, B, K, relaid.data());
  std::vector<double> o(tab);
  o.insert(o.end(), kept.begin(), kept.end());
  o.push_back(dropped);
  o.insert(o.end(), relaid.begin(), relaid.end());
  write_all(out, o);
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "run" && argc == 4) return run(argv[2], argv[3]);
  if (mode == "bob" && argc == 4) return bob(argv[2], argv[3]);
  if (mode == "sizeof") return std::printf("%zu\n", sizeof(qilqr_fleet_rule)), 0;
  if (mode == "refuse" && argc == 20) {
    char **a = argv + 2;  // rule radius weight range conflict flags reserved plan summary nbr spheres counts B n V K handle f32
    FleetCall c{};
    c.rule = std::atoi(a[0]) != 0;
    c.radius = num(a[1]); c.weight = num(a[2]); c.range = num(a[3]); c.conflict = num(a[4]);
    c.flags = std::strtoul(a[5], nullptr, 10);
    c.reserved = std::strtoul(a[6], nullptr, 10);
    c.plan = (const void *)std::strtoull(a[7], nullptr, 10);
    c.summary = (const void *)std::strtoull(a[8], nullptr, 10);
    c.nbr = (const void *)std::strtoull(a[9], nullptr, 10);
    c.spheres = (const void *)std::strtoull(a[10], nullptr, 10);
    c.counts = (const void *)std::strtoull(a[11], nullptr, 10);
    c.B = std::atol(a[12]); c.n = std::atol(a[13]); c.V = std::atol(a[14]); c.K = std::atol(a[15]);
    c.handle = std::atoi(a[16]) != 0;
    c.f32 = std::atoi(a[17]) != 0;
    const char *why = fleet_refusal(c);
    return std::printf("%s\n", why ? why : "ok"), 0;
  }
  if (mode == "refuse_bob" && argc == 9) {
    char **a = argv + 2;  // handle f32 spheres counts dropped B K
    const BobSetCall c{std::atoi(a[0]) != 0, std::atoi(a[1]) != 0, (const void *)std::strtoull(a[2], nullptr, 10), (const void *)std::strtoull(a[3], nullptr, 10),
                       (const void *)std::strtoull(a[4], nullptr, 10), std::atol(a[5]), std::atol(a[6])};
    const char *why = bob_set_refusal(c);
    return std::printf("%s\n", why ? why : "ok"), 0;
  }
  std::fprintf(stderr, "usage: host_fleet_harness run|bob IN OUT | refuse ... | refuse_bob ... | sizeof\n");
  return 2;
}
