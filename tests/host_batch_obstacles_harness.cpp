// host_batch_obstacles_harness.cpp -- CPU test harness (tests only, never part of the product library): the per-problem, moving spheres
// of quadrotorilqr_amd/csrc/obstacles.h (qilqr_set_batch_obstacles) compiled with g++, for tests/test_batch_obstacles_cpu.py.
#include <cstring>

#include "../quadrotorilqr_amd/csrc/obstacles.h"

using namespace qilqr;

extern "C" {
// One knot pt[18] as k_linearize's cost half sees it: the shared spheres (shared[n_shared x 5]), then problem `row`'s spheres
// 0 .. jend - 1 of the device table tab (K per problem) of which the first `count` are used, at time t.  cost, g[3], H[9] as in
// host_obstacles_harness.cpp.  Returns 1 if a sphere was active; *began counts the loader's calls (at most one).
int hb_knot(const double *pt, const double *shared, int n_shared, const double *tab, int K, long row, int count, int jend, double t,
            double *cost, double *g, double *H, int *began) {
  *began = 0;
  bool any = false;
  double R[9];
  auto begin = [&] { ++*began; };
  add_shared_spheres(shared, n_shared, pt, *cost, g, H, R, any, begin);
  add_problem_spheres(tab, K, row, count, jend, t, pt, *cost, g, H, R, any, begin);
  return any ? 1 : 0;
}
// one sphere row {cx, cy, cz, vx, vy, vz, radius, weight} of the caller's layout at time t
int hb_moving_sphere(const double *pt, const double *sp, double t, double *cost, double *g, double *H) {
  bool any = false;
  double R[9];
  add_moving_sphere(sp, 1, t, pt, *cost, g, H, R, any, [] {});
  return any ? 1 : 0;
}
// the shared table alone (what a qilqr_set_obstacles handle runs)
int hb_shared(const double *pt, const double *shared, int n_shared, double *cost, double *g, double *H) {
  return add_obstacles(shared, n_shared, pt, *cost, g, H, [] {}) ? 1 : 0;
}
long hb_count(long B, int K) { return bob_count(B, K); }
long hb_index(long row, int K, int j, int w) { return bob_index(row, K, j, w); }
void hb_relayout(const double *spheres, long B, int K, double *out) { bob_relayout(spheres, B, K, out); }
// the setter's checks: 0, or 1 with the reason (why[cap]) and the first bad (b, j)
int hb_check(const double *spheres, const int *counts, long B, long K, long *b, int *j, char *why, int cap) {
  BobCheck e;
  const int rc = bob_check(spheres, counts, B, K, OB_MAX, &e);
  *b = e.b;
  *j = e.j;
  std::strncpy(why, e.why ? e.why : "", cap - 1);
  why[cap - 1] = 0;
  return rc;
}
}
