// obstacles.h -- spherical obstacle penalties in the knot cost (qilqr_set_obstacles, an extension the reference does not have): "fly from A
// to B and stay clear of these spheres" as a soft cost term.
//
// An obstacle is a sphere {cx, cy, cz, radius, weight}; up to QILQR_MAX_OBSTACLES of them are shared by every problem of a handle.  At every
// knot i (all n, the last included), with p = (tx, ty, tz) the knot's position, d_j = |p - c_j| and h_j = radius_j - d_j, the knot cost is
//     tracking_cost + sum_j weight_j h_j^2      over the obstacles with h_j > 0,
// the terms added one at a time in index order after the tracking cost.  An inactive obstacle (h_j <= 0, or a NaN h_j) touches no
// accumulator: a handle whose obstacles no knot reaches gives the bits of a handle without obstacles.
//
// Differentials in the tangent order [rho, theta, dv, dw] and the reference's factor-2 convention (C_x = 2 dx^T Q J, C_xx = 2 J^T Q J).
// Under the right perturbation X Exp(delta) the position moves by R rho to first order (R the knot's attitude) and not at all with theta,
// so with n_j = (p - c_j) / d_j and m_j = R^T n_j:
//     C_x[0:3]        += -2 weight_j h_j m_j
//     C_xx[0:3, 0:3]  += 2 weight_j m_j m_j^T      (Gauss-Newton only, as the tracking cost's Hessian: Q_xx stays positive
//                                                   semi-definite, and the unpivoted LDL^T of the symmetric kernels stays valid)
// d_j == 0 exactly: the cost term is weight_j radius_j^2 and the differentials get nothing (the direction is undefined).
//
// Each increment is formed once and added to every record entry it belongs to, so C_xx[k][l] and C_xx[l][k] receive the same bits.
//
// Per-problem, moving spheres (qilqr_set_batch_obstacles): problem b has counts[b] <= K spheres of OB_BWORDS doubles
// {cx, cy, cz, vx, vy, vz, radius, weight}.  At knot i the centre is c + t_i v, t_i = i dt, per axis fma(t_i, v, c), so a sphere with
// v = 0 is centred at c exactly; from there the term is the one above, through the same per-sphere routine (add_sphere): a static
// per-problem sphere gives the bits of the shared sphere with the same {c, radius, weight}.  Order within a knot: the tracking cost,
// the shared spheres, then the problem's own, each in index order.  The centre depends on time only, so the differentials need no new
// terms.  The device table is tiled by 64 problems, [ceil(B / 64)][K][OB_BWORDS][64] (bob_index): word w of sphere j for the 64
// problems of a cost wavefront is one contiguous 512-byte load.  Rows j >= counts[b] are never read.
// Compiles under g++ (QILQR_HD, se3_math.h): tests/host_obstacles_harness.cpp and tests/host_batch_obstacles_harness.cpp check it
// against NumPy.
#pragma once

#include <cmath>
#include <cstdint>

#include "batch_models.h"
#include "se3_math.h"

namespace qilqr {

constexpr int OB_MAX = 64;   // QILQR_MAX_OBSTACLES of include/quadrotor_ilqr.h
constexpr int OB_WORDS = 5;  // cx, cy, cz, radius, weight
constexpr int OB_CX = 0, OB_RADIUS = 3, OB_WEIGHT = 4;

// the table as a kernel argument: [count][OB_WORDS], fp64, shared by every problem
struct Obstacles {
  const double *tab;
  int count;
};

// the obstacles beside per-problem models (qilqr_set_batch_models): ONE trailing argument of k_linearize that carries both -- a kernel of
// this extension, under a name of its own, not another instantiation of the models' kernels
struct ModelsObstacles {
  BatchModels models;
  Obstacles obstacles;
};
// the per-problem spheres (qilqr_set_batch_obstacles) beside the shared ones: ONE trailing argument of k_linearize that carries both
// tables (shared.count may be 0).  tab: [ceil(B / 64)][K][OB_BWORDS][64] (bob_index), counts: int32[B], both indexed by the problem's
// row: st.orig[slot] when by_orig (a compacting batch solve, after k_init has written the map), st.row0 + slot otherwise
struct ProblemObstacles {
  Obstacles shared;
  const double *tab;
  const int *counts;
  int K;
  int by_orig;
};
// ... and beside per-problem models (the form ModelsObstacles is for the shared table)
struct ModelsProblemObstacles {
  BatchModels models;
  ProblemObstacles obstacles;
};
// the tables out of a kernel's trailing pack, whichever form carries them
template <typename... P>
QILQR_HD const BatchModels &pack_models(const P &...p) {
  if constexpr (pack_has<ModelsObstacles, P...>) return pack_get<ModelsObstacles>(p...).models;
  else if constexpr (pack_has<ModelsProblemObstacles, P...>) return pack_get<ModelsProblemObstacles>(p...).models;
  else return pack_get<BatchModels>(p...);
}
template <typename... P>
QILQR_HD const ProblemObstacles &pack_problem_obstacles(const P &...p) {
  if constexpr (pack_has<ModelsProblemObstacles, P...>) return pack_get<ModelsProblemObstacles>(p...).obstacles;
  else return pack_get<ProblemObstacles>(p...);
}
template <typename... P>
QILQR_HD const Obstacles &pack_obstacles(const P &...p) {
  if constexpr (pack_has<ModelsObstacles, P...>) return pack_get<ModelsObstacles>(p...).obstacles;
  else if constexpr (pack_has<ProblemObstacles, P...> || pack_has<ModelsProblemObstacles, P...>) return pack_problem_obstacles(p...).shared;
  else return pack_get<Obstacles>(p...);
}

// One sphere's term at one knot (pt: an 18-double knot), added into the knot cost, the pose gradient g = C_x[0:3] and the pose block
// H = C_xx[0:3, 0:3] (row-major, both triangles).  sp: the sphere as OB_WORDS values {cx, cy, cz, radius, weight} (the weight is read
// only for an active sphere).  `begin` is called once per knot, before the first active sphere touches an accumulator (`any` records
// that it has been, and R then holds the knot's attitude): the caller fills g and H there (k_linearize reads them back from the knot's
// record), so a knot no sphere reaches costs no record access.  Every sphere of either table goes through here.
template <typename T, typename Begin>
QILQR_HD void add_sphere(const T *sp, const T *pt, T &cost, T g[3], T H[9], T R[9], bool &any, Begin &&begin) {
  const T e[3] = {pt[1] - sp[OB_CX], pt[2] - sp[OB_CX + 1], pt[3] - sp[OB_CX + 2]};
  const T d = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  const T h = sp[OB_RADIUS] - d;
  if (!(h > T(0))) return;
  if (!any) {
    any = true;
    begin();
    const T q[4] = {pt[5], pt[6], pt[7], pt[4]};  // (x, y, z, w)
    quat_to_R(q, R);
  }
  const T w = sp[OB_WEIGHT];
  cost += (w * h) * h;
  if (!(d > T(0))) return;  // d == 0: no direction, no differentials
  const T nv[3] = {e[0] / d, e[1] / d, e[2] / d};
  T m[3];
  mat3_tvec(R, nv, m);  // m = R^T n
  const T gc = T(-2) * w * h, hc = T(2) * w;
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] += gc * m[k];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = k; l < 3; ++l) {
      const T inc = (hc * m[k]) * m[l];
      H[3 * k + l] += inc;
      if (l != k) H[3 * l + k] += inc;
    }
}

// The shared table's terms of one knot (tab: count x OB_WORDS), in index order.  Returns whether any obstacle was active.
template <typename T, typename Begin>
QILQR_HD bool add_obstacles(const T *tab, int count, const T *pt, T &cost, T g[3], T H[9], Begin &&begin) {
  bool any = false;
  T R[9];
  for (int j = 0; j < count; ++j) add_sphere(tab + j * OB_WORDS, pt, cost, g, H, R, any, begin);
  return any;
}
// ... the same into accumulators the caller keeps (the shared table ahead of a problem's own spheres)
template <typename T, typename Begin>
QILQR_HD void add_shared_spheres(const T *tab, int count, const T *pt, T &cost, T g[3], T H[9], T R[9], bool &any, Begin &&begin) {
  for (int j = 0; j < count; ++j) add_sphere(tab + j * OB_WORDS, pt, cost, g, H, R, any, begin);
}

// ---- per-problem, moving spheres
constexpr int OB_BWORDS = 8;  // cx, cy, cz, vx, vy, vz, radius, weight (QILQR_OBSTACLE_WORDS)
constexpr int OB_BV = 3, OB_BRADIUS = 6, OB_BWEIGHT = 7;
constexpr int OB_TILE = 64;   // problems per tile of the device table: the lanes of a cost wavefront

// where word w of sphere j of problem `row` lives in the device table of K spheres per problem
QILQR_HD long bob_index(long row, int K, int j, int w) {
  return (((row / OB_TILE) * K + j) * OB_BWORDS + w) * OB_TILE + row % OB_TILE;
}
// doubles of the device table for B problems
inline long bob_count(long B, int K) { return (B + OB_TILE - 1) / OB_TILE * (long)K * OB_BWORDS * OB_TILE; }

// one moving sphere at time t: the centre fma(t, v, c) per axis (c exactly for v = 0), then add_sphere.  sp: word 0 of the sphere,
// ws: the distance between its words (OB_TILE in the device table, 1 in a row of the caller's layout)
template <typename T, typename Begin>
QILQR_HD void add_moving_sphere(const T *sp, int ws, T t, const T *pt, T &cost, T g[3], T H[9], T R[9], bool &any, Begin &&begin) {
  const T s5[OB_WORDS] = {fma(t, sp[OB_BV * ws], sp[0]), fma(t, sp[(OB_BV + 1) * ws], sp[ws]), fma(t, sp[(OB_BV + 2) * ws], sp[2 * ws]),
                          sp[OB_BRADIUS * ws], sp[OB_BWEIGHT * ws]};
  add_sphere(s5, pt, cost, g, H, R, any, begin);
}
// Problem `row`'s spheres 0 .. jend - 1 of the device table at time t; those at or beyond `count` do nothing (k_linearize runs every
// lane of a wavefront to the wavefront's largest count, jend; the host harness passes jend = count)
template <typename T, typename Begin>
QILQR_HD void add_problem_spheres(const T *tab, int K, long row, int count, int jend, T t, const T *pt, T &cost, T g[3], T H[9], T R[9],
                                  bool &any, Begin &&begin) {
  for (int j = 0; j < jend; ++j)
    if (j < count) add_moving_sphere(tab + bob_index(row, K, j, 0), OB_TILE, t, pt, cost, g, H, R, any, begin);
}

// ---- host side of qilqr_set_batch_obstacles
// the caller's B x K x OB_BWORDS (row-major) -> the device layout (bob_count(B, K) doubles; the rows of a partial last tile are zeros)
inline void bob_relayout(const double *spheres, long B, int K, double *out) {
  for (long k = 0; k < bob_count(B, K); ++k) out[k] = 0.0;
  for (long b = 0; b < B; ++b)
    for (int j = 0; j < K; ++j)
      for (int w = 0; w < OB_BWORDS; ++w) out[bob_index(b, K, j, w)] = spheres[(b * K + j) * OB_BWORDS + w];
}
// The setter's checks of a table (spheres NULL, counts NULL and B = K = 0 clear it; counts NULL: all K).  Returns 0, or 1 with the
// reason and the first bad index (b, j; -1 where none applies).  Only the used rows j < counts[b] are looked at.
struct BobCheck {
  const char *why = nullptr;
  long b = -1;
  int j = -1;
};
inline int bob_check(const double *spheres, const int32_t *counts, long B, long K, int max_k, BobCheck *out) {
  BobCheck &e = *out;
  e = BobCheck{};
  if (!spheres && !counts && B == 0 && K == 0) return 0;
  if (!spheres || B <= 0) return e.why = "B > 0 problems of K spheres, or spheres = counts = NULL and B = K = 0 to clear them", 1;
  if (K < 1 || K > max_k) return e.why = "K must be 1 ... QILQR_MAX_OBSTACLES", 1;
  for (long b = 0; b < B; ++b) {
    const long cnt = counts ? counts[b] : K;
    if (cnt < 0 || cnt > K) return e.why = "a count outside 0 ... K", e.b = b, 1;
    for (int j = 0; j < cnt; ++j) {
      const double *sp = spheres + (b * K + j) * OB_BWORDS;
      e.b = b;
      e.j = j;
      for (int w = 0; w < OB_BWORDS; ++w)
        if (!std::isfinite(sp[w])) return e.why = "a non-finite value", 1;
      if (!(sp[OB_BRADIUS] > 0.0)) return e.why = "radius <= 0", 1;
      if (!(sp[OB_BWEIGHT] >= 0.0)) return e.why = "weight < 0", 1;
    }
  }
  e = BobCheck{};
  return 0;
}

}  // namespace qilqr
