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
// Compiles under g++ (QILQR_HD, se3_math.h): tests/host_obstacles_harness.cpp checks it against NumPy.
#pragma once

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
// the two tables out of a kernel's trailing pack, whichever form carries them
template <typename... P>
QILQR_HD const BatchModels &pack_models(const P &...p) {
  if constexpr (pack_has<ModelsObstacles, P...>) return pack_get<ModelsObstacles>(p...).models;
  else return pack_get<BatchModels>(p...);
}
template <typename... P>
QILQR_HD const Obstacles &pack_obstacles(const P &...p) {
  if constexpr (pack_has<ModelsObstacles, P...>) return pack_get<ModelsObstacles>(p...).obstacles;
  else return pack_get<Obstacles>(p...);
}

// The obstacles' terms of one knot (pt: an 18-double knot), added into the knot cost, the pose gradient g = C_x[0:3] and the pose block
// H = C_xx[0:3, 0:3] (row-major, both triangles).  `begin` is called once, before the first active obstacle touches an accumulator: the
// caller fills g and H there (k_linearize reads them back from the knot's record), so a knot no obstacle reaches costs no record access.
// Returns whether any obstacle was active.  tab: count x OB_WORDS.
template <typename T, typename Begin>
QILQR_HD bool add_obstacles(const T *tab, int count, const T *pt, T &cost, T g[3], T H[9], Begin &&begin) {
  bool any = false;
  T R[9];
  for (int j = 0; j < count; ++j) {
    const T *sp = tab + j * OB_WORDS;
    const T e[3] = {pt[1] - sp[OB_CX], pt[2] - sp[OB_CX + 1], pt[3] - sp[OB_CX + 2]};
    const T d = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const T h = sp[OB_RADIUS] - d;
    if (!(h > T(0))) continue;
    if (!any) {
      any = true;
      begin();
      const T q[4] = {pt[5], pt[6], pt[7], pt[4]};  // (x, y, z, w)
      quat_to_R(q, R);
    }
    const T w = sp[OB_WEIGHT];
    cost += (w * h) * h;
    if (!(d > T(0))) continue;  // d == 0: no direction, no differentials
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
  return any;
}

}  // namespace qilqr
