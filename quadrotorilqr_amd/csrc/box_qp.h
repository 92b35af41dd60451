// box_qp.h -- the box-constrained QP of control-limited DDP (Tassa, Mansard & Todorov, ICRA 2014) for the per-rotor thrust limits
// (qilqr_set_control_limits, an extension the reference does not have):
//
//     minimise  1/2 x^T H x + g^T x   subject to  l <= x <= h        (H = Q_uu, g = Q_u, l = lo - u_i, h = hi - u_i; 4 x 4)
//
// by projected Newton with FIXED constants and a FIXED order of decisions, so that the device (k_backward<true, double, ControlLimits>,
// every lane on the same broadcast data), the host build of tests/host_box_harness.cpp and the NumPy restatement
// (tests/limited_numpy_ilqr.py) take the same decisions:
//
//     x = clamp(0, l, h); f = f(x); C_prev = none
//     for it in 0 .. 15:
//       grad = g + H x;  C = {a : (x_a == l_a and grad_a > 0) or (x_a == h_a and grad_a < 0)}
//       |C| == 4: stop
//       factor H with the rows / columns in C replaced by identity (unpivoted LDL^T); a pivot <= 0: FAILED
//       it > 0, C == C_prev and the last step was 1: stop (x is the optimum on the free set)
//       d_F = -H_FF^-1 (g_F + H_FC x_C) - x_F, d_C = 0
//       step = 1; up to 30 trials: x_t = clamp(x + step d, l, h); accept if f(x_t) - f <= 0.1 step grad^T d, else step *= 0.6
//       no trial accepted: stop
//       x, f, C_prev = x_t, f(x_t), C
//     C and the masked factor once more at the final x (the factor of the feedback gain K: K_C = 0, K_F = -H_FF^-1 Q_ux,F)
//
// Lane-local and branch-uniform on the device (the data is identical in every lane).  Compiles under g++ (QILQR_HD, se3_math.h).
#pragma once

#include "se3_math.h"

namespace qilqr {

// per-rotor bounds on u0..u3 (N); +-inf where a side is open.  A kernel argument of its own, only of the kernels of the extension.
struct ControlLimits {
  double lo[4], hi[4];
};

constexpr int BOXQP_ITERS = 16;          // projected Newton iterations
constexpr int BOXQP_TRIALS = 30;         // line-search trials per iteration
constexpr double BOXQP_ARMIJO = 0.1;     // sufficient decrease
constexpr double BOXQP_BACKTRACK = 0.6;  // step factor per rejected trial
constexpr unsigned BOXQP_NONE = 0x10u;   // "no clamped set yet" (a set is a 4-bit mask)

// (a NaN stays a NaN: both comparisons are false)
QILQR_HD double box_clamp(double c, double lo, double hi) { return c < lo ? lo : (c > hi ? hi : c); }

// unpivoted LDL^T of H (lower triangle read) with the rows and columns in the mask `clamped` replaced by identity
struct BoxLdl {
  double l10, l20, l30, l21, l31, l32, d0, d1, d2, d3;
};
QILQR_HD bool box_ldl(const double H[16], unsigned clamped, BoxLdl &f) {
  double m[16];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) m[a * 4 + b] = (((clamped >> a) | (clamped >> b)) & 1u) ? (a == b ? 1.0 : 0.0) : H[a * 4 + b];
  f.d0 = m[0];
  const double c10 = m[4], c20 = m[8], c30 = m[12];
  f.l10 = c10 / f.d0; f.l20 = c20 / f.d0; f.l30 = c30 / f.d0;
  f.d1 = m[5] - f.l10 * c10;
  const double c21 = m[9] - f.l20 * c10, c31 = m[13] - f.l30 * c10;
  f.l21 = c21 / f.d1; f.l31 = c31 / f.d1;
  f.d2 = m[10] - f.l20 * c20 - f.l21 * c21;
  const double c32 = m[14] - f.l30 * c20 - f.l31 * c21;
  f.l32 = c32 / f.d2;
  f.d3 = m[15] - f.l30 * c30 - f.l31 * c31 - f.l32 * c32;
  return !(f.d0 <= 0.0 || f.d1 <= 0.0 || f.d2 <= 0.0 || f.d3 <= 0.0);
}
// z = M^-1 r with the factors of box_ldl (M the masked matrix)
QILQR_HD void box_ldl_solve(const BoxLdl &f, const double r[4], double z[4]) {
  const double y0 = r[0];
  const double y1 = r[1] - f.l10 * y0;
  const double y2 = r[2] - f.l20 * y0 - f.l21 * y1;
  const double y3 = r[3] - f.l30 * y0 - f.l31 * y1 - f.l32 * y2;
  z[3] = y3 / f.d3;
  z[2] = y2 / f.d2 - f.l32 * z[3];
  z[1] = y1 / f.d1 - f.l21 * z[2] - f.l31 * z[3];
  z[0] = y0 / f.d0 - f.l10 * z[1] - f.l20 * z[2] - f.l30 * z[3];
}
QILQR_HD void box_grad(const double H[16], const double g[4], const double x[4], double grad[4]) {
  for (int a = 0; a < 4; ++a) grad[a] = g[a] + (H[a * 4 + 0] * x[0] + H[a * 4 + 1] * x[1] + H[a * 4 + 2] * x[2] + H[a * 4 + 3] * x[3]);
}
QILQR_HD double box_objective(const double H[16], const double g[4], const double x[4]) {
  double f = 0.0;
  for (int a = 0; a < 4; ++a) {
    const double hx = H[a * 4 + 0] * x[0] + H[a * 4 + 1] * x[1] + H[a * 4 + 2] * x[2] + H[a * 4 + 3] * x[3];
    f += x[a] * (0.5 * hx + g[a]);
  }
  return f;
}
QILQR_HD unsigned box_clamped_set(const double x[4], const double l[4], const double h[4], const double grad[4]) {
  unsigned c = 0;
  for (int a = 0; a < 4; ++a)
    if ((x[a] == l[a] && grad[a] > 0.0) || (x[a] == h[a] && grad[a] < 0.0)) c |= 1u << a;
  return c;
}

// The QP.  x: the feed-forward k; clamped: the final clamped set; f: the masked factor for K.  false: a pivot <= 0 (FAILED).
QILQR_HD bool box_qp(const double H[16], const double g[4], const double l[4], const double h[4], double x[4], unsigned &clamped,
                     BoxLdl &f) {
  for (int a = 0; a < 4; ++a) x[a] = box_clamp(0.0, l[a], h[a]);
  double fx = box_objective(H, g, x);
  unsigned prev = BOXQP_NONE;
  bool full = false;
  for (int it = 0; it < BOXQP_ITERS; ++it) {
    double grad[4];
    box_grad(H, g, x, grad);
    const unsigned c = box_clamped_set(x, l, h, grad);
    if (c == 0xfu) break;
    if (!box_ldl(H, c, f)) return false;
    if (it > 0 && c == prev && full) break;
    double r[4], z[4], d[4];
    for (int a = 0; a < 4; ++a) {
      double s = g[a];
      for (int b = 0; b < 4; ++b)
        if ((c >> b) & 1u) s += H[a * 4 + b] * x[b];
      r[a] = ((c >> a) & 1u) ? 0.0 : s;
    }
    box_ldl_solve(f, r, z);
    for (int a = 0; a < 4; ++a) d[a] = ((c >> a) & 1u) ? 0.0 : -z[a] - x[a];
    const double gd = grad[0] * d[0] + grad[1] * d[1] + grad[2] * d[2] + grad[3] * d[3];
    double step = 1.0, xt[4], ft = 0.0;
    bool accepted = false;
    for (int t = 0; t < BOXQP_TRIALS; ++t) {
      for (int a = 0; a < 4; ++a) xt[a] = box_clamp(x[a] + step * d[a], l[a], h[a]);
      ft = box_objective(H, g, xt);
      if (ft - fx <= BOXQP_ARMIJO * step * gd) {
        accepted = true;
        break;
      }
      step *= BOXQP_BACKTRACK;
    }
    if (!accepted) break;
    for (int a = 0; a < 4; ++a) x[a] = xt[a];
    fx = ft;
    prev = c;
    full = (step == 1.0);
  }
  double grad[4];
  box_grad(H, g, x, grad);
  clamped = box_clamped_set(x, l, h, grad);
  return box_ldl(H, clamped, f);
}

// one column of the feedback gain: K[:, j] = -H_FF^-1 Q_ux[F, j] on the free rows, 0 on the clamped rows
QILQR_HD void box_gain_column(const BoxLdl &f, unsigned clamped, const double qux[4], double kcol[4]) {
  double r[4], z[4];
  for (int a = 0; a < 4; ++a) r[a] = ((clamped >> a) & 1u) ? 0.0 : qux[a];
  box_ldl_solve(f, r, z);
  for (int a = 0; a < 4; ++a) kcol[a] = ((clamped >> a) & 1u) ? 0.0 : -z[a];
}

}  // namespace qilqr
