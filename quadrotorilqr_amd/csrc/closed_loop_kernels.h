// closed_loop_kernels.h -- k_closed_loop: the plan's feedback law flown from given states (qilqr_closed_loop[_device]).  On plain arrays
// of the caller, sample (b, j) of B problems x S samples:
//   x = x0[b, j] at knot i0;  for i = i0 .. i1:
//     dx = x (-) plan[b, i]                                   (se3_rminus_fast and the velocity differences, as rollout_problem forms them)
//     u  = plan[b, i, 14:18] + K_i dx                         (control_law's three partial sums per row; the feed-forward k is not read:
//                                                              the law at alpha = 0), clamped to the thrust limits while they are set
//     out[b, j, i] = {plan[b, i, 0], x, u}                    (only with an out_traj)
//     x <- one dynamics step under u, if i < i1               (rollout_problem's: body_acceleration_fast / se3_rplus_fast, or rk4_step,
//                                                              with model b S + j while per-problem models are set)
//   stats[b, j] = {max_i |dx_i[0:3]|, max_i |dx_i[3:6]|, |dx_i1|, clamped (knot, rotor) pairs}      (Euclidean norms; only with out_stats)
// The per-sample routine, closed_loop_sample, is rollout_problem (se3_math.h) with three changes: the state starts at x0 and knot i0, the
// operands of a knot come through a Fetch (so that a wavefront can share them), and the statistics ride on the dx the law needs anyway.
// Its arithmetic is one text for every form, so a sample's bits depend on its own inputs only.
//
// TWO FORMS of one kernel template, chosen by closed_loop_shared_form (the one place):
//   shared-operand (where its wavefronts are at least 63 / 64 full): a block is one wavefront of 64 samples of ONE problem.  The plan
//       knot and the 48 feedback gains are wave-uniform: 33 sixteen-byte pairs, loaded once per wavefront and knot by lanes 0..32 --
//       two knots ahead, into a register -- written to a double-buffered LDS image one knot ahead, and read by every lane at one
//       address (a broadcast, no bank conflict).  One barrier per knot.  Lanes past S fly a copy of sample S - 1 and store nothing.
//   flattened (every other S; S = 1 is the policy evaluation of mpc.RecedingHorizon.control): a lane per (b, j), per-lane loads.
// Part of closed_loop.hip's translation unit (gfx950 only); the per-sample routine is QILQR_HD and compiles under g++
// (tests/host_closed_loop_harness.cpp).
//
// THE SCORED FLIGHT (qilqr_closed_loop_scored[_device]; k_closed_loop_scored, compiled by closed_loop_scored.hip): two compile-time switches
// of the same routine.  With both off it is the routine above, statement for statement.
//   WRENCH: a disturbance {F (world frame, N), tau (body frame, N m)} per sample, constant or one row per step, held over the step from
//       knot i to i + 1.  It enters the body acceleration where thrust and moment do (cl_disturbed_acceleration: the order of the added
//       operations is written there, once, for both integrators and both forms).  Per lane: three sixteen-byte loads per knot.
//   SCORE: per sample {cost, min_clearance, knot_of_min_clearance, knots_in_collision} over knots i0 .. i1.  At knot i, after the law, the
//       clamp, the statistics and the trajectory store and BEFORE the step (the cost's temporaries are dead when the step's become live):
//           kc = knot_cost(Q_i, R, {flown state, applied control}, desired_i)      (se3_math.h, as it is: the general form, any Q)
//           for the shared spheres, then the problem's own, each in index order:   (cl_score_sphere: add_sphere's value terms restated,
//               h = radius - |p - c|;  if h > 0: kc += (weight h) h;                 because the clearance needs h of an inactive sphere too)
//               clear = min(clear, -h)                                              (-h is |p - c| - radius exactly)
//           cost += kc;  the smallest clearance so far, its knot (the first on ties) and the count of knots with clear < 0 follow.
//       The operands of the score that are the same for every sample of a plan -- the desired knot, the knot's state weights, the shared
//       sphere table and the plan's row of the per-problem table -- are wave-uniform in the shared-operand form: they join the LDS image
//       (ClSharedScoreFetch), the desired knot and a scheduled Q double-buffered beside the plan knot, the rest written once.
#pragma once

#include "batch_models.h"
#include "box_qp.h"
#include "obstacles.h"
#include "se3_math.h"

// (as in se3_math.h: a * b + c fuses where the source says so and nowhere else, so that the law and the step have rollout_problem's bits)
#if defined(__clang__)
#pragma clang fp contract(on)
#endif

namespace qilqr {

constexpr int CL_BLOCK = 64;        // threads of a block of either form: one wavefront
constexpr int CL_STATE = 13;        // words of a state: t(3), q w,x,y,z, v_lin(3), v_ang(3)
constexpr int CL_STATS = 4;         // words of a sample's statistics
constexpr int CL_PLAN_PAIRS = 9;    // sixteen-byte pairs of a plan knot
constexpr int CL_GAIN_PAIRS = 24;   // ... of a knot's feedback gains (words 4..51 of its 52)
constexpr int CL_PAIRS = CL_PLAN_PAIRS + CL_GAIN_PAIRS;
// The rule of the forms, measured on an MI355X (profiles/microbench/closed_loop.py).  A launch's time goes with its
// wavefronts -- cdiv(S, 64) per plan in the shared-operand form against S / 64 in the flattened one -- and a shared-operand wavefront takes
// 0.93 (operands from HBM: every plan read by one wavefront) to 0.99 (operands from the cache: S = 1024) of the time of a flattened one
// whose lanes fly one plan: those 64 loads of one address are one request, so sharing wins back the issue of the loads and, through its
// loads two knots ahead, their latency -- not their bytes.  So the shared form is taken where it cannot lose: where its wavefronts are at
// least 63 / 64 full, S = 63, 64, 126..128, 189..192, ... and every S >= 4032.  There is no S from which it stays ahead: at S = 96 with
// the machine full it is 1.24 times slower.
QILQR_HD bool closed_loop_shared_form(int S) {
  const long waves = ((long)S + CL_BLOCK - 1) / CL_BLOCK;
  return 64l * S >= 63l * CL_BLOCK * waves;
}

struct ClosedLoopArgs {
  const double *plan;    // [B][n][18]
  const double *gains;   // [B][n][52]
  const double *x0;      // [B][S][13]
  double *out_traj;      // [B][S][n][18], or null
  double *out_stats;     // [B][S][4], or null
  int B, n, S, i0, i1;
};

// two consecutive words, 16-byte aligned (a knot is 144 bytes, a knot's gains 416, a sample's statistics 32, and the arrays are 16-byte
// aligned): one load or store on the device
QILQR_HD void cl_load_pair(const double *p, double &a, double &b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef double dv2 __attribute__((ext_vector_type(2)));
  const dv2 w = *reinterpret_cast<const dv2 *>(p);
  a = w[0];
  b = w[1];
#else
  a = p[0];
  b = p[1];
#endif
}
QILQR_HD void cl_store_pair(double *p, double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef double dv2 __attribute__((ext_vector_type(2)));
  dv2 w;
  w[0] = a;
  w[1] = b;
  *reinterpret_cast<dv2 *>(p) = w;
#else
  p[0] = a;
  p[1] = b;
#endif
}

// The operands of knot i by per-lane (or host) loads: plan / gains point at the problem's first knot.  K[col * 4 + a] is word
// 4 + col * 4 + a of the knot's gains, as control_law indexes them.
struct ClFlatFetch {
  const double *plan, *gains;
  QILQR_HD void operator()(int i, double pt[18], double K[48]) const {
    const double *p = plan + (long)i * 18, *g = gains + (long)i * 52 + 4;
#pragma unroll
    for (int e = 0; e < CL_PLAN_PAIRS; ++e) cl_load_pair(p + 2 * e, pt[2 * e], pt[2 * e + 1]);
#pragma unroll
    for (int e = 0; e < CL_GAIN_PAIRS; ++e) cl_load_pair(g + 2 * e, K[2 * e], K[2 * e + 1]);
  }
};

// u = u_i + K dx: control_law (se3_math.h) at alpha = 0 without reading k -- (u_i + 0 k) is u_i for every finite k.  The same three
// independent partial sums per row, summed in the same order.
QILQR_HD void closed_loop_law(const double pt[18], const double K[48], const double dx[12], double u[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    double k0 = 0.0, k1 = 0.0, k2 = 0.0;
#pragma unroll
    for (int col = 0; col < 4; ++col) {
      k0 += K[col * 4 + a] * dx[col];
      k1 += K[(col + 4) * 4 + a] * dx[col + 4];
      k2 += K[(col + 8) * 4 + a] * dx[col + 8];
    }
    u[a] = pt[14 + a] + ((k0 + k1) + k2);
  }
}

// ---- the scored flight: what the two switches of closed_loop_sample read
constexpr int CL_WRENCH = 6;  // words of a wrench: F_x, F_y, F_z (world frame), tau_x, tau_y, tau_z (body frame)
constexpr int CL_SCORE = 4;   // words of a sample's score

// where knot i's operands of the score are read from (global memory, or the block's LDS image)
struct ClKnotScore {
  const double *pd;  // the desired knot, 18 words
  const double *Q;   // the knot's state weights, 12 x 12 row-major
};
// the two sphere tables as one sample reads them
struct ClSpheres {
  const double *shared;  // [n_shared][OB_WORDS]
  int n_shared;
  const double *own;     // word 0 of sphere 0 of the sample's problem: word w of sphere j is own[j * ss + w * ws]
  int n_own, ws, ss;
};
// one sample's part of a scored flight
struct ClSampleExtras {
  const double *wrench;  // the sample's first row (WRENCH), 16-byte aligned
  int wrench_step;       // doubles between the rows of successive knots: 0 (one wrench for the flight) or CL_WRENCH
  ClSpheres spheres;     // (SCORE)
  double *score;         // the sample's CL_SCORE words, or null: nothing is stored (SCORE)
  // the running score (SCORE).  Kept here, not in locals of closed_loop_sample: a declaration there, even of nothing, reorders the
  // routine's stack slots and with them the instructions of the instantiations that do not score.
  double cost = 0.0, clear = HUGE_VAL;
  int clear_knot = -1, hits = 0;
};

// The body acceleration under a wrench w = {F, tau}, held over the step.  body_acceleration[_fast] with two added operations, in this
// order (R = R(q) of the state the acceleration is evaluated at, quat_to_R; every line one rounding sequence, nothing fused across lines):
//     f[k]       = R[0][k] F_x + R[1][k] F_y + R[2][k] F_z          (mat3_tvec: R^T F, the velocities are body-frame)
//     acc_lin[k] = a[k] + f[k] / mass                               (a[k]: the undisturbed value, formed first)
//     rhs[k]     = (M[k] - (w x I w)[k]) + tau[k]                   (then inertia_inv rhs, as before)
// FAST: the gravity terms as body_acceleration_fast forms them (the Euler step), else from R (the Runge-Kutta stages).  A zero wrench
// leaves every value what it was (x + 0 = x).
template <bool FAST>
QILQR_HD void cl_disturbed_acceleration(const ModelConsts<double> &c, const double q[4], const double v[6], const double u[4], const double w[6],
                                        double acc[6]) {
  double R[9], f[3];
  quat_to_R(q, R);
  mat3_tvec(R, w, f);
  double r6 = R[6], r7 = R[7], r8 = R[8];
  if (FAST) {
    const double x = q[0], y = q[1], z = q[2], qw = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    r6 = tz * x - ty * qw;
    r7 = tz * y + tx * qw;
    r8 = 1.0 - (tx * x + ty * y);
  }
  const double usum = ((u[0] + u[1]) + u[2]) + u[3];
  const double a0 = -c.g * r6, a1 = -c.g * r7, a2 = -c.g * r8 + usum / c.mass;
  const double f0 = f[0] / c.mass, f1 = f[1] / c.mass, f2 = f[2] / c.mass;
  acc[0] = a0 + f0;
  acc[1] = a1 + f1;
  acc[2] = a2 + f2;
  double M[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) M[i] = c.arms[4 * i] * u[0] + c.arms[4 * i + 1] * u[1] + c.arms[4 * i + 2] * u[2] + c.arms[4 * i + 3] * u[3];
  const double *om = v + 3;
  double Iw[3], wIw[3], rhs[3];
  mat3_vec(c.inertia, om, Iw);
  cross3(om, Iw, wIw);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double r = M[i] - wIw[i];
    rhs[i] = r + w[3 + i];
  }
  mat3_vec(c.inertia_inv, rhs, acc + 3);
}
// rk4_step's state update (se3_math.h, without the Jacobians) with the wrench held over the four stages; R is each stage's own attitude
QILQR_HD void cl_rk4_step_wrench(const ModelConsts<double> &c, double t[3], double q[4], double v[6], const double u[4], const double w[6]) {
  const double coeffs[4] = {1.0 / 6.0, 2.0 / 6.0, 2.0 / 6.0, 1.0 / 6.0};
  const double hs[4] = {0.0, c.dt / 2.0, c.dt / 2.0, c.dt};
  double k[12], xdot[12];
  for (int e = 0; e < 12; ++e) { k[e] = 0.0; xdot[e] = 0.0; }
  for (int i = 0; i < 4; ++i) {
    double tau[6], ti[3], qi[4], vi[6], acc[6];
    for (int a = 0; a < 6; ++a) tau[a] = hs[i] * k[a];
    se3_rplus(t, q, tau, ti, qi);
    for (int a = 0; a < 6; ++a) vi[a] = v[a] + hs[i] * k[6 + a];
    cl_disturbed_acceleration<false>(c, qi, vi, u, w, acc);
    for (int a = 0; a < 6; ++a) { k[a] = vi[a]; k[6 + a] = acc[a]; }
    for (int e = 0; e < 12; ++e) xdot[e] += coeffs[i] * k[e];
  }
  double tau[6], tn[3], qn[4];
  for (int a = 0; a < 6; ++a) tau[a] = c.dt * xdot[a];
  se3_rplus(t, q, tau, tn, qn);
  for (int i = 0; i < 3; ++i) t[i] = tn[i];
  for (int i = 0; i < 4; ++i) q[i] = qn[i];
  for (int a = 0; a < 6; ++a) v[a] = v[a] + c.dt * xdot[6 + a];
}

// One sphere {cx, cy, cz, radius, weight} at the flown knot pt: add_sphere's (obstacles.h) distance, h and cost term, word for word, without
// the differentials -- and the clearance -h = |p - c| - radius of EVERY sphere, active or not, into the knot's minimum.  A weight of 0
// adds (0 h) h = +0 to the cost: its bits stay.  A NaN clearance is taken (the comparison fails), as the maxima of the statistics take one.
QILQR_HD void cl_score_sphere(const double sp[OB_WORDS], const double *pt, double &cost, double &clear) {
  const double e[3] = {pt[1] - sp[OB_CX], pt[2] - sp[OB_CX + 1], pt[3] - sp[OB_CX + 2]};
  const double d = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  const double h = sp[OB_RADIUS] - d;
  const double cl = -h;
  if (!(cl >= clear)) clear = cl;
  if (!(h > 0.0)) return;
  const double w = sp[OB_WEIGHT];
  cost += (w * h) * h;
}
// the sphere terms of one knot at time ts: the shared table, then the problem's own spheres at fma(ts, v, c) (add_moving_sphere's centre)
QILQR_HD void cl_score_spheres(const ClSpheres &s, double ts, const double *pt, double &cost, double &clear) {
  for (int j = 0; j < s.n_shared; ++j) {
    const double *sp = s.shared + j * OB_WORDS;
    const double s5[OB_WORDS] = {sp[0], sp[1], sp[2], sp[3], sp[4]};
    cl_score_sphere(s5, pt, cost, clear);
  }
  for (int j = 0; j < s.n_own; ++j) {
    const double *sp = s.own + (long)j * s.ss;
    const int ws = s.ws;
    const double s5[OB_WORDS] = {fma(ts, sp[OB_BV * ws], sp[0]), fma(ts, sp[(OB_BV + 1) * ws], sp[ws]), fma(ts, sp[(OB_BV + 2) * ws], sp[2 * ws]),
                                 sp[OB_BRADIUS * ws], sp[OB_BWEIGHT * ws]};
    cl_score_sphere(s5, pt, cost, clear);
  }
}

// the operands of a scored knot by per-lane (or host) loads: ClFlatFetch, and where the desired knot and the state weights of knot i lie
struct ClFlatScoreFetch {
  ClFlatFetch base;
  const double *desired;  // the first desired knot of the window: the plan's own, or the handle's at its horizon start
  const double *q;        // knot i's state weights are q + i * q_step (q_step = 0: the handle's Q at every knot)
  long q_step;
  QILQR_HD void operator()(int i, double pt[18], double K[48]) const { base(i, pt, K); }
  QILQR_HD ClKnotScore score(int i) const { return ClKnotScore{desired + (long)i * 18, q + (long)i * q_step}; }
};

// One sample: x0 points at its 13 words, out at its first knot (or null: no trajectory store is issued), stats at its 4 words (or null).
// c: the sample's model.  LIM: the control is clamped to [lo, hi] rotor by rotor, and the clamped control is what is stored and stepped
// with, as in rollout_problem<.., LIM>.  fetch(i, pt, K) is called once per knot, i0 .. i1 in order, by every caller of one block alike.
// WRENCH, SCORE: the scored flight (above); ex is read only with one of them, fetch.score(i) only with SCORE.
template <int INTEG, bool LIM, typename Fetch, bool WRENCH = false, bool SCORE = false>
QILQR_HD void closed_loop_sample(const ModelConsts<double> &c, Fetch &fetch, const double *x0, int i0, int i1, double *out, double *stats,
                                 const double *lo = nullptr, const double *hi = nullptr, ClSampleExtras *ex = nullptr) {
  double t[3] = {x0[0], x0[1], x0[2]};
  double q[4] = {x0[4], x0[5], x0[6], x0[3]};
  double v[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[a] = x0[7 + a];
  RolloutSeries<double> sr;  // series coefficients in registers for the whole loop, as rollout_problem holds them
  sr.load();
  // (the maxima are kept squared: the square root is monotone and correctly rounded, so the root of the maximum is the maximum of the roots)
  double pos2 = 0.0, ang2 = 0.0, last2 = 0.0;
  int clamped = 0;
  for (int i = i0; i <= i1; ++i) {
    double pt[18], K[48];
    fetch(i, pt, K);
    // dx = state (-) x_i
    double dx[12];
    const double qi[4] = {pt[5], pt[6], pt[7], pt[4]};
    se3_rminus_fast(t, q, pt + 1, qi, dx, sr);
#pragma unroll
    for (int a = 0; a < 6; ++a) dx[6 + a] = v[a] - pt[8 + a];
    double u[4];
    closed_loop_law(pt, K, dx, u);
    if (LIM) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double ua = u[a];
        clamped += (ua < lo[a] || ua > hi[a]) ? 1 : 0;
        u[a] = ua < lo[a] ? lo[a] : (ua > hi[a] ? hi[a] : ua);
      }
    }
    if (stats) {
      const double p2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2], a2 = (dx[3] * dx[3] + dx[4] * dx[4]) + dx[5] * dx[5];
      if (!(p2 <= pos2)) pos2 = p2;  // (a NaN is taken, and stays: the state it came from stays NaN)
      if (!(a2 <= ang2)) ang2 = a2;
      if (i == i1) {
        double s2 = p2 + a2;
#pragma unroll
        for (int a = 6; a < 12; ++a) s2 += dx[a] * dx[a];
        last2 = s2;
      }
    }
    if (out) {
      const double o[18] = {pt[0], t[0], t[1], t[2], q[3], q[0], q[1], q[2], v[0], v[1], v[2], v[3], v[4], v[5], u[0], u[1], u[2], u[3]};
#pragma unroll
      for (int e = 0; e < 9; ++e) cl_store_pair(out + (long)i * 18 + 2 * e, o[2 * e], o[2 * e + 1]);
    }
    if constexpr (SCORE) {
      const ClKnotScore ks = fetch.score(i);
      const double o[18] = {pt[0], t[0], t[1], t[2], q[3], q[0], q[1], q[2], v[0], v[1], v[2], v[3], v[4], v[5], u[0], u[1], u[2], u[3]};
      double edx[12], edu[4], sq[12], su[4];
      double kc = knot_cost<false, double, false>(ks.Q, c.R, o, ks.pd, edx, edu, sq, su);
      double kmin = HUGE_VAL;
      cl_score_spheres(ex->spheres, (double)i * c.dt, o, kc, kmin);
      ex->cost += kc;
      if (!(kmin >= ex->clear)) {  // (the first knot on ties; a NaN is taken)
        ex->clear = kmin;
        ex->clear_knot = i;
      }
      ex->hits += kmin < 0.0 ? 1 : 0;
    }
    if constexpr (WRENCH) {
      if (i < i1) {
        double w[CL_WRENCH];
        const double *wp = ex->wrench + (long)i * ex->wrench_step;
#pragma unroll
        for (int e = 0; e < CL_WRENCH / 2; ++e) cl_load_pair(wp + 2 * e, w[2 * e], w[2 * e + 1]);
        if (INTEG == 1) {
          cl_rk4_step_wrench(c, t, q, v, u, w);
        } else {
          double acc[6], tau[6];
          cl_disturbed_acceleration<true>(c, q, v, u, w, acc);
#pragma unroll
          for (int a = 0; a < 6; ++a) tau[a] = c.dt * v[a];  // pose integrates with the OLD velocity
          se3_rplus_fast(t, q, tau, sr);
#pragma unroll
          for (int a = 0; a < 6; ++a) v[a] = v[a] + c.dt * acc[a];
        }
      }
    } else if (i < i1) {
      if (INTEG == 1) {
        rk4_step(c, t, q, v, u, (double *)nullptr);
      } else {
        double acc[6], tau[6];
        body_acceleration_fast(c, q, v, u, acc);
#pragma unroll
        for (int a = 0; a < 6; ++a) tau[a] = c.dt * v[a];  // pose integrates with the OLD velocity
        se3_rplus_fast(t, q, tau, sr);
#pragma unroll
        for (int a = 0; a < 6; ++a) v[a] = v[a] + c.dt * acc[a];
      }
    }
  }
  if (stats) {
    cl_store_pair(stats, sqrt(pos2), sqrt(ang2));
    cl_store_pair(stats + 2, sqrt(last2), (double)clamped);
  }
  if constexpr (SCORE) {
    if (ex->score) {
      cl_store_pair(ex->score, ex->cost, ex->clear);
      cl_store_pair(ex->score + 2, (double)ex->clear_knot, (double)ex->hits);
    }
  }
}

#if defined(__HIPCC__)
typedef double cl_dv2 __attribute__((ext_vector_type(2)));

// The operands of knot i out of the block's LDS image (shared-operand form).  Every lane of the block calls prime() once and then the
// operator for i0 .. i1 in order.  Knot i is read from buf[i & 1]; the same call writes knot i + 1 (in `next` since the call before) to
// buf[(i + 1) & 1] and issues the loads of knot i + 2.  The barrier at the top of a call stands between the reads of a buffer and the
// next write to it, and between a write and its reads.
struct ClSharedFetch {
  const cl_dv2 *plan, *gains;  // the problem's first knot: pair e of knot i is plan[i * 9 + e], gains[i * 26 + e] (pairs 2..25: K)
  cl_dv2 (*buf)[CL_PAIRS];     // LDS, [2][CL_PAIRS]
  int lane, i1;
  cl_dv2 next;
  __device__ cl_dv2 load(int i) const {
    return lane < CL_PLAN_PAIRS ? plan[(long)i * 9 + lane] : gains[(long)i * 26 + 2 + (lane - CL_PLAN_PAIRS)];
  }
  __device__ void prime(int i0) {
    if (lane < CL_PAIRS) {
      buf[i0 & 1][lane] = load(i0);
      if (i0 + 1 <= i1) next = load(i0 + 1);
    }
  }
  __device__ void operator()(int i, double pt[18], double K[48]) {
    __syncthreads();
    if (lane < CL_PAIRS) {
      if (i + 1 <= i1) buf[(i + 1) & 1][lane] = next;
      if (i + 2 <= i1) next = load(i + 2);
    }
    const cl_dv2 *img = buf[i & 1];
#pragma unroll
    for (int e = 0; e < CL_PLAN_PAIRS; ++e) {
      const cl_dv2 w = img[e];
      pt[2 * e] = w[0];
      pt[2 * e + 1] = w[1];
    }
#pragma unroll
    for (int e = 0; e < CL_GAIN_PAIRS; ++e) {
      const cl_dv2 w = img[CL_PLAN_PAIRS + e];
      K[2 * e] = w[0];
      K[2 * e + 1] = w[1];
    }
  }
};

// Lim = ControlLimits: controls clamped to the box.  Lim = BatchModels: sample (b, j) steps with model b S + j.  Either, both
// (ControlLimits first), or neither, as k_rollout and k_shift take them.
// Grid: SHARED: B cdiv(S, 64) blocks, block g of problem g / cdiv(S, 64); flattened: cdiv(B S, 64) blocks over the samples in order.
template <int INTEG, bool SHARED, typename... Lim>
__global__ __launch_bounds__(CL_BLOCK) void k_closed_loop(ModelConsts<double> c, ClosedLoopArgs a, Lim... lim) {
  constexpr bool LIM = pack_has<ControlLimits, Lim...>;
  constexpr bool MOD = pack_has<BatchModels, Lim...>;
  const int lane = threadIdx.x;
  int b, j;
  bool live;
  if constexpr (SHARED) {
    const int per = (a.S + CL_BLOCK - 1) / CL_BLOCK;
    b = (int)blockIdx.x / per;  // (block-uniform; the host launches exactly B * per blocks)
    j = ((int)blockIdx.x - b * per) * CL_BLOCK + lane;
    live = j < a.S;
    if (!live) j = a.S - 1;  // (takes part in the loads and the barriers; stores nothing)
  } else {
    const long g = (long)blockIdx.x * CL_BLOCK + lane;
    if (g >= (long)a.B * a.S) return;
    b = (int)(g / a.S);
    j = (int)(g - (long)b * a.S);
    live = true;
  }
  const long row = (long)b * a.S + j;
  const double *x0 = a.x0 + row * CL_STATE;
  double *out = (live && a.out_traj) ? a.out_traj + row * a.n * 18 : nullptr;
  double *stats = (live && a.out_stats) ? a.out_stats + row * CL_STATS : nullptr;
  const double *lo = nullptr, *hi = nullptr;
  if constexpr (LIM) {
    const ControlLimits &L = pack_get<ControlLimits>(lim...);
    lo = L.lo;
    hi = L.hi;
  }
  const double *plan = a.plan + (long)b * a.n * 18, *gains = a.gains + (long)b * a.n * 52;
  auto fly = [&](auto &fetch) {
    if constexpr (MOD) {
      const ModelConsts<double> cm = problem_model(c, pack_get<BatchModels>(lim...), row);
      closed_loop_sample<INTEG, LIM>(cm, fetch, x0, a.i0, a.i1, out, stats, lo, hi);
    } else {
      closed_loop_sample<INTEG, LIM>(c, fetch, x0, a.i0, a.i1, out, stats, lo, hi);
    }
  };
  if constexpr (SHARED) {
    __shared__ cl_dv2 image[2][CL_PAIRS];
    ClSharedFetch fetch{reinterpret_cast<const cl_dv2 *>(plan), reinterpret_cast<const cl_dv2 *>(gains), image, lane, a.i1, cl_dv2{0.0, 0.0}};
    fetch.prime(a.i0);
    fly(fetch);
  } else {
    ClFlatFetch fetch{plan, gains};
    fly(fetch);
  }
}
#endif

}  // namespace qilqr

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
