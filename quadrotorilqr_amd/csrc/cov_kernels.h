// cov_kernels.h -- linear covariance analysis of a plan's closed loop (qilqr_covariance_device): k_cov_build, k_cov_chain, k_cov_summary.
// About a dynamically consistent plan the deviation dx_i = x_i (-) plan_i of the law u = u_i + K_i dx obeys, to first order,
//     dx_{i+1} = F_i dx_i + G_i w_i,     F_i = A_i + B_i K_i   (A_i, B_i: the step's Jacobians at plan[b, i]; d_gains == NULL: F_i = A_i)
// with w_i the wrench of the scored flight, held over the step, and G_i (12 x 6) the step's Jacobian with respect to it.  With the gust
// model's S_g = diag(sigma_c^2) and rho_c (gust_coeffs' formula; QILQR_COV_WRENCH_HELD: rho = 1), from knot i0:
//     Sigma_{i0} = diag(state_sigma^2)     C_{i0} = 0 (12 x 6)     m_{i0} = 0
//     Sigma_{i+1} = (F Sigma + G C^T) F^T + H G^T,     H = F C + G S_g     (= F Sigma F^T + F C G^T + G C^T F^T + G S_g G^T)
//     C_{i+1}     = H diag(rho)
//     m_{i+1}     = F m_i + G mean
// and Sigma_{i+1} is made exactly symmetric before it is stored and carried on: entry (k, l), k <= l, is mirrored.
//
// THREE LAUNCHES, so that nothing that is independent per knot sits on the chain over the knots:
//   k_cov_build<INTEG, Lim...>  a lane per (plan, knot) and part.  Euler: part 0 forms F_i (the six Jacobian blocks of linearize_dynamics,
//       then A + B K), part 1 G_i (exact).  Runge-Kutta: nine parts of two columns of F or G each, by cov_rk4_directions -- the routine
//       beside rk4_step (whose text stays) that carries directions {dx, du, dw} through the four stages; a column of F is the direction
//       {e_c, K[:, c], 0}, so B K costs nothing, and the dense 12 x 16 of rk4_step, which does not stay in registers beside that product
//       (4.7 KB of scratch memory a lane), is never formed.  All write the knot's OPERAND IMAGE into a scratch array the handle owns: 5 x 64
//       doubles, word c 64 + lane the element lane (j = lane & 15, kk = lane >> 4) supplies to v_mfma_f64_16x16x4_f64 for contraction chunk
//       c: F[j][4 c + kk] (c < 3), G[j][4 (c - 3) + kk] (c = 3, 4); rows j >= 12 and wrench columns 6, 7 are zeros, written once when the
//       scratch is allocated.  A chunk is at once the A operand of F (or G) and the B operand of F^T (or G^T) (backward_layout.h).
//   k_cov_chain  one wavefront per plan, the 12 x 12 state padded to the 16 x 16 tile.  Per knot 15 MFMAs and two trips through LDS:
//           W1 = F Sigma + G C^T      (Sigma's accumulator registers ARE the B operand's chunks: register r holds rows 4 r + kk)
//           Hm = F [C | m] + G [S_g | mean]        (the mean rides in column 6 of the cross term's tile)
//           W1, Hm -> LDS -> A layout (the one transposition)       Sigma' = W1 F^T + H G^T
//           Sigma' -> LDS -> mirrored                                [C | m]' = Hm scaled by column, C'^T's chunks = H's A layout scaled by rho
//       The next knot's image (five coalesced eight-byte loads per lane) is requested before the knot's products.
//   k_cov_summary  a wavefront per plan, a lane per knot (i0 + lane, + 64, ...): the traces, the control deviations and the sphere loop of
//       cov_knot_measures over the stored Sigma_i and m_i, then a reduction over the lanes (the first knot on ties).
// The routines that form F, G and a knot's measures are QILQR_HD and compile under g++, and cov_chain_reference states the recursion in
// plain loops (tests/host_cov_harness.cpp).  Part of cov.hip's translation unit (gfx950 only).
#pragma once

#include "backward_layout.h"
#include "batch_models.h"
#include "call_parts.h"
#include "closed_loop_kernels.h"
#include "cov_launch.h"
#include "obstacles.h"
#include "se3_math.h"

namespace qilqr {

constexpr int COV_WORDS = 144;    // QILQR_COV
constexpr int COV_SUMMARY = 8;    // QILQR_COV_SUMMARY
constexpr int COV_BLOCK = 64;     // threads of a block of every kernel here: one wavefront

// where element (row, col) of F (g == false, col < 12) or G (g == true, col < 6) lies in a knot's operand image
QILQR_HD int cov_image_index(bool g, int row, int col) { return (g ? 192 : 0) + (col >> 2) * 64 + (col & 3) * 16 + row; }

// the six Jacobian blocks of linearize_dynamics, kept where they are put
struct CovBlockSink {
  double v[LIN_M_BLOCKS];
  QILQR_HD void put(int k, double x) { v[k] = x; }
};

// ---- explicit Euler.  F = A + B K of the step from plan knot pt (18 words): A from the six Jacobian blocks of linearize_dynamics, B the
// constant J_u; K: words 4..51 of the knot's gains (K[col * 4 + a]), or null: F = A.  Every element goes to put(row, col, value).
template <typename Put>
QILQR_HD void cov_euler_closed_loop_jacobian(const ModelConsts<double> &c, const double *pt, const double *K, Put &&put) {
  CovBlockSink w;
  linearize_dynamics(c, pt, w);
#pragma unroll
  for (int r = 0; r < 12; ++r)
#pragma unroll
    for (int col = 0; col < 12; ++col) {
      double cst;
      const int off = m_source(r, col, c.Bu, &cst);
      double f = off >= 0 ? w.v[off] : cst;
      if (K && r >= PM_BU_ROW0) {  // (rows 0..7 of J_u are zero for every model)
        double bk = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) bk += c.Bu[r * 4 + a] * K[col * 4 + a];
        f += bk;
      }
      put(r, col, f);
    }
}
// G of the Euler step, exact: rows 6..8 x columns 0..2 are dt R(q)^T / mass, rows 9..11 x columns 3..5 dt I^-1, zero elsewhere (the pose
// integrates with the old velocity)
template <typename Put>
QILQR_HD void cov_euler_wrench_jacobian(const ModelConsts<double> &c, const double *pt, Put &&put) {
  const double q[4] = {pt[5], pt[6], pt[7], pt[4]};
  double R[9];
  quat_to_R(q, R);
#pragma unroll
  for (int r = 0; r < 12; ++r)
#pragma unroll
    for (int col = 0; col < 6; ++col) {
      double g = 0.0;
      if (r >= 6 && r < 9 && col < 3) g = c.dt * (R[3 * col + (r - 6)] / c.mass);  // (R^T F)[k] = sum_m R[3 m + k] F_m
      if (r >= 9 && col >= 3) g = c.dt * c.inertia_inv[3 * (r - 9) + (col - 3)];
      put(r, col, g);
    }
}

// ---- Runge-Kutta.  The new routine beside rk4_step (whose text stays): the derivative of cl_rk4_step_wrench's next state, at a zero
// wrench, along NC directions {dx (12, tangent), du (4), dw (6: the wrench held over the four stages)} at once -- rk4_step's own chain rule
// (its comment in se3_math.h) with the direction applied from the start instead of the 16 columns carried:
//     x_i = x (+) h k:   d x_i = [Ad(Exp(-tau)) on the pose rows, 1 on the velocities] dx + h [Jr(tau), 1] dk
//     k = f(x_i, u, w):  d k = [d x_i's velocities;  G d x_i[rot] + (J_u / dt) du + R(q_i)^T dF / mass;  D d x_i[omega] + ... + I^-1 dtau]
// A column of F = A + B K is the direction {e_c, K[:, c], 0}; a column of G is {0, 0, e_w}.  A lane carries two (cov_rk4_part): the dense
// 12 x 16 of rk4_step does not stay in registers beside the product with K.
template <int NC>
QILQR_HD void cov_rk4_directions(const ModelConsts<double> &c, const double t[3], const double q[4], const double v[6], const double u[4],
                                 const double (*dx)[12], const double (*du)[4], const double (*dw)[6], double (*out)[12]) {
  const double coeffs[4] = {1.0 / 6.0, 2.0 / 6.0, 2.0 / 6.0, 1.0 / 6.0};
  const double hs[4] = {0.0, c.dt / 2.0, c.dt / 2.0, c.dt};
  double k[12], xdot[12], dk[NC][12], sk[NC][12], direct[NC][6];
#pragma unroll
  for (int e = 0; e < 12; ++e) { k[e] = 0.0; xdot[e] = 0.0; }
#pragma unroll
  for (int d = 0; d < NC; ++d) {
#pragma unroll
    for (int e = 0; e < 12; ++e) { dk[d][e] = 0.0; sk[d][e] = 0.0; }
    // what du and dtau add to every stage's acceleration (the same at every stage); dF's part turns with the stage's attitude
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double bl = 0.0, bw = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        bl += c.Bu[(6 + r) * 4 + a] * du[d][a];
        bw += c.Bu[(9 + r) * 4 + a] * du[d][a];
      }
      direct[d][r] = bl / c.dt;
      direct[d][3 + r] = bw / c.dt + ((c.inertia_inv[3 * r] * dw[d][3] + c.inertia_inv[3 * r + 1] * dw[d][4]) + c.inertia_inv[3 * r + 2] * dw[d][5]);
    }
  }
  // d (x (+) h kk) along direction d, with `kd` the direction's dk: into a (12)
  auto through_plus = [&](const double tau[6], double h, int d, const double *kd, double *a) {
    ExpBlocks<double> eb;
    exp_blocks(tau, eb);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double top = 0.0, bot = 0.0, jt = 0.0, jb = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        top += eb.Rc[3 * r + m] * dx[d][m] + eb.SR[3 * r + m] * dx[d][3 + m];
        bot += eb.Rc[3 * r + m] * dx[d][3 + m];
        jt += eb.Jr[3 * r + m] * kd[m] + eb.Qm[3 * r + m] * kd[3 + m];
        jb += eb.Jr[3 * r + m] * kd[3 + m];
      }
      a[r] = top + h * jt;
      a[3 + r] = bot + h * jb;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) a[6 + r] = dx[d][6 + r] + h * kd[6 + r];
  };
  for (int i = 0; i < 4; ++i) {
    double tau[6], ti[3], qi[4], vi[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) tau[a] = hs[i] * k[a];
    se3_rplus(t, q, tau, ti, qi);
#pragma unroll
    for (int a = 0; a < 6; ++a) vi[a] = v[a] + hs[i] * k[6 + a];
    double acc[6];
    body_acceleration(c, qi, vi, u, acc);
#pragma unroll
    for (int a = 0; a < 6; ++a) { k[a] = vi[a]; k[6 + a] = acc[a]; }
    double Gc[9], D[9], R[9];
    continuous_blocks(c, qi, vi, Gc, D);
    quat_to_R(qi, R);
#pragma unroll
    for (int d = 0; d < NC; ++d) {
      double a[12];
      through_plus(tau, hs[i], d, dk[d], a);
#pragma unroll
      for (int r = 0; r < 6; ++r) dk[d][r] = a[6 + r];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double gl = (Gc[3 * r] * a[3] + Gc[3 * r + 1] * a[4]) + Gc[3 * r + 2] * a[5];
        const double dwr = (D[3 * r] * a[9] + D[3 * r + 1] * a[10]) + D[3 * r + 2] * a[11];
        const double rf = (R[r] * dw[d][0] + R[3 + r] * dw[d][1]) + R[6 + r] * dw[d][2];  // (R^T dF)[r]
        dk[d][6 + r] = gl + (direct[d][r] + rf / c.mass);
        dk[d][9 + r] = dwr + direct[d][3 + r];
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) sk[d][e] += coeffs[i] * dk[d][e];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) xdot[e] += coeffs[i] * k[e];
  }
  double tau[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) tau[a] = c.dt * xdot[a];
#pragma unroll
  for (int d = 0; d < NC; ++d) through_plus(tau, c.dt, d, sk[d], out[d]);
}
// The Runge-Kutta build in nine parts of two columns: parts 0..5 are columns 2 p, 2 p + 1 of F (K null: of A), parts 6..8 columns
// 2 (p - 6), + 1 of G.  put(g, row, col, value): g says which matrix.
constexpr int COV_RK4_PARTS = 9;
template <typename Put>
QILQR_HD void cov_rk4_part(const ModelConsts<double> &c, const double *pt, const double *K, int part, Put &&put) {
  const double t[3] = {pt[1], pt[2], pt[3]}, q[4] = {pt[5], pt[6], pt[7], pt[4]};
  double v[6], dx[2][12], du[2][4], dw[2][6], out[2][12];
#pragma unroll
  for (int i = 0; i < 6; ++i) v[i] = pt[8 + i];
  const bool g = part >= 6;
  const int col0 = 2 * (g ? part - 6 : part);
#pragma unroll
  for (int d = 0; d < 2; ++d) {
#pragma unroll
    for (int e = 0; e < 12; ++e) dx[d][e] = (!g && e == col0 + d) ? 1.0 : 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) dw[d][e] = (g && e == col0 + d) ? 1.0 : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) du[d][a] = (!g && K) ? K[(col0 + d) * 4 + a] : 0.0;
  }
  cov_rk4_directions<2>(c, t, q, v, pt + 14, dx, du, dw, out);
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 12; ++r) put(g, r, col0 + d, out[d][r]);
}

// ---- what the summary takes of one knot: Sigma (12 x 12 row-major), m (12), the plan knot, K (or null: the open loop) and the spheres at
// the knot's time ts.  P = Sigma[0:3, 0:3]; the tangent's first three words are body-frame (the state addition composes on the right), so
// the mean position is p + R m[0:3] and a world direction n_w has the variance (R^T n_w)^T P (R^T n_w).
struct CovKnotMeasures {
  double pos2, rot2;  // tr Sigma[0:3, 0:3], tr Sigma[3:6, 3:6]
  double z;           // the smallest (|d| - radius) / sqrt(n^T P n) over the spheres: +inf without one; taken by z < best, so never a NaN
  int sphere;         // its index (shared_count + j for the plan's own table), -1: none taken
  double u2;          // max over the rotors of K_a Sigma K_a^T; 0 in the open loop
};
QILQR_HD void cov_one_sphere(const double ctr[3], double radius, int index, const double p[3], const double R[9], const double *S, CovKnotMeasures &o) {
  const double d[3] = {p[0] - ctr[0], p[1] - ctr[1], p[2] - ctr[2]};
  const double dist = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  double nb[3];
  mat3_tvec(R, d, nb);
  for (int k = 0; k < 3; ++k) nb[k] = nb[k] / dist;
  double var = 0.0;
  for (int k = 0; k < 3; ++k) var += nb[k] * ((S[k * 12] * nb[0] + S[k * 12 + 1] * nb[1]) + S[k * 12 + 2] * nb[2]);
  const double z = (dist - radius) / sqrt(var);
  if (z < o.z) {
    o.z = z;
    o.sphere = index;
  }
}
QILQR_HD CovKnotMeasures cov_knot_measures(const double *S, const double *m, const double *pt, const double *K, const ClSpheres &sp, double ts) {
  CovKnotMeasures o;
  o.pos2 = (S[0] + S[13]) + S[26];
  o.rot2 = (S[39] + S[52]) + S[65];
  o.z = HUGE_VAL;
  o.sphere = -1;
  o.u2 = 0.0;
  if (sp.n_shared > 0 || sp.n_own > 0) {
    const double q[4] = {pt[5], pt[6], pt[7], pt[4]};
    double R[9], rm[3];
    quat_to_R(q, R);
    mat3_vec(R, m, rm);
    const double p[3] = {pt[1] + rm[0], pt[2] + rm[1], pt[3] + rm[2]};
    for (int j = 0; j < sp.n_shared; ++j) {
      const double *s5 = sp.shared + j * OB_WORDS;
      const double ctr[3] = {s5[OB_CX], s5[OB_CX + 1], s5[OB_CX + 2]};
      cov_one_sphere(ctr, s5[OB_RADIUS], j, p, R, S, o);
    }
    for (int j = 0; j < sp.n_own; ++j) {
      const double *s8 = sp.own + (long)j * sp.ss;
      const int ws = sp.ws;
      const double ctr[3] = {fma(ts, s8[OB_BV * ws], s8[0]), fma(ts, s8[(OB_BV + 1) * ws], s8[ws]), fma(ts, s8[(OB_BV + 2) * ws], s8[2 * ws])};
      cov_one_sphere(ctr, s8[OB_BRADIUS * ws], sp.n_shared + j, p, R, S, o);
    }
  }
  if (K) {
    for (int a = 0; a < 4; ++a) {
      double quad = 0.0;
      for (int k = 0; k < 12; ++k) {
        double row = 0.0;
        for (int l = 0; l < 12; ++l) row += S[k * 12 + l] * K[l * 4 + a];
        quad += K[k * 4 + a] * row;
      }
      if (quad > o.u2) o.u2 = quad;
    }
  }
  return o;
}

// a plan's running summary: the knots come in ascending order, so a strict comparison keeps the first on ties (and never takes a NaN)
struct CovPlanSummary {
  double pos2 = -1.0, rot2 = -1.0, last2 = 0.0, z = HUGE_VAL, u2 = 0.0;
  int pos_knot = -1, z_knot = -1, sphere = -1;
  QILQR_HD void take(const CovKnotMeasures &k, int i, int i1) {
    if (k.pos2 > pos2) { pos2 = k.pos2; pos_knot = i; }
    if (k.rot2 > rot2) rot2 = k.rot2;
    if (i == i1) last2 = k.pos2;
    if (k.z < z) { z = k.z; z_knot = i; sphere = k.sphere; }
    if (k.u2 > u2) u2 = k.u2;
  }
  // another lane's (or the other half's): the smaller knot on ties
  QILQR_HD void merge(const CovPlanSummary &o) {
    if (o.pos2 > pos2 || (o.pos2 == pos2 && o.pos_knot >= 0 && (pos_knot < 0 || o.pos_knot < pos_knot))) { pos2 = o.pos2; pos_knot = o.pos_knot; }
    if (o.rot2 > rot2) rot2 = o.rot2;
    if (o.z < z || (o.z == z && o.z_knot >= 0 && (z_knot < 0 || o.z_knot < z_knot))) { z = o.z; z_knot = o.z_knot; sphere = o.sphere; }
    if (o.u2 > u2) u2 = o.u2;
  }
  QILQR_HD void words(double out[COV_SUMMARY]) const {
    out[0] = sqrt(pos2 > 0.0 ? pos2 : 0.0);
    out[1] = (double)pos_knot;
    out[2] = sqrt(last2 > 0.0 ? last2 : 0.0);
    out[3] = sqrt(rot2 > 0.0 ? rot2 : 0.0);
    out[4] = z;
    out[5] = (double)z_knot;
    out[6] = (double)sphere;
    out[7] = sqrt(u2);
  }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// The recursion in plain loops over dense F (n x 144) and G (n x 72) of one plan: what k_cov_chain computes on the matrix core, for the
// host program.  cov (n x 144), mean (n x 12) and cross (n x 72: C_i, the host program's own output) may each be null; knots outside
// i0 .. i1 are left untouched.
inline void cov_chain_reference(const double *F, const double *G, const CovCoeffs &k, int i0, int i1, double *cov, double *mean, double *cross) {
  double S[144] = {0.0}, Cx[72] = {0.0}, m[12] = {0.0};
  for (int e = 0; e < 12; ++e) S[e * 12 + e] = k.s02[e];
  for (int i = i0;; ++i) {
    if (cov) for (int e = 0; e < 144; ++e) cov[(long)i * 144 + e] = S[e];
    if (mean) for (int e = 0; e < 12; ++e) mean[(long)i * 12 + e] = m[e];
    if (cross) for (int e = 0; e < 72; ++e) cross[(long)i * 72 + e] = Cx[e];
    if (i == i1) break;
    const double *Fi = F + (long)i * 144, *Gi = G + (long)i * 72;
    double W1[144], H[72], Sn[144], mn[12];
    for (int r = 0; r < 12; ++r)
      for (int col = 0; col < 12; ++col) {
        double s = 0.0;
        for (int e = 0; e < 12; ++e) s += Fi[r * 12 + e] * S[e * 12 + col];
        for (int w = 0; w < 6; ++w) s += Gi[r * 6 + w] * Cx[col * 6 + w];
        W1[r * 12 + col] = s;
      }
    for (int r = 0; r < 12; ++r) {
      for (int w = 0; w < 6; ++w) {
        double s = 0.0;
        for (int e = 0; e < 12; ++e) s += Fi[r * 12 + e] * Cx[e * 6 + w];
        H[r * 6 + w] = s + Gi[r * 6 + w] * k.sg2[w];
      }
      double s = 0.0;
      for (int e = 0; e < 12; ++e) s += Fi[r * 12 + e] * m[e];
      for (int w = 0; w < 6; ++w) s += Gi[r * 6 + w] * k.mean[w];
      mn[r] = s;
    }
    for (int r = 0; r < 12; ++r)
      for (int col = 0; col < 12; ++col) {
        double s = 0.0;
        for (int e = 0; e < 12; ++e) s += W1[r * 12 + e] * Fi[col * 12 + e];
        for (int w = 0; w < 6; ++w) s += H[r * 6 + w] * Gi[col * 6 + w];
        Sn[r * 12 + col] = s;
      }
    for (int r = 0; r < 12; ++r)
      for (int col = 0; col < 12; ++col) S[r * 12 + col] = r <= col ? Sn[r * 12 + col] : Sn[col * 12 + r];
    for (int r = 0; r < 12; ++r)
      for (int w = 0; w < 6; ++w) Cx[r * 6 + w] = H[r * 6 + w] * k.rho[w];
    for (int e = 0; e < 12; ++e) m[e] = mn[e];
  }
}
#endif

// ---- the kernels' arguments; every pointer a device one
struct CovBuildArgs {
  const double *plan;   // [B][n][18]
  const double *gains;  // [B][n][52], or null: the open loop
  double *image;        // [B][n][COV_IMAGE]: the handle's scratch, its pads zero
  int B, n, i0, i1;
};
struct CovChainArgs {
  const double *image;  // [B][n][COV_IMAGE]
  double *cov;          // [B][n][144], or null
  double *mean;         // [B][n][12], or null
  int n, i0, i1;
  CovCoeffs k;
};
struct CovSummaryArgs {
  const double *plan, *gains;  // gains may be null
  const double *cov, *mean;    // [B][n][144], [B][n][12]: the caller's outputs or the handle's scratch
  double *summary;             // [B][COV_SUMMARY]
  int n, i0, i1;
  double dt;
  SphereTables spheres;        // the handle's (call_parts.h)
};

#if defined(__HIPCC__)
typedef double cov_d4 __attribute__((ext_vector_type(4)));

// Lim = BatchModels: plan b takes model b.  Grid: (cdiv(B n, 64), parts); blockIdx.y is the part: Euler 0 forms F and 1 G, Runge-Kutta
// cov_rk4_part's nine.  Knots outside i0 .. i1 - 1 have no step in the window and write nothing.
template <int INTEG, typename... Lim>
__global__ __launch_bounds__(COV_BLOCK) void k_cov_build(ModelConsts<double> c, CovBuildArgs a, Lim... lim) {
  constexpr bool MOD = pack_has<BatchModels, Lim...>;
  const long id = (long)blockIdx.x * COV_BLOCK + threadIdx.x;
  if (id >= (long)a.B * a.n) return;
  const int b = (int)(id / a.n), i = (int)(id - (long)b * a.n);
  if (i < a.i0 || i >= a.i1) return;
  double pt[18];
  const double *p = a.plan + id * 18;
#pragma unroll
  for (int e = 0; e < CL_PLAN_PAIRS; ++e) cl_load_pair(p + 2 * e, pt[2 * e], pt[2 * e + 1]);
  double *img = a.image + id * COV_IMAGE;
  const double *K = a.gains ? a.gains + id * 52 + 4 : nullptr;
  const int part = (int)blockIdx.y;
  auto form = [&](const ModelConsts<double> &cm) {
    if constexpr (INTEG == 1) {
      cov_rk4_part(cm, pt, K, part, [&](bool g, int r, int col, double v) { img[cov_image_index(g, r, col)] = v; });
    } else {
      if (part == 0) cov_euler_closed_loop_jacobian(cm, pt, K, [&](int r, int col, double v) { img[cov_image_index(false, r, col)] = v; });
      else cov_euler_wrench_jacobian(cm, pt, [&](int r, int col, double v) { img[cov_image_index(true, r, col)] = v; });
    }
  };
  if constexpr (MOD) form(problem_model(c, pack_get<BatchModels>(lim...), (long)b));
  else form(c);
}

// Grid: B blocks of one wavefront.  Lane (j = lane & 15, kk = lane >> 4).
__global__ __launch_bounds__(COV_BLOCK) void k_cov_chain(CovChainArgs a) {
  __shared__ double tile[2][16][17];
  const int lane = threadIdx.x, j = lane & 15, kk = lane >> 4;
  const long knot0 = (long)blockIdx.x * a.n;
  const double *img = a.image + knot0 * COV_IMAGE + lane;
  double *cov = a.cov ? a.cov + knot0 * COV_WORDS : nullptr;
  double *mean = a.mean ? a.mean + knot0 * 12 : nullptr;
  // the lane's constants: the column scale of [C | m], the rows of [S_g | mean] it supplies as a B operand, rho of its contraction index
  double col_scale = j == 6 ? 1.0 : 0.0, sgm[2] = {0.0, 0.0}, rho_k[2] = {0.0, 0.0};
  cov_d4 S = {0.0, 0.0, 0.0, 0.0}, Cm = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int w = 0; w < 6; ++w) {
    if (j == w) col_scale = a.k.rho[w];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
      if (4 * ch + kk == w) {
        rho_k[ch] = a.k.rho[w];
        if (j == w) sgm[ch] = a.k.sg2[w];
        if (j == 6) sgm[ch] = a.k.mean[w];
      }
  }
#pragma unroll
  for (int e = 0; e < 12; ++e)
    if (j == e && (e & 3) == kk) S[e >> 2] = a.k.s02[e];
  double ctb[2] = {0.0, 0.0};
  const bool in12 = j < 12;
  auto store = [&](int i, const cov_d4 &m4) {
    if (cov && in12) {
#pragma unroll
      for (int r = 0; r < 3; ++r) cov[(long)i * COV_WORDS + (4 * r + kk) * 12 + j] = S[r];
    }
    if (mean && j == 6) {
#pragma unroll
      for (int r = 0; r < 3; ++r) mean[(long)i * 12 + 4 * r + kk] = m4[r];
    }
  };
  store(a.i0, Cm);
  double f[3], g[2];
  if (a.i0 < a.i1) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) f[ch] = img[(long)a.i0 * COV_IMAGE + ch * 64];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) g[ch] = img[(long)a.i0 * COV_IMAGE + 192 + ch * 64];
  }
  for (int i = a.i0; i < a.i1; ++i) {
    double fn[3] = {0.0, 0.0, 0.0}, gn[2] = {0.0, 0.0};
    if (i + 1 < a.i1) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) fn[ch] = img[(long)(i + 1) * COV_IMAGE + ch * 64];
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) gn[ch] = img[(long)(i + 1) * COV_IMAGE + 192 + ch * 64];
    }
    cov_d4 W1 = {0.0, 0.0, 0.0, 0.0}, Hm = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      W1 = __builtin_amdgcn_mfma_f64_16x16x4f64(f[ch], S[ch], W1, 0, 0, 0);
      Hm = __builtin_amdgcn_mfma_f64_16x16x4f64(f[ch], Cm[ch], Hm, 0, 0, 0);
    }
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      W1 = __builtin_amdgcn_mfma_f64_16x16x4f64(g[ch], ctb[ch], W1, 0, 0, 0);
      Hm = __builtin_amdgcn_mfma_f64_16x16x4f64(g[ch], sgm[ch], Hm, 0, 0, 0);
    }
    // the one transposition: both tiles to LDS in their accumulator layout, back in the A layout
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      tile[0][4 * r + kk][j] = W1[r];
      tile[1][4 * r + kk][j] = Hm[r];
    }
    __syncthreads();
    double w1a[3], ha[2];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) w1a[ch] = tile[0][j][4 * ch + kk];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) ha[ch] = (4 * ch + kk < 6) ? tile[1][j][4 * ch + kk] : 0.0;  // (columns 6, 7 of the tile are m and nothing)
    __syncthreads();
    cov_d4 Sn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) Sn = __builtin_amdgcn_mfma_f64_16x16x4f64(w1a[ch], f[ch], Sn, 0, 0, 0);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) Sn = __builtin_amdgcn_mfma_f64_16x16x4f64(ha[ch], g[ch], Sn, 0, 0, 0);
    // exactly symmetric: entry (k, l), k <= l, is mirrored
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[0][4 * r + kk][j] = Sn[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * r + kk;
      S[r] = row <= j ? tile[0][row][j] : tile[0][j][row];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) Cm[r] = Hm[r] * col_scale;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) ctb[ch] = ha[ch] * rho_k[ch];
    store(i + 1, Hm);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) f[ch] = fn[ch];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) g[ch] = gn[ch];
  }
}

// Grid: B blocks of one wavefront; lane t takes knots i0 + t, i0 + t + 64, ...
__global__ __launch_bounds__(COV_BLOCK) void k_cov_summary(CovSummaryArgs a) {
  const int lane = threadIdx.x;
  const long b = blockIdx.x, knot0 = b * a.n;
  const SphereTables &t = a.spheres;
  ClSpheres sp{t.shared, t.n_shared, t.own ? t.own + bob_index(b, t.own_K, 0, 0) : nullptr, t.own ? t.own_counts[b] : 0, OB_TILE, OB_BWORDS * OB_TILE};
  CovPlanSummary s;
  for (int i = a.i0 + lane; i <= a.i1; i += COV_BLOCK) {
    const double *K = a.gains ? a.gains + (knot0 + i) * 52 + 4 : nullptr;
    s.take(cov_knot_measures(a.cov + (knot0 + i) * COV_WORDS, a.mean + (knot0 + i) * 12, a.plan + (knot0 + i) * 18, K, sp, (double)i * a.dt), i, a.i1);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    CovPlanSummary o;
    o.pos2 = __shfl_xor(s.pos2, off);
    o.rot2 = __shfl_xor(s.rot2, off);
    o.last2 = 0.0;
    o.z = __shfl_xor(s.z, off);
    o.u2 = __shfl_xor(s.u2, off);
    o.pos_knot = __shfl_xor(s.pos_knot, off);
    o.z_knot = __shfl_xor(s.z_knot, off);
    o.sphere = __shfl_xor(s.sphere, off);
    const double last = __shfl_xor(s.last2, off);
    s.merge(o);
    s.last2 = s.last2 + last;  // (one lane holds knot i1; every other one 0)
  }
  if (lane == 0) {
    double w[COV_SUMMARY];
    s.words(w);
#pragma unroll
    for (int e = 0; e < COV_SUMMARY / 2; ++e) cl_store_pair(a.summary + b * COV_SUMMARY + 2 * e, w[2 * e], w[2 * e + 1]);
  }
}
#endif

}  // namespace qilqr
