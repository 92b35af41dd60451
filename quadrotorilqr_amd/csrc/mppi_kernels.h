// mppi_kernels.h -- a sampling planner on the device: the Monte-Carlo loop's generator, flight and score turned on
// the plan's CONTROLS, and the samples fed back into the plan (MPPI / path-integral control):
//   k_mppi_flight   score[B][S][4]: sample (b, j) flies plan b open loop under u_i = clamp(plan_u_i + eps_i) from x0[b] and is scored as
//                   the scored closed-loop flight scores a knot (closed_loop_kernels.h: the same knot_cost instantiation, cl_score_spheres)
//   k_mppi_update   out_plan[B][n][18], info[B][8]: the plan's controls moved to the exp(-J / lambda)-weighted mean perturbation
// and k_mppi_flight once more, with one sample, eps = 0 and its trajectory store on, fills the new plan's states and scores it.
// No perturbation ever lies in memory: eps is a function of (seed, b0 + b, j, i) alone (philox.h, stream MC_STREAM_CONTROLS), drawn in
// registers by the flight and REDRAWN by the update.
// mppi_flight_block, the block of a flight kernel, is written here once for k_mppi_flight and for k_mppi_flight_spread of
// mppi_adapt_kernels.h; mppi_flight_args and mppi_update_args fill the kernels' arguments for both units.  (k_mppi_adapt still repeats
// k_mppi_update's head: with one shared routine for it the update measured 0.1 to 0.2 % slower at 64 x 1024 x 100 -- DESIGN.md section 8p.)
//
// The per-lane routines are QILQR_HD and carry all the arithmetic; tests/host_mppi_harness.cpp runs the same text on the host.
//
// THE PERTURBATION of sample j at knot i, rotor a: gust_row's recursion (monte_carlo_kernels.h) per rotor --
//     g_0 = sigma_a xi_0,   g_i = fma(rho, g_{i-1}, kappa_a xi_i),   eps_i[a] = g_i
// with rho = tau_s > 0 ? exp(-dt / tau_s) : 0 and kappa_a = sigma_a sqrt((1 - rho)(1 + rho)) made once on the host (mppi_coeffs), and xi
// normal a % 2 of mc_draw(seed, b0 + b, j, i, MC_STREAM_CONTROLS, a / 2).  With MPPI_FIRST_IS_NOMINAL sample 0 has eps = 0 at every knot.
//
// THE UPDATE of plan b, in this order (one block of T = mppi_update_lanes(S) lanes, mppi_launch.h -- a function of S alone; "lane" t is thread t of the block):
//     J_j   = cost_j, or cost_j + collision_cost hits_j where hits_j > 0              (mppi_key; a key that is not finite: weight 0)
//     J_min = the smallest finite key, the smaller j on ties; n_f the finite keys     (exact: comparisons and integer sums)
//     w_j   = exp(-(J_j - J_min) / lambda)                                             (mppi_weight)
//     eta   = sum_j w_j,  q = sum_j w_j w_j,  d_i[a] = sum_j (w_j eps_j,i[a])          (product rounded, then added: no fma)
//     u_i[a] = clamp(plan_u_i[a] + d_i[a] / eta)                                       (without a finite key: plan_u_i[a], its bits)
// EVERY SUM over the samples has one order, written here once:
//     lane t folds its samples t, t + T, t + 2 T, ... in that (ascending) order, from 0.0             (mppi_lane_*)
//     the 64 lanes of a wavefront combine by the butterfly 32, 16, 8, 4, 2, 1 (IEEE additions, commutative: every lane ends with the
//         same bits), as k_reduce_scores combines its lanes
//     the wavefronts' sums combine in index order, ((s_0 + s_1) + s_2) + ...                          (mppi_waves_in_order)
// A plan's bits depend on its own rows only -- not on B, not on its neighbours; no atomics.
// info[b] = {J_min, its sample, eta^2 / q (the effective sample size), n_f, and the four score words of the new plan's own flight};
// without a finite key {NaN, -1, 0, 0, ...}.
#pragma once

#include <math.h>
#include <stdint.h>

#include "closed_loop_kernels.h"
#include "mppi_launch.h"
#include "philox.h"

namespace qilqr {

constexpr int MPPI_INFO = 8;                     // QILQR_MPPI_INFO
constexpr int MPPI_MAX_SAMPLES = 4096;           // QILQR_RISK_MAX_SAMPLES: the update's block carries a plan's weights in LDS
constexpr uint32_t MPPI_FIRST_IS_NOMINAL = 1;    // QILQR_MPPI_FIRST_IS_NOMINAL
constexpr int MPPI_PLAN_PAIRS = CL_PLAN_PAIRS;   // sixteen-byte pairs of a plan knot, and of a desired knot
constexpr int MPPI_KNOT_PAIRS = 2 * MPPI_PLAN_PAIRS;
constexpr int MPPI_UPDATE_MAX_THREADS = 1024;
constexpr int MPPI_PER_LANE = MPPI_MAX_SAMPLES / MPPI_UPDATE_MAX_THREADS;  // samples a lane of the update carries at most: 4
constexpr int MPPI_CHUNK = 8;                    // knots between two block-wide combinations of the update

// what the host makes of a qilqr_mppi_rule and the handle's dt
struct MppiCoeffs {
  double sigma[4], rho[4], kappa[4];
};
// gust_coeffs' formulas (monte_carlo_kernels.h), one correlation time for the four rotors
inline void mppi_coeffs(const double sigma[4], double tau_s, double dt, MppiCoeffs &m) {
  const double rho = tau_s > 0.0 ? exp(-dt / tau_s) : 0.0;
  for (int a = 0; a < 4; ++a) {
    m.sigma[a] = sigma[a];
    m.rho[a] = rho;
    m.kappa[a] = sigma[a] * sqrt((1.0 - rho) * (1.0 + rho));
  }
}

// (one rounding per operation written: the recursion's fma is spelled out, and a weighted term is a product, then a sum)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// g (the four perturbation states of one sample, carried by the caller) advanced to knot i; nominal: the sample that flies eps = 0
QILQR_HD void mppi_eps_row(const MppiCoeffs &m, uint64_t seed, uint32_t plan, uint32_t sample, uint32_t i, bool nominal, double g[4]) {
  if (nominal) {
    g[0] = g[1] = g[2] = g[3] = 0.0;
    return;
  }
#pragma unroll
  for (int pair = 0; pair < 2; ++pair) {
    double xi[2];
    mc_draw(seed, plan, sample, i, MC_STREAM_CONTROLS, (uint32_t)pair, xi[0], xi[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int a = 2 * pair + h;
      const double kx = m.kappa[a] * xi[h];
      g[a] = i == 0 ? m.sigma[a] * xi[h] : fma(m.rho[a], g[a], kx);
    }
  }
}
QILQR_HD bool mppi_is_nominal(uint32_t flags, int sample) { return (flags & MPPI_FIRST_IS_NOMINAL) && sample == 0; }

// ---- the update: the key of a sample from its four score words, and what a lane folds
QILQR_HD double mppi_key(const double *score, double collision_cost) {
  const double cost = score[0], hits = score[3];
  if (!(hits > 0.0)) return cost;
  const double fine = collision_cost * hits;
  return cost + fine;
}
struct MppiMin {
  double key;  // the smallest finite key (+inf: none)
  int j;       // its sample (-1: none)
  int n_finite;
};
QILQR_HD MppiMin mppi_min_empty() { return MppiMin{INFINITY, -1, 0}; }
// a and b in either order give the same answer: ties go to the smaller sample
QILQR_HD MppiMin mppi_min_combine(const MppiMin &a, const MppiMin &b) {
  const bool take_b = b.j >= 0 && (a.j < 0 || b.key < a.key || (b.key == a.key && b.j < a.j));
  return MppiMin{take_b ? b.key : a.key, take_b ? b.j : a.j, a.n_finite + b.n_finite};
}
QILQR_HD MppiMin mppi_lane_min(const double *plan_score, int S, int t, int T, double collision_cost) {
  MppiMin f = mppi_min_empty();
  for (int j = t; j < S; j += T) {
    const double key = mppi_key(plan_score + 4 * (long)j, collision_cost);
    if (isfinite(key)) f = mppi_min_combine(f, MppiMin{key, j, 1});
  }
  return f;
}
// the weight of a key given the smallest (a key that is not finite: 0)
QILQR_HD double mppi_weight(double key, double jmin, double lambda) {
  if (!isfinite(key)) return 0.0;
  const double d = key - jmin;
  const double x = -d / lambda;
  return exp(x);
}
// lane t's share of eta and of q, over weights[j] in ascending j
QILQR_HD void mppi_lane_weights(const double *weights, int S, int t, int T, double &eta, double &q) {
  eta = 0.0;
  q = 0.0;
  for (int j = t; j < S; j += T) {
    const double w = weights[j], ww = w * w;
    eta += w;
    q += ww;
  }
}
// one sample's term of d_i: acc[a] += w eps[a]
QILQR_HD void mppi_fold_term(double w, const double eps[4], double acc[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const double p = w * eps[a];
    acc[a] += p;
  }
}
// the wavefronts' sums in index order
QILQR_HD double mppi_waves_in_order(const double *wave_sums, int waves, int stride) {
  double s = wave_sums[0];
  for (int w = 1; w < waves; ++w) s += wave_sums[(long)w * stride];
  return s;
}
// the new control of one rotor
QILQR_HD double mppi_new_control(double plan_u, double d, double eta, bool any, bool limited, double lo, double hi) {
  if (!any) return plan_u;
  const double du = d / eta;
  const double u = plan_u + du;
  if (!limited) return u;
  return u < lo ? lo : (u > hi ? hi : u);
}
// words 0 .. 3 of a plan's info
QILQR_HD void mppi_info_words(const MppiMin &m, double eta, double q, double out[4]) {
  const bool any = m.j >= 0;
  out[0] = any ? m.key : NAN;
  out[1] = (double)m.j;
  out[2] = any ? (eta * eta) / q : 0.0;
  out[3] = (double)m.n_finite;
}

// (as in closed_loop_kernels.h: a * b + c fuses where the source says so and nowhere else, so that the step has rollout_problem's bits)
#if defined(__clang__)
#pragma clang fp contract(on)
#endif

// the operands of knot i by per-lane (or host) loads: the plan knot, and where the desired knot and the state weights of knot i lie
struct MppiFlatFetch {
  const double *plan, *desired;  // the plan's first knot; the first desired knot (the plan's own, or the handle's at its horizon start)
  const double *q;               // knot i's state weights are q + i * q_step (q_step = 0: the handle's Q at every knot)
  long q_step;
  QILQR_HD void operator()(int i, double pt[18]) const {
    const double *p = plan + (long)i * 18;
#pragma unroll
    for (int e = 0; e < MPPI_PLAN_PAIRS; ++e) cl_load_pair(p + 2 * e, pt[2 * e], pt[2 * e + 1]);
  }
  QILQR_HD ClKnotScore score(int i) const { return ClKnotScore{desired + (long)i * 18, q + (long)i * q_step}; }
};

// what one sample of a flight is given beside its model and its fetch
struct MppiSample {
  const double *x0;     // its 13 start words
  int n;                // knots 0 .. n - 1
  uint64_t seed;
  uint32_t plan, sample;  // the draw's indices: b0 + b, j
  bool nominal;           // eps = 0 at every knot
  ClSpheres spheres;
  double *score;          // its CL_SCORE words (16-byte aligned), or null: nothing is stored
  double *traj;           // its first knot, or null: no trajectory store is issued
};

// A fetch that says so here also gives the knot's deviations: the recursion is then the UNIT one and the fetch's eps(i, z, nominal, e)
// makes the perturbation of it (mppi_adapt_kernels.h: e = spread_i z, a rounded product).  The fetches of this file do not.
template <typename Fetch>
struct MppiFetchSpreads {
  static constexpr bool value = false;
};

// One sample: closed_loop_sample<.., SCORE> (closed_loop_kernels.h) with the law u = plan_u + K dx replaced by u = plan_u + eps_i, the
// state started at knot 0 and no statistics.  The clamp, the trajectory store, the score of a knot (the same knot_cost instantiation,
// cl_score_spheres, the same running minimum and count) and the step are that routine's, statement for statement.
template <int INTEG, bool LIM, typename Fetch>
QILQR_HD void mppi_sample(const ModelConsts<double> &c, const MppiCoeffs &m, Fetch &fetch, const MppiSample &s, const double *lo = nullptr,
                          const double *hi = nullptr) {
  const double *x0 = s.x0;
  double t[3] = {x0[0], x0[1], x0[2]};
  double q[4] = {x0[4], x0[5], x0[6], x0[3]};
  double v[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[a] = x0[7 + a];
  RolloutSeries<double> sr;
  sr.load();
  double g[4] = {0.0, 0.0, 0.0, 0.0};
  double cost = 0.0, clear = HUGE_VAL;
  int clear_knot = -1, hits = 0;
  const int i1 = s.n - 1;
  for (int i = 0; i <= i1; ++i) {
    double pt[18];
    fetch(i, pt);
    mppi_eps_row(m, s.seed, s.plan, s.sample, (uint32_t)i, s.nominal, g);
    double u[4];
    if constexpr (MppiFetchSpreads<Fetch>::value) {
      double e[4];
      fetch.eps(i, g, s.nominal, e);
#pragma unroll
      for (int a = 0; a < 4; ++a) u[a] = pt[14 + a] + e[a];
    } else {
#pragma unroll
      for (int a = 0; a < 4; ++a) u[a] = pt[14 + a] + g[a];
    }
    if (LIM) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double ua = u[a];
        u[a] = ua < lo[a] ? lo[a] : (ua > hi[a] ? hi[a] : ua);
      }
    }
    const double o[18] = {pt[0], t[0], t[1], t[2], q[3], q[0], q[1], q[2], v[0], v[1], v[2], v[3], v[4], v[5], u[0], u[1], u[2], u[3]};
    if (s.traj) {
#pragma unroll
      for (int e = 0; e < 9; ++e) cl_store_pair(s.traj + (long)i * 18 + 2 * e, o[2 * e], o[2 * e + 1]);
    }
    {
      const ClKnotScore ks = fetch.score(i);
      double edx[12], edu[4], sq[12], su[4];
      double kc = knot_cost<false, double, false>(ks.Q, c.R, o, ks.pd, edx, edu, sq, su);
      double kmin = HUGE_VAL;
      cl_score_spheres(s.spheres, (double)i * c.dt, o, kc, kmin);
      cost += kc;
      if (!(kmin >= clear)) {  // (the first knot on ties; a NaN is taken)
        clear = kmin;
        clear_knot = i;
      }
      hits += kmin < 0.0 ? 1 : 0;
    }
    if (i < i1) {
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
  if (s.score) {
    cl_store_pair(s.score, cost, clear);
    cl_store_pair(s.score + 2, (double)clear_knot, (double)hits);
  }
}

#if defined(__HIPCC__)
// what k_mppi_flight reads and writes; every pointer a device one
struct MppiFlightArgs {
  const double *plan;      // [B][n][18]
  const double *x0;        // sample (b, j) starts at x0 + b * x0_step: [B][13] (13), or words 1..13 of the plan's knot 0 (plan + 1; n * 18)
  long x0_step;
  ScoreOperands ops;       // the score's (call_parts.h)
  double *score;           // sample (b, j)'s four words are score + b * score_step + 4 j
  long score_step;         // 4 S; the nominal flight of the update: 8, into words 4 .. 7 of info
  double *traj;            // [B][n][18], or null (usually): sample 0's flight is stored -- the S = 1 launch of the update
  int B, n, S;
  uint32_t b0, flags;
  int all_nominal;         // eps = 0 for every sample (the nominal flight)
  uint64_t seed;
  MppiCoeffs m;
};
// (host) the arguments of a flight of S samples per plan over `plan` from a call's launch record; the coefficients are the caller's to fill
inline MppiFlightArgs mppi_flight_args(const MppiLaunch &call, const double *plan, int S, double *score, long score_step, bool nominal, double *traj) {
  MppiFlightArgs a{};
  a.plan = plan;
  a.x0 = call.d_x0 ? call.d_x0 : call.d_plan + 1;
  a.x0_step = call.d_x0 ? CL_STATE : 18l * call.n;
  a.ops = call.score;
  a.score = score;
  a.score_step = score_step;
  a.traj = traj;
  a.B = call.B;
  a.n = call.n;
  a.S = S;
  a.b0 = (uint32_t)call.b0;
  a.flags = call.rule.flags;
  a.all_nominal = nominal ? 1 : 0;
  a.seed = call.seed;
  return a;
}

// the LDS image of a block: what is the same for the 64 samples of a plan, read by every lane at one address (a broadcast: no bank conflict)
//     knot[2][18]   the plan knot (9 pairs) and the desired knot (9), double-buffered: loaded two knots ahead by lanes 0 .. 17 into a
//                   register, written one knot ahead (ClSharedScoreFetch's scheme without the gains)
//     Q[2][144]     the knot's state weights; double-buffered with a schedule, else the handle's Q written once to both halves
//     shared[320], own[512]   the sphere tables, written once
// 9 536 bytes a block.  One barrier per knot; the barrier of the first knot stands behind the writes of prime().
struct MppiImage {
  cl_dv2 knot[2][MPPI_KNOT_PAIRS];
  double Q[2][144];
  double shared[OB_MAX * OB_WORDS];
  double own[OB_MAX * OB_BWORDS];
};
constexpr int MPPI_Q_PAIRS = 72;

struct MppiSharedFetch {
  const cl_dv2 *plan, *desired;  // the plan's first knot of each
  const cl_dv2 *q;               // the state weights of knot 0
  int q_pairs;                   // pairs between the weights of successive knots: 72, or 0
  MppiImage *img;
  int lane, i1;
  cl_dv2 next, nextq0, nextq1;
  __device__ cl_dv2 load(int i) const {
    return lane < MPPI_PLAN_PAIRS ? plan[(long)i * 9 + lane] : desired[(long)i * 9 + (lane - MPPI_PLAN_PAIRS)];
  }
  __device__ void load_q(int i, cl_dv2 &a, cl_dv2 &b) const {
    const cl_dv2 *src = q + (long)i * q_pairs;
    a = src[lane];
    if (lane < MPPI_Q_PAIRS - 64) b = src[64 + lane];
  }
  __device__ void store_q(int half, const cl_dv2 &a, const cl_dv2 &b) {
    cl_dv2 *dst = reinterpret_cast<cl_dv2 *>(img->Q[half]);
    dst[lane] = a;
    if (lane < MPPI_Q_PAIRS - 64) dst[64 + lane] = b;
  }
  // knot 0, and the tables that do not change with the knot: sp (n_shared spheres), row `b` of the tiled per-problem table (n_own of K)
  __device__ void prime(const double *sp, int n_shared, const double *own, int K, long b, int n_own) {
    if (lane < MPPI_KNOT_PAIRS) {
      img->knot[0][lane] = load(0);
      if (1 <= i1) next = load(1);
    }
    load_q(0, nextq0, nextq1);
    store_q(0, nextq0, nextq1);
    if (q_pairs == 0) store_q(1, nextq0, nextq1);
    else if (1 <= i1) load_q(1, nextq0, nextq1);
    for (int k = lane; k < n_shared * OB_WORDS; k += CL_BLOCK) img->shared[k] = sp[k];
    for (int k = lane; k < n_own * OB_BWORDS; k += CL_BLOCK) img->own[k] = own[bob_index(b, K, k / OB_BWORDS, k % OB_BWORDS)];
  }
  __device__ void operator()(int i, double pt[18]) {
    __syncthreads();
    if (lane < MPPI_KNOT_PAIRS) {
      if (i + 1 <= i1) img->knot[(i + 1) & 1][lane] = next;
      if (i + 2 <= i1) next = load(i + 2);
    }
    if (q_pairs != 0) {
      if (i + 1 <= i1) store_q((i + 1) & 1, nextq0, nextq1);
      if (i + 2 <= i1) load_q(i + 2, nextq0, nextq1);
    }
    const cl_dv2 *im = img->knot[i & 1];
#pragma unroll
    for (int e = 0; e < MPPI_PLAN_PAIRS; ++e) {
      const cl_dv2 w = im[e];
      pt[2 * e] = w[0];
      pt[2 * e + 1] = w[1];
    }
  }
  __device__ ClKnotScore score(int i) const {
    return ClKnotScore{reinterpret_cast<const double *>(&img->knot[i & 1][MPPI_PLAN_PAIRS]), img->Q[i & 1]};
  }
};

// The block of both flight kernels (k_mppi_flight here, k_mppi_flight_spread of mppi_adapt_kernels.h), written once: a block is one
// wavefront of 64 samples of ONE plan; grid B cdiv(S, 64), block g of plan g / cdiv(S, 64).  Lanes past S fly a copy of sample S - 1 (they
// take part in the loads and the barriers) and store nothing.  `image` is the block's MppiImage, and wrap(base, b) makes the kernel's
// fetch of the MppiSharedFetch over it for plan b.  TRAJ: the kernel has a trajectory store (sample 0's flight over a.traj, where that is
// given); without it no store is compiled.  The arguments come BY VALUE, as a kernel's own do: handed over by reference the sixteen
// kernels are allocated registers differently and the eight of k_mppi_flight change length, by value each keeps its instructions.
template <int INTEG, bool TRAJ, typename Wrap, typename... Lim>
__device__ __forceinline__ void mppi_flight_block(const ModelConsts<double> &c, const MppiFlightArgs a, MppiImage &image, Wrap wrap, Lim... lim) {
  constexpr bool LIM = pack_has<ControlLimits, Lim...>;
  constexpr bool MOD = pack_has<BatchModels, Lim...>;
  const int lane = threadIdx.x;
  const int per = (a.S + CL_BLOCK - 1) / CL_BLOCK;
  const int b = (int)blockIdx.x / per;  // (block-uniform; the host launches exactly B * per blocks)
  int j = ((int)blockIdx.x - b * per) * CL_BLOCK + lane;
  const bool live = j < a.S;
  if (!live) j = a.S - 1;
  const double *lo = nullptr, *hi = nullptr;
  if constexpr (LIM) {
    const ControlLimits &L = pack_get<ControlLimits>(lim...);
    lo = L.lo;
    hi = L.hi;
  }
  const double *plan = a.plan + (long)b * a.n * 18, *desired = a.ops.desired + (long)b * a.ops.desired_step;
  const SphereTables &t = a.ops.spheres;
  const int n_own = t.own ? t.own_counts[b] : 0;
  MppiSample s;
  s.x0 = a.x0 + (long)b * a.x0_step;
  s.n = a.n;
  s.seed = a.seed;
  s.plan = a.b0 + (uint32_t)b;
  s.sample = (uint32_t)j;
  s.nominal = a.all_nominal != 0 || mppi_is_nominal(a.flags, j);
  s.spheres = ClSpheres{image.shared, t.n_shared, image.own, n_own, 1, OB_BWORDS};
  s.score = live ? a.score + (long)b * a.score_step + 4 * (long)j : nullptr;
  s.traj = (TRAJ && live && j == 0 && a.traj) ? a.traj + (long)b * a.n * 18 : nullptr;
  auto fetch = wrap(MppiSharedFetch{reinterpret_cast<const cl_dv2 *>(plan), reinterpret_cast<const cl_dv2 *>(desired), reinterpret_cast<const cl_dv2 *>(a.ops.q),
                                    a.ops.q_step / 2, &image, lane, a.n - 1, cl_dv2{0.0, 0.0}, cl_dv2{0.0, 0.0}, cl_dv2{0.0, 0.0}},
                    b);
  fetch.prime(t.shared, t.n_shared, t.own, t.own_K, b, n_own);
  if constexpr (MOD) {
    const ModelConsts<double> cm = problem_model(c, pack_get<BatchModels>(lim...), (long)b);
    mppi_sample<INTEG, LIM>(cm, a.m, fetch, s, lo, hi);
  } else {
    mppi_sample<INTEG, LIM>(c, a.m, fetch, s, lo, hi);
  }
}

// Lim as k_closed_loop takes it: ControlLimits, BatchModels (plan b steps with model b), both (ControlLimits first) or neither.
template <int INTEG, typename... Lim>
__global__ __launch_bounds__(CL_BLOCK) void k_mppi_flight(ModelConsts<double> c, MppiFlightArgs a, Lim... lim) {
  __shared__ MppiImage image;
  mppi_flight_block<INTEG, true>(c, a, image, [](const MppiSharedFetch &base, int) { return base; }, lim...);
}

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

struct MppiUpdateArgs {
  const double *plan;    // [B][n][18]
  const double *score;   // [B][S][4]
  double *out_plan;      // [B][n][18]: time and states copied, controls new
  double *info;          // [B][8]: words 0 .. 3
  int n, S;
  uint32_t b0, flags;
  uint64_t seed;
  double lambda, collision_cost;
  MppiCoeffs m;
  int limited;               // the thrust limits are set: lim_lo, lim_hi per rotor
  double lim_lo[4], lim_hi[4];
};

// (host) the arguments of an update from a call's launch record and the recursion's coefficients
inline MppiUpdateArgs mppi_update_args(const MppiLaunch &call, const MppiCoeffs &m) {
  MppiUpdateArgs a{};
  a.plan = call.d_plan;
  a.score = call.d_score;
  a.out_plan = call.d_out_plan;
  a.info = call.d_info;
  a.n = call.n;
  a.S = call.S;
  a.b0 = (uint32_t)call.b0;
  a.flags = call.rule.flags;
  a.seed = call.seed;
  a.lambda = call.rule.lambda;
  a.collision_cost = call.rule.collision_cost;
  a.m = m;
  a.limited = call.limits ? 1 : 0;
  for (int r = 0; r < 4; ++r) {
    a.lim_lo[r] = call.limits ? call.limits->lo[r] : 0.0;
    a.lim_hi[r] = call.limits ? call.limits->hi[r] : 0.0;
  }
  return a;
}

__device__ __forceinline__ MppiMin mppi_min_from(const MppiMin &f, int off) {
  MppiMin o;
  o.key = __shfl_xor(f.key, off);
  o.j = __shfl_xor(f.j, off);
  o.n_finite = __shfl_xor(f.n_finite, off);
  return o;
}

// One block of THREADS = mppi_update_lanes(S) lanes (mppi_launch.h) per plan: grid B.  Static LDS: the plan's weights (32 KB at the cap) and the
// wavefronts' partial sums of MPPI_CHUNK knots -- nothing that grows with n.  A lane carries the recursion state of its (at most four)
// samples in registers through the knots, redrawing what the flight drew.
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_mppi_update(const MppiUpdateArgs a) {
  constexpr int WAVES = THREADS / 64;
  __shared__ double weights[THREADS == MPPI_UPDATE_MAX_THREADS ? MPPI_MAX_SAMPLES : THREADS];  // (below the cap S <= THREADS)
  __shared__ double part[MPPI_CHUNK][WAVES][4];
  __shared__ double wmin_key[WAVES], wsum[2][WAVES];
  __shared__ int wmin_j[WAVES], wmin_n[WAVES];
  const int t = (int)threadIdx.x, wave = t >> 6, b = (int)blockIdx.x, S = a.S, n = a.n;
  const double *plan = a.plan + (long)b * n * 18, *mine = a.score + 4 * (long)b * S;
  double *out = a.out_plan + (long)b * n * 18;
  // time and states: pairs 0 .. 6 of every knot, word for word (pairs 7 and 8, the controls, are written below)
  for (long p = t; p < 7l * n; p += THREADS) {
    const long i = p / 7, e = p - 7 * i;
    reinterpret_cast<cl_dv2 *>(out)[i * 9 + e] = reinterpret_cast<const cl_dv2 *>(plan)[i * 9 + e];
  }
  // J_min, its sample and the count of finite keys
  MppiMin f = mppi_lane_min(mine, S, t, THREADS, a.collision_cost);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) f = mppi_min_combine(f, mppi_min_from(f, off));
  if ((t & 63) == 0) {
    wmin_key[wave] = f.key;
    wmin_j[wave] = f.j;
    wmin_n[wave] = f.n_finite;
  }
  __syncthreads();
  f = MppiMin{wmin_key[0], wmin_j[0], wmin_n[0]};
  for (int w = 1; w < WAVES; ++w) f = mppi_min_combine(f, MppiMin{wmin_key[w], wmin_j[w], wmin_n[w]});
  const bool any = f.j >= 0;
  // the weights, then eta and q
  for (int j = t; j < S; j += THREADS) weights[j] = any ? mppi_weight(mppi_key(mine + 4 * (long)j, a.collision_cost), f.key, a.lambda) : 0.0;
  double eta, q;
  mppi_lane_weights(weights, S, t, THREADS, eta, q);  // (a lane reads back what it wrote: no barrier)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    eta += __shfl_xor(eta, off);
    q += __shfl_xor(q, off);
  }
  if ((t & 63) == 0) {
    wsum[0][wave] = eta;
    wsum[1][wave] = q;
  }
  __syncthreads();
  eta = mppi_waves_in_order(wsum[0], WAVES, 1);
  q = mppi_waves_in_order(wsum[1], WAVES, 1);
  if (t == 0) {
    double w4[4];
    mppi_info_words(f, eta, q, w4);
    cl_store_pair(a.info + (long)b * MPPI_INFO, w4[0], w4[1]);
    cl_store_pair(a.info + (long)b * MPPI_INFO + 2, w4[2], w4[3]);
  }
  // the weighted perturbations, MPPI_CHUNK knots between two combinations of the wavefronts
  double g[MPPI_PER_LANE][4];
#pragma unroll
  for (int k = 0; k < MPPI_PER_LANE; ++k) g[k][0] = g[k][1] = g[k][2] = g[k][3] = 0.0;
  const uint32_t pl = a.b0 + (uint32_t)b;
  for (int c0 = 0; c0 < n; c0 += MPPI_CHUNK) {
    const int now = n - c0 < MPPI_CHUNK ? n - c0 : MPPI_CHUNK;
    for (int ii = 0; ii < now; ++ii) {
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < MPPI_PER_LANE; ++k) {
        const int j = t + k * THREADS;
        if (j < S) {
          mppi_eps_row(a.m, a.seed, pl, (uint32_t)j, (uint32_t)(c0 + ii), mppi_is_nominal(a.flags, j), g[k]);
          mppi_fold_term(weights[j], g[k], acc);
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += __shfl_xor(acc[r], off);
      }
      if ((t & 63) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[ii][wave][r] = acc[r];
      }
    }
    __syncthreads();
    if (t < 4 * now) {
      const int ii = t >> 2, r = t & 3;
      const double d = mppi_waves_in_order(&part[ii][0][r], WAVES, 4);
      const long w = (long)(c0 + ii) * 18 + 14 + r;
      double lo = a.lim_lo[0], hi = a.lim_hi[0];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        lo = r == k ? a.lim_lo[k] : lo;
        hi = r == k ? a.lim_hi[k] : hi;
      }
      out[w] = mppi_new_control(plan[w], d, eta, any, a.limited != 0, lo, hi);
    }
    __syncthreads();
  }
}
#endif

}  // namespace qilqr

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
