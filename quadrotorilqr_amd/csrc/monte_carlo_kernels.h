// monte_carlo_kernels.h -- the ends of the Monte-Carlo loop about a plan, on the device:
//   k_sample_gusts    wrench[B][S][n_w][6], a stationary first-order Gauss-Markov gust per component (white noise when tau = 0)
//   k_sample_states   x0[b, s] = x_nom[b] (+) delta, delta_c = sigma_c xi_c over the 12 tangent words [rho, theta, dv, dw]
//   k_reduce_scores   summary[B][8] from score[B][S][4]: what a caller wants to know about a plan
// between them flies k_closed_loop_scored (closed_loop_scored_kernels.h), which reads the first two arrays and writes the third's input.
// The normals are philox.h's: a word of the output is a function of (seed, b0 + b, s0 + s, row, component) and of the model alone.
//
// The per-lane routines are QILQR_HD and carry all the arithmetic; tests/host_monte_carlo_harness.cpp runs the same text on the host,
// the reduction's 64 lanes and its tree included.
//
// k_sample_gusts.  The recursion is sequential in the row and independent across (flight, pair of components): a lane owns one pair of
// one flight and makes one Philox call and 16 bytes per row.  A flight's rows are contiguous, flights lie n_w * 48 bytes apart: stored
// from where they are made, a wave-instruction would touch 21 flights with 48 bytes each -- many short pieces in many rows, the
// shape the write path serves far below the rate of contiguous segments.  So a block of 192 lanes (64 flights x 3 pairs) makes
// MC_GUST_ROWS rows into LDS and then stores them in the array's own order, 16 bytes per lane: runs of MC_GUST_ROWS * 48 = 384
// contiguous bytes per flight, 2 2/3 runs per wave-instruction.  The LDS image is the output's order with one 16-byte slot of padding per
// flight, so the stores read it linearly and the lanes that fill it (a flight apart: 25 slots = 400 bytes) spread over the banks.
//
// k_reduce_scores.  One wavefront per plan; lane l folds samples l, l + 64, ... in order, the lanes are combined by the butterfly
// 32, 16, 8, 4, 2, 1 (__shfl_xor; the combination is commutative, so every lane ends with the bits lane 0 of the tree 32 ... 1 has), the
// mean goes back to every lane and the squared deviations take the same two steps.  No atomics, and a plan's bits depend on its rows only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "philox.h"
#include "se3_math.h"

// (one rounding per operation written: the recursion's fma is spelled out, and mean + sigma xi stays a product and a sum)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace qilqr {

constexpr int MC_SUMMARY = 8;       // QILQR_MC_SUMMARY
constexpr int MC_GUST_FLIGHTS = 64; // flights of a block of k_sample_gusts
constexpr int MC_GUST_BLOCK = 3 * MC_GUST_FLIGHTS;
constexpr int MC_GUST_ROWS = 8;     // rows between two write-outs
constexpr int MC_GUST_SLOTS = 3 * MC_GUST_ROWS + 1;  // 16-byte slots of a flight in LDS (one of padding)
constexpr int MC_STATE_BLOCK = 64;
constexpr uint32_t MC_FIRST_IS_NOMINAL = 1;  // flags of k_sample_states

// what the host makes of a qilqr_gust_model and the handle's dt
struct GustCoeffs {
  double mean[6], sigma[6], rho[6], kappa[6];
};
// rho = exp(-dt / tau) (0: white), kappa = sigma sqrt((1 - rho)(1 + rho)): the stationary recursion g_i = rho g_{i-1} + kappa xi_i
inline void gust_coeffs(const double mean[6], const double sigma[6], double tau_force_s, double tau_torque_s, double dt, GustCoeffs &g) {
  for (int c = 0; c < 6; ++c) {
    const double tau = c < 3 ? tau_force_s : tau_torque_s;
    const double rho = tau > 0.0 ? exp(-dt / tau) : 0.0;
    g.mean[c] = mean[c];
    g.sigma[c] = sigma[c];
    g.rho[c] = rho;
    g.kappa[c] = sigma[c] * sqrt((1.0 - rho) * (1.0 + rho));
  }
}

// one row of one pair of components: g (the two gust states, carried by the caller) advanced to row i, and the two words of the wrench
QILQR_HD void gust_row(const GustCoeffs &m, uint64_t seed, uint32_t plan, uint32_t sample, uint32_t i, int pair, double g[2], double w[2]) {
  double xi[2];
  mc_draw(seed, plan, sample, i, MC_STREAM_GUSTS, (uint32_t)pair, xi[0], xi[1]);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 2 * pair + h;
    g[h] = i == 0 ? m.sigma[c] * xi[h] : fma(m.rho[c], g[h], m.kappa[c] * xi[h]);
    w[h] = m.mean[c] + g[h];
  }
}

// one start state: x (13 words: t, q w x y z, v, w) = x_nom (+) sigma xi, the pose by se3_rplus, the velocities by addition
QILQR_HD void sample_state(const double *x_nom, const double sigma[12], uint64_t seed, uint32_t plan, uint32_t sample, uint32_t flags, double x[13]) {
  if ((flags & MC_FIRST_IS_NOMINAL) && sample == 0) {
#pragma unroll
    for (int a = 0; a < 13; ++a) x[a] = x_nom[a];
    return;
  }
  double d[12];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double z0, z1;
    mc_draw(seed, plan, sample, 0, MC_STREAM_STATES, (uint32_t)j, z0, z1);
    d[2 * j] = sigma[2 * j] * z0;
    d[2 * j + 1] = sigma[2 * j + 1] * z1;
  }
  const double t[3] = {x_nom[0], x_nom[1], x_nom[2]}, q[4] = {x_nom[4], x_nom[5], x_nom[6], x_nom[3]};
  double tn[3], qn[4];
  se3_rplus(t, q, d, tn, qn);
  x[0] = tn[0]; x[1] = tn[1]; x[2] = tn[2];
  x[3] = qn[3]; x[4] = qn[0]; x[5] = qn[1]; x[6] = qn[2];
#pragma unroll
  for (int a = 0; a < 6; ++a) x[7 + a] = x_nom[7 + a] + d[6 + a];
}

// ---- the reduction: what a lane has folded, the fold of one sample, and the combination of two lanes
struct McFold {
  double sum;        // of the finite costs
  double max_cost;   // the largest finite cost (-inf: none)
  double min_clear;  // the smallest clearance (+inf: none below it)
  int n_finite, i_max, i_min, n_collide, n_bad;
};
QILQR_HD McFold mc_fold_empty() { return McFold{0.0, -INFINITY, INFINITY, 0, -1, -1, 0, 0}; }
// sample j of a plan: its four score words {cost, min_clearance, knot_of_min_clearance, knots_in_collision}
QILQR_HD void mc_fold_sample(McFold &f, const double *score, int j) {
  const double cost = score[0], clear = score[1], hits = score[3];
  if (isfinite(cost)) {
    f.sum += cost;
    f.n_finite += 1;
    if (cost > f.max_cost) { f.max_cost = cost; f.i_max = j; }
  } else {
    f.n_bad += 1;
  }
  if (clear < f.min_clear) { f.min_clear = clear; f.i_min = j; }  // (a NaN and +inf are never below)
  if (hits > 0.0) f.n_collide += 1;
}
// a and b in either order give the same bits: sums are commutative, and the extremes break ties by the smaller index
QILQR_HD McFold mc_fold_combine(const McFold &a, const McFold &b) {
  McFold o;
  o.sum = a.sum + b.sum;
  o.n_finite = a.n_finite + b.n_finite;
  o.n_collide = a.n_collide + b.n_collide;
  o.n_bad = a.n_bad + b.n_bad;
  const bool b_max = b.i_max >= 0 && (a.i_max < 0 || b.max_cost > a.max_cost || (b.max_cost == a.max_cost && b.i_max < a.i_max));
  o.max_cost = b_max ? b.max_cost : a.max_cost;
  o.i_max = b_max ? b.i_max : a.i_max;
  const bool b_min = b.i_min >= 0 && (a.i_min < 0 || b.min_clear < a.min_clear || (b.min_clear == a.min_clear && b.i_min < a.i_min));
  o.min_clear = b_min ? b.min_clear : a.min_clear;
  o.i_min = b_min ? b.i_min : a.i_min;
  return o;
}
// the lane's share of the second pass: the squared deviations of its finite costs from the mean, in sample order
QILQR_HD double mc_fold_deviations(const double *plan_score, int S, int lane, double mean) {
  double ss = 0.0;
  for (int j = lane; j < S; j += 64) {
    const double cost = plan_score[4 * (long)j];
    if (isfinite(cost)) {
      const double d = cost - mean;
      ss += d * d;
    }
  }
  return ss;
}
QILQR_HD McFold mc_fold_lane(const double *plan_score, int S, int lane) {
  McFold f = mc_fold_empty();
  for (int j = lane; j < S; j += 64) mc_fold_sample(f, plan_score + 4 * (long)j, j);
  return f;
}
// the eight words from the whole plan's fold and its summed squared deviations (without a finite cost: NaN, NaN, NaN, -1)
QILQR_HD void mc_summary(const McFold &f, double ss, int S, double out[MC_SUMMARY]) {
  const bool any = f.n_finite > 0;
  out[0] = any ? f.sum / (double)f.n_finite : NAN;
  out[1] = any ? sqrt(ss / (double)f.n_finite) : NAN;
  out[2] = any ? f.max_cost : NAN;
  out[3] = (double)f.i_max;
  out[4] = (double)f.n_collide / (double)S;
  out[5] = f.min_clear;
  out[6] = (double)f.i_min;
  out[7] = (double)f.n_bad / (double)S;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qilqr {

struct SampleGustsArgs {
  double *wrench;  // [B][S][n_w][6], 16-byte aligned
  int B, S, n_w;
  uint32_t b0, s0;
  uint64_t seed;
  GustCoeffs m;
};

__global__ void __launch_bounds__(MC_GUST_BLOCK) k_sample_gusts(const SampleGustsArgs a) {
  __shared__ double2 rows[MC_GUST_FLIGHTS * MC_GUST_SLOTS];
  const int t = (int)threadIdx.x, fl = t / 3, pair = t - 3 * fl;
  const long flights = (long)a.B * a.S, first = (long)blockIdx.x * MC_GUST_FLIGHTS, f = first + fl;
  const bool live = f < flights;
  const uint32_t plan = a.b0 + (uint32_t)(live ? f / a.S : 0), sample = a.s0 + (uint32_t)(live ? f % a.S : 0);
  double2 *const out = reinterpret_cast<double2 *>(a.wrench);
  double g[2] = {0.0, 0.0};
  for (int r0 = 0; r0 < a.n_w; r0 += MC_GUST_ROWS) {
    const int rows_now = a.n_w - r0 < MC_GUST_ROWS ? a.n_w - r0 : MC_GUST_ROWS;
    if (live)
      for (int k = 0; k < rows_now; ++k) {
        double w[2];
        gust_row(a.m, a.seed, plan, sample, (uint32_t)(r0 + k), pair, g, w);
        rows[fl * MC_GUST_SLOTS + 3 * k + pair] = make_double2(w[0], w[1]);
      }
    __syncthreads();
    // the block's rows in the array's order: slot q of flight e is the 16 bytes at ((first + e) n_w + r0) * 48 + 16 q
    // (the walk is over whole chunks, so that the divisor is a constant; a last, shorter chunk leaves lanes idle)
    constexpr int per = 3 * MC_GUST_ROWS;
#pragma unroll
    for (int q = t; q < MC_GUST_FLIGHTS * per; q += MC_GUST_BLOCK) {
      const int e = q / per, w = q - e * per;
      if (first + e < flights && w < 3 * rows_now) out[((first + e) * a.n_w + r0) * 3 + w] = rows[e * MC_GUST_SLOTS + w];
    }
    __syncthreads();
  }
}

struct SampleStatesArgs {
  const double *x_nom;  // [B][13]
  double *x0;           // [B][S][13]
  int B, S;
  uint32_t b0, s0, flags;
  uint64_t seed;
  double sigma[12];
};

__global__ void __launch_bounds__(MC_STATE_BLOCK) k_sample_states(const SampleStatesArgs a) {
  const long r = (long)blockIdx.x * MC_STATE_BLOCK + threadIdx.x;
  if (r >= (long)a.B * a.S) return;
  const long b = r / a.S, s = r % a.S;
  double x[13];
  sample_state(a.x_nom + 13 * b, a.sigma, a.seed, a.b0 + (uint32_t)b, a.s0 + (uint32_t)s, a.flags, x);
  double *o = a.x0 + 13 * r;
#pragma unroll
  for (int k = 0; k < 13; ++k) o[k] = x[k];
}

__device__ __forceinline__ McFold mc_fold_from(const McFold &f, int off) {
  McFold o;
  o.sum = __shfl_xor(f.sum, off);
  o.max_cost = __shfl_xor(f.max_cost, off);
  o.min_clear = __shfl_xor(f.min_clear, off);
  o.n_finite = __shfl_xor(f.n_finite, off);
  o.i_max = __shfl_xor(f.i_max, off);
  o.i_min = __shfl_xor(f.i_min, off);
  o.n_collide = __shfl_xor(f.n_collide, off);
  o.n_bad = __shfl_xor(f.n_bad, off);
  return o;
}

// one wavefront per plan: grid B, block 64
__global__ void __launch_bounds__(64) k_reduce_scores(const double *score, int B, int S, double *summary) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const double *mine = score + 4 * (long)b * S;
  McFold f = mc_fold_lane(mine, S, lane);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) f = mc_fold_combine(f, mc_fold_from(f, off));
  const double mean = f.n_finite > 0 ? f.sum / (double)f.n_finite : 0.0;
  double ss = mc_fold_deviations(mine, S, lane, mean);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
  if (lane == 0) {
    double out[MC_SUMMARY];
    mc_summary(f, ss, S, out);
#pragma unroll
    for (int k = 0; k < MC_SUMMARY; ++k) summary[(long)b * MC_SUMMARY + k] = out[k];
  }
}

}  // namespace qilqr
#endif

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
