// risk_kernels.h -- what a caller flies samples for, on the device:
//   k_risk_scores    risk[B][L][4] from score[B][S][4]: per plan the order statistic at each level (VaR) and the mean of the tail
//                    behind it (CVaR), of the cost or of the negated clearance -- a sort of the plan's S keys
//   k_select_plans   choice[V], info[V][4]: of the C candidate plans of a vehicle (plan b = c V + v) the best feasible one
//   k_gather_plans   out_plan[V][n][18], out_gains[V][n][52]: the chosen candidates' plans and laws, word for word
// They follow k_reduce_scores (monte_carlo_kernels.h) on the handle's stream and read what it and the scored flight wrote.
//
// The per-lane routines are QILQR_HD and carry all the decisions: the key of a sample, the order of two samples, the sorting network's
// schedule, a lane's share of a tail sum, the choice of a vehicle.  tests/host_risk_harness.cpp runs the same text on the host.
//
// k_risk_scores.  One block per plan.  Sample j's key is its cost, or minus its clearance, so that the bad end is always the upper
// tail; a NaN key is +inf (a diverged flight is the worst outcome -- unlike word 0 of the summary, which skips it).  The samples are
// ordered by (key, j): a total order, so the sorted permutation is unique whatever network produced it.  The network is the bitonic
// one over P = the power of two >= S slots in LDS, keys (8 bytes) and sample indices (4 bytes) in separate arrays, padding slots
// (+inf, j >= S) behind every real sample.  risk_comparator(k, j, t) is the schedule: comparator t of P / 2 in the stage (k, j) --
// k = 2, 4, ..., P the length of the runs being merged, j = k / 2, ..., 1 the distance of the pair.  A lane owns a comparator; a stage
// ends with a block barrier (with THREADS = 64, S <= 128, the block is one wavefront and the compiler leaves no barrier instruction:
// the LDS operations of a wavefront complete in order).  After the sort wavefront 0 produces every level: with k the rank and
// m = S - k, lane l folds the keys at sorted positions k + l, k + l + 64, ... in that order, the lanes combine by the butterfly
// 32, 16, 8, 4, 2, 1 with IEEE additions (as k_reduce_scores), and lane 0 writes {t_0, sum / m, sample at position k, m} -- words 0
// and 1 negated for the clearance column.  No atomics; a plan's words depend on the multiset of its keys only (word 2: on their order).
#pragma once

#include <math.h>
#include <stdint.h>

#include "se3_math.h"  // QILQR_HD

// (one rounding per operation written)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace qilqr {

constexpr int RISK_WORDS = 4;           // QILQR_MC_RISK
constexpr int RISK_MAX_LEVELS = 8;      // QILQR_RISK_MAX_LEVELS
constexpr int RISK_MAX_SAMPLES = 4096;  // QILQR_RISK_MAX_SAMPLES
constexpr int RISK_COST = 0, RISK_CLEARANCE = 1;
constexpr int SELECT_INFO = 4;          // QILQR_SELECT_INFO
constexpr int GATHER_BLOCK = 256;
constexpr int GATHER_PLAN16 = 9, GATHER_GAIN16 = 26;  // 16-byte pieces of a knot of the plan (18 words) and of its gains (52 words)

// the slots of the network: the power of two >= S
QILQR_HD int risk_slots(int S) {
  int P = 1;
  while (P < S) P <<= 1;
  return P;
}
// the lanes of a block: one per comparator, at least a wavefront, at most 1024
QILQR_HD int risk_threads(int P) { return P / 2 < 64 ? 64 : (P / 2 > 1024 ? 1024 : P / 2); }

// the rank of a level in [0, 1) among S samples, in double: k = min(S - 1, max(0, ceil(level S) - 1)).  Host only.
inline int risk_rank(double level, int S) {
  const double k = ceil(level * (double)S) - 1.0;
  return k < 0.0 ? 0 : (k > (double)(S - 1) ? S - 1 : (int)k);
}

// the key of a sample from its four score words {cost, min_clearance, ...}
QILQR_HD double risk_key(const double *score, int column) {
  const double v = column == RISK_COST ? score[0] : -score[1];
  return v != v ? INFINITY : v;
}
// (ka, ja) lies before (kb, jb): the keys hold no NaN
QILQR_HD bool risk_before(double ka, int ja, double kb, int jb) { return ka < kb || (ka == kb && ja < jb); }

// the schedule: comparator t (0 <= t < P / 2) of stage (k, j) meets slots lo < hi = lo + j, and leaves the earlier of the two in lo
// when `up`, in hi otherwise
struct RiskPair {
  int lo, hi;
  bool up;
};
QILQR_HD RiskPair risk_comparator(int k, int j, int t) {
  const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  return RiskPair{lo, lo | j, (lo & k) == 0};
}
QILQR_HD void risk_exchange(double *keys, int *idx, const RiskPair p) {
  const double ka = keys[p.lo], kb = keys[p.hi];
  const int ja = idx[p.lo], jb = idx[p.hi];
  if (risk_before(kb, jb, ka, ja) == p.up) {
    keys[p.lo] = kb; idx[p.lo] = jb;
    keys[p.hi] = ka; idx[p.hi] = ja;
  }
}

// lane's share of the tail sum: the keys at sorted positions k + lane, k + lane + 64, ... below S, in that order
QILQR_HD double risk_tail_lane(const double *sorted_keys, int S, int k, int lane) {
  double sum = 0.0;
  for (int p = k + lane; p < S; p += 64) sum += sorted_keys[p];
  return sum;
}
// the four words of a level from the order statistic, the whole tail's sum, the sample at the rank and the tail's count
QILQR_HD void risk_words(double t0, double sum, int sample, int m, int column, double out[RISK_WORDS]) {
  const double mean = sum / (double)m;
  out[0] = column == RISK_COST ? t0 : -t0;
  out[1] = column == RISK_COST ? mean : -mean;
  out[2] = (double)sample;
  out[3] = (double)m;
}

// ---- the choice among a vehicle's candidates
struct SelectRule {       // qilqr_select_rule
  int32_t objective;      // 0: summary word 0; 1: summary word 2; 2: risk word 0; 3: risk word 1
  int32_t level;
  double max_collision_fraction, max_diverged_fraction, min_clearance;
};
QILQR_HD double select_objective(const SelectRule &r, const double *summary, const double *risk, int n_levels, long b) {
  if (r.objective == 0) return summary[8 * b];
  if (r.objective == 1) return summary[8 * b + 2];
  return risk[(b * n_levels + r.level) * RISK_WORDS + (r.objective == 2 ? 0 : 1)];
}
// vehicle v of V with C candidates: the feasible candidate with the smallest (objective, c); without one, the smallest
// (collision fraction, diverged fraction, objective with NaN as +inf, c).  Every comparison is exact.
QILQR_HD int select_vehicle(const SelectRule &r, const double *summary, const double *risk, int n_levels, int V, int C, int v, double info[SELECT_INFO]) {
  int best = -1, n_feasible = 0, back = -1;
  double best_obj = 0.0, back_coll = 0.0, back_div = 0.0, back_obj = 0.0;
  for (int c = 0; c < C; ++c) {
    const long b = (long)c * V + v;
    const double obj = select_objective(r, summary, risk, n_levels, b), coll = summary[8 * b + 4], clear = summary[8 * b + 5], div = summary[8 * b + 7];
    if (coll <= r.max_collision_fraction && div <= r.max_diverged_fraction && clear >= r.min_clearance && obj == obj) {
      n_feasible += 1;
      if (best < 0 || obj < best_obj) { best = c; best_obj = obj; }
    }
    const double o = obj != obj ? INFINITY : obj;
    if (back < 0 || coll < back_coll || (coll == back_coll && (div < back_div || (div == back_div && o < back_obj)))) {
      back = c; back_coll = coll; back_div = div; back_obj = o;
    }
  }
  const int c = best >= 0 ? best : back;
  const long b = (long)c * V + v;
  info[0] = select_objective(r, summary, risk, n_levels, b);
  info[1] = (double)n_feasible;
  info[2] = summary[8 * b + 4];
  info[3] = best >= 0 ? 0.0 : 1.0;
  return c;
}

}  // namespace qilqr

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace qilqr {

struct RiskScoresArgs {
  const double *score;  // [B][S][4]
  double *risk;         // [B][n_levels][4]
  int S, P, column, n_levels;
  int rank[RISK_MAX_LEVELS];
};

// grid B, block THREADS = risk_threads(P), dynamic LDS 12 P bytes: keys[P] (8-byte) and behind them idx[P] (4-byte)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_risk_scores(const RiskScoresArgs a) {
  extern __shared__ __attribute__((aligned(16))) double risk_lds[];  // (the kernel has no static LDS before it: the base is 0)
  double *const keys = risk_lds;
  int *const idx = reinterpret_cast<int *>(risk_lds + a.P);
  const int t = (int)threadIdx.x, S = a.S, P = a.P;
  const double *mine = a.score + 4 * (long)blockIdx.x * S;
  for (int p = t; p < P; p += THREADS) {
    keys[p] = p < S ? risk_key(mine + 4 * (long)p, a.column) : INFINITY;
    idx[p] = p;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j >= 1; j >>= 1) {
      for (int c = t; c < P / 2; c += THREADS) risk_exchange(keys, idx, risk_comparator(k, j, c));
      __syncthreads();
    }
  if (t >= 64) return;
  for (int l = 0; l < a.n_levels; ++l) {
    const int k = a.rank[l];
    double sum = risk_tail_lane(keys, S, k, t);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (t == 0) {
      double out[RISK_WORDS];
      risk_words(keys[k], sum, idx[k], S - k, a.column, out);
      double *o = a.risk + ((long)blockIdx.x * a.n_levels + l) * RISK_WORDS;
#pragma unroll
      for (int w = 0; w < RISK_WORDS; ++w) o[w] = out[w];
    }
  }
}

struct SelectPlansArgs {
  const double *summary;  // [C V][8]
  const double *risk;     // [C V][n_levels][4], or null (objectives 0 and 1)
  int32_t *choice;        // [V]
  double *info;           // [V][4]
  int n_levels, V, C;
  SelectRule rule;
};

// a lane per vehicle: grid ceil(V / 64), block 64
__global__ void __launch_bounds__(64) k_select_plans(const SelectPlansArgs a) {
  const int v = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (v >= a.V) return;
  double info[SELECT_INFO];
  a.choice[v] = select_vehicle(a.rule, a.summary, a.risk, a.n_levels, a.V, a.C, v, info);
#pragma unroll
  for (int w = 0; w < SELECT_INFO; ++w) a.info[(long)v * SELECT_INFO + w] = info[w];
}

struct GatherPlansArgs {
  const int32_t *choice;  // [V], read from device memory: k_select_plans wrote it
  const double2 *plan, *gains;  // [C V][n][9], [C V][n][26] 16-byte pieces
  double2 *out_plan, *out_gains;
  int V, C, n;
};

// grid (V, pieces of a vehicle's n * 35 16-byte words), block GATHER_BLOCK
__global__ void __launch_bounds__(GATHER_BLOCK) k_gather_plans(const GatherPlansArgs a) {
  const int v = (int)blockIdx.x, c = a.choice[v];
  if (c < 0 || c >= a.C) return;  // (never k_select_plans' answer: nothing is read outside the arrays whatever the word holds)
  const long b = (long)c * a.V + v, np = (long)a.n * GATHER_PLAN16, ng = (long)a.n * GATHER_GAIN16;
  for (long q = (long)blockIdx.y * GATHER_BLOCK + threadIdx.x; q < np + ng; q += (long)gridDim.y * GATHER_BLOCK) {
    if (q < np) a.out_plan[v * np + q] = a.plan[b * np + q];
    else a.out_gains[v * ng + (q - np)] = a.gains[b * ng + (q - np)];
  }
}

}  // namespace qilqr
#endif

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
