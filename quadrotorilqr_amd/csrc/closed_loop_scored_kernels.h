// closed_loop_scored_kernels.h -- k_closed_loop_scored: the closed-loop flight of closed_loop_kernels.h under a disturbance wrench and / or
// with a score per sample (qilqr_closed_loop_scored[_device]).  The per-sample routine is closed_loop_sample with its WRENCH and SCORE
// switches (closed_loop_kernels.h, where the arithmetic and its order are written); this file is the kernel around it: which sample a lane
// flies, where its operands come from, and the LDS image of the shared-operand form.  The two forms and their rule
// (closed_loop_shared_form) are k_closed_loop's.
//
// Shared-operand form with SCORE: everything of the score that is the same for the 64 samples of a block sits in LDS and is read by
// every lane at one address (a broadcast):
//     knot[2][42]   the plan knot (9 pairs), the gains (24) and the desired knot (9), double-buffered: loaded two knots ahead by lanes
//                   0 .. 41 into a register, written one knot ahead (ClSharedFetch's scheme, nine lanes wider)
//     Q[2][144]     the knot's state weights.  With a schedule: double-buffered like the knot, two more registers per lane (pairs
//                   0 .. 63 by every lane, 64 .. 71 by lanes 0 .. 7).  Without: the handle's Q, written once to both halves.
//     shared[320]   the shared sphere table, written once
//     own[512]      the plan's row of the per-problem table, gathered once out of the tiled device layout (bob_index) into
//                   [sphere][OB_BWORDS]
// 10 304 bytes a block.  One barrier per knot, as before; the barrier of the first knot stands behind the writes of prime().
// With WRENCH alone the image is ClSharedFetch's: the wrench is per lane.
// Part of closed_loop_scored.hip's translation unit (gfx950 only).
#pragma once

#include "call_parts.h"
#include "closed_loop_kernels.h"

#if defined(__clang__)
#pragma clang fp contract(on)
#endif

namespace qilqr {

// what a scored call reads beside ClosedLoopArgs; every pointer a device one
struct ClosedLoopScoreArgs {
  const double *wrench;    // [B][S][n_w][6], or null (then WRENCH is off)
  int n_w;                 // 1 or n
  ScoreOperands ops;       // the score's (call_parts.h); not read without out_score
  double *out_score;       // [B][S][4], or null
};

#if defined(__HIPCC__)
struct ClScoreImage {
  cl_dv2 knot[2][CL_PAIRS + CL_PLAN_PAIRS];
  double Q[2][144];
  double shared[OB_MAX * OB_WORDS];
  double own[OB_MAX * OB_BWORDS];
};
constexpr int CL_SCORE_PAIRS = CL_PAIRS + CL_PLAN_PAIRS;  // 42
constexpr int CL_Q_PAIRS = 72;

// ClSharedFetch with the score's operands.  Every lane of the block calls prime() once, then the operator and score() for i0 .. i1 in order.
struct ClSharedScoreFetch {
  const cl_dv2 *plan, *gains, *desired;  // the problem's first knot of each
  const cl_dv2 *q;                       // the state weights of knot 0 of the call
  int q_pairs;                           // pairs between the weights of successive knots: 72, or 0
  ClScoreImage *img;
  int lane, i1;
  cl_dv2 next, nextq0, nextq1;
  __device__ cl_dv2 load(int i) const {
    if (lane < CL_PLAN_PAIRS) return plan[(long)i * 9 + lane];
    if (lane < CL_PAIRS) return gains[(long)i * 26 + 2 + (lane - CL_PLAN_PAIRS)];
    return desired[(long)i * 9 + (lane - CL_PAIRS)];
  }
  __device__ void load_q(int i, cl_dv2 &a, cl_dv2 &b) const {
    const cl_dv2 *src = q + (long)i * q_pairs;
    a = src[lane];
    if (lane < CL_Q_PAIRS - 64) b = src[64 + lane];
  }
  __device__ void store_q(int half, const cl_dv2 &a, const cl_dv2 &b) {
    cl_dv2 *dst = reinterpret_cast<cl_dv2 *>(img->Q[half]);
    dst[lane] = a;
    if (lane < CL_Q_PAIRS - 64) dst[64 + lane] = b;
  }
  // the tables that do not change with the knot: sp (n_shared spheres), and row `b` of the tiled per-problem table (n_own of K spheres)
  __device__ void prime(int i0, const double *sp, int n_shared, const double *own, int K, long b, int n_own) {
    if (lane < CL_SCORE_PAIRS) {
      img->knot[i0 & 1][lane] = load(i0);
      if (i0 + 1 <= i1) next = load(i0 + 1);
    }
    load_q(i0, nextq0, nextq1);
    store_q(i0 & 1, nextq0, nextq1);
    if (q_pairs == 0) store_q((i0 + 1) & 1, nextq0, nextq1);
    else if (i0 + 1 <= i1) load_q(i0 + 1, nextq0, nextq1);
    for (int k = lane; k < n_shared * OB_WORDS; k += CL_BLOCK) img->shared[k] = sp[k];
    for (int k = lane; k < n_own * OB_BWORDS; k += CL_BLOCK) img->own[k] = own[bob_index(b, K, k / OB_BWORDS, k % OB_BWORDS)];
  }
  __device__ void operator()(int i, double pt[18], double K[48]) {
    __syncthreads();
    if (lane < CL_SCORE_PAIRS) {
      if (i + 1 <= i1) img->knot[(i + 1) & 1][lane] = next;
      if (i + 2 <= i1) next = load(i + 2);
    }
    if (q_pairs != 0) {
      if (i + 1 <= i1) store_q((i + 1) & 1, nextq0, nextq1);
      if (i + 2 <= i1) load_q(i + 2, nextq0, nextq1);
    }
    const cl_dv2 *im = img->knot[i & 1];
#pragma unroll
    for (int e = 0; e < CL_PLAN_PAIRS; ++e) {
      const cl_dv2 w = im[e];
      pt[2 * e] = w[0];
      pt[2 * e + 1] = w[1];
    }
#pragma unroll
    for (int e = 0; e < CL_GAIN_PAIRS; ++e) {
      const cl_dv2 w = im[CL_PLAN_PAIRS + e];
      K[2 * e] = w[0];
      K[2 * e + 1] = w[1];
    }
  }
  __device__ ClKnotScore score(int i) const {
    return ClKnotScore{reinterpret_cast<const double *>(&img->knot[i & 1][CL_PAIRS]), img->Q[i & 1]};
  }
};

// k_closed_loop with the two switches; Lim and the grid as there.  WRENCH: e.wrench is given.  SCORE: the score's operands are read and
// e.out_score, when not null, written (a call may ask for the score's side effects on nothing: the host never launches that).
template <int INTEG, bool SHARED, bool WRENCH, bool SCORE, typename... Lim>
__global__ __launch_bounds__(CL_BLOCK) void k_closed_loop_scored(ModelConsts<double> c, ClosedLoopArgs a, ClosedLoopScoreArgs e, Lim... lim) {
  static_assert(WRENCH || SCORE, "without either switch the kernel is k_closed_loop");
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
  ClSampleExtras ex;
  ex.wrench = nullptr;
  ex.wrench_step = 0;
  ex.score = nullptr;
  if constexpr (WRENCH) {
    ex.wrench = e.wrench + row * e.n_w * CL_WRENCH;
    ex.wrench_step = e.n_w == 1 ? 0 : CL_WRENCH;
  }
  int n_own = 0;
  const SphereTables &t = e.ops.spheres;
  if constexpr (SCORE) {
    ex.score = (live && e.out_score) ? e.out_score + row * CL_SCORE : nullptr;
    if (t.own) n_own = t.own_counts[b];
  }
  auto fly = [&](auto &fetch) {
    using F = std::remove_reference_t<decltype(fetch)>;
    if constexpr (MOD) {
      const ModelConsts<double> cm = problem_model(c, pack_get<BatchModels>(lim...), row);
      closed_loop_sample<INTEG, LIM, F, WRENCH, SCORE>(cm, fetch, x0, a.i0, a.i1, out, stats, lo, hi, &ex);
    } else {
      closed_loop_sample<INTEG, LIM, F, WRENCH, SCORE>(c, fetch, x0, a.i0, a.i1, out, stats, lo, hi, &ex);
    }
  };
  if constexpr (SCORE) {
    const double *desired = e.ops.desired + (long)b * e.ops.desired_step;
    if constexpr (SHARED) {
      __shared__ ClScoreImage image;
      ex.spheres = ClSpheres{image.shared, t.n_shared, image.own, n_own, 1, OB_BWORDS};
      ClSharedScoreFetch fetch{reinterpret_cast<const cl_dv2 *>(plan), reinterpret_cast<const cl_dv2 *>(gains), reinterpret_cast<const cl_dv2 *>(desired),
                               reinterpret_cast<const cl_dv2 *>(e.ops.q), e.ops.q_step / 2, &image, lane, a.i1, cl_dv2{0.0, 0.0}, cl_dv2{0.0, 0.0}, cl_dv2{0.0, 0.0}};
      fetch.prime(a.i0, t.shared, t.n_shared, t.own, t.own_K, b, n_own);
      fly(fetch);
    } else {
      ex.spheres = ClSpheres{t.shared, t.n_shared, t.own ? t.own + bob_index(b, t.own_K, 0, 0) : nullptr, n_own, OB_TILE, OB_BWORDS * OB_TILE};
      ClFlatScoreFetch fetch{ClFlatFetch{plan, gains}, desired, e.ops.q, (long)e.ops.q_step};
      fly(fetch);
    }
  } else if constexpr (SHARED) {
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
