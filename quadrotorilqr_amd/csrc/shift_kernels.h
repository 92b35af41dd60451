// shift_kernels.h -- k_shift: the step between two solves of a receding horizon (qilqr_shift_batch[_device]).  Problem by problem, on
// plain [B][n][18] arrays of the caller:
//   out[b, i]  = in[b, i + steps]                                   i < n - steps      (kept knots: all 18 words, bit for bit)
//   out[b, j]  = one dynamics step from out[b, j - 1] under the     j >= n - steps     (the tail; out[b, n - 1 - steps] = in[b, n - 1])
//                control stored there; its own control is the tail
//                control (held or hover, clamped with limits); its
//                time is in[b, n - 1, 0] + (j - (n - 1 - steps)) dt
//   out[b, 0, 1..13] = x0[b]                                        with x0             (re-anchoring; time and control of knot 0 stay)
// The step is rollout_problem's (se3_math.h): body_acceleration_fast / se3_rplus_fast, or rk4_step for the Runge-Kutta extension, with the
// problem's own model while per-problem models are set.  No cost is evaluated.
//
// ONE launch, two kinds of block, both reading only the input (the host refuses overlapping arrays):
//   tail blocks (the first cdiv(B, 64)): a lane per problem rolls the tail, and writes knot 0's state pairs when x0 is given
//   copy blocks: a 16-byte pair per thread; a knot is nine pairs, the kept pairs of a problem are contiguous in both arrays and
//                consecutive threads take consecutive pairs (rows coalesce)
// Every output word has exactly one writer: x0 does not fall on pair boundaries (words 0 | 1 share a pair), so with x0 the seven pairs that
// hold words 0..13 of knot 0 belong to the problem's tail lane (which copies word 0) and no copy thread touches them.
// Part of shift.hip's translation unit (gfx950 only); the per-problem routines are QILQR_HD and compile under g++ (tests/host_shift_harness.cpp).
#pragma once

#include "batch_models.h"
#include "box_qp.h"
#include "se3_math.h"

// (as in se3_math.h: a * b + c fuses where the source says so and nowhere else, so that the step has rollout_problem's bits)
#if defined(__clang__)
#pragma clang fp contract(on)
#endif

namespace qilqr {

constexpr int SHIFT_BLOCK = 64;        // threads of either kind of block
constexpr int SHIFT_STATE = 13;        // words 1..13 of a knot: t(3), q w,x,y,z, v_lin(3), v_ang(3)
constexpr int SHIFT_STATE_PAIRS = 7;   // the pairs of a knot that hold words 0..13
constexpr int SHIFT_TAIL_HOLD = 0, SHIFT_TAIL_HOVER = 1;

struct ShiftArgs {
  const double *in;   // [B][n][18]
  const double *x0;   // [B][13], or null
  double *out;        // [B][n][18]
  int B, n, steps, tail;
  int tail_blocks;    // blocks of the launch that roll tails (0: steps = 0 and no x0)
};

// two consecutive words, 16-byte aligned (a knot is 144 bytes and the arrays are 16-byte aligned): one store on the device
QILQR_HD void shift_store_pair(double *p, double a, double b) {
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

// pairs the copy blocks move
QILQR_HD long shift_copy_pairs(const ShiftArgs &a) { return (long)a.B * (a.n - a.steps) * 9; }

// copy pair g of the launch (0 <= g < shift_copy_pairs): pair r of problem b's kept knots
QILQR_HD void shift_copy_pair(const ShiftArgs &a, long g) {
  const long kept = (long)(a.n - a.steps) * 9;
  const long b = g / kept, r = g - b * kept;
  if (a.x0 && r < SHIFT_STATE_PAIRS) return;  // knot 0's state pairs: the tail lane's
  const long dst = (b * a.n * 9 + r) * 2, src = dst + (long)a.steps * 18;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef double dv2 __attribute__((ext_vector_type(2)));
  *reinterpret_cast<dv2 *>(a.out + dst) = *reinterpret_cast<const dv2 *>(a.in + src);
#else
  a.out[dst] = a.in[src];
  a.out[dst + 1] = a.in[src + 1];
#endif
}

// The tail of one problem, and knot 0's state pairs with x0: in / out point at the problem's first knot, x0 at its 13 words (or null).
// c: the problem's model.  LIM: the tail control is clamped to [lo, hi] (the control stored at in[n - 1] is stepped with as given).
template <int INTEG, bool LIM>
QILQR_HD void shift_tail_problem(const ModelConsts<double> &c, const double *in, const double *x0, double *out, int n, int steps, int tail,
                                 const double *lo = nullptr, const double *hi = nullptr) {
  if (x0) {
    shift_store_pair(out, in[(long)steps * 18], x0[0]);
#pragma unroll
    for (int e = 1; e < SHIFT_STATE_PAIRS; ++e) shift_store_pair(out + 2 * e, x0[2 * e - 1], x0[2 * e]);
  }
  if (steps <= 0) return;
  const double *last = in + (long)(n - 1) * 18;
  double t[3] = {last[1], last[2], last[3]};
  double q[4] = {last[5], last[6], last[7], last[4]};
  double v[6], u[4], ut[4];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[a] = last[8 + a];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    u[a] = last[14 + a];  // the control stored at output knot n - 1 - steps
    ut[a] = tail == SHIFT_TAIL_HOVER ? c.mass * c.g / 4 : u[a];
    if (LIM) ut[a] = box_clamp(ut[a], lo[a], hi[a]);
  }
  const double time0 = last[0];
  RolloutSeries<double> sr;  // series coefficients in registers for the whole loop, as rollout_problem holds them
  if (INTEG == 0) sr.load();
  double *o = out + (long)(n - steps) * 18;
  for (int k = 1; k <= steps; ++k, o += 18) {
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
#pragma unroll
    for (int a = 0; a < 4; ++a) u[a] = ut[a];  // every tail knot stores, and is stepped from with, the tail control
    const double w[18] = {time0 + (double)k * c.dt, t[0], t[1], t[2], q[3], q[0], q[1], q[2], v[0], v[1], v[2], v[3], v[4], v[5],
                          u[0], u[1], u[2], u[3]};
#pragma unroll
    for (int e = 0; e < 9; ++e) shift_store_pair(o + 2 * e, w[2 * e], w[2 * e + 1]);
  }
}

#if defined(__HIPCC__)
// Lim = ControlLimits: the tail control clamped to the box.  Lim = BatchModels: each lane steps with its problem's model.  Either, both
// (ControlLimits first), or neither, as k_rollout takes them.
template <int INTEG, typename... Lim>
__global__ __launch_bounds__(SHIFT_BLOCK) void k_shift(ModelConsts<double> c, ShiftArgs a, Lim... lim) {
  constexpr bool LIM = pack_has<ControlLimits, Lim...>;
  constexpr bool MOD = pack_has<BatchModels, Lim...>;
  if ((int)blockIdx.x >= a.tail_blocks) {
    const long g = (long)((int)blockIdx.x - a.tail_blocks) * SHIFT_BLOCK + threadIdx.x;
    if (g < shift_copy_pairs(a)) shift_copy_pair(a, g);
    return;
  }
  const int b = blockIdx.x * SHIFT_BLOCK + threadIdx.x;
  if (b >= a.B) return;
  const double *in = a.in + (long)b * a.n * 18;
  double *out = a.out + (long)b * a.n * 18;
  const double *x0 = a.x0 ? a.x0 + (long)b * SHIFT_STATE : nullptr;
  const double *lo = nullptr, *hi = nullptr;
  if constexpr (LIM) {
    const ControlLimits &L = pack_get<ControlLimits>(lim...);
    lo = L.lo;
    hi = L.hi;
  }
  if constexpr (MOD) {
    const ModelConsts<double> cm = problem_model(c, pack_get<BatchModels>(lim...), (long)b);
    shift_tail_problem<INTEG, LIM>(cm, in, x0, out, a.n, a.steps, a.tail, lo, hi);
  } else {
    shift_tail_problem<INTEG, LIM>(c, in, x0, out, a.n, a.steps, a.tail, lo, hi);
  }
}
#endif

}  // namespace qilqr

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
