// backward1_kernel.h -- k_backward<SYM, S> (and k_backward_models<SYM>, the same body for the per-problem models): one wavefront per trajectory -- SYM = false is the GENERAL kernel (non-symmetric weights,
// force_general = 1: the reference's own forms of ilqr.hh:126-133 with Eigen's pivoted LDL^T, backward_layout.h), SYM = true the
// one-wavefront form of the symmetric recursion (force_general = 2, the Runge-Kutta extension).
// Part of the device code of libquadrotor_ilqr.so (gfx950 only); ilqr_kernels.h includes every part.
#pragma once

#include "backward_common.h"
#include "batch_models.h"
#include "box_qp.h"

namespace qilqr {

// arm_line_search (kernels_common.h) for the box form: a QP that failed at any knot ends the problem with QILQR_STATUS_QP_FAILED on
// its current iterate, without a line search.  The same store pattern (every word stored with a selected VALUE, no complementary
// branches: kernels_common.h, store_settled).
__device__ __forceinline__ void arm_line_search_box(const SolveParams &p, const BatchState &st, int b, int iters_now, double cost_now,
                                                    double QuTk, double kTQuuk, bool qp_failed) {
  st.prev_cost[b] = cost_now;
  const bool conv = !qp_failed && iters_now > 0 && is_converged(p, cost_now, cost_now + cost_reduction(QuTk, kTQuuk, 1.0));
  const bool none = !qp_failed && !conv && iters_now > 0 && p.ls_max_iters <= 0;
  const bool search = !(qp_failed || conv || none);
  st.alpha[b] = 1.0;
  st.trial[b] = 0;
  if (!search) st.status[b] = qp_failed ? 4 : (conv ? 0 : 3);  // 4: QILQR_STATUS_QP_FAILED
  st.flags[b] = search ? (F_ACTIVE | F_SEARCH) : 0;
}

// SYM = true: Q and R are exactly symmetric, so V_xx and H are symmetric to rounding and the
// accumulator tile can be reused as the next knot's A operand without a transpose; no LDS and no
// barrier remain in the loop (Q_uu/Q_u are broadcast with DPP row broadcasts, the right-hand sides with
// ds_bpermute).  SYM = false: general weights, hand-offs go through padded LDS tiles.
// Lim = ControlLimits (SYM = true, S = double only): the box form of the symmetric recursion for the per-rotor thrust limits
// (qilqr_set_control_limits): box QP per knot (box_qp.h), the full value updates, status QILQR_STATUS_QP_FAILED.
// k_backward_models (below, fp64, either SYM, with or without ControlLimits): the per-problem models (qilqr_set_batch_models): the
// constant rows of J_u come from the block's own problem's record (batch_models.h) instead of the shared constant table.
// Without limits (an empty pack) k_backward takes exactly the arguments it always took; the models reach only k_backward_models.
template <bool SYM, typename S, typename... Lim>
__global__ __launch_bounds__(64) void k_backward(ModelConsts<double> c, SolveParams p, BatchState st,
                                                 int B, int n, int force, Lim... lim) {
  constexpr bool BOX = pack_has<ControlLimits, Lim...>;
  constexpr bool MOD = false;
  static_assert(!BOX || (SYM && std::is_same<S, double>::value), "the box form is the symmetric fp64 recursion");
#define BW1_EXT lim...
#include "backward1_body.inc"
#undef BW1_EXT
}

// the per-problem models extension (fp64): the same body with the table (and, Lim = ControlLimits, the box form).  A kernel of its own
// name: every pre-existing instantiation of k_backward stays what it was.
template <bool SYM, typename... Lim>
__global__ __launch_bounds__(64) void k_backward_models(ModelConsts<double> c, SolveParams p, BatchState st,
                                                        int B, int n, int force, BatchModels models, Lim... lim) {
  typedef double S;
  constexpr bool BOX = pack_has<ControlLimits, Lim...>;
  constexpr bool MOD = true;
  static_assert(!BOX || SYM, "the box form is the symmetric fp64 recursion");
#define BW1_EXT models, lim...
#include "backward1_body.inc"
#undef BW1_EXT
}

}  // namespace qilqr
