// mppi_adapt_launch.h -- what mppi_adapt.hip gives the rest of the library: the launches of k_mppi_flight_spread and k_mppi_adapt
// (mppi_adapt_kernels.h) for qilqr_mppi_flight_spread_device and qilqr_mppi_adapt_device, and the rule of what those calls refuse.
// Declarations and host code only, as mppi_launch.h; hidden: not part of the C ABI.  The rule compiles under g++
// (tests/host_mppi_adapt_harness.cpp).  The grids are mppi_launch.h's: the flight's of k_mppi_flight, the adaptation's of k_mppi_update.
#pragma once

#include "mppi_launch.h"

namespace qilqr {

// ---- the refusals.  ONE rule for both calls; base.update says which (the adaptation is the update's call with a spread).  THE ORDER:
// mppi_refusal's rows 1 .. 11 on the common arguments, with its texts; then
//   a  a NULL d_spread, or for the adaptation a NULL adapt rule
//   b  a floor that is NaN or negative
//   c  a cap that is NaN, infinite or below its floor
//   d  a rate not in (0, 1]
//   e  a nonzero reserved word of the adapt rule
//   f  d_spread or d_out_spread off a 16-byte boundary
//   g  d_out_spread overlapping an input (d_spread among them: not in place), d_out_plan or d_info
//   h  the flight's d_score, or the adaptation's d_out_plan or d_info, overlapping d_spread
// then mppi_refusal's row 12 and what it says of the handle.  (b .. e look at the adapt rule and so only at the adaptation.)
struct MppiSpreadCall {
  MppiCall base;                 // base.update: qilqr_mppi_adapt_device (else qilqr_mppi_flight_spread_device)
  bool adapt;                    // there is an adapt rule (the four fields below are its)
  double floor[4], cap[4], rate, reserved[3];
  const void *spread, *out_spread;  // out_spread may be null: the mean only
};
inline const char *mppi_spread_refusal(const MppiSpreadCall &c, bool *length) {
  // the common arguments first, before any handle is looked at: a handle that admits everything stands in for the caller's
  MppiCall args = c.base;
  args.handle = true;
  args.f32 = args.modeled = false;
  args.pobs_B = args.n_sched = args.k0 = 0;
  args.n_desired = args.n + 1;
  if (const char *why = mppi_refusal(args, length)) return why;
  const bool adapt = c.base.update;
  if (!c.spread) return "mppi: null argument (d_spread is needed)";
  if (adapt && !c.adapt) return "mppi: null argument (the adapt rule is needed)";
  if (adapt) {
    for (int a = 0; a < 4; ++a)
      if (!(c.floor[a] >= 0.0)) return "mppi: every floor must be a number and not negative";
    for (int a = 0; a < 4; ++a)
      if (!std::isfinite(c.cap[a]) || !(c.cap[a] >= c.floor[a])) return "mppi: every cap must be finite and not below its floor";
    if (!(c.rate > 0.0 && c.rate <= 1.0)) return "mppi: rate must lie in (0, 1]";
    for (int k = 0; k < 3; ++k)
      if (c.reserved[k] != 0.0) return "mppi: the adapt rule's reserved words must be 0";
  }
  if (off_16_bytes({c.spread}) || (adapt && off_16_bytes({c.out_spread}))) return "mppi: d_spread and d_out_spread must be 16-byte aligned";
  const MppiCall &m = c.base;
  const size_t knots = sizeof(double) * 18 * (size_t)m.B * (size_t)m.n, states = sizeof(double) * 13 * (size_t)m.B,
               scores = sizeof(double) * 4 * (size_t)m.B * (size_t)m.S, infos = sizeof(double) * 8 * (size_t)m.B,
               spreads = sizeof(double) * 4 * (size_t)m.B * (size_t)m.n;
  if (adapt && c.out_spread) {
    const struct { const void *p; size_t bytes; } other[7] = {{m.plan, knots}, {m.x0, states}, {m.desired, knots}, {m.score, scores},
                                                              {c.spread, spreads}, {m.out_plan, knots}, {m.info, infos}};
    for (int k = 0; k < 7; ++k)
      if (ranges_overlap(c.out_spread, spreads, other[k].p, other[k].bytes))
        return k < 5 ? "mppi: d_out_spread overlaps an input (the adaptation does not work in place)" : "mppi: d_out_spread overlaps d_out_plan or d_info";
  }
  if (!adapt && ranges_overlap(m.score, scores, c.spread, spreads)) return "mppi: d_score overlaps d_spread";
  if (adapt && (ranges_overlap(m.out_plan, knots, c.spread, spreads) || ranges_overlap(m.info, infos, c.spread, spreads)))
    return "mppi: d_out_plan or d_info overlaps d_spread";
  return mppi_refusal(c.base, length);  // (its rows 1 .. 11 have passed: the handle's remain)
}

}  // namespace qilqr

#if defined(__HIPCC__)
namespace qilqr {

// one call's launch record: MppiLaunch (base.rule.sigma is not read: the draws are the unit recursion's) and the spread
struct MppiSpreadLaunch {
  MppiLaunch base;
  const double *d_spread;       // [B][n][4]
  double *d_out_spread;         // [B][n][4], or null (the adaptation)
  qilqr_mppi_adapt_rule adapt;  // the caller's (the adaptation)
};

// each enqueues its launches on `stream` and returns what they returned; nothing is waited for.  The adaptation is two launches:
// k_mppi_adapt, then mppi.hip's nominal flight over d_out_plan (launch_mppi_nominal_flight).
__attribute__((visibility("hidden"))) hipError_t launch_mppi_flight_spread(hipStream_t stream, const ModelConsts<double> &consts, const MppiSpreadLaunch &call);
__attribute__((visibility("hidden"))) hipError_t launch_mppi_adapt(hipStream_t stream, const ModelConsts<double> &consts, const MppiSpreadLaunch &call);

}  // namespace qilqr
#endif
