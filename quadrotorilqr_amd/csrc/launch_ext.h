// launch_ext.h -- the four-way choice every kernel of the small units (shift.hip, closed_loop.hip, closed_loop_scored.hip) is instantiated
// over: the handle's thrust limits and the per-problem models, each there or not, as trailing kernel arguments.  For those units only:
// ilqr_capi.hip does not include this.
#pragma once

#include "batch_models.h"
#include "box_qp.h"

namespace qilqr {

// go(), go(limits), go(models) or go(limits, models): what is null is left out
template <typename Go>
auto with_extensions(const ControlLimits *limits, const double *d_models, Go &&go) {
  const BatchModels bm{d_models};
  if (limits && d_models) return go(*limits, bm);
  if (limits) return go(*limits);
  if (d_models) return go(bm);
  return go();
}

}  // namespace qilqr
