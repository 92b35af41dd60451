// Host build of quadrotorilqr_amd/csrc/route.h and schedule.h for tests/test_schedule_cpu.py: the route of a handle with a state-weight
// schedule (RouteInputs::scheduled), the k_linearize key it takes, and the setter's check of a schedule.  Test scaffolding only.
#include "../quadrotorilqr_amd/csrc/route.h"
#include "../quadrotorilqr_amd/csrc/schedule.h"

using namespace qilqr;

// in: {symmetric, layout_kind, q_diag, integrator, limited, modeled, obstacles, problem_obstacles, force_general, persistent, compaction,
//      streams, single_wave_rollout, round_launch, B, scheduled}
// out: {backward (BW_ONE = 2), tiled, combined, fuse_kinds, round_kernel, late_tail, persistent, lin_kind, k_linearize key, key admitted,
//       rollout (RO_LANE = 0, RO_16 = 1, RO_THREE = 2, RO_THREE_THEN_16 = 3), compact, parts}
extern "C" int hs_route(const long *in, long *out) {
  RouteInputs ri;
  ri.symmetric = in[0];
  ri.layout_kind = (int)in[1];
  ri.q_diag = in[2];
  ri.integrator = (int)in[3];
  ri.limited = in[4];
  ri.modeled = in[5];
  ri.obstacles = in[6] || in[7];
  ri.problem_obstacles = in[7];
  ri.dev.force_general = (int)in[8];
  ri.dev.persistent = (int)in[9];
  ri.dev.compaction = (int)in[10];
  ri.dev.streams = (int)in[11];
  ri.dev.single_wave_rollout = (int)in[12];
  ri.dev.round_launch = (int)in[13];
  ri.dev.sync_every = 2;
  ri.scheduled = in[15];
  const Route r = plan_route(ri, in[14], CallFacts{});
  const ExtArgs &x = r.linearize_ext;
  const int ext = (x.models ? LIN_MODELS : LIN_PLAIN) | (x.obstacles ? LIN_OBSTACLES : LIN_PLAIN) | (x.problem_obstacles ? LIN_PROBLEM : LIN_PLAIN);
  const int key = lin_key(r.lin_kind, r.integrator, r.tiled, r.f32, ext);
  long *o = out;
  *o++ = r.backward;
  *o++ = r.tiled;
  *o++ = r.combined;
  *o++ = r.fuse_kinds;
  *o++ = r.round_kernel;
  *o++ = r.late_tail;
  *o++ = r.persistent;
  *o++ = r.lin_kind;
  *o++ = key;
  *o++ = key >= 0 && key < LIN_KEYS && lin_instantiated(key);
  *o++ = r.rollout == RO_LANE ? 0 : r.rollout == RO_16 ? 1 : r.rollout == RO_THREE ? 2 : 3;
  *o++ = r.compact;
  *o++ = r.parts;
  return (int)(o - out);
}

// sched_check: 0 and *symmetric, or 1 with the first bad (knot, row, column) in where[3] (-1 each when the fault is not an entry's)
extern "C" int hs_check(const double *Qs, long n_knots, int *symmetric, long *where) {
  SchedCheck e;
  const int rc = sched_check(Qs, n_knots, &e);
  *symmetric = e.symmetric ? 1 : 0;
  where[0] = e.knot;
  where[1] = e.row;
  where[2] = e.col;
  return rc;
}
