// Host build of quadrotorilqr_amd/csrc/route.h for tests/test_route_cpu.py: one row of tests/golden/routes.json's inputs in, the
// route's choices out, in the table's encoding; and the keys of the k_linearize instantiations the rule admits (hr_lin_keys), for
// tests/golden/linearize_keys.json; and the k_round instantiation of a launch (hr_round_form), for tests/test_round_cases_cpu.py.  Test
// scaffolding only.
#include "../quadrotorilqr_amd/csrc/route.h"

using namespace qilqr;

namespace {
long backward_code(const Route &r, long live) {
  switch (backward_now(r, live)) {
    case BW_ONE: return 0;
    case BW_FUSED: return 1;
    case BW_TWO: return 5;
    default: return gradient_factors(r, live) ? 2 : r.many ? 3 : 4;
  }
}
long ext_bits(const ExtArgs &x) { return (x.limits ? 1 : 0) | (x.models ? 2 : 0) | (x.obstacles ? 4 : 0); }
}  // namespace

extern "C" int hr_route(const long *in, long *out) {
  RouteInputs ri;
  const long fg = in[9];
  ri.symmetric = in[0] && fg != 1;                    // (qilqr_create: force_general = 1 takes the general forms)
  const bool q_sym = in[1] && fg != 1, ur_zero = in[2];
  ri.layout_kind = !q_sym ? 0 : (ur_zero ? 2 : 1);   // (se3_math.h, layout_kind)
  ri.q_diag = in[3];
  ri.f32 = in[4];
  ri.integrator = (int)in[5];
  ri.limited = in[6];
  ri.modeled = in[7];
  ri.obstacles = in[8];
  ri.dev.force_general = (int)fg;
  ri.dev.single_wave_rollout = (int)in[10];
  ri.dev.round_launch = (int)in[11];
  ri.dev.compaction = (int)in[12];
  ri.dev.streams = (int)in[13];
  ri.dev.persistent = (int)in[14];
  ri.dev.rounds_per_launch = (int)in[15];
  ri.dev.sync_every = (int)in[16];
  const long B = in[17];
  ri.hw_queues = (int)in[18];
  ri.num_cus = 256;
  CallFacts call;
  call.sync_every = (int)in[16];
  call.desired_batch = in[19];
  call.cost_hist = in[20];
  call.early_out = in[21];
  call.iterates = in[22];
  const Route r = plan_route(ri, B, call);
  const TailFuse tf = tail_fuse(r, r.compact, r.parts);
  long *o = out;
  *o++ = r.persistent;
  *o++ = r.tiled;
  *o++ = r.backward;
  *o++ = r.backward == BW_ONE ? ext_bits(r.backward_ext) : 0;
  *o++ = r.rollout == RO_LANE ? 0 : r.rollout == RO_16 ? 1 : r.rollout == RO_THREE ? 2 : 3;
  *o++ = r.rollout == RO_LANE ? ext_bits(r.rollout_ext) : 0;
  *o++ = r.lin_kind;
  *o++ = ext_bits(r.linearize_ext);
  *o++ = r.tiled;
  *o++ = r.fuse_kinds;
  *o++ = r.combined;
  *o++ = r.round_kernel;
  *o++ = r.rounds_per_launch;
  *o++ = r.late_tail;
  *o++ = r.late_from;
  *o++ = r.parts;
  *o++ = r.compact;
  *o++ = tf.kinds;
  *o++ = tf.slots;
  *o++ = tf.stop;
  *o++ = tf.from;
  for (long live : {B, 1L, 3071L, 3072L}) *o++ = backward_code(r, live);
  *o++ = (r.round_kernel && (r.fuse_kinds || r.late_tail)) ? r.lin_kind : -1;
  for (long seen : {B, std::max(1L, B / 8)}) {
    *o++ = round_form(r, false, true, (unsigned)seen, B).six;
    *o++ = round_form(r, true, true, (unsigned)seen, B).six;
    *o++ = round_form(r, true, false, (unsigned)seen, B).six;
  }
  return (int)(o - out);
}

// The k_linearize key and the backward kernel of a stand-alone pass or a batch solve of B problems, from the RouteInputs a handle makes of
// itself (tests/linearize_cases.py restates host/api_handle.h), `scheduled` and `problem_obstacles` among them.
// in:  {symmetric, q_diag, layout_kind, f32, integrator, limited, modeled, obstacles, problem_obstacles, scheduled, force_general, B}
// out: {lin_kind, integrator, tiled, f32, ext, backward kind (route.h, BackwardKind), admitted by lin_instantiated}
extern "C" int hr_lin_route(const long *in, long *out) {
  RouteInputs ri;
  ri.symmetric = in[0];
  ri.q_diag = in[1];
  ri.layout_kind = (int)in[2];
  ri.f32 = in[3];
  ri.integrator = (int)in[4];
  ri.limited = in[5];
  ri.modeled = in[6];
  ri.obstacles = in[7];
  ri.problem_obstacles = in[8];
  ri.scheduled = in[9];
  ri.dev.force_general = (int)in[10];
  ri.dev.sync_every = 2;
  const Route r = plan_route(ri, in[11], CallFacts{});
  const ExtArgs &x = r.linearize_ext;
  const int ext = (x.models ? LIN_MODELS : LIN_PLAIN) | (x.obstacles ? LIN_OBSTACLES : LIN_PLAIN) | (x.problem_obstacles ? LIN_PROBLEM : LIN_PLAIN);
  long *o = out;
  *o++ = r.lin_kind;
  *o++ = r.integrator;
  *o++ = r.tiled;
  *o++ = r.f32;
  *o++ = ext;
  *o++ = r.backward;
  *o++ = lin_instantiated(lin_key(r.lin_kind, r.integrator, r.tiled, r.f32, ext));
  return (int)(o - out);
}

// The k_round instantiation of one launch of a solve's single-stream rounds (host/batch_solve.h, run_solve), from the RouteInputs a handle
// makes of itself (tests/round_cases.py, predicates) and what the host knows when it enqueues the launch: plan_route, then
// round_form with forced = true, then the rules by which launch_round picks among the instantiations (round_lk, round_instance) and the slot
// it counts the launch in (round_slot).
// in:  {symmetric, q_diag, layout_kind, force_general, round_launch, rounds_per_launch, B, desired_batch, cost_hist, early_out,
//       several (the launches may hold several rounds), seen_active (the last count of running trajectories the host has read), used (slots)}
// out: {the rounds are k_round launches (the combined launch, no compaction), LK, ROUNDS, SIX, slot in qilqr_round_launches' counts}
extern "C" int hr_round_form(const long *in, long *out) {
  RouteInputs ri;
  ri.symmetric = in[0];
  ri.q_diag = in[1];
  ri.layout_kind = (int)in[2];
  ri.dev.force_general = (int)in[3];
  ri.dev.round_launch = (int)in[4];
  ri.dev.rounds_per_launch = (int)in[5];
  ri.dev.sync_every = 2;
  CallFacts call;
  call.desired_batch = in[7];
  call.cost_hist = in[8];
  call.early_out = in[9];
  const Route r = plan_route(ri, in[6], call);
  const RoundForm f = round_instance(round_form(r, in[10] != 0, /*forced=*/true, (unsigned)in[11], in[12]));
  const int lk = round_lk(r);
  long *o = out;
  *o++ = r.combined && !r.compact && r.round_kernel;
  *o++ = lk;
  *o++ = f.rounds;
  *o++ = f.six;
  *o++ = round_slot(lk, f.rounds, f.six);
  return (int)(o - out);
}

// Every key of the key space that lin_instantiated admits, as rows of {lin_kind, integrator, tiled, f32, ext} in key order; returns the
// number of rows (cap rows are written), or -1 when the rule by key and the rule by fields disagree or a key leaves the key space.
extern "C" int hr_lin_keys(long *out, int cap) {
  int rows = 0;
  for (int ext = 0; ext < 8; ++ext)
    for (int f32 = 0; f32 < 2; ++f32)
      for (int tiled = 0; tiled < 2; ++tiled)
        for (int integ = 0; integ < 2; ++integ)
          for (int lk = 0; lk < 4; ++lk) {
            const int key = lin_key(lk, integ, tiled != 0, f32 != 0, ext);
            if (key < 0 || key >= LIN_KEYS || lin_instantiated(key) != lin_instantiated(lk, integ, tiled != 0, f32 != 0, ext)) return -1;
            if (!lin_instantiated(key)) continue;
            if (rows < cap) {
              const long row[5] = {lk, integ, tiled, f32, ext};
              for (int q = 0; q < 5; ++q) out[5 * rows + q] = row[q];
            }
            ++rows;
          }
  return rows;
}
