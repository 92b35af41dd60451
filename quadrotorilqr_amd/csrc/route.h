// route.h -- which kernels a call of B problems on a handle takes: ONE pure decision from the handle's inputs and the call's own facts
// (plan_route), the helpers for the choices that depend on counts the host learns while the call runs, and the rule that says which
// k_linearize instantiations exist (lin_instantiated).  The host side plans the route once per call (begin_batch, host/launches.h) and
// its launch helpers read it; launch_linearize instantiates exactly the keys the rule admits; qilqr_describe renders the route.  Host code
// only, no HIP: tests/test_route_cpu.py builds it with g++ and checks it against a table of the choices and a list of the admitted keys.
#pragma once

#include <algorithm>

#include "../../include/quadrotor_ilqr.h"

namespace qilqr {

inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

#ifndef QILQR_REGIME_B
#define QILQR_REGIME_B 4096
#endif
constexpr long REGIME_B = QILQR_REGIME_B;  // calls with more trajectories in flight take the kernels built for a full chip
constexpr long R16_MAX_B = REGIME_B;  // k_rollout16 for every rollout up to this many trajectories (launch_rollout)
#ifndef QILQR_ROLLOUT16_FROM
#define QILQR_ROLLOUT16_FROM 16
#endif
constexpr long ROLLOUT16_FROM = QILQR_ROLLOUT16_FROM;
constexpr int MAX_PARTS = 8;  // sub-batch streams of a handle

// Which backward kernel a call with `load_B` trajectories in flight takes (symmetric weights), by how many trajectories share
// the chip's 1024 SIMDs:
//   up to 4096: k_backward4<.., FUSED>: four wavefronts that each carry the matrix AND the gradient recursion of a trajectory,
//               and one loader wavefront, per four trajectories (the wavefronts are bound by latencies, the gradient's 40
//               instructions ride along: +0.3 to +1.7 % of a whole solve against the form below, profiles/r03_ab_backward.txt)
//   beyond:     k_backward4: four matrix wavefronts, ONE gradient wavefront and the loader per four trajectories, knot loop
//               unrolled (four blocks per CU: the SIMDs are bound by what their wavefronts issue, and one gradient wavefront
//               for four trajectories issues a quarter: 426k against 408k solves/s at 8192)
// Until round 4 the one-wavefront kernel (k_backward<true>) took over above 8192 trajectories: a block per trajectory wastes
// nothing on finished neighbours.  With the live trajectories compacted (k_compact_*) the blocks of four are full, and the
// six-wavefront form is ahead at every size measured (profiles/r04_compaction.txt: 12288: 554k against 464k solves/s,
// 16384: 593k / 512k, 65536: 654k / 587k); the one-wavefront kernel stays for force_general = 2.
// k_backward2 (a matrix and a gradient wavefront per trajectory) was the choice below 512 trajectories in rounds 1 and 2; it
// wins nowhere by more than 2 % and lives in the diagnostics build (force_general = 3 there).
// The Runge-Kutta extension, the thrust limits, the per-problem models, non-symmetric weights and a state-weight schedule take the
// one-wavefront kernel at every size.
#ifndef QILQR_GFAC_MIN_LIVE
#define QILQR_GFAC_MIN_LIVE 3072
#endif
constexpr long GFAC_MIN_LIVE = QILQR_GFAC_MIN_LIVE;  // running trajectories from which the gradient wavefront factors Q_uu (launch_backward)
enum BackwardKind { BW_FOUR, BW_TWO, BW_ONE, BW_FUSED };

// Which rollout kernel, by how many trajectories share the chip (qilqr_device_config.single_wave_rollout):
//   k_rollout16  sixteen lanes per trajectory, four trajectories per block: the shortest chain per trajectory and a
//                block on every CU from 1024 trajectories on; up to R16_MAX_B trajectories
//   k_rollout3   a lane per trajectory, three cooperating wavefronts per 64 trajectories: beyond
//   k_rollout    a lane per trajectory, one wavefront (the Runge-Kutta extension; forced).  It was the choice above 16384
//                trajectories until the live trajectories were compacted: with full wavefronts k_rollout3 is ahead there too
//                (65536: 698k against 655k solves/s, 16384: 596k / 543k, profiles/r04_compaction.txt)
// RO_THREE_THEN_16: k_rollout3 for a trajectory's first ROLLOUT16_FROM rollouts, k_rollout16 from there on (rollout16_now)
enum RolloutRule { RO_LANE, RO_16, RO_THREE, RO_THREE_THEN_16 };

// ---- compaction of the live trajectories (bookkeeping_kernels.h, k_compact_plan): between a round's backward pass and its rollout.
// Worth its two launches while the live trajectories fill more blocks than the device runs side by side; below
// COMPACT_STOP running trajectories every kernel of a round is a lone dependent chain whatever the slots are.
#ifndef QILQR_COMPACT_STOP
#define QILQR_COMPACT_STOP 512
#endif
constexpr unsigned COMPACT_STOP = QILQR_COMPACT_STOP;
#ifndef QILQR_LATE_TAIL
#define QILQR_LATE_TAIL 1  // (0: batches beyond 4096 keep three launches per round to the end -- A/B)
#endif

// What of a handle the choice reads
struct RouteInputs {
  bool symmetric = false;  // Q == Q^T and R == R^T exactly (and force_general != 1)
  bool q_diag = false;     // Q exactly diagonal (and dense_weights == 0)
  int layout_kind = 0;     // layout_kind(RecLayout) of the knot records: 0 dense, 1 symmetric, 2 symmetric with a zero upper-right block
  bool f32 = false;        // the mixed-precision mode
  int integrator = 0;      // 0 explicit Euler, 1 Runge-Kutta
  bool limited = false, modeled = false, obstacles = false;  // the extensions set on the handle (models: as the call sees them)
  qilqr_device_config dev{};  // force_general, single_wave_rollout, streams, persistent, compaction, round_launch, rounds_per_launch
  int num_cus = 256;
  int hw_queues = 4;  // hardware queues of the process (GPU_MAX_HW_QUEUES as the runtime read it)
  bool problem_obstacles = false;  // per-problem spheres (qilqr_set_batch_obstacles): `obstacles` is set beside it, k_linearize takes their form
  // a state-weight schedule is set (qilqr_set_state_weight_schedule): the route of non-symmetric weights -- dense records of kind 0, in which
  // all of C_xx travels, and the one-wavefront backward kernel, which reads no constant derived from Q -- whatever the handle's Q is;
  // `symmetric` then says whether R and every Q_i are (k_backward<true> or the general kernel)
  bool scheduled = false;
};
// What of the call itself the choice reads
struct CallFacts {
  int sync_every = 2;          // qilqr_device_config.sync_every
  bool desired_batch = false;  // per-problem desired trajectories
  bool cost_hist = false;      // the per-iteration cost history is recorded (options.populate_debug)
  bool early_out = false;      // the copy-back under the tail of qilqr_solve_batch
  bool iterates = true;        // max_iters > 0
};
// the extension arguments a kernel family receives
struct ExtArgs {
  bool limits = false, models = false, obstacles = false;
  bool problem_obstacles = false;  // (k_linearize) the form that carries the per-problem spheres beside the shared ones
};

struct Route {
  long B = 0;                  // trajectories in flight in the call: every choice below goes by it
  bool symmetric = false, f32 = false;
  int integrator = 0;
  int force_general = 0;
  bool persistent = false;     // the one-launch solve, k_solve4
  bool tiled = false;          // the knot records are placed for the kernels that stage them through LDS
  BackwardKind backward = BW_ONE;
  bool many = false;           // k_backward4's register budget and unrolled knot loop for four blocks per CU
  RolloutRule rollout = RO_LANE;
  int lin_kind = 0;            // record kind of k_linearize and k_round: layout_kind, or 3 for a diagonal Q (fp64, Euler)
  ExtArgs backward_ext, rollout_ext, linearize_ext;
  bool fuse_kinds = false;     // the round's kernels are the two the combined launch stands for
  bool combined = false;       // ... and every block of four has a CU to itself: k_backward_rollout (or k_round)
  bool round_kernel = false;   // the combined launch may be k_round
  int rounds_per_launch = 4;
  bool late_tail = false;      // a batch beyond REGIME_B changes over to the combined launch in its tail
  long late_from = 0;          // ... from this round on
  int parts = 1;               // sub-batch streams
  bool compact = false;        // the compaction of the running trajectories may run (a batch solve turns it on)
  int compaction = 0;          // qilqr_device_config.compaction
  int num_cus = 256;
};

inline BackwardKind backward_kind(const RouteInputs &in, long load_B) {
  const int fg = in.dev.force_general;
  if (in.integrator == 1 || !in.symmetric || in.limited || in.modeled || in.scheduled) return BW_ONE;
#ifdef QILQR_WITH_BACKWARD2
  if (fg == 3) return BW_TWO;
#endif
  if (fg == 5 || (fg == 0 && load_B <= REGIME_B)) return BW_FUSED;
  if (fg != 2) return BW_FOUR;
  return BW_ONE;
}

inline int auto_parts(const RouteInputs &in, long B) {
  const long tiles = (B + 63) / 64;
  // Measured (MI355X, N = 100): up to a few thousand trajectories every kernel is latency-bound and sharing
  // SIMDs with another part's kernels only slows both (B = 1024, round 3: 194k solves/s on one stream, 168k on two,
  // 153k on four); from 4096 on two parts gain 4-5%.  Between 4096 and 16384 FOUR parts are better still when
  // every part's stream has a hardware queue of its own -- GPU_MAX_HW_QUEUES=8 in the environment before the runtime
  // starts: 5120: 366k against 356k solves/s, 6144: 403k / 377k, 7168: 437k / 406k,
  // 8192: 461k / 429k, 10240: 441k / 424k, 12288: 472k / 460k; level at 4096, 16384 and 65536; with HIP's default four queues
  // the parts collide with each other and with the caller's streams and two are the safer choice.
  // Round 4 (compaction, k_backward4 and k_rollout3 at every size beyond 4096): four parts are ahead at 16384 and 65536 as well
  // (596k against 591k, 698k against 686k).
  int want = in.dev.streams > 0 ? in.dev.streams : (B >= REGIME_B ? ((B > REGIME_B && in.hw_queues >= 8) ? 4 : 2) : 1);
  if (want > MAX_PARTS) want = MAX_PARTS;
  while (want > 1 && tiles < 2 * want) --want;  // at least two tiles per part
  return want;
}

inline Route plan_route(const RouteInputs &in, long B, const CallFacts &call) {
  const qilqr_device_config &d = in.dev;
  const int fg = d.force_general, swr = d.single_wave_rollout;
  Route r;
  r.B = B;
  r.symmetric = in.symmetric;
  r.f32 = in.f32;
  r.integrator = in.integrator;
  r.force_general = fg;
  r.compaction = d.compaction;
  r.num_cus = in.num_cus;
  // The persistent solve (solve4.h): every trajectory from its first linearisation to its exit status in ONE launch.
  // Requirements: symmetric weights (the matrix-core recursion of k_backward4), no per-round host visibility (debug capture
  // of trajectories uses the rounds).  qilqr_device_config.persistent: 0 = by measurement, 1 = always, 2 = never.
  // By measurement (profiles/microbench/persistent_sweep.py, MI355X, N = 100, device-resident, ms per batch solve) the rounds are
  // level or ahead at every batch size but one -- 256: 4.15 vs 4.45, 1024: 5.63 vs 5.74, 1536: 7.52 vs 7.21, 2048: 8.1 vs 9.5,
  // 8192: 22.0 vs 27.6: both paths are bound by (iterations of the slowest trajectory) x (latency of one iteration), and inside
  // k_solve4 the forward phase ends one linearisation task (~11 us) after the rollout while its step waves run beside three
  // linearising wavefronts.
  // So 0 selects the rounds; the persistent solve stays selectable and tested.
#ifdef QILQR_WITH_SOLVE4
  r.persistent = in.symmetric && d.persistent == 1 && in.integrator == 0 && !in.limited && !in.modeled && !in.obstacles && !in.scheduled;
#endif  // (otherwise k_solve4 is in the diagnostics build: qilqr_create refuses persistent = 1 here)
  r.backward = backward_kind(in, B);
  // The knot records are placed for their reader (se3_math.h, rec_base): tiled for the kernels that stage them through LDS
  // (k_backward4, k_backward2, k_solve4), plain for the one-wavefront kernel (which addresses its operands through rec_elem and
  // reads either).
  r.tiled = r.persistent || r.backward != BW_ONE;
#ifdef QILQR_FORCE_MANY  // (experiment: the four-blocks-per-CU register budget and the unrolled knot loop at every size)
  r.many = true;
#else
  r.many = B > REGIME_B;
#endif
  if (in.integrator == 1 || in.limited || in.modeled || swr == 1) r.rollout = RO_LANE;  // (a forced choice is honoured at every batch size)
  else if (swr == 3 || (swr == 0 && B <= R16_MAX_B)) r.rollout = RO_16;
  else r.rollout = swr == 0 ? RO_THREE_THEN_16 : RO_THREE;
  // diagonal Q: the record of kind 2, cheaper arithmetic, the same bits in fp64 (tests/test_gpu_parity.py).  (Not in the
  // mixed mode: there the two instantiations differ in the last fp32 bit of a third of the knot costs -- the compiler
  // contracts the single-precision expressions differently -- and "the same results whatever the weights' structure" is
  // worth more than 1 % of k_linearize.)  The Runge-Kutta records hold a dense M at their head and have no such kind.
  // A state-weight schedule: the dense kind whatever the handle's Q is (k_round and k_backward4 keep 2 Q_vv in a constant table).
  r.lin_kind = in.scheduled ? 0 : (in.integrator == 0 && in.layout_kind == 2 && in.q_diag && !in.f32) ? 3 : in.layout_kind;
  r.backward_ext = r.rollout_ext = ExtArgs{in.limited, in.modeled, false};
  r.linearize_ext = ExtArgs{false, in.modeled, in.obstacles, in.problem_obstacles};
  // k_backward_rollout (round_kernels.h): the backward pass and the rollout of a round in one launch, when every block of four
  // trajectories has a CU to itself (the rollout's register budget allows one block per CU) and the round's kernels are the
  // fused k_backward4 and k_rollout16 anyway.  qilqr_device_config.round_launch = 1 keeps them apart (A/B).
  // (force_general = 8 with the combined launch: k_round with the six-wavefront backward pass in EVERY launch -- tests, A/B; only k_round has
  // the form: not k_backward_rollout)
  const bool plain = d.round_launch != 1 && in.integrator == 0 && !in.limited && !in.modeled && in.symmetric && r.tiled;
  r.fuse_kinds = plain && (fg == 0 || fg == 5 || fg == 8) && (fg == 8 || r.backward == BW_FUSED) &&
                 !(fg == 8 && (d.round_launch != 0 || in.f32 || in.obstacles)) && (swr == 0 || swr == 3) && B <= R16_MAX_B;
  r.combined = r.fuse_kinds && cdiv(B, 4) <= (unsigned)in.num_cus;
  // k_round (round_kernels.h): the combined launch and the linearisation of its candidates in one.  fp64 storage only (the mixed mode keeps
  // the two launches).  The round's counts go into the counter set of its parity; the launch publishes the round before it.
  // A handle with obstacles keeps the two launches as well: k_round linearises with linearize_cost alone (the same bits as
  // k_backward_rollout + k_linearize, round_kernels.h), and only k_linearize adds the penalties.
  r.round_kernel = d.round_launch == 0 && !in.f32 && !in.obstacles && !in.scheduled;  // (k_round fills Q from the handle's constants itself)
  // rounds per launch of k_round where a launch may hold several (qilqr_device_config.rounds_per_launch = 1, 2 or 4: A/B; 0 = 4)
  r.rounds_per_launch = (d.rounds_per_launch == 1 || d.rounds_per_launch == 2) ? d.rounds_per_launch : 4;
  // A batch of 1025 ... 4096 trajectories runs the same two kernels apart, with the compaction between them; once the running
  // trajectories fit the combined launch -- `slots` of them for this (sub-)batch: a block of four per CU over all the sub-batches --
  // the compaction has nothing left to give and the rounds change over to the one launch.
  // Round 6: a batch BEYOND 4096 does the same from the round in which its rollouts are k_rollout16's anyway (launch_rollout: the 17th, or
  // every round with single_wave_rollout = 3) -- the backward pass is one arithmetic in every form, so the combined launch's fused form gives
  // the bits of the six-wavefront launches it replaces, and a problem's bits stay independent of its batch.
  r.late_tail = QILQR_LATE_TAIL && plain && fg == 0 && B > R16_MAX_B && r.backward == BW_FOUR && (swr == 0 || swr == 3);
  r.late_from = r.late_tail && swr == 0 ? ROLLOUT16_FROM : 0;
  r.parts = call.sync_every > 1 ? auto_parts(in, B) : 1;
  // compaction: free-running rounds only (the host never waits for a plan), not beside the copy-back under the tail (it gathers by
  // slot), the per-iteration cost history (rows by slot), per-problem desired trajectories or per-problem models (they would have to move along)
  // Automatic (qilqr_device_config.compaction = 0): whenever the round's backward pass is a k_backward4 (blocks of four trajectories)
  // and not part of the combined launch of B <= 1024 -- measured, one configuration per process (profiles/r04_compaction.txt): 1280:
  // +5 %, 2048: +5.5 %, 3072: +13 %, 4096: +8 %, 8192: +6 %; with the one-wavefront backward kernel (general weights, the Runge-Kutta
  // extension, force_general = 2), whose blocks hold one trajectory, it gains nothing (12288-32768: -2 to +1 %) and stays off.
  r.compact = d.compaction >= 0 && call.sync_every > 1 && !r.persistent && !call.cost_hist && !call.desired_batch && !call.early_out && !in.modeled &&
              call.iterates && (d.compaction == 1 || (!r.combined && r.backward != BW_ONE && r.tiled));
  return r;
}

// ---- the choices that go by counts the host learns while the call runs

// The backward pass's form of a launch while `live` trajectories are known to be running.
// Since round 6 the fused and the six-wavefront forms give the same bits, so a batch of up to 4096 trajectories takes the six-wavefront form
// (Q_uu factored by the gradient wavefront, four blocks per CU) for the launches in which most of it is still running -- every trajectory live,
// per launch: 4096: 248 against 293 us, 3072: 177 / 184, 2048: 123 / 127, 1024: 86 / 74 -- and the fused form from there on.
inline BackwardKind backward_now(const Route &r, long live) {
  return (r.backward == BW_FUSED && r.force_general == 0 && live >= GFAC_MIN_LIVE) ? BW_FOUR : r.backward;
}
// Who factors Q_uu (round 6; the same bits either way, backward4_kernel.h): the gradient wavefront when the chip is saturated -- a SIMD
// is then bound by what its wavefronts issue, and one instruction stream factors four trajectories' Q_uu instead of four (a launch with
// every trajectory live, MI355X, N = 100: B = 65536 3807 -> 3515 us, 8192 509 -> 484) -- and the matrix wavefronts when a launch's
// wavefronts are alone on their SIMDs and its time is the chain of one knot's dependent instructions (B = 64: 75.3 against 85.3 us;
// level at 2048).
inline bool gradient_factors(const Route &r, long live) {
  const int fg = r.force_general;
  return fg == 7 || (fg != 8 && (r.many || fg == 0) && live >= GFAC_MIN_LIVE);
}
// ordinal: which rollout of its solve this is for every trajectory that takes part (a running trajectory rolls out exactly once per round, so
// the k-th rollout of ANY problem happens in round k of ANY call: a property of the problem, not of the batch); -1: the stand-alone entry points
inline bool rollout16_now(const Route &r, long ordinal) {
  return r.rollout == RO_16 || (r.rollout == RO_THREE_THEN_16 && ordinal >= ROLLOUT16_FROM);
}

// A k_round launch: how many rounds it holds and whether its backward pass takes the six-wavefront form, by how many trajectories a block
// holds on average (the same bits: round_kernels.h) -- and only in launches of several rounds: with one round per launch the 384-thread form
// measured slower.  several: the launches may hold several rounds.  forced: force_general chooses as well (the single-stream rounds: 8 takes
// the form in every launch, any other value but 0 never); the sub-batch streams go by the count alone.
struct RoundForm {
  int rounds;
  bool six;
};
inline RoundForm round_form(const Route &r, bool several, bool forced, unsigned seen_active, long used) {
  RoundForm f{several ? r.rounds_per_launch : 1, false};
  const bool sparse = f.rounds > 1 && 2L * (long)seen_active <= cdiv(used, 4) * 4L;
  f.six = forced ? (r.force_general == 8 || (r.force_general == 0 && sparse)) : sparse;
  return f;
}
// LK of the instantiation a launch takes (launch_round): the record kind of k_linearize; k_round takes the symmetric ones
inline int round_lk(const Route &r) { return std::max(r.lin_kind, 1); }
// ... and its form: the six-wavefront form is instantiated for launches of one and of four rounds
inline RoundForm round_instance(RoundForm f) {
  if (f.rounds == 2) f.six = false;
  return f;
}
// its slot in qilqr_round_launches' counts: 5 (LK - 1) + j, j = 0..4 for (rounds, six) = (1, no), (1, yes), (2, no), (4, no), (4, yes)
constexpr int round_slot(int lk, int rounds, bool six) { return 5 * (lk - 1) + (rounds == 1 ? (six ? 1 : 0) : rounds == 2 ? 2 : (six ? 4 : 3)); }

// When a compacted (sub-)batch changes over to the combined launch for the rest of its solve.
struct TailFuse {
  bool kinds = false;  // the round's kernels are the fused k_backward4 and k_rollout16 (or, from round `from` on, stand for the same bits)
  long slots = 0;      // slots in use at or below which this (sub-)batch's rounds are one launch
  unsigned stop = 0;   // the compaction runs while more trajectories than this are running
  long from = 0;       // first round in which the changeover may happen
};
// compacting: the call runs the compaction; nparts: its sub-batch streams
inline TailFuse tail_fuse(const Route &r, bool compacting, int nparts) {
  TailFuse t;
  t.stop = r.compaction == 1 ? 0u : COMPACT_STOP;
  if (!compacting || r.compaction == 1) return t;  // (forced: the compaction runs to the last trajectory)
  t.kinds = r.fuse_kinds || r.late_tail;
  t.from = r.late_from;
  if (t.kinds) {
    // (a block of four per CU over the sub-batches of ONE stream, two per CU over two streams', three over three and more: measured once
    // the tail ran on k_round -- profiles/r06_ab.txt section 14: B = 4096 + 1 %, 8192 + 2-3 %, 16384 + 1.5 %; a single stream at two blocks
    // per CU loses 17 % at B = 2048, whose whole solve would then be the tail)
    t.slots = std::max<long>(64, std::min(nparts, 3) * 4L * r.num_cus / nparts / 64 * 64);
    t.stop = std::max<unsigned>(t.stop, (unsigned)t.slots);
  }
  return t;
}

// ---- the instantiations of k_linearize (linearize_kernels.h): the record kind, the integrator, the placement of the records, the storage
// precision and the extension argument that rides behind the common ones, as one key.  launch_linearize (host/launches.h) walks the key
// space at compile time and instantiates the kernel for the keys lin_instantiated admits, and for no other.
enum { LIN_PLAIN, LIN_MODELS, LIN_OBSTACLES, LIN_BOTH, LIN_PROBLEM = 4 };  // (ext: bits; LIN_PROBLEM rides on LIN_OBSTACLES)
constexpr int LIN_KEYS = 256;
constexpr int lin_key(int lk, int integ, bool tiled, bool f32, int ext) { return lk + 4 * integ + 8 * tiled + 16 * f32 + 32 * ext; }
// Every instantiation the routes take: the extensions are fp64 and plain-placed but for the obstacles' tiled records (the symmetric kinds),
// the Runge-Kutta records (integ = 1) are plain and have no diagonal kind.  (The placement of the records was chosen with the call's backward
// kernel: Route::tiled.)
constexpr bool lin_instantiated(int lk, int integ, bool tiled, bool f32, int ext) {
  const bool models = ext & LIN_MODELS, obstacles = ext & LIN_OBSTACLES, problem = ext & LIN_PROBLEM;
  if (problem && !obstacles) return false;                              // the per-problem spheres are a form of the obstacle argument
  if (f32 && (lk == 3 || integ == 1 || ext != LIN_PLAIN)) return false;  // the mixed mode has no diagonal kind, and the extensions are fp64
  if (integ == 1 && (tiled || lk == 3)) return false;                   // Runge-Kutta records are plain and have no diagonal kind
  if (tiled && models) return false;                                    // models take the one-wavefront backward kernel: plain records
  if (tiled && obstacles && lk == 0) return false;                      // tiled obstacle forms for the symmetric kinds only
  return lk >= 0 && lk <= 3 && (integ == 0 || integ == 1) && ext >= 0 && ext < 8;
}
constexpr bool lin_instantiated(int key) { return lin_instantiated(key & 3, (key >> 2) & 1, (key >> 3) & 1, (key >> 4) & 1, key >> 5); }

}  // namespace qilqr
