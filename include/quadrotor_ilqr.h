/*
 * quadrotor_ilqr.h -- C ABI of the MI355X-native batched iLQR solver for the
 * SE(3) x R^6 quadrotor.  This is the drop-in boundary for the one hot path of
 * nitishthatte/QuadrotorILQR: everything reachable from ILQR<QuadrotorModel>::solve
 * (reference src/ilqr.hh:53-87).  Plain pointers and sizes, no exceptions, no C++
 * or torch types.  The shared library is libquadrotor_ilqr.so (HIP, gfx950 only;
 * there is no CPU fallback: every entry point that computes fails with
 * QILQR_ERR_NO_DEVICE when no GPU is present).
 *
 * Conventions
 *   knot   p[18]  = [time_s, tx,ty,tz, qw,qx,qy,qz, v_lin(3), v_ang(3), u0..u3]
 *                   (= IDX of reference src/quadrotor_ilqr.py:19-37; quaternion in the
 *                   wire order w,x,y,z of src/trajectory.proto:27-30)
 *   trajectory    = n x 18 doubles, row-major; a batch is B x n x 18
 *   tangent order = [rho(3), theta(3), dv_lin(3), dv_ang(3)]  (quadrotor_model.hh:30-37)
 *   matrices      = row-major (Q is 12x12 in tangent order, R is 4x4)
 *   gains  g[52]  = [k(4) ; K(4x12) column-major]  = the reference's
 *                   ControlUpdate{ff_update, feedback} (ilqr.hh:43-46)
 */
#ifndef QUADROTOR_ILQR_H
#define QUADROTOR_ILQR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QILQR_KNOT 18
#define QILQR_GAIN 52

/* return codes */
#define QILQR_OK 0
#define QILQR_ERR_BAD_INERTIA 1     /* "Inertia matrix is not positive definite!" quadrotor_model.cc:21-24 */
#define QILQR_ERR_LENGTH_MISMATCH 2 /* initial trajectory longer than desired: cost.hh:39-40 (.at) */
#define QILQR_ERR_INVALID_ARG 3
#define QILQR_ERR_BAD_QUATERNION 4  /* manif's SO3 constructor check, | |q| - 1 | > 1e-10 */
#define QILQR_ERR_NO_DEVICE 5
#define QILQR_ERR_HIP 6
#define QILQR_ERR_LINE_SEARCH 7     /* single solve only: ilqr.hh:191-193 throws */

/* per-problem exit path of solve(), numbered after the reference's return sites */
#define QILQR_STATUS_CONVERGED_EXPECTED 0 /* ilqr.hh:66-68 */
#define QILQR_STATUS_CONVERGED 1          /* ilqr.hh:82-84 */
#define QILQR_STATUS_MAX_ITERS 2          /* ilqr.hh:86    */
#define QILQR_STATUS_LINE_SEARCH_FAILED 3 /* ilqr.hh:191-193 */
#define QILQR_STATUS_QP_FAILED 4          /* extension (qilqr_set_control_limits): a knot's box QP broke down; the iterate is kept */

/* QuadrotorModel constructor arguments: quadrotor_model.hh:7-9, binding.cc:20-23 */
typedef struct {
  double mass_kg;
  double inertia[9];
  double arm_length_m;
  double torque_to_thrust_ratio_m;
  double g_mpss;
} qilqr_model;

/* ILQROptions: ilqr_options.hh:4-22 / ilqr_options.proto:5-21 */
typedef struct {
  double step_update;            /* LineSearchParams */
  double desired_reduction_frac;
  int32_t ls_max_iters;
  double rtol;                   /* ConvergenceCriteria */
  double atol;
  double max_iters;              /* a double in the reference */
  int32_t populate_debug;
} qilqr_options;

/* device-side configuration (no counterpart in the reference, which is CPU only) */
typedef struct {
  int32_t device;   /* HIP device ordinal */
  int32_t profile;  /* start/stop HIP events attached to kernel dispatches.  Low byte: 0 off; 1 k_backward and
                       k_rollout; 2 every kernel; 3 k_backward only; 4 k_rollout only.  Second byte: sampling
                       stride s (0 or 1: every selected launch; s > 1: every s-th launch of a kind is timed, the
                       averages of qilqr_profile_get are over the timed launches).  Bit 16 (0x10000): roctx ranges -- the host thread
                       marks a batch solve, every round it enqueues and, for a batch on sub-batch streams, every part's share of a round
                       ("qilqr round 17 part 2"), for `rocprofv3 --marker-trace --kernel-trace` (libroctx64 is bound at first use; absent,
                       no ranges) */
  int32_t sync_every; /* 1: the host waits for every round's count of active trajectories; k > 1 (default 2 when no
                         configuration is given): it reads the count k rounds late, i.e. keeps the stream k rounds
                         ahead of the device (k <= 6).  The results do not depend on it. */
  int32_t force_general; /* backward kernel.  0: by the weights and the batch (symmetric Q, R: k_backward4 in its fused form --
                            four wavefronts that each carry the matrix and the gradient recursion of a trajectory, plus a
                            loader wavefront, per four trajectories -- up to 4096 trajectories; in its six-wavefront form --
                            four matrix wavefronts, one gradient and one loader wavefront -- beyond (until ABI version 6 one wavefront
                            per trajectory took over above 8192: with the running trajectories compacted, see `compaction`, the blocks of
                            four are ahead at every size); non-symmetric Q or R: the general kernel); 1: the general kernel even when
                            Q, R are symmetric; 2: the one-wavefront kernel for symmetric weights (k_backward<true>);
                            3: k_backward2 (diagnostics build only); 4: k_backward4, six wavefronts (Q_uu factored by the gradient
                            wavefront in launches with 3072 or more running trajectories, by the matrix wavefronts otherwise; 7 / 8:
                            the one / the other at every launch -- 8 where the round is the combined launch k_round: its backward phase in
                            the six-wavefront form in every launch, which 0 takes for the launches in which at most two trajectories per
                            block still run); 5: k_backward4, fused
                            (its wavefronts meet through tagged LDS slots, no block barrier in the knot loop: what 0
                            selects up to 4096 trajectories; forced, it is used at every size); 6: retired in round 4
                            (the fused form with a block barrier per knot: refused by name).  When the round's kernels are the fused k_backward4 and k_rollout16 and
                            every block of four trajectories has a CU to itself (B <= 4 x the device's CUs: 1024 on
                            MI355X), the two are ONE launch (k_backward_rollout: the block's backward pass, a block
                            barrier, the rollout of its own four trajectories; same arithmetic, same bits) -- in fp64 together with
                            the linearisation of the block's candidates, four rounds to a launch (k_round: same bits again).
                            Since ABI version 7 / round 6 every form of k_backward4 performs ONE arithmetic (H accumulated in one
                            order, the gradient's sums in one order, Q_uu the same bits whoever factors it): a backward pass does not
                            depend on the batch size, and 0 also takes the six-wavefront form for the launches of a batch of up to 4096
                            in which 3072 or more trajectories still run.
                            WHICH ARITHMETIC A CALLER GETS.  The general kernel evaluates ilqr.hh:118-140 in the
                            reference's own forms: Q_uu factored by Eigen's diagonally pivoted LDL^T (largest |d_ii| of
                            the trailing block, first on ties), V_x = Q_x - K^T Q_uu k, V_xx = Q_xx - K^T Q_uu K, not
                            symmetrised -- force_general = 1 evaluates THE REFERENCE'S FORMULAS (the same products and sums; the
                            grouping of M^T V M alternates with the knot's parity -- (M^T V) M at odd knots, M^T (V M) at even ones --
                            because the accumulator tile is used transposed every other knot: not one fixed evaluation order of
                            ilqr.hh:118-124, equal to it to rounding), including the reference's loss of accuracy
                            beyond about 150 knots (the unsymmetrised recursion amplifies rounding asymmetry until the
                            gains are noise -- in the reference, the oracle and this kernel alike, of different magnitudes:
                            DESIGN.md section 4).  The symmetric-weight kernels (selected silently
                            whenever Q == Q^T and R == R^T exactly, i.e. for every weight the reference's demo and tests
                            use) DELIBERATELY DIFFER: unpivoted LDL^T (same result in exact arithmetic for positive
                            definite Q_uu; loses eps / p for an indefinite Q_uu with a tiny leading entry p) and the
                            equivalent forms V_x = Q_x + K^T Q_u, V_xx = Q_xx + Q_xu K on a symmetric accumulator, which
                            agree with the reference to rounding up to about 150 knots and stay bounded and convergent
                            beyond, where the reference's results are rounding noise. */
  int32_t single_wave_rollout; /* rollout kernel: 0 (default) = by the batch: sixteen lanes per trajectory, four
                                  trajectories per block (k_rollout16) up to 4096 trajectories; beyond, a lane per trajectory
                                  in three cooperating wavefronts (k_rollout3) for a trajectory's first 16 rollouts and k_rollout16
                                  from its 17th on (round 6: by then a fifth of a batch still runs and the kernels are lone dependent
                                  chains, where sixteen lanes per trajectory are a third faster; a running trajectory rolls out once per
                                  round, so the ordinal of a rollout is the round in EVERY call -- the choice is a property of the
                                  problem and of which side of 4096 its call is on, never of the other problems in the batch);
                                  1 = k_rollout (a lane per trajectory, one wavefront: the Runge-Kutta extension's kernel);
                                  2 = k_rollout3; 3 = k_rollout16 */
  int32_t precision; /* 0: fp64 everywhere (reference parity).  1: mixed: trajectories, gains and knot records
                        stored in fp32, rollout and linearisation computed in fp32, Riccati recursion on the fp64
                        matrix core, cost sums / Armijo / convergence tests in fp64 (BASELINE.json configs[2]) */
  int32_t streams; /* batch solves with sync_every > 1: number of contiguous sub-batches that run their rounds on
                      their own HIP streams (their kernels are bound by different resources and overlap);
                      0 = automatic (1 below 4096 trajectories, 2 at 4096, beyond 4 when the process runs with
                      GPU_MAX_HW_QUEUES >= 8 and 2 otherwise: see auto_parts in route.h), at most 8 */
  int32_t persistent; /* the solve as ONE launch (k_solve4: blocks of eight wavefronts own four trajectories each from the
                         first linearisation to the exit status, no rounds, no host in the loop; symmetric weights only):
                         0 = the rounds of three launches at every batch size (by measurement they are level or ahead at every size
                         but one, DESIGN.md section 4: the library never selects the one-launch solve by itself), 1 = always k_solve4,
                         2 = never (the same as 0 today) */
  int32_t compaction; /* (ABI version 6) device-resident batch solves with sync_every > 1: between a round's backward pass and its
                         rollout the trajectories still running are moved into a dense prefix of the workspace, the finished
                         ones they replace leaving for the caller's result arrays at once -- a batch takes as many rounds as its
                         slowest problem and the kernels hand out work in groups of 4 and 64 trajectories that cost the same
                         with one running as with all.  Results are bit-identical with and without.  0 = automatic (whenever the
                         round's backward pass is a k_backward4 launch of its own, i.e. symmetric weights and more than 1024
                         trajectories, while more than 512 of a sub-batch are running, and until the running ones fit the combined launch
                         -- k_backward_rollout, then k_round -- which the rounds then change over to: at once in a call of up to 4096
                         trajectories, in a larger one from the round in which its rollouts are k_rollout16's anyway, see
                         single_wave_rollout), 1 = at every size and count the call allows
                         (not with populate_debug's cost history, per-problem desired trajectories, or the copy-back under the
                         tail of qilqr_solve_batch), -1 = never */
  int32_t round_launch; /* (ABI version 7; until then the environment variables QILQR_FUSE_BACKWARD_ROLLOUT / QILQR_ROUND_KERNEL) how a round of
                           up to 4 x CUs trajectories is launched when its kernels are the fused k_backward4 and k_rollout16: 0 = automatic
                           (ONE launch: k_round, fp64 -- backward pass, rollout and linearisation of the candidates -- or k_backward_rollout +
                           k_linearize in the mixed mode), 1 = three launches (k_backward4, k_rollout16, k_linearize), 2 = two launches
                           (k_backward_rollout + k_linearize).  The same bits in every form: A/B measurements and the bit-identity tests */
  int32_t rounds_per_launch; /* (ABI version 7; was QILQR_ROUNDS_PER_LAUNCH) rounds in one k_round launch where a launch may hold several:
                                0 = automatic (4), or 1, 2, 4 */
  int32_t fuse_in_flight; /* (ABI version 7; was QILQR_FUSE_IN_FLIGHT) 1 = keep the combined launches although other batch solves of the
                             process are in flight on the device (0: a solve that is not alone launches the kernels apart) */
  int32_t dense_weights; /* (ABI version 7; was QILQR_NO_DIAG_Q) 1 = a diagonal Q is multiplied as a dense matrix instead of scaling rows
                            (the same bits: tests/test_gpu_parity.py::test_diagonal_weights_path_gives_the_same_bits) */
} qilqr_device_config;
/* The structure only ever grows at its end.  qilqr_create_sized / qilqr_sharded_create_sized take the size the CALLER was compiled with
 * (fields beyond it keep their defaults: 0, sync_every 2), so a caller built against an older header runs against a newer library;
 * with this header `qilqr_create(...)`, `qilqr_sharded_create(...)` and `qilqr_sharded_create_mask(...)` in source code ARE the sized calls
 * (macros below).  The exported symbols of those three names remain for binaries built before ABI version 7 -- and for callers that bind
 * symbols by name (dlsym, ctypes, function pointers: bind the *_sized names instead): they read ONLY the eight fields of ABI version 5
 * (32 bytes) and IGNORE every field behind them, whatever the caller's structure holds -- `compaction` of ABI version 6 (36 bytes: a
 * version-6 binary's value is not honoured through the raw symbols) and the four switches of version 7 keep their defaults there. */
#define QILQR_DEVICE_CONFIG_BYTES_ABI5 32

/* One arithmetic at every batch size: k_rollout16 is forced, so that a problem's result does not depend on the size of the batch it is
 * solved in, on sharding, or on sub-batch streams (the reference is trivially batching-independent: it solves one problem per call).
 * Since round 6 the backward pass needs no pinning (every form of k_backward4 performs the same arithmetic; the macro no longer forces
 * the fused form, which cost throughput above 4096 trajectories per call); the sixteen-lane rollout still costs some there. */
#define QILQR_PIN_ARITHMETIC(cfg) do { (cfg).single_wave_rollout = 3; } while (0)

/* A handle owns its device workspace and stream: use it from one thread at a time (different handles are
 * independent; the reference's ILQR object is const and re-entrant). */
typedef struct qilqr_solver qilqr_solver;

/* per-kernel device time accumulated since the last reset: *_ms and *_launches cover the launches that carried
 * events (kernels not selected by `profile`, and launches skipped by the sampling stride, do not), *_seen counts
 * every launch of the kind while profiling was on */
typedef struct {
  double backward_ms;  int32_t backward_launches;
  double rollout_ms;   int32_t rollout_launches;
  double linearize_ms; int32_t linearize_launches;
  double other_ms;     int32_t other_launches;
  int32_t backward_seen, rollout_seen, linearize_seen, other_seen;
  double solve_ms;     int32_t solve_launches;  /* persistent solves (k_solve4: one launch per batch solve) */
  int32_t solve_seen;
} qilqr_profile;

/* Replaces src::init, quadrotor_ilqr_binding.cc:20-32 (QuadrotorModel ctor + CostFunction +
 * ILQR ctor).  `desired` is n_desired x 18 (time column ignored).  Everything is copied. */
int qilqr_create(const qilqr_model *model, const double *Q, const double *R,
                 const double *desired, int32_t n_desired, double dt_s,
                 const qilqr_options *options, const qilqr_device_config *dev,
                 qilqr_solver **out);
int qilqr_create_sized(const qilqr_model *model, const double *Q, const double *R,
                       const double *desired, int32_t n_desired, double dt_s,
                       const qilqr_options *options, const qilqr_device_config *dev, size_t dev_bytes,
                       qilqr_solver **out);
void qilqr_destroy(qilqr_solver *s);

/* text of the last error on the calling thread */
const char *qilqr_last_error(void);

/* Replaces src::solve, quadrotor_ilqr_binding.cc:34-41 -> ILQR::solve, ilqr.hh:53-87.
 * One problem.  debug_cost[debug_cap] / debug_trajs[debug_cap x n x 18] receive, when
 * options.populate_debug, one entry per completed forward pass (ilqr.hh:78-80); n_debug the
 * count.  Returns QILQR_ERR_LINE_SEARCH where the reference throws (outputs untouched). */
int qilqr_solve(qilqr_solver *s, const double *init, int32_t n, double *out_traj,
                double *out_cost, int32_t *out_status, int32_t *out_iters,
                double *debug_cost, double *debug_trajs, int32_t debug_cap, int32_t *n_debug);

/* B independent problems sharing model, cost weights, dt and options.  Host buffers.
 * init B x n x 18.  desired_batch: NULL (use the desired trajectory given at create) or
 * B x n x 18 per-problem desired trajectories.  Any output pointer may be NULL.
 * Line-search exhaustion is reported per problem in out_status, not as an error. */
int qilqr_solve_batch(qilqr_solver *s, const double *init, const double *desired_batch,
                      int32_t B, int32_t n, double *out_traj, double *out_cost,
                      int32_t *out_status, int32_t *out_iters, int32_t *out_n_bwd,
                      int32_t *out_n_fwd);

/* Same, with every buffer already resident in device memory (HBM) of the solver's device: plain contiguous
 * B x n x 18 doubles / B doubles / B int32, caller-owned, outputs at least that large (nothing is checked on the
 * device side; any output may be NULL).  Stream ordering: the solve runs on the solver's OWN stream (qilqr_stream,
 * created non-blocking: it is not ordered with the null stream or with any other stream).  Inputs written by
 * asynchronous work on another stream must be ordered first: record an event there and pass it to
 * qilqr_stream_wait_event (or synchronise that stream).  The call returns after the solver's stream has drained,
 * so the outputs may be read from any stream afterwards. */
int qilqr_solve_batch_device(qilqr_solver *s, const double *d_init, const double *d_desired_batch,
                             int32_t B, int32_t n, double *d_out_traj, double *d_out_cost,
                             int32_t *d_out_status, int32_t *d_out_iters, int32_t *d_out_n_bwd,
                             int32_t *d_out_n_fwd);

/* The passes the reference's tests call directly (ilqr_test.cc:102-190), batched, host buffers. */
/* ILQR::cost_trajectory, ilqr.hh:89-95 */
int qilqr_cost_trajectory(qilqr_solver *s, const double *traj, int32_t B, int32_t n, double *cost);
/* ILQR::backwards_pass, ilqr.hh:97-147: gains B x n x 52, terms B x 2 = {QuTk, kTQuuk} */
int qilqr_backwards_pass(qilqr_solver *s, const double *traj, int32_t B, int32_t n, double *gains,
                         double *terms);
/* ILQR::forward_sim, ilqr.hh:149-172: alpha[B] */
int qilqr_forward_sim(qilqr_solver *s, const double *traj, const double *gains,
                      const double *alpha, int32_t B, int32_t n, double *out_traj);
/* ILQR::line_search, ilqr.hh:174-194: cost[B], terms B x 2 -> out_traj, out_cost[B], out_step[B],
 * out_status[B] (0 accepted, QILQR_STATUS_LINE_SEARCH_FAILED where the reference throws) */
int qilqr_line_search(qilqr_solver *s, const double *traj, const double *cost, const double *gains,
                      const double *terms, int32_t B, int32_t n, double *out_traj,
                      double *out_cost, double *out_step, int32_t *out_status);

/* Cost history of the last batch solve (options.populate_debug = 1): hist is B x cap, row b holds
 * new_cost after each completed forward pass of problem b (what ILQRDebug.cost would hold, ilqr.hh:78-80;
 * trajectories are only captured by the single-problem qilqr_solve), unused entries are NaN.
 * cap = the largest number of entries any problem can have (= min(ceil(max_iters), 1e6): the loop of ilqr.hh:58
 * runs while i < max_iters, a double); returned in *out_cap
 * when hist is NULL. */
int qilqr_cost_history(qilqr_solver *s, int32_t B, double *hist, int32_t cap, int32_t *out_cap);

/* profiling (HIP events on the solver's stream) */
int qilqr_profile_reset(qilqr_solver *s);
int qilqr_profile_get(qilqr_solver *s, qilqr_profile *out);
/* change qilqr_device_config.profile of a live solver (drains the stream, resets the accumulated times) */
int qilqr_profile_mode(qilqr_solver *s, int32_t mode);

/* Levenberg-Marquardt restarts -- an EXTENSION the reference does not have (SURVEY.md section 8f row 4;
 * BASELINE.json configs[4] "line-search/regularisation restarts"); off by default and when mu_init == 0,
 * and then every result is the reference's.  Where ILQR::line_search would throw after ls_max_iters trials
 * (ilqr.hh:191-193) the problem instead keeps its iterate, sets mu = mu_init (then mu *= mu_factor on each
 * further exhaustion), repeats ILQR::backwards_pass with Q_uu + mu 1 in place of Q_uu in every formula of
 * ilqr.hh:126-140, and searches again from a full step.  An accepted step divides mu by mu_factor (below
 * mu_init it returns to 0).  Past mu_max the problem ends with QILQR_STATUS_LINE_SEARCH_FAILED as before.
 * Restarts are not iterations; they show in out_n_bwd.  Requires mu_factor > 1, mu_max >= mu_init. */
int qilqr_set_regularisation(qilqr_solver *s, double mu_init, double mu_factor, double mu_max);

/* Runge-Kutta integration of the dynamics -- an EXTENSION: the four-stage step that
 * quadrotor_model.cc:51-63 sketches in a comment and the reference never executes,
 *     k_0 = f(x, u), k_i = f(x (+) h_i k_{i-1}, u) with h = {0, dt/2, dt/2, dt};  x_next = x (+) dt (k_0 + 2 k_1 + 2 k_2 + k_3) / 6,
 * in place of the explicit Euler step of quadrotor_model.cc:33-49 in every pass (forward simulation, and the Jacobians
 * J_x, J_u of the backward pass by the chain rule through the stages).  integrator = 0 (default): the reference's step, and
 * then every result is the reference's; 1: the extension (fp64 solvers only).  Stated in the oracle from the reference's
 * own primitives; measured order of accuracy on SE(3): two, against Euler's
 * one (tests/test_oracle_rk4.py explains why not four).  The extension runs on the general kernels -- a lane per
 * trajectory rollout, the one-wavefront backward pass over dense Jacobian records -- not on the tuned Euler path. */
int qilqr_set_integrator(qilqr_solver *s, int32_t integrator);

/* Per-rotor thrust limits -- an EXTENSION (control-limited DDP, Tassa, Mansard & Todorov, ICRA 2014): lo[4], hi[4] bound u0..u3 (N);
 * +-inf leaves a side open.  Every knot of the backward pass solves the box QP  min 1/2 du^T Q_uu du + Q_u^T du  subject to
 * lo - u_i <= du <= hi - u_i  by projected Newton (quadrotorilqr_amd/csrc/box_qp.h); the feedback gain has zero rows for the rotors at a
 * bound, and the value function takes the full updates.  The rollout clamps every control to [lo, hi] after the control law (so an
 * initial guess outside the box becomes feasible in the first rollout).  Applies to every computing entry point of the handle: the
 * solves, qilqr_backwards_pass, qilqr_forward_sim, qilqr_line_search (a sharded handle: one call per shard, qilqr_sharded_solver).
 * Runs on the one-wavefront backward kernel and the lane-per-trajectory rollout, with either integrator and with restarts.
 * A problem whose QP breaks down at some knot (a pivot <= 0: numerical only, Q_uu stays positive definite when R is) ends with
 * QILQR_STATUS_QP_FAILED on its current iterate.
 * QILQR_ERR_INVALID_ARG unless lo[a] < hi[a] and neither is NaN for every rotor, and for a mixed-precision handle, non-symmetric
 * Q or R (or force_general = 1), or R that is not positive definite; a solve with persistent = 1 is refused while limits are set.
 * lo = hi = NULL clears the limits: every result is then again the handle's without them.  Waits for the handle's stream. */
int qilqr_set_control_limits(qilqr_solver *s, const double *lo, const double *hi);

/* Per-problem models -- an EXTENSION: from this call on, problem b of every computing entry point of the handle (qilqr_solve_batch,
 * qilqr_solve_batch_device, qilqr_backwards_pass, qilqr_forward_sim, qilqr_line_search) is solved with models[b] -- its own mass, g,
 * inertia, arm length and torque ratio -- for a fleet of airframes, payloads of different mass, or one start under sampled models.
 * dt, Q, R, the desired trajectory, the options, the integrator, restarts and thrust limits stay the handle's.  qilqr_cost_trajectory
 * does not depend on the model (and takes any B).  The call copies the models into one record per problem (mass, g, inertia, its
 * inverse, moment arms, the constant rows of J_u: quadrotorilqr_amd/csrc/batch_models.h), uploads them once, and waits for the
 * handle's stream.  Runs on the general kernels -- the one-wavefront backward pass, the lane-per-trajectory rollout, k_linearize
 * reading each problem's record -- with either integrator, with restarts, with thrust limits and with any weights they take; the
 * compaction of the running trajectories is off.
 * QILQR_ERR_BAD_INERTIA for a model qilqr_create would refuse ("Inertia matrix is not positive definite! (batch models: problem k)",
 * k the first such index); QILQR_ERR_INVALID_ARG for a mixed-precision handle (precision = 1), and, while models are set, for a
 * computing call whose B is not this B, a solve with persistent = 1, and qilqr_solve (one problem, the handle's model by definition).
 * models = NULL with B = 0 clears them: every result is then again the handle's without them. */
int qilqr_set_batch_models(qilqr_solver *s, const qilqr_model *models, int32_t B);

/* Spherical obstacles -- an EXTENSION: a soft penalty in the cost of every entry point that evaluates or differentiates it
 * (qilqr_solve, qilqr_solve_batch[_device], qilqr_cost_trajectory, qilqr_backwards_pass, qilqr_line_search, and so
 * qilqr_cost_history), shared by every problem of the handle.  spheres is count x 5 doubles {cx, cy, cz, radius, weight}.
 * At every knot i (the last included), with p the knot's position, d_j = |p - c_j| and h_j = radius_j - d_j, the knot cost becomes
 *     tracking_cost + sum_j weight_j h_j^2   over the spheres with h_j > 0, added in index order after the tracking cost.
 * A sphere with h_j <= 0 does no arithmetic on the result: obstacles that no knot reaches give the bits of a handle without them.
 * Differentials (tangent order [rho, theta, dv, dw], the reference's factor 2): with R the knot's attitude, n_j = (p - c_j) / d_j and
 * m_j = R^T n_j, C_x[0:3] += -2 weight_j h_j m_j and C_xx[0:3, 0:3] += 2 weight_j m_j m_j^T (Gauss-Newton, as the tracking cost's
 * Hessian: Q_xx stays positive semi-definite).  d_j == 0 exactly: the cost term is weight_j radius_j^2 and the differentials get
 * nothing (the direction is undefined).  Composes with either integrator, restarts, thrust limits, per-problem models, any weights,
 * force_general, the compaction and sub-batch streams; the rounds take k_backward_rollout + k_linearize or three launches where they
 * would have taken the one-launch round kernel (the same bits).  Validates, uploads the table once, and waits for the handle's stream.
 * QILQR_ERR_INVALID_ARG for count > QILQR_MAX_OBSTACLES, a non-finite value, radius <= 0, weight < 0, a mixed-precision handle
 * (precision = 1), and, while obstacles are set, a solve with persistent = 1.  spheres = NULL with count = 0 clears them: every
 * result is then again the handle's without them. */
#define QILQR_MAX_OBSTACLES 64
int qilqr_set_obstacles(qilqr_solver *s, const double *spheres, int32_t count);

/* Per-problem, moving spheres -- an EXTENSION beside qilqr_set_obstacles: problem b of the batch gets its own counts[b] <= K spheres,
 * for a fleet in its own surroundings, receding-horizon use with predicted obstacles, or sampled obstacle fields.  spheres is
 * B x K x QILQR_OBSTACLE_WORDS doubles (row-major) {cx, cy, cz, vx, vy, vz, radius, weight}; counts (int32[B]) may be NULL for all K.
 * At knot i (0-based, the last included) the centre is c + t_i v, t_i = i dt (dt the handle's), per axis fma(t_i, v, c): a sphere
 * with v = 0 is centred at c exactly.  From there the term, its gradient and Gauss-Newton block, the d == 0 rule and "an inactive
 * sphere touches nothing" are those of qilqr_set_obstacles, by the same arithmetic (a static sphere here gives the bits of the same
 * shared sphere).  A caller who solves from time t0 shifts c by t0 v.  Order within a knot cost: the tracking cost, the handle's
 * shared spheres, then the problem's own, each in index order; both tables may be set at once.  Rows j >= counts[b] are never read.
 * Used by every entry point that evaluates or differentiates the cost (qilqr_solve_batch[_device], qilqr_cost_trajectory,
 * qilqr_backwards_pass, qilqr_line_search, the cost history, and qilqr_solve as B = 1), each of which is then refused for another B;
 * qilqr_forward_sim evaluates no cost and takes any B.  Composes as the shared spheres do (the compaction included: the table is read
 * by the problem's row).  Validates, re-lays the table out for the device (tiles of 64 problems) and uploads it once, and waits for the
 * handle's stream.  QILQR_ERR_INVALID_ARG, with the reason and the first bad (problem, sphere) in qilqr_last_error, for K outside
 * 1 ... QILQR_MAX_OBSTACLES, a count outside 0 ... K, a non-finite word in a used row, radius <= 0, weight < 0, a mixed-precision
 * handle, and, while the table is set, a solve with persistent = 1.  spheres = counts = NULL with B = K = 0 clears the table. */
#define QILQR_OBSTACLE_WORDS 8
int qilqr_set_batch_obstacles(qilqr_solver *s, const double *spheres, const int32_t *counts, int32_t B, int32_t K);

/* Per-knot state weights -- an EXTENSION: Qs is n_knots x 12 x 12 doubles (row-major, tangent order [rho, theta, dv, dw]), and from this
 * call on knot i (0-based; the last knot has a cost like every other, ilqr.hh:89-95) of every problem takes Qs[i] wherever the handle's Q
 * stood: the knot cost, C_x and C_xx.  A terminal weight ("be at this pose at the end": Q_f >> Q at the last knot) and waypoints (a large
 * weight at a few knots, little or none between them) are schedules.  R, the desired trajectory, the model, dt and the options stay the
 * handle's.  The index is the absolute knot index, as for the desired trajectory (cost.hh:39-40): a call with n < n_knots uses the first n
 * matrices, a call with n > n_knots is refused with QILQR_ERR_LENGTH_MISMATCH.  The schedule is shared by every problem of the handle and
 * used by every entry point that evaluates or differentiates the cost (qilqr_solve, qilqr_solve_batch[_device], qilqr_cost_trajectory,
 * qilqr_backwards_pass, qilqr_line_search, and so qilqr_cost_history); qilqr_forward_sim evaluates no cost and is unaffected.
 * While a schedule is set the handle takes the route of non-symmetric weights whatever its own Q is: dense knot records, in which all of
 * C_xx travels, the one-wavefront backward kernel and three launches per round (qilqr_describe says so) -- in its symmetric-weight form
 * when R and every Qs[i] are bit-exactly symmetric and force_general != 1, in the reference's own forms otherwise.  Definiteness is not
 * checked (the handle's Q is not checked either): the symmetric-weight form factors Q_uu = 2 R + J_u^T V_xx J_u by an UNPIVOTED LDL^T and
 * needs it positive definite, which holds for positive semi-definite Qs[i] and positive definite R.  Composes with either integrator,
 * restarts, thrust limits (which need every Qs[i] symmetric), per-problem models, both sphere tables, per-problem desired trajectories,
 * sub-batch streams, compaction = 1 and sharding.  The setter copies, uploads once, and waits for the handle's stream.
 * QILQR_ERR_INVALID_ARG for a non-finite entry (qilqr_last_error names the first bad knot, row and column), n_knots < 1 with Qs given,
 * a mixed-precision handle (precision = 1), a change that would leave thrust limits on non-symmetric weights (a non-symmetric Qs[i], or
 * clearing a schedule that stands in for a non-symmetric Q: clear the limits first), and, while a schedule is set, a solve with
 * persistent = 1.  Qs = NULL with n_knots = 0 clears: every result is then bit for bit the handle's without a schedule. */
int qilqr_set_state_weight_schedule(qilqr_solver *s, const double *Qs, int32_t n_knots);

/* Receding-horizon control -- an EXTENSION in two parts: a window into the handle's desired trajectory and schedule, and the step from
 * one solve's plan to the next solve's initial trajectory.  At every control tick a caller drops the knots that have been flown, anchors
 * knot 0 at the measured state, extends the end of the horizon and solves again (quadrotorilqr_amd/mpc.py does this on device buffers).
 *
 * Horizon start.  From this call on, knot i of every call of the handle takes desired[k0 + i] of the desired trajectory given at create
 * and, wherever a state-weight schedule is read, Qs[k0 + i]: a mission of 1000 knots is flown with a 100-knot horizon on ONE handle, without
 * a per-problem desired_batch (which also switches the compaction off).  A call of n knots needs n <= n_desired - k0 when no desired_batch
 * is given and, where it evaluates the cost, n <= n_knots - k0 of the schedule: QILQR_ERR_LENGTH_MISMATCH otherwise.  A per-problem
 * desired_batch is already the caller's window and is unaffected.  BOTH SPHERE TABLES ARE UNAFFECTED: a moving sphere's time stays i dt
 * from the call's first knot, because that table is a prediction made at tick time (set it again at the tick, centres at their positions
 * then).  The route, the records and every kernel are those of the handle without a start: the start is an offset of two pointers, and
 * k0 = 0 restores the handle bit for bit.  Nothing is waited for.  QILQR_ERR_INVALID_ARG unless 0 <= k0 < n_desired, and k0 < n_knots
 * while a schedule is set (0 is always accepted), and for a non-zero start on a mixed-precision handle (precision = 1); a refused call
 * leaves the start that was in force.  The rule holds from the other side too: while a start is in force, qilqr_set_state_weight_schedule
 * refuses a schedule with n_knots <= k0 (QILQR_ERR_INVALID_ARG, the handle keeps the schedule it had): lower the start first. */
int qilqr_set_horizon_start(qilqr_solver *s, int32_t k0);

/* The shift.  Arrays are plain B x n x 18 as everywhere; 0 <= steps <= n - 1.  Problem by problem:
 *   kept knots     out[b, i] = traj[b, i + steps] for i < n - steps: all 18 words bit for bit, the time column included
 *   tail           j = n - steps .. n - 1: the state of knot j is ONE DYNAMICS STEP from the state of output knot j - 1 under the control
 *                  stored there (output knot n - 1 - steps is traj[b, n - 1] as given, its control included).  The step is the handle's:
 *                  its dt, its integrator (qilqr_set_integrator) and models[b] while per-problem models are set, in the arithmetic of the
 *                  solver's own rollout.  The control stored at a tail knot is traj[b, n - 1, 14:18] (QILQR_TAIL_HOLD) or mass g / 4 of
 *                  the problem's model on every rotor (QILQR_TAIL_HOVER), clamped to the thrust limits while they are set.  Its time is
 *                  traj[b, n - 1, 0] + k dt, k = j - (n - 1 - steps)
 *   re-anchoring   with x0 (B x QILQR_STATE: words 1..13 of a knot -- t(3), q w,x,y,z, v_lin(3), v_ang(3)) words 1..13 of output knot 0
 *                  are x0[b]; its time and control stay.  Nothing else is rolled again -- the tail starts from traj[b, n - 1] whatever x0
 *                  is, and the solver's first closed-loop rollout starts from knot 0.  x0 = NULL: no re-anchoring
 * The shift evaluates no cost: spheres, schedules and the horizon start play no part.  One launch (k_shift) reads traj and writes out.
 * Both forms: QILQR_ERR_INVALID_ARG for a NULL traj or out, steps or tail out of range, a mixed-precision handle, another B than the
 * per-problem models were set for, an array that is not 16-byte aligned, and an out that overlaps traj or x0 (the copy is parallel: in
 * place is a race).  qilqr_shift_batch (host arrays) checks x0's quaternions as initial trajectories are checked
 * (QILQR_ERR_BAD_QUATERNION, naming the problem) and returns when out is written.  qilqr_shift_batch_device (arrays in the memory of the
 * handle's device) checks nothing on the device, ENQUEUES on the handle's stream (qilqr_stream) and returns WITHOUT draining it: the next
 * solve on the handle is ordered behind it; work on any other stream that writes d_traj / d_x0 or reads d_out orders itself as for
 * qilqr_solve_batch_device -- an event passed to qilqr_stream_wait_event before the call, or synchronise the stream (hipStreamSynchronize
 * on qilqr_stream, or any draining call of the handle) before reading. */
#define QILQR_STATE 13
#define QILQR_TAIL_HOLD 0
#define QILQR_TAIL_HOVER 1
int qilqr_shift_batch_device(qilqr_solver *s, const double *d_traj, const double *d_x0, int32_t B, int32_t n, int32_t steps, int32_t tail,
                             double *d_out);
int qilqr_shift_batch(qilqr_solver *s, const double *traj, const double *x0, int32_t B, int32_t n, int32_t steps, int32_t tail,
                      double *out);

/* ---- the other half of the plan: its feedback law (an extension; the reference keeps its gains inside ILQR::solve).  iLQR computes, with
 * every plan, the time-varying law u = u_i + K_i (x (-) x_i) that flies it from a state off the plan.  Two calls bring it to a caller of
 * the device path: the gains about a plan that sits in device memory, and the law applied from measured or sampled states.
 *
 * qilqr_backwards_pass_device is qilqr_backwards_pass over plain device arrays (d_traj B x n x 18, d_gains B x n x 52, d_terms B x 2 or
 * NULL): the same linearisation and backward pass, honouring every extension the host form honours (schedule, spheres, limits, models,
 * integrator, horizon start), the same bits, without the two copies of B x n x 52 doubles over the host.  It is a pass of its own, and not
 * a by-product of the solve, because the gains a solve holds when it returns belong to the iterate BEFORE its last accepted step: they
 * were computed about the trajectory the last line search started from.  Gains about the RETURNED plan are one more backward pass on it --
 * this one.  It returns after the handle's stream has drained, as qilqr_solve_batch_device does (order the inputs the same way).
 *
 * The closed loop.  plan is B x n x 18, gains B x n x 52 (of which the feed-forward part k, words 0..3 of a knot, is NOT read: the law at
 * alpha = 0), x0 is B x S x QILQR_STATE: S states per plan.  0 <= i0 <= i1 <= n - 1, S >= 1.  Sample (b, j) has state x0[b, j] at knot
 * i0, and for i = i0 .. i1:
 *   dx = x (-) plan[b, i]                      the 12 tangent words the solver's rollout forms
 *   u  = plan[b, i, 14:18] + K_i dx            clamped to the thrust limits while they are set
 *   knot i of the sample is recorded           its time is plan[b, i, 0], then the state, then u
 *   if i < i1: one dynamics step under u       the handle's: its dt, its integrator, and models[b S + j] while per-problem models are set --
 *                                              they must then have been set for B S problems; plant / model mismatch is expressed this way
 * in the arithmetic of the solver's own rollout: with S = 1, x0 = plan[:, 0, 1:14], i0 = 0 and i1 = n - 1 the result has the bits of
 * qilqr_forward_sim(plan, gains, alpha = 0) on a handle with single_wave_rollout = 1.  A sample's bits depend on its own inputs only --
 * not on S, on j, or on which of the kernel's two forms carried it (a wavefront of 64 samples of one plan that shares the plan's operands,
 * or a lane per sample for small S).  i0 = i1 is the plain policy evaluation at a measured state.  No cost is evaluated: spheres, schedules
 * and the horizon start play no part (qilqr_closed_loop_scored, below, scores the flight).
 *   d_out_traj    B x S x n x 18 or NULL: knots i0 .. i1 of every sample are written, every other knot is left untouched; with NULL no
 *                 trajectory store is issued (a Monte-Carlo caller reads the statistics only)
 *   d_out_stats   B x S x QILQR_CL_STATS or NULL, from the dx the law computes anyway: {max_i |dx_i[0:3]|, max_i |dx_i[3:6]|, |dx_i1|,
 *                 the number of (knot, rotor) pairs that were clamped, as a double} -- Euclidean norms of the position error, the
 *                 rotation error and, at the last knot, of all 12 words
 * Both forms: QILQR_ERR_INVALID_ARG, before the device is touched, for a NULL plan, gains or x0, both outputs NULL, a non-positive B, n or
 * S, knots out of range, an array that is not 16-byte aligned, an output that overlaps an input or the other output, a NULL or
 * mixed-precision handle, and per-problem models set for another count than B S.  qilqr_closed_loop (host arrays) checks x0's quaternions
 * (QILQR_ERR_BAD_QUATERNION, naming problem and sample) and returns when the outputs are written.  The device form checks nothing on the
 * device, ENQUEUES on the handle's stream and returns WITHOUT draining it, with the ordering rules of the device form of the shift.
 * Sharded handles have neither call: use a shard's solver (qilqr_sharded_solver) with the arrays of its device. */
#define QILQR_CL_STATS 4
int qilqr_backwards_pass_device(qilqr_solver *s, const double *d_traj, int32_t B, int32_t n, double *d_gains, double *d_terms);
int qilqr_closed_loop_device(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0, int32_t B, int32_t n,
                             int32_t S, int32_t i0, int32_t i1, double *d_out_traj, double *d_out_stats);
int qilqr_closed_loop(qilqr_solver *s, const double *plan, const double *gains, const double *x0, int32_t B, int32_t n, int32_t S,
                      int32_t i0, int32_t i1, double *out_traj, double *out_stats);

/* The scored flight (extension): the closed loop above flown under a disturbance and scored on the device -- what a Monte-Carlo caller
 * flies samples for, without the B x S x n x 18 trajectories.  The law, the clamp, the step, out_traj and out_stats are
 * qilqr_closed_loop's, word for word; with wrench, desired and out_score all NULL the call launches the same kernels and gives the bits
 * of qilqr_closed_loop[_device].
 *
 * The disturbance.  wrench is NULL or B x S x n_w x QILQR_WRENCH doubles {F_x, F_y, F_z, tau_x, tau_y, tau_z}: F a force in newtons in
 * the WORLD frame, tau a torque in N m in the BODY frame.  n_w = 1: one wrench per sample for the whole flight; n_w = n: wrench[b, j, i]
 * acts during the step from knot i to knot i + 1 (a zero-order hold); rows of steps outside i0 .. i1 - 1 are never read.  The wrench
 * enters the continuous dynamics where thrust and moment do, with the sample's model.  With R = R(q) the attitude of the state the
 * acceleration is evaluated at (under Runge-Kutta each stage's own, the wrench held over the four stages), in this order:
 *     f[k]       = R[0][k] F_x + R[1][k] F_y + R[2][k] F_z        (R^T F: the velocities of this model are body-frame)
 *     acc_lin[k] = a[k] + f[k] / mass                             (a[k]: the undisturbed linear acceleration, formed first)
 *     rhs[k]     = (M[k] - (w x I w)[k]) + tau[k]                 (then acc_ang = I^-1 rhs, as without a wrench)
 * one text for both forms of the kernel, so a sample's bits still depend on its own inputs only.  A zero wrench flies the flight
 * without one (equal values).
 *
 * The score.  out_score is NULL or B x S x QILQR_CL_SCORE doubles {cost, min_clearance, knot_of_min_clearance, knots_in_collision}:
 *   cost            the sum over i = i0 .. i1, in knot order, of the handle's knot cost at the flown state and the applied (clamped)
 *                   control: the tracking cost with the handle's Q (Qs[k0 + i] while a schedule is set) and R against desired[k0 + i] of
 *                   the handle -- or, when d_desired (B x n x 18, one per plan, as desired_batch of the solves) is given, against
 *                   d_desired[b, i], whatever k0 is -- then the shared spheres, then row b of the per-problem table (centres at
 *                   c + i dt v), each table in index order: what qilqr_cost_trajectory charges those knots of that trajectory
 *   min_clearance   the minimum of |p - c_j(i)| - radius_j over i = i0 .. i1 and every sphere of both tables; +inf without spheres
 *   knot_of_min_clearance   the knot where it is attained, the first on ties; -1 without spheres
 *   knots_in_collision      the number of knots whose smallest clearance is < 0
 * At a knot: h_j = radius_j - |p - c_j|; if h_j > 0 the knot cost grows by (weight_j h_j) h_j; the clearance is -h_j.  A sphere of
 * weight 0 leaves the cost's bits and still counts for the clearance (an "observe only" obstacle; inflate its radius by the vehicle's).
 * A NaN is taken, not dropped, as the maxima of the statistics take one.
 *
 * Any of the three outputs may be NULL, not all three; with out_traj NULL no trajectory store is issued.  Refused, after what
 * qilqr_closed_loop refuses about the same arguments: n_w other than 1 or n while a wrench is given; wrench, desired or out_score off a
 * 16-byte boundary; the score array overlapping an input or another output (or an output the wrench or desired); then, after the
 * handle's own refusals, scoring while a per-problem sphere table is set for another B (QILQR_ERR_INVALID_ARG all), and
 * QILQR_ERR_LENGTH_MISMATCH when scoring without desired needs i1 >= n_desired - k0, or with a schedule i1 >= n_knots - k0.  The host
 * form also refuses a non-finite wrench word, naming (problem, sample, knot).  The device form checks nothing on the device, ENQUEUES
 * on the handle's stream and does not drain it, with the ordering rules of qilqr_closed_loop_device. */
#define QILQR_WRENCH 6
#define QILQR_CL_SCORE 4
int qilqr_closed_loop_scored_device(qilqr_solver *s, const double *d_plan, const double *d_gains, const double *d_x0,
                                    const double *d_wrench, int32_t n_w, const double *d_desired, int32_t B, int32_t n, int32_t S,
                                    int32_t i0, int32_t i1, double *d_out_traj, double *d_out_stats, double *d_out_score);
int qilqr_closed_loop_scored(qilqr_solver *s, const double *plan, const double *gains, const double *x0, const double *wrench,
                             int32_t n_w, const double *desired, int32_t B, int32_t n, int32_t S, int32_t i0, int32_t i1,
                             double *out_traj, double *out_stats, double *out_score);

/* The ends of the Monte-Carlo loop on the device (extension): what the scored flight reads is sampled, and what it writes is reduced,
 * where it lies -- sample, fly, reduce are four enqueues on the handle's stream, the only host input the measured state of each plan,
 * the only output QILQR_MC_SUMMARY words per plan.  Device arrays only; sharded handles have no such call (use a shard's solver).
 *
 * The normals.  Philox4x32-10 with counter {i, s0 + s, b0 + b, stream << 16 | j} and key {seed & 0xffffffff, seed >> 32}: i the row
 * (knot), s the sample, b the plan, stream 0 for gusts and 1 for start states, j the pair of normals within the row.  Of the four output
 * words w0..w3: u1 = ((w0 >> 5) 2^26 + (w1 >> 6) + 1) 2^-53 in (0, 1], t = ((w2 >> 5) 2^26 + (w3 >> 6)) 2^-53 in [0, 1),
 * r = sqrt(-2 log u1), z0 = r cos(2 pi t), z1 = r sin(2 pi t).  A draw depends on (seed, b0 + b, s0 + s, i, stream, j) and on nothing
 * else -- not on B, S or what else is in the batch: a call at (b0, s0) for a sub-block writes the bits of that slice of the whole.
 *
 * qilqr_sample_gusts_device writes d_wrench, B x S x n_w x QILQR_WRENCH -- the wrench array of qilqr_closed_loop_scored_device -- all
 * n_w rows of it.  Component c of a flight is a stationary first-order Gauss-Markov process about mean[c] with deviation sigma[c] and
 * correlation time tau_force_s (c < 3) or tau_torque_s: with rho = tau > 0 ? exp(-dt / tau) : 0 (dt the handle's) and
 * kappa = sigma sqrt((1 - rho)(1 + rho)), computed on the host in double, and xi_i normal z(c % 2) of pair j = c / 2 of row i:
 *     g_0 = sigma xi_0,   g_i = fma(rho, g_{i-1}, kappa xi_i),   wrench[b, s, i, c] = mean + g_i
 * tau = 0 is white noise per step (mean + sigma xi_i); n_w = 1 is row 0 of any longer call.
 *
 * qilqr_sample_states_device writes d_x0, B x S x QILQR_STATE: x0[b, s] = x_nom[b] (+) delta with delta[c] = sigma12[c] xi_c over the 12
 * tangent words in the solver's order [rho, theta, dv, dw] (stream 1, row 0, pairs 0..5), (+) the solver's state addition: the pose
 * composed with Exp([rho; theta]) on the right, the two body velocities added.  d_x_nom is B x QILQR_STATE on the device, sigma12 12
 * doubles on the host.  flags bit 0: sample s0 + s == 0 is x_nom[b] itself, word for word (an undisturbed baseline in every batch).
 *
 * qilqr_reduce_scores_device reads d_score, B x S x QILQR_CL_SCORE as the scored flight writes it, and writes d_summary,
 * B x QILQR_MC_SUMMARY:
 *     0  the mean cost over the samples whose cost is finite      4  the fraction of samples with knots_in_collision > 0
 *     1  the population standard deviation of those costs          5  the smallest min_clearance (+inf without spheres; a NaN is skipped)
 *     2  the largest finite cost                                   6  its sample, the smallest on ties; -1 if every one is +inf
 *     3  its sample, the smallest on ties; -1 if none              7  the fraction of samples whose cost is not finite (diverged flights)
 * Words 0 .. 2 are NaN when no cost is finite.  One wavefront reduces a plan: lane l folds samples l, l + 64, ... in order, the lanes
 * are combined by the tree 32, 16, 8, 4, 2, 1, and the deviation is a second pass about the mean: a plan's bits depend on its S rows only.
 *
 * All three ENQUEUE on the handle's stream and do not drain it, with the ordering rules of qilqr_closed_loop_device, and need the
 * handle for its stream, its device and its dt only: every precision mode is accepted.  QILQR_ERR_INVALID_ARG, before the device is
 * touched, for a NULL pointer or model, a non-positive B, S or n_w, a negative b0 or s0, a device array off a 16-byte boundary, a
 * negative or non-finite sigma or tau, a non-finite mean, unknown flag bits, d_x0 overlapping d_x_nom, d_summary overlapping d_score,
 * and -- last -- a NULL handle. */
#define QILQR_MC_SUMMARY 8
typedef struct {
  double mean[6];      /* N, N, N (world frame), N m, N m, N m (body frame) */
  double sigma[6];     /* the stationary standard deviations */
  double tau_force_s;  /* the correlation time of the three forces; 0: white noise per step */
  double tau_torque_s; /* ... of the three torques */
} qilqr_gust_model;
int qilqr_sample_gusts_device(qilqr_solver *s, const qilqr_gust_model *m, uint64_t seed, int32_t B, int32_t S, int32_t n_w, int32_t b0,
                              int32_t s0, double *d_wrench);
int qilqr_sample_states_device(qilqr_solver *s, const double *d_x_nom, const double *sigma12, uint64_t seed, int32_t B, int32_t S,
                               int32_t b0, int32_t s0, uint32_t flags, double *d_x0);
int qilqr_reduce_scores_device(qilqr_solver *s, const double *d_score, int32_t B, int32_t S, double *d_summary);

/* Risk measures per plan and the choice among candidate plans, on the device (extension): what follows the reduction on the handle's
 * stream when the caller asks for tail measures instead of a mean, and for the decision the samples were flown for.  Device arrays
 * only; sharded handles have no such call (use a shard's solver).
 *
 * qilqr_risk_scores_device reads d_score, B x S x QILQR_CL_SCORE as the scored flight writes it, and writes d_risk,
 * B x n_levels x QILQR_MC_RISK; levels is a host array of n_levels doubles in [0, 1).  The key of sample j of plan b is
 *     score[b, j, 0]    for column QILQR_RISK_COST,         -score[b, j, 1]    for column QILQR_RISK_CLEARANCE
 * so that the bad end is always the upper tail, and a NaN key counts as +inf: a diverged flight is the worst outcome here, NOT a
 * skipped one as in word 0 of the summary.  The samples are ordered by (key, j), the sample index breaking ties.  Per level the host
 * computes the rank in double, k = min(S - 1, max(0, ceil(level S) - 1)), and m = S - k; with t_0 <= ... <= t_(m-1) the keys at
 * sorted positions k ... S - 1 the words are
 *     0  t_0, the order statistic: the cost that a fraction `level` of the flights stay under (VaR); clearance column: -t_0, the
 *        clearance that all but the worst m flights keep
 *     1  (sum t_i) / m, the mean of the tail (CVaR); clearance column: -(sum t_i) / m, the mean of the m smallest clearances
 *     2  the sample at sorted position k (the smaller index on equal keys)
 *     3  m
 * The order of the sum: lane l of one wavefront folds t_l, t_(l+64), ... in that order, and the lanes are combined by the butterfly
 * 32, 16, 8, 4, 2, 1 with IEEE additions, as qilqr_reduce_scores_device combines its lanes; a tail that holds a +inf gives +inf.  The
 * sum runs over SORTED positions: words 0, 1 and 3 depend on the multiset of the plan's keys only -- permuting the samples changes no
 * bit of them -- and a plan's words depend neither on B nor on the other plans.  One block sorts a plan, so S is at most
 * QILQR_RISK_MAX_SAMPLES.
 *
 * qilqr_select_plans_device chooses among candidates.  The batch is V vehicles x C candidates, candidate-major: plan b = c V + v.
 * (The samplers' draws depend on (seed, b0 + b, s0 + s, ...): sampling each candidate's slice [c V, (c + 1) V) with b0 = 0 gives every
 * candidate of a vehicle the same start states and gusts -- common random numbers.)  d_summary is (C V) x QILQR_MC_SUMMARY from
 * qilqr_reduce_scores_device, d_risk (C V) x n_levels x QILQR_MC_RISK on the cost column (it may be NULL for objectives 0 and 1).  A
 * candidate is feasible when summary[4] <= max_collision_fraction, summary[7] <= max_diverged_fraction, summary[5] >= min_clearance
 * and its objective is not NaN.  The choice is the feasible candidate with the smallest (objective, c); without a feasible one, the
 * smallest (collision fraction, diverged fraction, objective with NaN as +inf, c).  d_choice[v] = c, and d_info[v], QILQR_SELECT_INFO
 * words: the chosen objective, the number of feasible candidates, the chosen collision fraction, 1.0 if the fallback chose (else 0.0).
 * Every comparison is exact.  The gather is optional -- d_plan (C V x n x 18), d_gains (C V x n x 52), d_out_plan (V x n x 18) and
 * d_out_gains (V x n x 52) are given all together or not at all: a second launch on the same stream that reads d_choice from device
 * memory and copies the chosen plan and its gains word for word.
 *
 * Both ENQUEUE on the handle's stream and do not drain it, with the ordering rules of qilqr_closed_loop_device, and need the handle
 * for its stream and its device only: every precision mode is accepted.  QILQR_ERR_INVALID_ARG, before the device is touched, in this
 * order.  Risk: a NULL d_score, levels or d_risk; a non-positive B or S; S above QILQR_RISK_MAX_SAMPLES; an unknown column; n_levels
 * outside 1 ... QILQR_RISK_MAX_LEVELS; a level that is NaN or outside [0, 1); an array off a 16-byte boundary; d_risk overlapping
 * d_score.  Selection: a NULL d_summary, rule, d_choice or d_info; a non-positive V or C; an objective outside 0 ... 3 or, for
 * objectives 2 and 3, n_levels or the level out of range; d_risk NULL for objective 2 or 3; a NaN threshold; an array off a 16-byte
 * boundary; a partial set of gather pointers, or a non-positive n with a full set; an output overlapping an input or another output.
 * Last, for both, a NULL handle. */
#define QILQR_MC_RISK 4
#define QILQR_RISK_MAX_LEVELS 8
#define QILQR_RISK_MAX_SAMPLES 4096
#define QILQR_RISK_COST 0
#define QILQR_RISK_CLEARANCE 1
int qilqr_risk_scores_device(qilqr_solver *s, const double *d_score, int32_t B, int32_t S, int32_t column, const double *levels,
                             int32_t n_levels, double *d_risk);
#define QILQR_SELECT_INFO 4
typedef struct {
  int32_t objective;             /* 0: summary word 0 (mean cost); 1: summary word 2 (worst finite cost); 2: risk word 0; 3: risk word 1 */
  int32_t level;                 /* which of the risk array's levels (objectives 2 and 3) */
  double max_collision_fraction; /* feasible: summary[4] <= this */
  double max_diverged_fraction;  /* feasible: summary[7] <= this */
  double min_clearance;          /* feasible: summary[5] >= this; -inf asks nothing */
} qilqr_select_rule;
int qilqr_select_plans_device(qilqr_solver *s, const double *d_summary, const double *d_risk, int32_t n_levels,
                              const qilqr_select_rule *rule, int32_t V, int32_t C, int32_t *d_choice, double *d_info,
                              const double *d_plan, const double *d_gains, int32_t n, double *d_out_plan, double *d_out_gains);

/* A sampling planner on the device (extension; MPPI / path-integral control): the Monte-Carlo loop's generator, flight and score turned
 * on the plan's controls, and the samples fed back into the plan.  Device arrays only; sharded handles have no such call.
 *
 * qilqr_mppi_flight_device flies S control-perturbed copies of each of B plans OPEN LOOP and writes d_score, B x S x QILQR_CL_SCORE --
 * the layout of the scored closed-loop flight, so qilqr_reduce_scores_device and qilqr_risk_scores_device work on it unchanged.  Sample
 * (b, j) starts at d_x0[b] (QILQR_STATE words; d_x0 NULL: words 1..13 of knot 0 of plan b) and at knots i = 0 .. n - 1 applies
 *     u_i = d_plan[b, i, 14:18] + eps_i,   clamped to the thrust limits while they are set (the clamped control is scored and stepped with)
 * where eps_i[a], rotor a, is the recursion of qilqr_sample_gusts_device per rotor -- g_0 = sigma[a] xi_0, g_i = fma(rho, g_{i-1},
 * kappa_a xi_i) with rho = tau_s > 0 ? exp(-dt / tau_s) : 0 and kappa_a = sigma[a] sqrt((1 - rho)(1 + rho)) -- over the normals of draw
 * (seed; b0 + b, j, row i, stream 2, pair a / 2), normal a % 2.  With QILQR_MPPI_FIRST_IS_NOMINAL sample 0 flies eps = 0.  A knot is
 * scored as qilqr_closed_loop_scored scores it (the handle's Q or schedule from its horizon start, R, d_desired -- B x n x 18, one per
 * plan -- or the handle's desired trajectory, the shared and the per-problem spheres), and stepped with the handle's integrator and,
 * while per-problem models are set (for B problems), the model of plan b.  No perturbation is ever stored: it is a function of its indices.
 *
 * qilqr_mppi_update_device moves each plan's controls to the weighted mean perturbation and leaves a consistent trajectory in
 * d_out_plan, B x n x 18.  With J_j = cost_j + collision_cost hits_j (words 0 and 3 of d_score[b, j]; a key that is not finite has
 * weight 0), J_min the smallest finite key (the smaller j on ties) and w_j = exp(-(J_j - J_min) / lambda):
 *     eta = sum_j w_j,    du_i[a] = (sum_j w_j eps_j,i[a]) / eta,    u_i[a] = clamp(d_plan[b, i, 14 + a] + du_i[a])
 * with eps REDRAWN from the same indices (as drawn, not as clamped; rule, seed, S and b0 must be the flight's).  Without a finite key the
 * controls are the plan's, bit for bit.  Every sum has one order: with T the power of two >= S (64 at the least, 1024 at the most) lane
 * t folds samples t, t + T, ... in that order, the 64 lanes of a wavefront combine by the butterfly 32, 16, 8, 4, 2, 1, the wavefronts in
 * index order; a term w_j eps is rounded before it is added.  A plan's bits depend on neither B nor its neighbours.  A second launch
 * flies the new controls from x0 with eps = 0, writes the flown states into d_out_plan -- a valid initial trajectory for
 * qilqr_solve_batch_device -- and scores that flight.  d_info[b], QILQR_MPPI_INFO words:
 *     0  J_min (NaN without a finite key)          2  the effective sample size eta^2 / sum_j w_j^2 (0 without)
 *     1  the sample at J_min (-1 without)          3  the number of finite keys          4 .. 7  the four score words of the new plan
 *
 * Both ENQUEUE on the handle's stream and do not drain it, with the ordering rules of qilqr_closed_loop_device.
 * QILQR_ERR_INVALID_ARG, before the device is touched, in this order: a NULL rule, d_plan or d_score (the update: or d_out_plan, d_info);
 * B, n or S not positive, or n < 2; S above QILQR_RISK_MAX_SAMPLES; a negative b0; a sigma that is NaN or negative; lambda not > 0;
 * a tau_s or collision_cost that is NaN or negative; unknown flag bits or reserved != 0; an array off a 16-byte boundary; the flight's
 * d_score or the update's d_out_plan overlapping an input; d_info overlapping anything; a NULL handle; then, as the scored closed-loop
 * flight, a handle in a mixed-precision mode, per-problem models or spheres set for another B, and (QILQR_ERR_LENGTH_MISMATCH) knots
 * beyond the handle's desired trajectory or schedule. */
#define QILQR_MPPI_INFO 8
#define QILQR_MPPI_FIRST_IS_NOMINAL 1u
typedef struct {
  double   sigma[4];        /* N per rotor: deviation of the control perturbation, >= 0 */
  double   tau_s;           /* correlation time along the horizon; 0: white (as qilqr_gust_model) */
  double   lambda;          /* temperature of the weights, > 0 */
  double   collision_cost;  /* added to a sample's key per knot in collision, >= 0 */
  uint32_t flags;           /* QILQR_MPPI_FIRST_IS_NOMINAL = 1: sample 0 flies eps = 0 */
  uint32_t reserved;        /* 0 */
} qilqr_mppi_rule;          /* 64 bytes */
int qilqr_mppi_flight_device(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0,
                             const double *d_desired, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_score);
int qilqr_mppi_update_device(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0,
                             const double *d_desired, const double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0,
                             double *d_out_plan, double *d_info);

/* The planner's spread per plan, knot and rotor, adapted on the device (extension; covariance adaptation of the MPPI / CEM family, the
 * diagonal only).  A SPREAD is a device array d_spread, B x n x 4 doubles: the deviation, N, of the perturbation of plan b at knot i,
 * rotor a.  A caller initialises it (from rule->sigma, say); rule->sigma is checked as before and NOT read for the draws.
 *
 * qilqr_mppi_flight_spread_device is qilqr_mppi_flight_device with
 *     eps_i[a] = d_spread[b, i, a] * z_i[a]   (a rounded product),   z the recursion above with sigma = {1, 1, 1, 1}:
 *     z_0 = xi_0,  z_i = fma(rho, z_{i-1}, kappa1 xi_i),  kappa1 = sqrt((1 - rho)(1 + rho))
 * over the same draws.  With tau_s = 0 and d_spread[b, i, a] = sigma[a] everywhere d_score has the bits of qilqr_mppi_flight_device.
 *
 * qilqr_mppi_adapt_device is qilqr_mppi_update_device (the same keys, weights, eta, fold orders, d_out_plan and d_info, the same second
 * launch) over those perturbations, and also writes d_out_spread, B x n x 4 (NULL: the mean only).  Per knot and rotor, with the sums
 * in the update's order and every product rounded before it is added:
 *     m1 = sum_j w_j eps,   m2 = sum_j (w_j eps) eps,   du = m1 / eta,   var = m2 / eta - du du   (not > 0: 0)
 *     v = (1 - rate) s_old^2 + rate var,   s_new = sqrt(v) clamped to [floor[a], cap[a]]
 * Without a finite key controls and spread are the inputs', bit for bit.  The call does not work in place.  Nothing is checked on the
 * device: a NaN spread gives NaN controls, a NaN cost and weight 0.
 *
 * Both ENQUEUE on the handle's stream and do not drain it.  QILQR_ERR_INVALID_ARG: what the two calls above refuse of the common
 * arguments, in their order and before the handle is looked at; then a NULL d_spread (the adaptation: or a NULL adapt); a floor that is
 * NaN or negative; a cap that is NaN, infinite or below its floor; a rate not in (0, 1]; a nonzero reserved word; d_spread or
 * d_out_spread off a 16-byte boundary; d_out_spread overlapping an input (d_spread among them), d_out_plan or d_info; the flight's
 * d_score or the adaptation's d_out_plan or d_info overlapping d_spread; then the NULL handle and the handle's reasons as above. */
typedef struct {
  double floor[4];     /* N per rotor: the smallest deviation a new spread may have, >= 0 */
  double cap[4];       /* the largest; finite, >= floor */
  double rate;         /* in (0, 1]: new variance = (1 - rate) old + rate weighted */
  double reserved[3];  /* 0 */
} qilqr_mppi_adapt_rule;   /* 96 bytes */
int qilqr_mppi_flight_spread_device(qilqr_solver *s, const qilqr_mppi_rule *rule, uint64_t seed, const double *d_plan, const double *d_x0,
                                    const double *d_desired, const double *d_spread, int32_t B, int32_t n, int32_t S, int32_t b0,
                                    double *d_score);
int qilqr_mppi_adapt_device(qilqr_solver *s, const qilqr_mppi_rule *rule, const qilqr_mppi_adapt_rule *adapt, uint64_t seed,
                            const double *d_plan, const double *d_x0, const double *d_desired, const double *d_spread,
                            const double *d_score, int32_t B, int32_t n, int32_t S, int32_t b0, double *d_out_plan,
                            double *d_out_spread, double *d_info);

/* Linear covariance analysis of a plan's closed loop on the device (extension): how far the flights of qilqr_closed_loop_scored_device
 * stray from a plan under a gust model and an uncertain start, to first order and without a sample.  Device arrays only; sharded handles
 * have no such call (use a shard's solver).
 *
 * About a dynamically consistent plan the deviation dx_i = x_i (-) plan_i (the solver's tangent order [rho, theta, dv, dw]) of the law
 * u = u_i + K_i dx obeys dx_{i+1} = F_i dx_i + G_i w_i for plan b over knots i0 .. i1, with F_i = A_i + B_i K_i:
 *   - A_i, B_i are the Jacobians of the handle's step (its integrator, qilqr_set_integrator) at plan[b, i], with the model of problem b
 *     while per-problem models are set for B;
 *   - K_i is words 4..51 of d_gains[b, i], as the closed loop reads them; d_gains == NULL is the open loop, F_i = A_i;
 *   - w_i is the wrench {F world frame, tau body frame} held over the step, and G_i (12 x 6) the step's Jacobian with respect to it.
 *     Explicit Euler, exact: rows 6..8, columns 0..2 are dt R(q_i)^T / mass; rows 9..11, columns 3..5 are dt I^-1; zero elsewhere.
 *     Runge-Kutta: the six wrench columns carried through the four stages.
 * With S_g = diag(sigma_c^2) of rule->gust and rho_c = tau > 0 ? exp(-dt / tau) : 0 (qilqr_sample_gusts_device's, on the host in double):
 *     Sigma_{i0} = diag(state_sigma^2)     C_{i0} = 0 (12 x 6)     m_{i0} = 0
 *     Sigma_{i+1} = F Sigma F^T + F C G^T + G C^T F^T + G S_g G^T
 *     C_{i+1}     = (F C + G S_g) diag(rho)          (rho = 0: white noise, C stays 0)
 *     m_{i+1}     = F m_i + G mean
 * QILQR_COV_WRENCH_HELD (rule->flags) is the n_w = 1 case, one wrench per flight: rho = 1 in the C recursion.
 * IGNORED: the thrust limits (the clamp is not linear), the state-weight schedule, the desired trajectory, and the horizon start (sphere
 * j of the plan's own table stands at c + i dt v at knot i of the call, as the scored flight places it).
 *
 * Any output may be NULL, but not all of them.
 *   d_cov      B x n x QILQR_COV: Sigma_i row-major for i0 <= i <= i1; other knots are left untouched.  Exactly symmetric: entry (k, l)
 *              with k <= l is mirrored, so cov[k][l] and cov[l][k] have the same bits.
 *   d_mean     B x n x 12: m_i, likewise.
 *   d_summary  B x QILQR_COV_SUMMARY, with P_i = Sigma_i[0:3, 0:3]:
 *     0  max_i sqrt(tr P_i), m                      4  the smallest z = (|d| - radius_j) / sqrt(n^T P_i n) over the knots and every
 *     1  its knot, the first on ties                   sphere of both tables (the shared one first, then row b of the per-problem table):
 *     2  sqrt(tr P_i1)                                 d = p_i + R_i m_i[0:3] - c_j(i), n = R_i^T d / |d| (the tangent's first three
 *     3  max_i sqrt(tr Sigma_i[3:6, 3:6]), rad         words are body-frame); +inf without spheres; taken by z < best: never a NaN
 *     7  max over i and rotor a of                  5  its knot (-1: none was taken)
 *        sqrt(K_a Sigma_i K_a^T), N; 0 in the       6  its sphere: j, or shared_count + j for the plan's own table; -1: none
 *        open loop
 *
 * ENQUEUES on the handle's stream (three launches: the knots' F and G, the chain over the knots, the summary) and does not drain it, with
 * the ordering rules of qilqr_closed_loop_device; scratch the handle owns grows at the call that needs more.  QILQR_ERR_INVALID_ARG,
 * before the device is touched, in this order: a NULL rule or d_plan; every output NULL; a non-positive B or n; knots not
 * 0 <= i0 <= i1 <= n - 1; a negative or non-finite sigma or tau; a non-finite mean; unknown flag bits or reserved != 0; an array off a
 * 16-byte boundary; an output overlapping an input or another output; a NULL handle, a mixed-precision one; per-problem models or
 * per-problem spheres set for another B. */
#define QILQR_COV 144
#define QILQR_COV_SUMMARY 8
#define QILQR_COV_WRENCH_HELD 1u
typedef struct {
  double state_sigma[12];  /* the deviations of the start state at knot i0 over the tangent [rho, theta, dv, dw] (qilqr_sample_states_device's sigma12) */
  qilqr_gust_model gust;   /* mean, sigma and correlation times of the wrench */
  uint32_t flags;          /* QILQR_COV_WRENCH_HELD, or 0 */
  uint32_t reserved;       /* 0 */
} qilqr_cov_rule;          /* 216 bytes */
int qilqr_covariance_device(qilqr_solver *s, const qilqr_cov_rule *rule, const double *d_plan, const double *d_gains, int32_t B, int32_t n,
                            int32_t i0, int32_t i1, double *d_cov, double *d_mean, double *d_summary);

/* The device-side twin of qilqr_set_batch_obstacles (extension): a per-problem sphere table that was MADE on the device -- by
 * qilqr_fleet_neighbours_device below, or by the caller's own kernels -- put into the handle without the host.  d_spheres is
 * B x K x QILQR_OBSTACLE_WORDS doubles in device memory, the host setter's layout; d_counts is int32[B] in device memory, or NULL for
 * all K; d_dropped is NULL or one int32 in device memory.
 * ENQUEUES on the handle's stream and returns; it is not waited for, as every _device call here (the ordering rules of
 * qilqr_closed_loop_device).  The handle's table and counts are kept and reused while they are large enough, and grow -- with one wait
 * for the stream -- at the call that needs more: a tick costs one small launch (k_bob_set; and a 4-byte memset for d_dropped) and no
 * allocation.  qilqr_set_batch_obstacles, the clear included, behaves as before and gives the memory back.
 * THE ROWS.  What the host setter refuses of the values cannot be looked at without a wait, so the kernel applies it as a rule: per
 * problem the count is clamped to 0 ... K; a used row with a non-finite word, radius <= 0 or weight < 0 is DROPPED; the rows kept stay
 * in order and move up, the count becomes the number kept, and the number of rows dropped over the batch goes to *d_dropped.  The table
 * is written in the tiled device layout with zeros in the rows at or beyond a count and in the padding of the last tile: for a table
 * whose used rows all pass (and whose other rows are zeros) its bytes are those the host setter uploads.
 * THE HANDLE is then in the state qilqr_set_batch_obstacles(B, K) leaves: the route, persistent = 1 refused, every call that evaluates
 * the cost refused for another B, scored flights, the planner and the covariance summary read the table as they read a host-set one.
 * The largest count and whether a sphere moves are unknown to the host: qilqr_describe says "set on the device" in their place.
 * QILQR_ERR_INVALID_ARG, before the device is touched, in this order: a NULL handle or d_spheres; B not positive; K outside
 * 1 ... QILQR_MAX_OBSTACLES; d_spheres off a 16-byte boundary, d_counts or d_dropped off a 4-byte one; a mixed-precision handle. */
int qilqr_set_batch_obstacles_device(qilqr_solver *s, const double *d_spheres, const int32_t *d_counts, int32_t B, int32_t K,
                                     int32_t *d_dropped);

/* Fleet deconfliction on the device (extension): who is near whom over the horizon, and each near partner as the moving sphere
 * qilqr_set_batch_obstacles[_device] takes.  Device arrays only; sharded handles have no such call (use a shard's solver).
 *
 * d_plan is B x n x 18: plans in ONE world frame on ONE time base -- knot i of every plan is the same instant t_i = i dt (dt the
 * handle's).  Rows b with equal b / V form a fleet (V divides B; V = B: one fleet), and only the vehicles of one fleet interact.
 * THE PAIR.  For ego a and partner b != a of its fleet, at knot i: e = p_a,i - p_b,i per axis (the position is words 1..3 of a knot)
 * and d2 = fma(ez, ez, fma(ey, ey, ex ex)); the pair's value is the smallest d2 over the knots, taken by strict < from +inf (the first
 * knot wins a tie; a comparison with a NaN is false), with its knot.  A pair without a finite d2 has d2 = +inf and knot -1 and is
 * never a neighbour.
 * THE LIST.  The candidates of ego a are its partners -- under QILQR_FLEET_YIELD_TO_LOWER only those in a smaller row (prioritised
 * planning: vehicle 0 of a fleet yields to nobody).  The list is the min(K, candidates) candidates smallest in the total order (d2,
 * partner row), in that order; it does not depend on how the kernels cut the partners into chunks.  K <= QILQR_FLEET_MAX_NEIGHBOURS.
 * The neighbours are the leading list entries with d2 < range^2 (the square rounded once; distances are compared as squares, with
 * `conflict` too).
 * THE LINE of a vehicle, once per vehicle, per axis, sequentially over the knots: pbar = (sum_i p_i) / n, tbar = (n - 1) dt / 2,
 * Stt = dt^2 n (n^2 - 1) / 12, v = (sum_i fma(t_i - tbar, p_i - pbar, .)) / Stt, c = fma(-tbar, v, pbar) (n = 1: v = 0, c = p_0), and
 * the residual max_i |p_i - fma(t_i, v, c)| (Euclidean; NaN for a line with a word that is not finite).  fma(t_i, v, c) is where a
 * per-problem sphere {c, v} stands at knot i.
 *
 * Any output may be NULL, but not all of them; each has the bits it has among the others.
 *   d_nbr      B x K x QILQR_FLEET_NBR: per list entry {partner row in the batch, sqrt(d2), its knot, the partner's residual}; an empty
 *              entry is {-1, +inf, -1, 0}.
 *   d_spheres  B x K x QILQR_OBSTACLE_WORDS: per neighbour, in the list's order, {c, v, rule->radius (+ the partner's residual under
 *              QILQR_FLEET_COVER), rule->weight}.  A partner whose line is not finite becomes no sphere and is skipped; rows at and
 *              beyond the count are zeros.
 *   d_counts   int32[B]: the spheres written for row b.
 *   d_summary  B x QILQR_FLEET_SUMMARY, over ALL partners of the fleet, whatever the yield flag:
 *     0  the smallest distance (+inf: no partner at a finite one)     3  the partners with d2 < conflict^2
 *     1  its knot (-1: none)                                          4  d_counts[b]
 *     2  its partner's row (ties: the smaller row; -1: none)          5  the largest radius written (0: none)      6, 7  zero
 *
 * ENQUEUES three launches on the handle's stream (the lines and a staged copy of the positions; all pairs; the merge and the outputs)
 * and does not drain it, with the ordering rules of qilqr_closed_loop_device; scratch the handle owns grows at the call that needs
 * more.  QILQR_ERR_INVALID_ARG, before the device is touched, in this order: a NULL rule or d_plan; every output NULL; B, n or V not
 * positive, or V not dividing B; K outside 1 ... QILQR_FLEET_MAX_NEIGHBOURS; a rule field out of its range, unknown flag bits or
 * reserved != 0; an array off a 16-byte boundary (d_counts: 4-byte); an output overlapping the plan or another output; a NULL handle,
 * a mixed-precision one. */
#define QILQR_FLEET_MAX_NEIGHBOURS 16
#define QILQR_FLEET_NBR 4
#define QILQR_FLEET_SUMMARY 8
#define QILQR_FLEET_COVER 1u
#define QILQR_FLEET_YIELD_TO_LOWER 2u
typedef struct qilqr_fleet_rule {
  double radius;     /* centre-to-centre distance to keep: the radius of the sphere a neighbour becomes; finite, > 0 */
  double weight;     /* that sphere's weight; finite, >= 0 */
  double range;      /* a partner becomes a sphere only if its smallest distance over the horizon is < range; > 0, +inf allowed */
  double conflict;   /* partners whose smallest distance is < conflict are counted in the summary; finite, >= 0 */
  uint32_t flags;    /* QILQR_FLEET_COVER | QILQR_FLEET_YIELD_TO_LOWER */
  uint32_t reserved; /* 0 */
} qilqr_fleet_rule;  /* 40 bytes */
int qilqr_fleet_neighbours_device(qilqr_solver *s, const qilqr_fleet_rule *rule, const double *d_plan, int32_t B, int32_t n, int32_t V,
                                  int32_t K, double *d_summary, double *d_nbr, double *d_spheres, int32_t *d_counts);

/* device the solver is bound to, and the HIP stream it launches on (hipStream_t as void*) */
int qilqr_device(const qilqr_solver *s);
void *qilqr_stream(const qilqr_solver *s);
/* make the solver's stream wait (on the device) for a hipEvent_t recorded on another stream */
int qilqr_stream_wait_event(qilqr_solver *s, void *hip_event);

/* Pinned host memory for the buffers handed to the host-buffer entry points (qilqr_solve_batch copies with plain
 * hipMemcpy: direct DMA from / to pinned memory, HIP's chunked staging for pageable memory).  NULL on failure. */
void *qilqr_host_alloc(size_t bytes);
void qilqr_host_free(void *p);

/* ---- one batch over several devices, in ONE process (BASELINE.json configs[3]: independent problems, contiguous shards,
 * no exchange between them -- the reference has no counterpart: its ILQR object solves one problem on one core).
 * A sharded handle owns one qilqr_solver per entry of `devices` (an ordinal may repeat: two shards then overlap on that
 * device through two handles and two streams).  qilqr_solve_batch_sharded cuts the B problems into n_devices contiguous
 * shards in the order of `devices` -- B / n_devices each, the first B % n_devices one more (qilqr_shard_range; the rule of
 * quadrotorilqr_amd/sharding.py for the one-process-per-GPU deployment) -- and solves shard r on devices[r] from a host
 * thread of its own: its input slice goes to the device, its results come back into the caller's arrays at the shard's
 * offset (the "gather" is the copy back itself: ragged shards need no padding), the call returns when every shard has.
 * Arguments and results are those of qilqr_solve_batch.  Problem by problem they are bit-identical to a single-device solve
 * of the same batch WHEN SHARD AND WHOLE BATCH TAKE THE SAME ROLLOUT KERNEL.  The backward pass, the linearisation, the cost sums and
 * every decision are one arithmetic at every batch size (since round 6: tests/test_gpu_parity.py::
 * test_backward_pass_bits_do_not_depend_on_the_batch_size); what remains is the rollout: with single_wave_rollout = 0 a call with up to
 * 4096 trajectories in flight on its device takes k_rollout16 (sixteen lanes per trajectory) for every rollout and a larger one k_rollout3
 * (a lane per trajectory) for a trajectory's first 16 rollouts and k_rollout16 from the 17th on -- a rule in the call's side of 4096 and
 * the rollout's ordinal, which is the round number in every call, never in what else the batch holds --, the two kernels evaluate the
 * same formulas in different orders, and the same problem differs by about 1e-10 relative in its trajectory between, say, a batch of
 * 8192 and its eight shards of 1024 (a batch of 65536 and its shards of 8192 are on one side: the same bits) -- the exit path of a
 * problem that sits within rounding of a convergence threshold can differ with them.  Forcing one rollout kernel (single_wave_rollout = 2 or 3; QILQR_PIN_ARITHMETIC below) makes a problem's bits
 * independent of how the caller batches or shards it.  A shard that fails makes the call return its error (the lowest failing shard's; text through
 * qilqr_last_error, prefixed with the shard and device); the other shards still complete. */
typedef struct qilqr_sharded qilqr_sharded;
/* dev: as for qilqr_create, its `device` field is ignored (NULL = defaults) */
int qilqr_sharded_create(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                         int32_t n_desired, double dt_s, const qilqr_options *options, const qilqr_device_config *dev,
                         const int32_t *devices, int32_t n_devices, qilqr_sharded **out);
int qilqr_sharded_create_sized(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                               int32_t n_desired, double dt_s, const qilqr_options *options, const qilqr_device_config *dev,
                               size_t dev_bytes, const int32_t *devices, int32_t n_devices, qilqr_sharded **out);
/* the same with the devices given as a bit mask (bit d = HIP device d), lowest ordinal first */
int qilqr_sharded_create_mask_sized(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                                    int32_t n_desired, double dt_s, const qilqr_options *options,
                                    const qilqr_device_config *dev, size_t dev_bytes, uint64_t device_mask, qilqr_sharded **out);
int qilqr_sharded_create_mask(const qilqr_model *model, const double *Q, const double *R, const double *desired,
                              int32_t n_desired, double dt_s, const qilqr_options *options,
                              const qilqr_device_config *dev, uint64_t device_mask, qilqr_sharded **out);
void qilqr_sharded_destroy(qilqr_sharded *h);
int32_t qilqr_sharded_count(const qilqr_sharded *h);
/* the solver of shard r (to set regularisation, read profiles or cost histories shard by shard); NULL if r is out of range */
qilqr_solver *qilqr_sharded_solver(qilqr_sharded *h, int32_t r);
/* problems [*begin, *begin + *count) of a batch of B belong to shard r of n_shards */
int qilqr_shard_range(int32_t B, int32_t n_shards, int32_t r, int32_t *begin, int32_t *count);
int qilqr_solve_batch_sharded(qilqr_sharded *h, const double *init, const double *desired_batch, int32_t B, int32_t n,
                              double *out_traj, double *out_cost, int32_t *out_status, int32_t *out_iters,
                              int32_t *out_n_bwd, int32_t *out_n_fwd);

/* The same batch solve with the results gathered in ONE device's memory (BASELINE.json configs[3]: "sharded ... with RCCL
 * gather over xGMI"; the C counterpart of quadrotorilqr_amd/sharding.gather_to_root for a host that drives every GPU from
 * one process).  Inputs are host arrays as for qilqr_solve_batch_sharded; d_out_* are device arrays on the device of shard
 * `root` (devices[root]), B x n x 18 doubles / B doubles / B int32, any of them may be NULL.  Every shard's rows travel from
 * its solver's staging buffers straight into their place in the root's arrays -- ragged shards, no padding, no second
 * copy -- as soon as that shard has finished, by the handle's transport:
 *   QILQR_TRANSPORT_RCCL       ncclSend on the shard's device / ncclRecv on the root's, ONE GROUP PER SHARD, issued by that
 *                              shard's own host thread when its solve has finished (a communicator executes in issue order:
 *                              the groups reach the root's in the order the shards finish, so a shard's rows travel while
 *                              slower shards still solve), over one communicator per distinct
 *                              device (ncclCommInitAll: all in this process); librccl.so.1 is loaded when the first
 *                              communicator is needed.  Exercised with ONE rank so far (every shard on the one GPU of the
 *                              test box: self send / receive); the multi-rank path has not run on hardware -- its schedule
 *                              (ranks, offsets, counts) is checked on the CPU through qilqr_gather_schedule
 *   QILQR_TRANSPORT_PEER_COPY  hipMemcpyPeerAsync
 *   QILQR_TRANSPORT_AUTO       (default) RCCL when the shards sit on more than one device, device copies when they all share
 *                              one; falls back to peer copies if RCCL cannot be loaded or initialised
 * qilqr_sharded_transport says in words which one a handle uses (and why, after a fallback); forcing _RCCL fails instead of
 * falling back.  gather_ms (may be NULL): the exposed part of the gather -- from the moment the slowest shard's solve has
 * finished to the moment the root holds every row.  Results are, problem by problem, those of qilqr_solve_batch. */
#define QILQR_TRANSPORT_AUTO 0
#define QILQR_TRANSPORT_RCCL 1
#define QILQR_TRANSPORT_PEER_COPY 2
int qilqr_sharded_set_transport(qilqr_sharded *h, int32_t transport);

/* qilqr_set_batch_models for a sharded handle: shard r's solver gets models[begin .. begin + count) (qilqr_shard_range of B), and the
 * sharded solves (qilqr_solve_batch_sharded, qilqr_solve_batch_sharded_device) refuse another B.  The models are checked for the whole
 * batch first (the index in an error is the batch's); a failure leaves every shard without models.  NULL, 0 clears them. */
int qilqr_sharded_set_batch_models(qilqr_sharded *h, const qilqr_model *models, int32_t B);

/* qilqr_set_obstacles on every shard's solver (the same spheres for the whole batch); checked once first, and a failure leaves
 * every shard without obstacles.  NULL, 0 clears them. */
int qilqr_sharded_set_obstacles(qilqr_sharded *h, const double *spheres, int32_t count);

/* qilqr_set_batch_obstacles for a sharded handle: shard r's solver gets rows [begin, begin + count) (qilqr_shard_range of B), and the
 * sharded solves refuse another B.  The whole batch is checked first (the index in an error is the batch's); a failure leaves every
 * shard cleared.  NULL, NULL, 0, 0 clears. */
int qilqr_sharded_set_batch_obstacles(qilqr_sharded *h, const double *spheres, const int32_t *counts, int32_t B, int32_t K);

/* qilqr_set_state_weight_schedule on every shard's solver (the same schedule for the whole batch); checked once first, and any failure
 * leaves every shard without a schedule -- but for a shard whose own setter refuses the clear (thrust limits set on that shard's solver
 * over a non-symmetric Q, which only a symmetric schedule makes possible): it keeps the schedule it had.  NULL, 0 clears it. */
int qilqr_sharded_set_state_weight_schedule(qilqr_sharded *h, const double *Qs, int32_t n_knots);

/* qilqr_set_horizon_start on every shard's solver (the same start for the whole batch); checked once first, all or none: a failure leaves
 * every shard at start 0. */
int qilqr_sharded_set_horizon_start(qilqr_sharded *h, int32_t k0);
const char *qilqr_sharded_transport(qilqr_sharded *h);
int qilqr_solve_batch_sharded_device(qilqr_sharded *h, const double *init, const double *desired_batch, int32_t B, int32_t n,
                                     int32_t root, double *d_out_traj, double *d_out_cost, int32_t *d_out_status,
                                     int32_t *d_out_iters, int32_t *d_out_n_bwd, int32_t *d_out_n_fwd, double *gather_ms);

/* The transfers qilqr_solve_batch_sharded_device issues for a batch of B problems of n knots over n_shards shards on `devices`
 * (HIP ordinals; equal ordinals share a communicator rank, ranks numbered in order of first appearance), gathered on shard
 * `root`'s device -- computed, not issued: no device is touched, so a host without eight GPUs can check the schedule of eight.
 * arrays: bit mask of the outputs asked for (1 traj, 2 cost, 4 status, 8 iters, 16 n_bwd, 32 n_fwd).  out receives 7 int64 per
 * transfer, {shard, array (0 traj .. 5 n_fwd), src_rank, dst_rank, src_off, dst_off, count} -- offsets and counts in elements
 * of the array's type; src_off into the shard's staging buffer (the four int32 arrays sit one behind the other there), dst_off
 * into the root's array -- shard by shard in the order a shard enqueues them (at run time each shard's transfers are ONE
 * ncclGroup of send / receive pairs, or peer copies, enqueued by the shard's own host thread behind its solve).  Returns the
 * number of transfers (at most `cap` are written; out may be NULL), -1 on bad arguments. */
int qilqr_gather_schedule(int32_t B, int32_t n, const int32_t *devices, int32_t n_shards, int32_t root, uint32_t arrays,
                          int64_t *out, int32_t cap);

/* trajectories moved by the compaction (qilqr_device_config.compaction) in the last batch solve of this handle; 0 when it was
 * off for that call.  Waits for the handle's stream. */
int qilqr_compaction_moves(qilqr_solver *s, int64_t *moves);

/* k_round launches of this handle per instantiation k_round<LK, ROUNDS, SIX>, since the handle was created or since
 * qilqr_profile_reset: counted on the host where a launch is enqueued, whatever qilqr_device_config.profile is (nothing is waited for).
 * counts[5 * (LK - 1) + j]: LK the record kind of the cost half -- 1 dense symmetric Q with a non-zero pose x velocity block, 2
 * symmetric Q with that block exactly zero, 3 diagonal Q -- and j = 0..4 for (ROUNDS, SIX) = (1, no), (1, yes), (2, no), (4, no),
 * (4, yes): rounds in the launch, and whether its backward pass takes the six-wavefront form. */
#define QILQR_ROUND_KERNELS 15
int qilqr_round_launches(qilqr_solver *s, int32_t counts[15]);

/* In words, which arithmetic and which kernels a batch solve of B problems on this handle uses: the reference's own forms or the
 * symmetric-weight forms (the choice is made by whether Q and R are bit-exactly symmetric and by force_general: see
 * qilqr_device_config.force_general), the integrator, the precision, the backward and rollout kernels, how a round is launched,
 * sub-batch streams, compaction.  buf receives a NUL-terminated text of at most cap - 1 characters. */
int qilqr_describe(qilqr_solver *s, int32_t B, char *buf, size_t cap);

/* ABI version of this header: 7 (qilqr_device_config grew by round_launch, rounds_per_launch, fuse_in_flight, dense_weights -- the
 * switches that were environment variables -- and the *_sized entry points carry the caller's structure size; version 6 added
 * `compaction`).  qilqr_set_control_limits, QILQR_STATUS_QP_FAILED, qilqr_set_batch_models, qilqr_sharded_set_batch_models,
 * qilqr_set_obstacles, qilqr_sharded_set_obstacles, QILQR_MAX_OBSTACLES, qilqr_set_batch_obstacles, qilqr_sharded_set_batch_obstacles,
 * QILQR_OBSTACLE_WORDS, qilqr_set_state_weight_schedule, qilqr_sharded_set_state_weight_schedule, qilqr_set_horizon_start,
 * qilqr_sharded_set_horizon_start, qilqr_shift_batch, qilqr_shift_batch_device, QILQR_STATE, QILQR_TAIL_HOLD, QILQR_TAIL_HOVER,
 * qilqr_backwards_pass_device, qilqr_closed_loop, qilqr_closed_loop_device, QILQR_CL_STATS, qilqr_closed_loop_scored,
 * qilqr_closed_loop_scored_device, QILQR_WRENCH, QILQR_CL_SCORE, qilqr_sample_gusts_device, qilqr_sample_states_device,
 * qilqr_reduce_scores_device, qilqr_gust_model, QILQR_MC_SUMMARY, qilqr_risk_scores_device, qilqr_select_plans_device,
 * qilqr_select_rule, QILQR_MC_RISK, QILQR_RISK_MAX_LEVELS, QILQR_RISK_MAX_SAMPLES, QILQR_RISK_COST, QILQR_RISK_CLEARANCE,
 * QILQR_SELECT_INFO, qilqr_mppi_flight_device, qilqr_mppi_update_device, qilqr_mppi_rule, QILQR_MPPI_INFO,
 * QILQR_MPPI_FIRST_IS_NOMINAL, qilqr_mppi_flight_spread_device, qilqr_mppi_adapt_device, qilqr_mppi_adapt_rule, qilqr_covariance_device,
 * qilqr_cov_rule, QILQR_COV, QILQR_COV_SUMMARY, QILQR_COV_WRENCH_HELD, qilqr_round_launches, QILQR_ROUND_KERNELS,
 * qilqr_set_batch_obstacles_device, qilqr_fleet_neighbours_device, qilqr_fleet_rule, QILQR_FLEET_MAX_NEIGHBOURS, QILQR_FLEET_NBR,
 * QILQR_FLEET_SUMMARY, QILQR_FLEET_COVER and QILQR_FLEET_YIELD_TO_LOWER were added within version 7: no structure changed. */
#define QILQR_ABI_VERSION 7
int qilqr_abi_version(void);

#ifdef __cplusplus
}
#endif

/* In source code compiled against this header the create calls pass the size of the structure they were compiled with. */
#ifndef QILQR_NO_SIZED_MACROS
#define qilqr_create(model, Q, R, desired, n_desired, dt_s, options, dev, out) \
  qilqr_create_sized(model, Q, R, desired, n_desired, dt_s, options, dev, sizeof(qilqr_device_config), out)
#define qilqr_sharded_create(model, Q, R, desired, n_desired, dt_s, options, dev, devices, n_devices, out) \
  qilqr_sharded_create_sized(model, Q, R, desired, n_desired, dt_s, options, dev, sizeof(qilqr_device_config), devices, n_devices, out)
#define qilqr_sharded_create_mask(model, Q, R, desired, n_desired, dt_s, options, dev, device_mask, out) \
  qilqr_sharded_create_mask_sized(model, Q, R, desired, n_desired, dt_s, options, dev, sizeof(qilqr_device_config), device_mask, out)
#endif
#endif
