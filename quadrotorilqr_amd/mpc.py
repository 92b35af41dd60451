"""Receding-horizon control on device buffers: at every tick the last plan is shifted on the device (QuadrotorILQRBatch.shift_device:
the flown knots dropped, the horizon's end extended by dynamics steps, knot 0 anchored at the measured state), the handle's horizon
start advanced along its desired trajectory and schedule (set_horizon_start), and the shifted plan solved again as a warm start
(solve_batch_device).  Nothing but the measured states goes through the host.

    rh = RecedingHorizon(solver, B, n)
    first = rh.start(init)                      # a plain solve
    while flying:
        res = rh.tick(x0)                       # x0: (B, 13) measured states, words 1..13 of a knot
        apply(res["u0"])                        # (B, 4) first controls, a view of the plan on the device

Between two ticks the plan can be flown closed loop: tick(x0, gains=True) also leaves the feedback gains about the new plan on the device
(QuadrotorILQRBatch.backwards_pass_device), and control(x, i) evaluates the law u = u_i + K_i (x (-) plan_i) at measured states
(closed_loop_device with one sample per plan and i0 = i1 = i); evaluate(x0, wrench) flies S sampled states per plan under that law -- and
under sampled disturbances -- and returns the statistics and the score of every flight (closed_loop_device with out_score), on device
buffers.  Ahead of a solve, start / tick(..., explore=dict(S=, seed=, sigma=, lambda_=)) runs rounds of the sampling planner on the
shifted plan (mppi_flight_device, mppi_update_device): the solve then polishes what the samples found.  With one more key,
adapt=dict(rate=, floor=, cap=), the planner's spread is kept per plan, knot and rotor in `self.spread` (B, n, 4), adapted by every round
(mppi_flight_spread_device, mppi_adapt_device) and shifted along the horizon with the plan.  With deconflict=dict(radius=, weight=, K=, ...) the B plans are vehicles that share
airspace: before its solve every vehicle gets its nearest partners' last plans as moving spheres (fleet_neighbours_device,
set_batch_obstacles_device), on the device.
"""
import numpy as np

from . import capi


class RecedingHorizon:
    """B problems of n knots on `solver` (a QuadrotorILQRBatch whose desired trajectory covers the mission).  Owns two device
    trajectory buffers, used alternately (the shift does not work in place), and the result arrays of the solves."""

    def __init__(self, solver, B, n):
        import torch
        self.solver, self.B, self.n = solver, int(B), int(n)
        self.device = torch.device("cuda", capi.load().qilqr_device(solver._h))
        # the solver's own stream as torch sees it: what reads a buffer between the shift and the solve is ordered behind it (_solve)
        self._stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(solver._h), device=self.device)
        self._buf = [torch.zeros((self.B, self.n, capi.KNOT), dtype=torch.float64, device=self.device) for _ in range(2)]
        self._x0 = torch.zeros((self.B, capi.STATE), dtype=torch.float64, device=self.device)
        self.cost = torch.zeros(self.B, dtype=torch.float64, device=self.device)
        self.status, self.iters, self.n_bwd, self.n_fwd = (torch.zeros(self.B, dtype=torch.int32, device=self.device) for _ in range(4))
        self._cur = 0
        self.k0 = 0        # the horizon start of the last solve
        self.init = None   # a copy of the initial trajectory of the last solve, when it was asked for (keep_init)
        # the feedback law of the last plan: allocated by the first start / tick that asks for gains, and by the first control()
        self.gains = self.terms = None   # (B, n, 52), (B, 2): about the plan of the last solve while _have_gains
        self._have_gains = False
        self._xc = self._ctl = None      # control()'s states (B, 1, 13) and the knots it writes (B, 1, n, 18)
        self._eval = None                # evaluate()'s buffers for the last S: (S, n_w, x0, wrench, stats, score)
        self._cov = None                 # evaluate_covariance()'s: [summary, cov or None]
        self._mc = None                  # evaluate_sampled()'s for the last (S, n_w): (S, n_w, x_nom, x0, wrench, stats, score, summary)
        self.sampled = None              # ... and what its last call sampled: (x0 (B, S, 13), wrench (B, S, n_w, 6) or None), its buffers
        self._risk = None                # evaluate_sampled()'s risk array (B, L, 4) for the last L
        self._last = None                # what select() works on: (summary, risk or None, its column) of the last evaluate_sampled()
        self._pad = None                 # evaluate_sampled()'s copies with padded candidates: (C, S, x_nom (C, V + 1, 13), x0 (C, V S + 1, 13) or None)
        self._sel = None                 # select()'s outputs for the last C: (C, choice, info, plan, gains)
        self._mppi = None                # _explore()'s buffers for the last S: (S, a scratch plan (B, n, 18), score (B, S, 4), info (B, 8))
        self.spread = None               # the planner's spread (B, n, 4) while explore carries `adapt`: what the last round left
        self._spread_scratch = None      # ... and the buffer the next round writes
        self._held = None                # the shifted spread of a tick that was refused
        self._fleet = None               # _deconflict()'s buffers for the last K: (K, summary (B, 8), nbr (B, K, 4), spheres (B, K, 8), counts (B), dropped (1))

    def _to_device(self, a, dst):
        import torch
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        if tuple(a.shape) != tuple(dst.shape):
            raise TypeError(f"expected shape {tuple(dst.shape)}, not {tuple(a.shape)}")
        dst.copy_(a)  # (on torch's current stream; the solver's stream is ordered behind it by the calls below)
        return dst

    def _solve(self, keep_init, gains=False):
        import torch
        buf = self._buf[self._cur]
        self.init = None
        if keep_init:
            # The shift that wrote `buf` was enqueued on the solver's stream and not waited for, and the solver's stream (non-blocking) is
            # ordered with no other: torch's stream waits for an event recorded behind the shift before the copy reads the buffer.  The
            # solve below is then ordered behind the copy (solve_batch_device makes the solver's stream wait for torch's).
            torch.cuda.current_stream(self.device).wait_event(self._stream.record_event())
            self.init = buf.clone()
        self.solver.solve_batch_device(buf, buf, self.cost, self.status, self.iters, self.n_bwd, self.n_fwd)  # (in place: drained on return)
        res = dict(u0=buf[:, 0, 14:18], traj=buf, cost=self.cost, status=self.status, iters=self.iters)
        self._have_gains = False
        if gains:
            # The gains a solve ends with belong to the iterate before its last accepted step: the law about the plan it returned is one
            # more backward pass on that plan (at the handle's current horizon start: the one the plan was solved at).
            if self.gains is None:
                self.gains = torch.zeros((self.B, self.n, capi.GAIN), dtype=torch.float64, device=self.device)
                self.terms = torch.zeros((self.B, 2), dtype=torch.float64, device=self.device)
            self.solver.backwards_pass_device(buf, self.gains, self.terms)  # (drained on return)
            self._have_gains = True
            res["gains"] = self.gains
        return res

    def _explore(self, explore, steps=None):
        """`iterations` rounds of the sampling planner on the plan in the current buffer, before its solve: S control-perturbed flights
        from the plan's knot 0 (QuadrotorILQRBatch.mppi_flight_device) and the plan moved to their weighted mean (mppi_update_device),
        out of the current buffer into a scratch buffer, which then becomes the current one.  Enqueued on the solver's stream, behind
        torch's current stream, and not waited for: the solve that follows is ordered behind it.  Returns the last round's info (B, 8).
        With explore["adapt"] a round is mppi_flight_spread_device and mppi_adapt_device over `self.spread`, which the round replaces;
        before the first round the spread is set to sigma (steps None: a start) or shifted `steps` knots with a tail of sigma (a tick), by
        torch on its current stream -- the first enqueue is ordered behind it."""
        import torch
        known = {"S", "seed", "sigma", "lambda_", "tau_s", "collision_cost", "iterations", "first_is_nominal", "adapt"}
        if not isinstance(explore, dict) or not {"S", "seed", "sigma", "lambda_"} <= set(explore) or set(explore) - known:
            raise TypeError("explore must be a dict with S, seed, sigma, lambda_ and optionally tau_s, collision_cost, iterations, first_is_nominal, adapt")
        S, rounds = int(explore["S"]), int(explore.get("iterations", 1))
        if S <= 0 or rounds <= 0:
            raise TypeError("explore: S and iterations must be positive")
        adapt = explore.get("adapt")
        if adapt is not None and (not isinstance(adapt, dict) or set(adapt) != {"rate", "floor", "cap"}):
            raise TypeError("explore: adapt must be a dict with rate, floor and cap")
        if self._mppi is None or self._mppi[0] != S:
            new = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)
            self._mppi = (S, new(self.B, self.n, capi.KNOT), new(self.B, S, capi.CL_SCORE), new(self.B, capi.MPPI_INFO))
        _, scratch, d_score, d_info = self._mppi
        kw = dict(tau_s=explore.get("tau_s", 0.0), collision_cost=explore.get("collision_cost", 0.0), first_is_nominal=explore.get("first_is_nominal", True))
        if adapt is None:
            self.spread = None  # (a later adaptation starts from sigma again)
        else:
            sig = np.atleast_1d(np.asarray(explore["sigma"], dtype=np.float64))
            if sig.shape not in ((1,), (4,)):
                raise TypeError("sigma must have 1 or 4 words")
            sig = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(sig, (4,)))).to(self.device)
            k = self.n if steps is None or self.spread is None else min(int(steps), self.n)
            # (a new tensor: the spread before this tick stays what it was, for a tick that is refused)
            self.spread = torch.cat([self.spread[:, k:], sig.expand(self.B, k, 4)], dim=1).contiguous() if k < self.n else sig.expand(self.B, self.n, 4).contiguous()
            if self._spread_scratch is None:
                self._spread_scratch = torch.zeros((self.B, self.n, 4), dtype=torch.float64, device=self.device)
        for r in range(rounds):
            src, seed = self._buf[self._cur], int(explore["seed"]) + r  # (a round's draws are its own)
            if adapt is None:
                self.solver.mppi_flight_device(src, d_score, seed, explore["sigma"], explore["lambda_"], wait_current_stream=r == 0, **kw)
                self.solver.mppi_update_device(src, d_score, scratch, d_info, seed, explore["sigma"], explore["lambda_"], wait_current_stream=False, **kw)
            else:
                self.solver.mppi_flight_spread_device(src, self.spread, d_score, seed, explore["sigma"], explore["lambda_"], wait_current_stream=r == 0, **kw)
                self.solver.mppi_adapt_device(src, self.spread, d_score, scratch, self._spread_scratch, d_info, seed, explore["sigma"], explore["lambda_"],
                                              adapt["floor"], adapt["cap"], adapt["rate"], wait_current_stream=False, **kw)
                self.spread, self._spread_scratch = self._spread_scratch, self.spread
            self._buf[self._cur], scratch = scratch, src
            self._mppi = (S, scratch, d_score, d_info)
        return d_info

    def _deconflict(self, deconflict):
        """The plans in the current buffer -- every vehicle's latest intent -- as each other's obstacles, before their solve: the
        neighbours of every vehicle as constant-velocity spheres (QuadrotorILQRBatch.fleet_neighbours_device) into buffers this object owns,
        and those as the handle's per-problem sphere table (set_batch_obstacles_device).  Both enqueued on the solver's stream, behind
        torch's current stream, and not waited for: the solve that follows is ordered behind them.  Returns (summary (B, 8), nbr (B, K, 4))."""
        import torch
        known = {"radius", "weight", "K", "fleet", "range", "conflict", "cover", "yield_to_lower"}
        if not isinstance(deconflict, dict) or not {"radius", "weight", "K"} <= set(deconflict) or set(deconflict) - known:
            raise TypeError("deconflict must be a dict with radius, weight, K and optionally fleet, range, conflict, cover, yield_to_lower")
        K = int(deconflict["K"])
        V = self.B if deconflict.get("fleet") is None else int(deconflict["fleet"])
        if K <= 0 or K > capi.FLEET_MAX_NEIGHBOURS:
            raise TypeError(f"deconflict: K must be 1 ... {capi.FLEET_MAX_NEIGHBOURS}")
        if V <= 0 or self.B % V:
            raise TypeError(f"deconflict: fleet must divide B = {self.B}")
        if self._fleet is None or self._fleet[0] != K:
            new = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device=self.device)
            self._fleet = (K, new(self.B, capi.FLEET_SUMMARY), new(self.B, K, capi.FLEET_NBR), new(self.B, K, 8), new(self.B, dtype=torch.int32),
                           new(1, dtype=torch.int32))
        _, d_sum, d_nbr, d_sph, d_cnt, d_drop = self._fleet
        self.solver.fleet_neighbours_device(self._buf[self._cur], V, K, deconflict["radius"], deconflict["weight"], range=deconflict.get("range", np.inf),
                                            conflict=deconflict.get("conflict"), cover=deconflict.get("cover", False),
                                            yield_to_lower=deconflict.get("yield_to_lower", False), summary=d_sum, nbr=d_nbr, spheres=d_sph, counts=d_cnt)
        self.solver.set_batch_obstacles_device(d_sph, d_cnt, d_drop, wait_current_stream=False)
        return d_sum, d_nbr

    def _plan(self, keep_init, gains, explore, deconflict, steps=None):
        """what start and tick do with the plan in the current buffer: the planner's rounds, the neighbours' spheres, the solve"""
        info = None if explore is None else self._explore(explore, steps)
        fleet = None if deconflict is None else self._deconflict(deconflict)
        res = self._solve(keep_init, gains)
        if info is not None:
            res["explore"] = info
        if fleet is not None:
            res["separation"], res["neighbours"] = fleet
        return res

    def start(self, init, keep_init=False, gains=False, explore=None, deconflict=None):
        """A plain solve of `init` (B, n, 18; NumPy or torch) from the start of the handle's desired trajectory (horizon start 0).
        gains=True, explore, deconflict: as for tick."""
        self.solver.set_horizon_start(0)
        self.k0 = 0
        self._to_device(init, self._buf[self._cur])
        return self._plan(keep_init, gains, explore, deconflict)

    def control(self, x, i=0):
        """The (B, 4) controls of the last plan's feedback law at knot `i` for the measured states x (B, 13; NumPy or torch):
        u = plan[:, i, 14:18] + K_i (x (-) plan[:, i]), clamped to the handle's thrust limits while they are set.  Needs the gains of the
        last plan (start / tick with gains=True).  A new tensor, complete on torch's current stream."""
        import torch
        if not self._have_gains:
            raise RuntimeError("control() needs the gains of the last plan: call start() or tick() with gains=True")
        if self._xc is None:
            self._xc = torch.zeros((self.B, 1, capi.STATE), dtype=torch.float64, device=self.device)
            self._ctl = torch.zeros((self.B, 1, self.n, capi.KNOT), dtype=torch.float64, device=self.device)
        self._to_device(x, self._xc[:, 0])
        i = int(i)
        self.solver.closed_loop_device(self._buf[self._cur], self.gains, self._xc, out_traj=self._ctl, i0=i, i1=i)
        # (enqueued on the solver's stream and not waited for: torch's stream waits for it before it reads the knot)
        torch.cuda.current_stream(self.device).wait_event(self._stream.record_event())
        return self._ctl[:, 0, i, 14:18].clone()

    def evaluate(self, x0, wrench=None):
        """The last plan's feedback law scored from sampled states: x0 (B, S, 13; NumPy or torch) flown over the whole horizon (knots
        0 .. n - 1) under wrench (None, or (B, S, n_w, 6) with n_w 1 or n: QuadrotorILQRBatch.closed_loop's), at the handle's current
        horizon start -- the one the plan was solved at.  Needs the gains of the last plan (start / tick with gains=True), as control()
        does.  Returns {"stats": (B, S, 4), "score": (B, S, 4)}: device tensors this object owns (valid until the next evaluate with another
        S), complete on torch's current stream.  No trajectory is written."""
        import torch
        if not self._have_gains:
            raise RuntimeError("evaluate() needs the gains of the last plan: call start() or tick() with gains=True")
        shape = tuple(x0.shape)
        if len(shape) != 3 or shape[0] != self.B or shape[2] != capi.STATE:
            raise TypeError(f"x0 must be ({self.B}, S, {capi.STATE})")
        S = shape[1]
        n_w = 0
        if wrench is not None:
            wshape = tuple(wrench.shape)
            if len(wshape) != 4 or wshape[:2] != (self.B, S) or wshape[3] != capi.WRENCH:
                raise TypeError(f"wrench must be ({self.B}, {S}, n_w, {capi.WRENCH})")
            n_w = wshape[2]
        if self._eval is None or self._eval[0] != S or self._eval[1] != n_w:
            new = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)
            self._eval = (S, n_w, new(self.B, S, capi.STATE), new(self.B, S, n_w, capi.WRENCH) if n_w else None, new(self.B, S, capi.CL_STATS),
                          new(self.B, S, capi.CL_SCORE))
        _, _, d_x0, d_w, d_stats, d_score = self._eval
        self._to_device(x0, d_x0)
        if d_w is not None:
            self._to_device(wrench, d_w)
        self.solver.closed_loop_device(self._buf[self._cur], self.gains, d_x0, out_stats=d_stats, wrench=d_w, out_score=d_score)
        # (enqueued on the solver's stream and not waited for: torch's stream waits for it before anything reads the results)
        torch.cuda.current_stream(self.device).wait_event(self._stream.record_event())
        return dict(stats=d_stats, score=d_score)

    def evaluate_covariance(self, state_sigma, gust=None, wrench_held=False, cov=False):
        """Linear covariance analysis about the last plan and its gains over the whole horizon (QuadrotorILQRBatch.covariance_device): how
        far flights of the law stray from the plan for start-state deviations state_sigma (12 words over [rho, theta, dv, dw], or one
        number) under `gust` (None, or a dict with the fields of qilqr_gust_model, as evaluate_sampled takes it) -- the first-order answer
        to what evaluate_sampled samples, from one enqueue.  Needs the gains of the last plan (start / tick with gains=True), as evaluate()
        does.  Returns {"summary": (B, 8), "cov": (B, n, 12, 12) or None}: views of device tensors this object owns, complete on torch's
        current stream."""
        import torch
        if not self._have_gains:
            raise RuntimeError("evaluate_covariance() needs the gains of the last plan: call start() or tick() with gains=True")
        if self._cov is None:
            self._cov = [torch.zeros((self.B, capi.COV_SUMMARY), dtype=torch.float64, device=self.device), None]
        if cov and self._cov[1] is None:
            self._cov[1] = torch.zeros((self.B, self.n, capi.COV), dtype=torch.float64, device=self.device)
        d_sum, d_cov = self._cov[0], self._cov[1] if cov else None
        self.solver.covariance_device(self._buf[self._cur], self.gains, state_sigma, gust=gust, wrench_held=wrench_held, cov=d_cov, summary=d_sum)
        # (enqueued on the solver's stream and not waited for: torch's stream waits for it before anything reads the results)
        torch.cuda.current_stream(self.device).wait_event(self._stream.record_event())
        return dict(summary=d_sum, cov=None if d_cov is None else d_cov.view(self.B, self.n, 12, 12))

    def evaluate_sampled(self, x, S, seed, state_sigma, gust=None, n_w=None, first_is_nominal=True, risk_levels=None, risk_column="cost", candidates=1):
        """The Monte-Carlo loop about the last plan without the host: S start states per plan sampled about the measured states x (B, 13;
        NumPy or torch) with deviations state_sigma (12 words over [rho, theta, dv, dw], or one number), gusts sampled from `gust` (None: no
        disturbance; else a dict with the fields of qilqr_gust_model -- sigma, and optionally mean, tau_force_s, tau_torque_s) for n_w
        knots (1, or n: the default), the law flown and scored over the whole horizon as evaluate() does, and the scores reduced per plan.
        Four enqueues on the solver's stream, then torch's current stream waits once.  first_is_nominal: sample 0 starts at x itself.
        Returns {"stats": (B, S, 4), "score": (B, S, 4), "summary": (B, 8)} (QuadrotorILQRBatch.reduce_scores_device's words): device
        tensors this object owns, valid until the next call with another S or n_w.  The sampled states and wrenches stay in
        `self.sampled` = (x0, wrench).  Needs the gains of the last plan, as evaluate().
        risk_levels (up to 8 numbers in [0, 1); S <= 4096): the result also carries "risk", (B, L, 4) -- per level the order statistic
        (VaR) and the tail mean (CVaR) of the cost, or with risk_column="clearance" of the clearance (QuadrotorILQRBatch.risk_scores_device's
        words), one more enqueue behind the reduction.  candidates = C (B divisible by C): the batch is B / C vehicles x C candidate plans,
        plan b = c V + v, and the samplers are called once per candidate on its V plans with plan offset 0, so that every candidate of a
        vehicle flies the same sampled start states (about its own row of x) and gusts -- common random numbers; select() then chooses."""
        import torch
        if not self._have_gains:
            raise RuntimeError("evaluate_sampled() needs the gains of the last plan: call start() or tick() with gains=True")
        S = int(S)
        if S <= 0:
            raise TypeError("S must be positive")
        n_w = 0 if gust is None else (self.n if n_w is None else int(n_w))
        if gust is not None and n_w not in (1, self.n):
            raise TypeError(f"n_w must be 1 or {self.n}")
        if self._mc is None or self._mc[0] != S or self._mc[1] != n_w:
            new = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)
            self._mc = (S, n_w, new(self.B, capi.STATE), new(self.B, S, capi.STATE), new(self.B, S, n_w, capi.WRENCH) if n_w else None,
                        new(self.B, S, capi.CL_STATS), new(self.B, S, capi.CL_SCORE), new(self.B, capi.MC_SUMMARY))
        _, _, d_nom, d_x0, d_w, d_stats, d_score, d_sum = self._mc
        C = int(candidates)
        if C <= 0 or self.B % C:
            raise TypeError(f"candidates must divide B = {self.B}")
        levels = None if risk_levels is None else np.atleast_1d(np.asarray(risk_levels, dtype=np.float64))
        if levels is not None and (self._risk is None or self._risk.shape[1] != len(levels)):
            self._risk = torch.zeros((self.B, len(levels), capi.RISK), dtype=torch.float64, device=self.device)
        self._last = None
        self._to_device(x, d_nom)  # (on torch's current stream: the first enqueue below makes the solver's stream wait for it)
        V = self.B // C
        # A candidate's V plans are contiguous: slices of the buffers (one candidate: the whole batch).  The calls want 16-byte
        # boundaries, and a row of 13 words puts a slice with an odd number of rows before it 8 bytes off one: the measured states, and the
        # sampled ones when V S is odd, then go through a copy whose candidates lie one row further apart.
        nom_of = x0_of = None
        if C > 1 and V % 2:
            if self._pad is None or self._pad[:2] != (C, S):  # (kept: the solver's stream reads them after this returns)
                new = lambda rows: torch.zeros((C, rows, capi.STATE), dtype=torch.float64, device=self.device)
                self._pad = (C, S, new(V + 1), new(V * S + 1) if S % 2 else None)
            nom_pad, x0_pad = self._pad[2:]
            nom_pad[:, :V].copy_(d_nom.view(C, V, capi.STATE))  # (torch's current stream, before the first enqueue)
            nom_of = lambda c: nom_pad[c, :V]
            if x0_pad is not None:
                x0_of = lambda c: x0_pad[c, :V * S].view(V, S, capi.STATE)
        for c in range(C):
            rows = slice(c * V, (c + 1) * V)
            self.solver.sample_states_device(nom_of(c) if nom_of else d_nom[rows], x0_of(c) if x0_of else d_x0[rows], seed, state_sigma,
                                             first_is_nominal=first_is_nominal, wait_current_stream=c == 0)
            if d_w is not None:
                self.solver.sample_gusts_device(d_w[rows], seed, gust["sigma"], gust.get("mean"), gust.get("tau_force_s", 0.0), gust.get("tau_torque_s", 0.0),
                                                wait_current_stream=False)
        if x0_of:
            with torch.cuda.stream(self._stream):  # (behind the samplers, before the flight: the solver's own stream)
                d_x0.view(C, V * S, capi.STATE).copy_(x0_pad[:, :V * S])
        self.solver.closed_loop_device(self._buf[self._cur], self.gains, d_x0, out_stats=d_stats, wrench=d_w, out_score=d_score, wait_current_stream=False)
        self.solver.reduce_scores_device(d_score, d_sum, wait_current_stream=False)
        res = dict(stats=d_stats, score=d_score, summary=d_sum)
        if levels is not None:
            self.solver.risk_scores_device(d_score, self._risk, levels, column=risk_column, wait_current_stream=False)
            res["risk"] = self._risk
        # (all enqueued on the solver's stream, in order, and none waited for: torch's stream waits once, behind the last)
        torch.cuda.current_stream(self.device).wait_event(self._stream.record_event())
        self.sampled = (d_x0, d_w)
        self._last = (d_sum, self._risk if levels is not None else None, risk_column)
        return res

    def select(self, C, objective="cvar", level=0, max_collision_fraction=1.0, max_diverged_fraction=1.0, min_clearance=-np.inf):
        """The choice among the C candidate plans of each of the B / C vehicles (plan b = c V + v) from the last evaluate_sampled() result
        (QuadrotorILQRBatch.select_plans_device: the feasible candidate with the smallest objective -- "mean", "worst", or "var", "cvar" at
        `level` of that call's risk_levels, which must have been on the cost column -- else the fallback order), and the gather of the
        chosen plans and their gains.  Returns {"choice": (V,) int32, "info": (V, 4), "plan": (V, n, 18), "gains": (V, n, 52), "u0": (V, 4),
        a view of the plan}: device tensors this object owns (valid until the next select with another C), complete on torch's current
        stream after one wait."""
        import torch
        if self._last is None or not self._have_gains:
            raise RuntimeError("select() works on the last evaluate_sampled() result: call it first")
        C = int(C)
        if C <= 0 or self.B % C:
            raise TypeError(f"C must divide B = {self.B}")
        d_sum, d_risk, column = self._last
        risky = objective in ("var", "cvar")
        if risky and d_risk is None:
            raise RuntimeError(f"objective {objective!r} needs evaluate_sampled(..., risk_levels=...)")
        if risky and column != "cost":
            raise RuntimeError(f"objective {objective!r} needs the risk of the cost column, not of {column!r}")
        V = self.B // C
        if self._sel is None or self._sel[0] != C:
            new = lambda *s, dtype=torch.float64: torch.zeros(s, dtype=dtype, device=self.device)
            self._sel = (C, new(V, dtype=torch.int32), new(V, capi.SELECT_INFO), new(V, self.n, capi.KNOT), new(V, self.n, capi.GAIN))
        _, d_choice, d_info, d_plan, d_gains = self._sel
        self.solver.select_plans_device(d_sum, C, d_choice, d_info, objective=objective, level=level, risk=d_risk if risky else None,
                                        max_collision_fraction=max_collision_fraction, max_diverged_fraction=max_diverged_fraction, min_clearance=min_clearance,
                                        plan=self._buf[self._cur], gains=self.gains, out_plan=d_plan, out_gains=d_gains)
        # (two launches on the solver's stream; torch's stream waits once, behind the gather)
        torch.cuda.current_stream(self.device).wait_event(self._stream.record_event())
        return dict(choice=d_choice, info=d_info, plan=d_plan, gains=d_gains, u0=d_plan[:, 0, 14:18])

    def tick(self, x0, steps=1, tail="hold", advance=True, keep_init=False, gains=False, explore=None, deconflict=None):
        """One control tick: the horizon start advanced by `steps` (advance=False: the desired trajectory is relative to the vehicle and
        stays), the last plan shifted into the other buffer with knot 0 at x0 (B, 13; NumPy or torch; None keeps the plan's own), and the
        solve from there.  Returns views (valid until the next tick but one) of the first controls u0 = traj[:, 0, 14:18], the plan, cost,
        status and iterations, read after the solve has drained the solver's stream.  keep_init=True also keeps a copy of the shifted plan
        the solve started from in `self.init`: made on torch's current stream, which is made to wait for the shift on the solver's stream
        first (the two streams are ordered with each other only where one is told to wait).  gains=True also leaves the feedback gains about
        the new plan in `self.gains` (B, n, 52; a device buffer this object owns, allocated at the first such call) and returns them under
        "gains": one more backward pass on the plan (backwards_pass_device), what control() evaluates.  explore (None: nothing changes): a dict
        with S, seed, sigma, lambda_ and optionally tau_s, collision_cost, iterations (1) and first_is_nominal (True) -- between the shift
        and the solve `iterations` rounds of the sampling planner run on the solver's stream (_explore: round r with seed + r, S perturbed
        flights from knot 0 and the plan moved to their weighted mean, through a scratch buffer), the solve polishes what they found, and
        the result carries "explore", the last round's info (B, 8; QuadrotorILQRBatch.mppi_update_device's words).  With the key adapt =
        dict(rate=, floor=, cap=) the rounds adapt the spread per plan, knot and rotor (`self.spread`, (B, n, 4): set to sigma by start,
        shifted `steps` knots with a tail of sigma by every tick; mppi_flight_spread_device and mppi_adapt_device).  A tick that is refused -- steps or tail out of
        range, or no window of n knots left behind the new start -- raises and leaves the object and the handle's start as they were.
        deconflict (None: nothing changes, bit for bit): a dict with radius, weight, K and optionally fleet (None: B, one fleet), range (inf),
        conflict (None: radius), cover (False) and yield_to_lower (False) -- the B plans are vehicles in one world frame on one time base, rows b
        with equal b // fleet sharing airspace.  Between the shift (and the planner's rounds, if any) and the solve, the K nearest partners
        of every vehicle over the horizon become moving spheres of `radius` and `weight` (QuadrotorILQRBatch.fleet_neighbours_device on the
        shifted plans, then set_batch_obstacles_device, on the solver's stream), and the result carries "separation", the (B, 8) summary
        (smallest distance to a partner, its knot, its partner, partners closer than `conflict`, spheres written, largest radius), and
        "neighbours", (B, K, 4): views of buffers this object owns.  This REPLACES the handle's per-problem sphere table (set_batch_obstacles),
        and the table stays set afterwards: a later tick without deconflict still avoids the spheres of the last one that had it, until
        clear_batch_obstacles().  Every vehicle avoids the others' PREVIOUS plans, not the ones this tick's solve produces: two vehicles that
        meet head-on may both give way to the same side, tick after tick.  yield_to_lower is the remedy for such symmetric encounters --
        a vehicle then avoids only partners in a smaller row, and row 0 of a fleet yields to nobody (prioritised planning).  A tick that is
        refused after the table was set leaves the table set."""
        steps = int(steps)
        x0 = None if x0 is None else self._to_device(x0, self._x0)
        # (refuses steps or a tail out of range before anything of this object or of the handle has changed; the buffer it writes holds the
        # plan before last, which nobody reads any more)
        self.solver.shift_device(self._buf[self._cur], self._buf[self._cur ^ 1], x0=x0, steps=steps, tail=tail)
        had_k0, had_cur, had_spread = self.k0, self._cur, self.spread
        try:
            if advance:
                self.solver.set_horizon_start(had_k0 + steps)
                self.k0 = had_k0 + steps
            self._cur ^= 1
            return self._plan(keep_init, gains, explore, deconflict, steps)
        except Exception:
            # a refused start or solve (past the end of the mission no window of n knots is left) leaves the last plan, its buffer and the
            # start it was solved at in force
            self.solver.set_horizon_start(had_k0)
            self._held = self.spread  # (a flight that was enqueued before the refusal may still read the shifted spread: it is kept, not freed)
            self.k0, self._cur, self.spread = had_k0, had_cur, had_spread
            raise
