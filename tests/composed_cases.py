"""The inputs of the tests of the extensions together (tests/test_composed_cpu.py, tests/test_gpu_composed.py): handles with a state-weight
schedule, per-problem moving spheres, a shared sphere and per-problem models at once, for single passes, whole solves and a horizon start,
and the composed restatement's solves.  Test infrastructure only."""
import functools

import numpy as np

from tests import desired_cases as dc, linearize_cases as lc, schedule_cases as sc
from tests.composed_numpy_ilqr import ComposedILQR
from tests.independent_numpy_ilqr import Model
from tests.test_gpu_batch_obstacles import moving_on

# ---- single passes: every extension on one handle (models, the shared spheres and the per-problem ones), B = 3, n = 12


def _every(schedule, integrator, limits=0):
    return lc.Case("diag", integrator, 0, 0, 0, limits, 1, 1, 1, schedule)


PASS_CASES = tuple(_every(s, i) for s in ("terminal", "dense", "nonsym") for i in (0, 1)) + \
    (_every("terminal", 0, 1), _every("dense", 0, 1), _every("dense", 1, 1))  # thrust limits beside the symmetric schedules


def pass_seed(c):
    return 5000 + PASS_CASES.index(c)


# ---- whole solves: schedule_cases' problems (config2(B=6, N, seed=7)), the terminal schedule and moving spheres, without and with models

SIZES = (12, 24)
PROBLEMS = tuple(range(6))
SOLVE_COUNTS = np.array([3, 2, 3, 1, 3, 0])
SOLVE_SEED = 19  # (chosen on the CPU: the restatement's counts stay when the spheres move by 1e-13, tests/test_composed_cpu.py)
COUNTS = sc.COUNTS


def solve_inputs(N, models):
    cfg = sc.config(N)
    table = moving_on(cfg["init"], cfg["dt"], np.random.default_rng(SOLVE_SEED + N))
    mods = [dict(cfg["model"], mass_kg=cfg["model"]["mass_kg"] * (0.8 + 0.1 * b), arm_length_m=1.0 - 0.05 * b) for b in range(len(cfg["init"]))] \
        if models else None
    return dict(cfg=cfg, Qs=sc.schedule("terminal", N), table=table, counts=SOLVE_COUNTS, mods=mods)


def solve_restatement(x, b, nudge=0.0):
    """problem b's composed restatement (recursion 1: symmetric schedule); nudge: every sphere centre moved by it along each axis"""
    cfg = x["cfg"]
    o = ComposedILQR(Model(**(x["mods"][b] if x["mods"] else cfg["model"])), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]),
                     recursion=1)
    own = x["table"][b, :x["counts"][b]].copy()
    own[:, :3] += nudge
    o.set_problem_obstacles(own)
    o.set_state_weight_schedule(x["Qs"])
    return o


@functools.lru_cache(maxsize=None)
def compute(N, models, b, nudge=0.0):
    """the restatement's solve of problem b (a fraction of a second: computed once per process and shared, read-only)"""
    x = solve_inputs(N, models)
    out = solve_restatement(x, b, nudge).solve(x["cfg"]["init"][b])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- the horizon start beside spheres: a 40-knot time-varying desired trajectory, a 40-matrix dense schedule, k0 = 7, calls of 24 knots

N_DES, K0, N, SEED = 40, 7, 24, 21


def window_inputs(B, k0=K0):
    """the handle's config (desired trajectory and schedule of N_DES knots), initial trajectories for the window [k0, k0 + N) and moving
    spheres timed from the call's first knot (they contain knots of those initial trajectories at i dt)"""
    cfg, _ = dc.tracking_case(B, N_DES, SEED, shared=True)
    init = dc.start_from(np.repeat(cfg["desired"][None, k0:k0 + N], B, axis=0), np.arange(B), SEED)
    table = moving_on(init, cfg["dt"], np.random.default_rng(SEED + 1))
    counts = np.resize([3, 2, 1, 0, 3, 2], B)
    return dict(cfg=cfg, init=init, table=table, counts=counts, Qs=sc.schedule("dense", N_DES))


def window_restatement(x, b, desired, Qs, own=None, recursion=1):
    """the composed restatement of problem b from a desired trajectory and a schedule (slices of the handle's, or what a wrong index reads)"""
    cfg = x["cfg"]
    o = ComposedILQR(Model(**cfg["model"]), cfg["Q"], cfg["R"], desired, cfg["dt"], dict(cfg["options"]), recursion=recursion)
    o.set_problem_obstacles(x["table"][b, :x["counts"][b]] if own is None else own)
    o.set_state_weight_schedule(Qs)
    return o


def later(own, t):
    """a problem's spheres as a kernel would see them that took (k0 + i) dt for their time: the centres t further along"""
    own = np.array(own, dtype=float).reshape(-1, 8)
    own[:, :3] += t * own[:, 3:6]
    return own
