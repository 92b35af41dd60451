"""The inputs of the state-weight-schedule tests (tests/test_schedule_cpu.py, tests/test_gpu_schedule.py): problems, the three
schedules, and the restatement's solves of them, computed once per process and shared.  Test infrastructure only."""
import functools
import os

import numpy as np

from quadrotorilqr_amd import problems as pb
from tests.independent_numpy_ilqr import Model
from tests.schedule_numpy_ilqr import ScheduleILQR, ScheduleLimitedILQR

SIZES = (12, 24, 40)
KINDS = ("terminal", "waypoint", "dense")
PROBLEMS = (0, 1, 2)  # of config2(B=6, N=N, seed=7): the problems the restatement solves


def config(N, B=6):
    return pb.config2(B=B, N=N, seed=7)


def schedule(kind, N):
    """(N, 12, 12), every matrix bit-exactly symmetric"""
    if kind == "terminal":
        return pb.terminal_schedule(0.01 * pb.Q_DEMO, 10.0 * pb.Q_DEMO, N)
    if kind == "waypoint":  # semi-definite between the waypoints: no pose weight there
        return pb.waypoint_schedule(np.diag([0.0] * 6 + [0.1] * 6), 5.0 * pb.Q_DEMO, N, (N // 2, N - 1))
    if kind == "constant":
        return pb.terminal_schedule(pb.Q_DEMO, pb.Q_DEMO, N)
    assert kind == "dense", kind
    r = np.random.default_rng(1)
    Qs = np.zeros((N, 12, 12))
    for i in range(N):
        A = r.standard_normal((12, 12))
        M = A @ A.T
        Qs[i] = (1 + i % 5) * (0.5 * (M + M.T) / 12.0 + 0.1 * np.eye(12))  # (M + M^T) / 2: the product's rounding is not symmetric by contract
    return Qs


def one_nonsymmetric(Qs):
    """the schedule with one entry of one matrix changed: the general kernel's input"""
    Qs = np.array(Qs)
    Qs[len(Qs) // 3, 2, 7] += 0.25
    return Qs


def restatement(cfg, Qs, recursion, model=None, limits=None, integrator=0, spheres=None):
    m = Model(**(model or cfg["model"]))
    if limits is None:
        o = ScheduleILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), integrator=integrator, recursion=recursion)
    else:  # (the box form is the symmetric recursion)
        o = ScheduleLimitedILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), *limits, integrator=integrator)
    if spheres is not None:
        o.set_obstacles(spheres)
    o.set_state_weight_schedule(Qs)
    return o


@functools.lru_cache(maxsize=None)
def compute(N, kind, b, recursion):
    """the restatement's solve of problem b, computed here (seconds each; read-only: shared between tests)"""
    cfg = config(N)
    out = restatement(cfg, schedule(kind, N), recursion).solve(cfg["init"][b])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_solves.npz")
COUNTS = ("status", "iters", "n_bwd", "n_fwd")


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def solved(N, kind, b):
    """compute(N, kind, b, 1) as recorded in tests/golden/schedule_solves.npz (tests/golden/make_schedule_golden.py wrote it;
    tests/test_schedule_cpu.py compares the record with a fresh computation): what the GPU tests compare whole solves against"""
    g, key = _golden(), f"{kind}_{N}_{b}"
    out = dict(traj=g[key + "_traj"], cost=float(g[key + "_cost"]), cost_hist=g[key + "_hist"])
    out.update(zip(COUNTS, (int(x) for x in g[key + "_counts"])))
    return out
