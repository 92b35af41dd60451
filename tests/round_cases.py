"""The fifteen instantiations of k_round (round_kernels.h; host/launches.h, launch_round) as a table -- one row per k_round<LK, ROUNDS, SIX>
with the handle that reaches it -- and the problem families tests/test_gpu_round_instantiations.py solves on each row's handle and on the
three launches (k_backward4 + k_rollout16 + k_linearize, round_launch = 1).  tests/test_round_cases_cpu.py proves from route.h that each row's
handle takes the row's own instantiation, and from the oracle that the families hold what the comparisons need (iteration counts that differ
inside a block, backtracking, a failed search beside running neighbours, restarts, the iteration cap at every position of a launch).

LK, the record kind of the cost half, follows from the weights (qilqr_create's bit-exact predicates):
  "sym"    LK 1  dense symmetric Q with a non-zero pose x velocity block -- test_dense_coupled_weights_solve's weights
  "block"  LK 2  the same with the two 6 x 6 coupling blocks exactly zero
  "diag"   LK 3  Q_DEMO, R_DEMO
(ROUNDS, SIX), the rounds in a launch and the form of its backward pass, from force_general and rounds_per_launch (FORMS).
No assertions here, no GPU; the oracle only where a caller asks for a family's reference solution."""
import collections
import functools

import numpy as np

from quadrotorilqr_amd import problems as pb
from tests.desired_cases import tracking_case

KEYS = ("traj", "cost", "status", "iters", "n_bwd", "n_fwd")
LK_OF = {"sym": 1, "block": 2, "diag": 3}
# (ROUNDS, SIX) in the order of qilqr_round_launches' slots, j = 0..4, and the device configuration that takes each in EVERY launch
FORMS = collections.OrderedDict([((1, False), dict(force_general=5, rounds_per_launch=1)), ((1, True), dict(force_general=8, rounds_per_launch=1)),
                                 ((2, False), dict(force_general=5, rounds_per_launch=2)), ((4, False), dict(force_general=5, rounds_per_launch=0)),
                                 ((4, True), dict(force_general=8, rounds_per_launch=0))])
COMPARAND = dict(round_launch=1, force_general=5)  # the three launches
N_MAX = 65  # the longest horizon of any family: the handles' desired trajectory has this many knots

Row = collections.namedtuple("Row", "weights lk rounds six kw slot")


def slot(lk, rounds, six):
    """index into qilqr_round_launches' counts (include/quadrotor_ilqr.h)"""
    return 5 * (lk - 1) + list(FORMS).index((rounds, six))


ROWS = tuple(Row(w, lk, rounds, six, dict(kw), slot(lk, rounds, six)) for w, lk in LK_OF.items() for (rounds, six), kw in FORMS.items())


def row_id(row):
    return f"{row.weights}-{row.rounds}-{'six' if row.six else 'fused'}"


def mangled(row):
    """qilqr::k_round<LK, ROUNDS, SIX> in the Itanium mangling, as tests/golden/kernel_symbols.json lists it"""
    return (f"_ZN5qilqr7k_roundILi{row.lk}ELi{row.rounds}ELb{int(row.six)}EEE"
            "vNS_11ModelConstsIdEEPKS2_NS_11SolveParamsENS_10BatchStateEiiPii")


@functools.lru_cache(maxsize=None)
def weights(kind):
    """(Q, R) of the kind; "sym" is built as test_dense_coupled_weights_solve builds its weights"""
    if kind == "diag":
        return pb.Q_DEMO, pb.R_DEMO
    r = np.random.default_rng(21)
    A = r.uniform(-1, 1, (12, 12))
    D = np.sqrt(np.diag(pb.Q_DEMO))
    A4 = r.uniform(-1, 1, (4, 4))
    Q = pb.Q_DEMO + 0.1 * (D[:, None] * (A + A.T) * D[None, :]) / 2
    R = pb.R_DEMO + 0.1 * (A4 + A4.T)
    if kind == "block":
        Q = Q.copy()
        Q[:6, 6:] = 0.0
        Q[6:, :6] = 0.0
    return Q, R


def predicates(kind):
    """the bit-exact predicates qilqr_create takes of Q and R (host/api_handle.h), and what they make of the handle for the route:
    (symmetric, q_diag, layout_kind)"""
    from tests.linearize_cases import predicates as of_weights  # (here: the module draws in the cases of other GPU tests)
    p = of_weights(*weights(kind))
    return p["q_sym"] and p["r_sym"], p["q_diag"], 0 if not p["q_sym"] else (2 if p["ur_zero"] else 1)


# ---- the problems: pb.config2 (model A, hover at identity, random starts) with the weights swapped in

HOVER = pb.hover_desired(N_MAX, pb.DT_DEMO, pb.hover_thrust(pb.MODEL_A))
OPTIONS = dict(pb.OPTIONS_DEMO, populate_debug=False)

# name: of the case; init (B, n, 18); desired (B, n, 18) per-problem desired trajectories or None (the hover); options: changes to OPTIONS;
# mu: None, or the arguments of set_regularisation
Problem = collections.namedtuple("Problem", "name init desired options mu")


def _problem(name, init, desired=None, options=(), mu=None):
    init.setflags(write=False)
    if desired is not None:
        desired.setflags(write=False)
    return Problem(name, init, desired, tuple(sorted(dict(options).items())), mu)


PLAIN_B, PLAIN_N = (1, 7, 9), (1, 2, 3, 5, 16, 17, 33, 65)
HARD_SHAPES = TRACKING_SHAPES = ((7, 17), (9, 33))
# The seeds of the two families, by shape.  Each is the nearest to 40 + B (hard) and 60 + B (tracking) at which the oracle's solution has,
# under all three kinds of weights, at least three distinct iteration counts in the first block of four and a longest solve of at least 17
# iterations -- and, for hard(7, 17), a failed one-trial search beside running neighbours and restarts (tests/test_round_cases_cpu.py).
# 47 gives hard(7, 17) the counts [15, 74, 15, 15] under the diagonal weights, 69 ends tracking(9, 33) after 16 iterations under two kinds.
HARD_SEEDS = {(7, 17): 46, (9, 33): 49}
TRACKING_SEEDS = {(7, 17): 67, (9, 33): 68}
ORACLE_PLAIN_N = (3, 17, 65)
CAPS = (1, 2, 3, 4, 5, 6)


@functools.lru_cache(maxsize=None)
def plain(B, n):
    """horizons of one, two and three knots, both sides of R16_CHUNK and of the 64-knot task of a lone trajectory; last blocks of three rows
    and of one row"""
    return _problem(f"plain({B}, {n})", pb.config2(B=B, N=n, seed=30 + B)["init"])


@functools.lru_cache(maxsize=None)
def hard(B, n, **options):
    """starts far from the hover: long solves, backtracking line searches"""
    init = pb.random_start_batch(np.arange(B), HOVER[:n], HARD_SEEDS[B, n], pos_m=3.0, ang_rad=2.5, vel_sigma=2.0)
    return _problem(f"hard({B}, {n})" + "".join(f", {k}={v}" for k, v in sorted(options.items())), init, options=options)


def one_trial():
    """one line-search trial: a problem ends with status 3 while its block neighbours run on"""
    return hard(7, 17, ls_max_iters=1)


def restarts():
    """... and with Levenberg-Marquardt restarts instead"""
    return one_trial()._replace(name="hard(7, 17), ls_max_iters=1, restarts", mu=(1.0, 4.0, 1e6))


def capped(max_iters):
    """every problem ends at the iteration cap: over 1..6 the cap falls on every position of a four-round and of a two-round launch"""
    return hard(7, 17, max_iters=max_iters)


@functools.lru_cache(maxsize=None)
def tracking(B, n):
    """per-problem desired trajectories that change from knot to knot (tests/desired_cases.py)"""
    cfg, des = tracking_case(B, n, TRACKING_SEEDS[B, n])
    return _problem(f"tracking({B}, {n})", cfg["init"], desired=des)


def config(kind, problem):
    """the problems-style config of a handle (or oracle) for the problem: the hover of N_MAX knots as the handle's desired trajectory -- every
    knot of it is the same but for the time column, which the ABI ignores, so a solve of n <= N_MAX knots on it is pb.config2's"""
    Q, R = weights(kind)
    return dict(model=pb.MODEL_A, Q=Q, R=R, dt=pb.DT_DEMO, options=dict(OPTIONS, **dict(problem.options)), desired=HOVER)


def every_bit_family():
    """the problems compared bit for bit with the three launches"""
    return ([plain(B, n) for B in PLAIN_B for n in PLAIN_N] + [hard(B, n) for B, n in HARD_SHAPES] + [one_trial(), restarts()] +
            [tracking(B, n) for B, n in TRACKING_SHAPES])


def every_oracle_family():
    """the problems held to the oracle"""
    return ([plain(B, n) for B in PLAIN_B for n in ORACLE_PLAIN_N] + [hard(B, n) for B, n in HARD_SHAPES] +
            [tracking(B, n) for B, n in TRACKING_SHAPES])


# ---- the oracle's solutions, computed once per process and left unchanged

def _oracle(kind, problem, desired):
    from oracle import oracle as orc
    cfg = config(kind, problem)
    o = orc.OracleSolver(orc.model_params(**cfg["model"]), cfg["Q"], cfg["R"], desired, cfg["dt"], orc.options(**cfg["options"]))
    if problem.mu:
        o.set_regularisation(*problem.mu)
    return o


_SOLUTIONS = {}


def oracle_solution(kind, problem):
    """(oracles, ref): the oracle of each row -- one for all under the hover, one per row's own desired trajectory otherwise, as
    tests/test_gpu_desired.oracle_rows -- and the solutions as arrays over the batch"""
    key = (kind, problem.name)  # (the names are the families' own arguments: one problem each)
    if key not in _SOLUTIONS:
        _SOLUTIONS[key] = _solve(kind, problem)
    return _SOLUTIONS[key]


def _solve(kind, problem):
    B = len(problem.init)
    if problem.desired is None:
        o = _oracle(kind, problem, HOVER)
        oracles, ref = [o] * B, o.solve_batch(problem.init)
    else:
        oracles = [_oracle(kind, problem, problem.desired[b]) for b in range(B)]
        res = [o.solve(problem.init[b]) for b, o in enumerate(oracles)]
        ref = {k: np.array([r[k] for r in res]) for k in KEYS}
    for v in ref.values():
        v.setflags(write=False)
    return oracles, ref
