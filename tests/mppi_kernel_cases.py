"""The cases of tests/test_gpu_mppi_kernel_cases.py: one per instantiation of the sampling planner's kernels -- k_mppi_flight (mppi.hip, 8),
k_mppi_flight_spread (mppi_adapt.hip, 8): {Euler, Runge-Kutta} x {plain, limits, models, both}; k_mppi_update (5) and k_mppi_adapt (5):
the block sizes 64 .. 1024 -- each with the symbol of its kernel and the shape that selects it (tests/test_mppi_kernel_cases_cpu.py
proves the map one to one against the two compiled units and the harness's grid rule).  And the inputs of that file's other tests, built
once and read-only, with the restatement's own flights of them: horizons at the ends of the knot loops, sphere tables at capacity, a
second tile of the per-problem table, a desired trajectory per plan.  Test infrastructure only; nothing here asserts."""
import collections
import functools

import numpy as np

from tests import closed_loop_cases as cc, closed_loop_numpy as cn, desired_cases as dc, mppi_adapt_cases as ac, mppi_adapt_numpy as ma
from tests import mppi_cases as mc, mppi_numpy as mp

SEED = 77
TAU_S = 0.3
LAMBDA, COLLISION_COST = 400.0, 30.0
EXTS = ("plain", "limits", "models", "both")
KNOT_ENDS = (2, 8, 9, 16, 17)  # no i + 2; one chunk of the update and nothing to prefetch; a chunk of one knot; two chunks; the longest the handle admits
N_LONG = 17                    # mc.schedule(): 20 knots from horizon start 3
S_FLIGHT = 70                  # two blocks per plan, the second with 58 idle lanes
RAGGED = (1025, 2500, 4095)    # lanes with one sample more than others: 1 of 1024, 452 of 1024, all but one
N_RAGGED, N_BLOCKS = 9, 12

Flight = collections.namedtuple("Flight", "spread integrator ext n S")
Block = collections.namedtuple("Block", "adapt threads S")
# a flight kernel has no size of its own: each case flies one of KNOT_ENDS, and the eight of a unit fly them all
FLIGHTS = tuple(Flight(sp, i, e, KNOT_ENDS[(4 * i + k) % len(KNOT_ENDS)], S_FLIGHT) for sp in (False, True) for i in (0, 1) for k, e in enumerate(EXTS))
BLOCKS = tuple(Block(ad, t, s) for ad in (False, True) for t, s in ((64, 64), (128, 100), (256, 200), (512, 300), (1024, 1025)))
CASES = FLIGHTS + BLOCKS

_PACK = {"plain": "", "limits": "NS_13ControlLimitsE", "models": "NS_11BatchModelsE", "both": "NS_13ControlLimitsENS_11BatchModelsE"}


def name(c):
    if isinstance(c, Flight):
        return "%s-%s-%s-n%d" % ("flight_spread" if c.spread else "flight", "rk4" if c.integrator else "euler", c.ext, c.n)
    return "%s-%d-S%d" % ("adapt" if c.adapt else "update", c.threads, c.S)


def unit(c):
    """the translation unit that holds the case's kernel"""
    return "mppi_adapt" if (c.spread if isinstance(c, Flight) else c.adapt) else "mppi"


def kernel_name(c):
    """the symbol of the kernel a call of the case launches (the Itanium mangling of the template arguments)"""
    if isinstance(c, Flight):
        if c.spread:
            return "_ZN5qilqr20k_mppi_flight_spreadILi%dEJ%sEEEvNS_11ModelConstsIdEENS_20MppiFlightSpreadArgsEDpT0_" % (c.integrator, _PACK[c.ext])
        return "_ZN5qilqr13k_mppi_flightILi%dEJ%sEEEvNS_11ModelConstsIdEENS_14MppiFlightArgsEDpT0_" % (c.integrator, _PACK[c.ext])
    if c.adapt:
        return "_ZN5qilqr12k_mppi_adaptILi%dEEEvNS_13MppiAdaptArgsE" % c.threads
    return "_ZN5qilqr13k_mppi_updateILi%dEEEvNS_14MppiUpdateArgsE" % c.threads


def frozen(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def draws(spread, seed, S, dt, b0=0, first_is_nominal=False, B=None, n=None):
    """the restatement's perturbations of either flight: `spread` is the rule's sigma (4,) or a field (B, n, 4)"""
    spread = np.asarray(spread, dtype=np.float64)
    if spread.ndim == 3:
        return ma.perturbations(seed, spread, S, dt, tau_s=TAU_S, b0=b0, first_is_nominal=first_is_nominal)
    return mp.perturbations(seed, B, S, n, dt, spread, tau_s=TAU_S, b0=b0, first_is_nominal=first_is_nominal)


# ---- B = 2 plans of n <= 17 knots with every operand of the score (mc.everything's case at another length)

KB = 2


def spheres_beside(traj, seed):
    """mc.spheres_on_the_way for any n >= 2: 8 shared spheres beside flown knots of traj (B, S, n, 18) and a moving one per plan"""
    r = np.random.default_rng(seed)
    b, S, n = traj.shape[:3]
    shared = np.zeros((8, 5))
    for j in range(8):
        shared[j, :3] = traj[j % b, j % S, (1 + 3 * j) % n, 1:4] + 0.12 * (2.0 * r.random(3) - 1.0)
        shared[j, 3] = 0.10 + 0.03 * (j % 3)
        shared[j, 4] = 20.0 + 5.0 * j
    own = np.zeros((b, 2, 8))
    for k in range(b):
        own[k, 0, :3] = traj[k, 0, n - 1, 1:4] + 0.1
        own[k, 0, 3:6] = (0.05, -0.04, 0.03)
        own[k, 0, 6:8] = (0.15, 40.0)
    return shared, own, [1] * b


@functools.lru_cache(maxsize=None)
def horizon(n):
    """(host keywords, restatement keywords, cfg, plan (2, n, 18), x0, spread (2, n, 4)): the first n knots of two 17-knot plans, a start
    state off knot 0, limits at the 20th and 80th percentile of the perturbed controls, two models, the schedule and the handle's desired
    trajectory of mc.schedule() from horizon start 3, and spheres beside the flown paths"""
    cfg, plan = cn.plans(KB, N_LONG, mc.SEED + 40)
    plan = np.ascontiguousarray(np.array(plan)[:, :n])
    x0 = np.ascontiguousarray(cn.sample_states(plan, 1, 0, mc.SEED + 41, pos_m=0.1, ang_rad=0.1, vel_sigma=0.1)[:, 0])
    hd, Qs = mc.schedule()
    eps = mp.perturbations(SEED, KB, S_FLIGHT, n, cfg["dt"], mc.SIGMA, tau_s=TAU_S)
    u = plan[:, None, :, 14:18] + eps
    limits = (float(np.percentile(u, 20)), float(np.percentile(u, 80)))
    models = mc.MODELS3[:KB]
    free = mp.flight(plan, x0, eps[:, :8], cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], hd[mc.K0:mc.K0 + n], models=models, limits=limits)[3]
    shared, own, counts = spheres_beside(free, mc.SEED + 42)
    host = dict(x0=x0, models=models, limits=limits, handle_desired=hd, Qs=Qs, k0=mc.K0, shared=shared, own=own, counts=counts, tau_s=TAU_S)
    rest = dict(models=models, limits=limits, desired=hd[mc.K0:mc.K0 + n], Qs=Qs[mc.K0:mc.K0 + n], shared=shared, own=[own[k, :counts[k]] for k in range(KB)])
    frozen((plan, x0, hd, Qs, shared, own))
    return host, rest, cfg, plan, x0, frozen([ac.spread_field(KB, n)])[0]


def with_ext(keywords, ext):
    """the keywords of a flight case: limits and models only where its kernel takes them"""
    return dict(keywords, limits=keywords["limits"] if ext in ("limits", "both") else None, models=keywords["models"] if ext in ("models", "both") else None)


@functools.lru_cache(maxsize=None)
def flown(c):
    """the restatement's flight of a flight case: (score (2, S, 4), clear, gap)"""
    host, rest, cfg, plan, x0, spread = horizon(c.n)
    eps = draws(spread if c.spread else mc.SIGMA, SEED, c.S, cfg["dt"], B=KB, n=c.n)
    want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], integrator=c.integrator, **with_ext(rest, c.ext))
    return frozen((want, clear)) + (gap,)


# ---- tables at capacity: B = 3, 64 shared spheres, K = 64 per problem with counts 64, 0 and 37, on a plain handle (no schedule: the
# state weights are the handle's Q, staged once)

CAP_B, CAP_N, CAP_S, CAP_K, CAP_COUNTS = 3, 8, (63, 130), 64, (64, 0, 37)
CAP_AIMED = (("shared", 63, 1, 4), ("own", 63, 0, 3), ("own", 36, 2, 2))  # (table, its last sphere in use, the plan, the sample it is put in the way of)
CAP_NEAR = 8  # the shared spheres the reduced tables keep (and sphere 0 of every problem's own)
CAP_DEEP = 0.19  # the aimed spheres' radius; every other is at most 0.16


def free_paths(cfg, plan, x0, eps, integrator, models=None):
    """(B, S, n, 18): the restatement's flights without a sphere (a sphere changes the score of a flight, not the flight)"""
    return mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], cfg["desired"][:plan.shape[1]], integrator=integrator, models=models)[3]


def tables_along(paths, dt, seed, n_shared, K, reach, aimed=(), deep=CAP_DEEP, beside=None):
    """(shared (n_shared, 5), own (B, K, 8)): every sphere beside the flown position of one sample at one knot from 2 on -- the shared
    ones beside the plans `beside` in turn (None: all), the moving ones there at that knot's time -- `reach` m off it per axis at the
    most; the spheres of `aimed` centred on the last knot of their sample, with the largest radius of all"""
    r = np.random.default_rng(seed)
    B, S, n = paths.shape[:3]
    beside = tuple(range(B)) if beside is None else beside
    at = lambda b, j: paths[b, (7 * j + 3 * b) % min(S, 63), 2 + j % (n - 2), 1:4]  # noqa: E731
    shared, own = np.zeros((n_shared, 5)), np.zeros((B, K, 8))
    for j in range(n_shared):
        shared[j, :3] = at(beside[j % len(beside)], j) + reach * (2.0 * r.random(3) - 1.0)
        shared[j, 3:] = (0.10 + 0.03 * (j % 3), 20.0 + 5.0 * (j % 9))
    for b in range(B):
        for j in range(K):
            v = 0.2 * (2.0 * r.random(3) - 1.0)
            own[b, j, :3] = at(b, j + 1) + reach * (2.0 * r.random(3) - 1.0) - v * (2 + (j + 1) % (n - 2)) * dt
            own[b, j, 3:] = (*v, 0.10 + 0.03 * (j % 3), 30.0 + 2.0 * (j % 7))
    for kind, j, b, sample in aimed:
        p = paths[b, sample, n - 1, 1:4]
        if kind == "shared":
            shared[j, :4] = (*p, deep)
        else:
            own[b, j, :3], own[b, j, 3:6], own[b, j, 6] = p, 0.0, deep
    return shared, own


@functools.lru_cache(maxsize=None)
def capacity_inputs(integrator):
    """plans, one start state per plan, a spread field and two placements of full tables.  "full": spheres beside the paths the
    restatement flies with this integrator (the two part by 0.2 m over the horizon) -- the shared ones beside plans 0 and 2, so that
    plan 1, which has none of its own, keeps samples that hit nothing -- the last one in use of each table deepest in a sample's way
    (CAP_AIMED).  "far": the first CAP_NEAR shared spheres and every problem's own sphere 0 as in "full", every other sphere in use 5 m
    and more away."""
    cfg, plan = cn.plans(CAP_B, CAP_N, mc.SEED + 50)
    plan = np.array(plan)
    x0 = np.ascontiguousarray(cn.sample_states(plan, 1, 0, mc.SEED + 51, pos_m=0.1, ang_rad=0.1, vel_sigma=0.1)[:, 0])
    spread = ac.spread_field(CAP_B, CAP_N)
    counts = np.array(CAP_COUNTS, dtype=np.int32)
    paths = free_paths(cfg, plan, x0, draws(mc.SIGMA, SEED, max(CAP_S), cfg["dt"], B=CAP_B, n=CAP_N), integrator)
    shared, own = tables_along(paths, cfg["dt"], mc.SEED + 54, cc.OB_MAX, CAP_K, 0.18, aimed=CAP_AIMED, beside=(0, 2))
    far_shared, far_own = shared.copy(), own.copy()
    r = np.random.default_rng(mc.SEED + 53)
    away = lambda k: np.array([5.0, -6.0, 7.0]) * r.choice([-1.0, 1.0], (k, 3)) + r.random((k, 3))  # noqa: E731
    far_shared[CAP_NEAR:, :3] += away(cc.OB_MAX - CAP_NEAR)
    for b in range(CAP_B):
        far_own[b, 1:, :3] += away(CAP_K - 1)
        far_own[b, 1:, 3:6] *= 0.1
    return frozen(dict(cfg=cfg, plan=plan, x0=x0, spread=spread, counts=counts, shared=shared, own=cc.unused_rows(own, counts, plan),
                       far_shared=far_shared, far_own=cc.unused_rows(far_own, counts, plan)))


def restate(x, spread, integrator, S, shared, own, counts, rows=None, b0=0, desired=None):
    """mp.flight over the inputs x (of the plans `rows`, drawn as plans b0 + ...) with the given tables: (score, clear, traj), read-only"""
    rows = list(range(len(x["plan"]))) if rows is None else list(rows)
    cfg, plan = x["cfg"], x["plan"][rows]
    n = plan.shape[1]
    eps = draws(x["spread"][rows] if spread else mc.SIGMA, SEED, S, cfg["dt"], b0=b0, B=len(rows), n=n)
    want, clear, _, traj = mp.flight(plan, x["x0"][rows], eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"],
                                     cfg["desired"][:n] if desired is None else desired, integrator=integrator, shared=shared,
                                     own=[own[b, :counts[b]] for b in rows], models=[x["models"][b] for b in rows] if "models" in x else None)
    return frozen((want, clear, traj))


@functools.lru_cache(maxsize=None)
def capacity_flown(spread, integrator, tables="full"):
    """the restatement's flights of max(CAP_S) samples under the full tables ("full"), or under the near spheres of "far" alone ("short");
    a sample's draws do not depend on S, so the first 63 are the flights of S = 63"""
    x = capacity_inputs(integrator)
    if tables == "full":
        return restate(x, spread, integrator, max(CAP_S), x["shared"], x["own"], x["counts"])
    return restate(x, spread, integrator, max(CAP_S), x["far_shared"][:CAP_NEAR], x["far_own"][:, :1], np.minimum(x["counts"], 1))


def sweeps_felt(clear_by_sphere, n_shared, count, depth=1e-3):
    """of one plan's clearances (S, n, n_shared + count) to every sphere: (sweeps of 64 words of the shared table's image, of the own
    table's) that hold a whole sphere some flight is `depth` inside -- whose penalty is in that flight's cost"""
    inside = (clear_by_sphere < -depth).any(axis=(0, 1))
    sh = {(5 * j) // 64 for j in range(n_shared) if inside[j] and (5 * j) // 64 == (5 * j + 4) // 64}
    ow = {j // 8 for j in range(count) if inside[n_shared + j]}
    return sh, ow


# ---- a second tile of the per-problem table: B = 70, n = 4, K = 3

TILE_B, TILE_N, TILE_K, TILE_S, TILE_ROWS = 70, 4, 3, (5, 130), (0, 63, 64, 69)


@functools.lru_cache(maxsize=None)
def tile_inputs():
    """70 plans of 4 knots, 4 shared spheres and 3 own spheres per problem with counts[b] = (b + 1) % 4 -- 1 for rows 0 and 64, 0 for row
    63, 2 for row 69 -- sphere 0 of every problem that has one centred on the last knot of its sample 0 (of the Euler flight; the
    Runge-Kutta one ends centimetres from it), deeper than any other reaches; plan b flies with model b % 3 of mc.MODELS3"""
    cfg, plan = cn.plans(TILE_B, TILE_N, mc.SEED + 60)
    plan = np.array(plan)
    x0 = np.ascontiguousarray(cn.sample_states(plan, 1, 0, mc.SEED + 61, pos_m=0.1, ang_rad=0.1, vel_sigma=0.1)[:, 0])
    spread = ac.spread_field(TILE_B, TILE_N)
    counts = ((np.arange(TILE_B) + 1) % 4).astype(np.int32)
    models = [mc.MODELS3[b % 3] for b in range(TILE_B)]
    paths = free_paths(cfg, plan, x0, draws(mc.SIGMA, SEED, 2, cfg["dt"], B=TILE_B, n=TILE_N), 0, models=models)
    shared, own = tables_along(paths, cfg["dt"], mc.SEED + 62, 4, TILE_K, 0.3, aimed=tuple(("own", 0, b, 0) for b in range(TILE_B) if counts[b]), deep=0.3)
    return frozen(dict(cfg=cfg, plan=plan, x0=x0, spread=spread, counts=counts, shared=shared, own=cc.unused_rows(own, counts, plan), models=models))


@functools.lru_cache(maxsize=None)
def tile_flown(spread, integrator, S, rows):
    """the restatement's flights of the plans `rows` of tile_inputs(), each drawn as plan `row`: (score, clear, traj) stacked by row"""
    x = tile_inputs()
    each = [restate(x, spread, integrator, S, x["shared"], x["own"], x["counts"], rows=[b], b0=b) for b in rows]
    return frozen(tuple(np.concatenate([e[k] for e in each]) for k in range(3)))


# ---- a desired trajectory per plan: B = 3, every plan's its own and none the handle's

DES_B, DES_N, DES_S = 3, 12, 70


@functools.lru_cache(maxsize=None)
def desired_inputs():
    """mc.everything's case, and three desired trajectories of the family none of which is the handle's (desired_cases.tracking_case)"""
    host, rest, cfg, plan, x0, _ = mc.everything(5, SEED)
    _, per_plan = dc.tracking_case(DES_B, DES_N, mc.SEED + 70, shared=False)
    return host, rest, cfg, plan, x0, frozen([ac.spread_field()])[0], frozen([np.ascontiguousarray(per_plan)])[0]
