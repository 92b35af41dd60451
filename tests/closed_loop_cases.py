"""The cases of tests/test_gpu_closed_loop_cases.py: one per instantiation of k_closed_loop (closed_loop_kernels.h, 16) and of
k_closed_loop_scored (closed_loop_scored_kernels.h, 48) -- {Euler, Runge-Kutta} x {flattened, shared-operand form} x {wrench} x {score} x
{thrust limits} x {per-sample models} -- with the name of the kernel each case launches (tests/test_closed_loop_cases_cpu.py proves the map
one to one against the compiled units), the small inputs the cases share, the handle of a case, and what the tests of the full tables and
of the second tile need: guarded device outputs, the restatement's commanded thrusts and nearest spheres.  Test infrastructure only."""
import collections
import functools
import itertools
import re

import numpy as np

from oracle import oracle as orc
from quadrotorilqr_amd import problems as pb
from tests import closed_loop_numpy as cn, moving_obstacle_numpy_ilqr as mov
from tests.test_gpu_closed_loop import MODELS3

SEED = 33
B, N = 2, 6
S_SHARED, S_FLAT = 63, 5  # closed_loop_shared_form: 63 is the shared-operand form's smallest S (one idle lane), 5 takes the flattened one
LIMITS = (1.0, 4.0)
OB_MAX = 64  # QILQR_MAX_OBSTACLES: the spheres a table holds, and the LDS image of the shared-operand form
GUARD = 64  # bytes behind the end of every device output, prefilled with 0xFF like the output (tests/test_gpu_risk.py)

Case = collections.namedtuple("Case", "integrator shared wrench score limits models")
CASES = tuple(Case(i, sh, w, sc, lim, m) for i, sh, lim, m, w, sc in itertools.product((0, 1), (False, True), (False, True), (False, True),
                                                                                      (False, True), (False, True)))


def name(c):
    ext = "+".join(k for k, on in (("limits", c.limits), ("models", c.models)) if on) or "plain"
    switches = "+".join(k for k, on in (("wrench", c.wrench), ("score", c.score)) if on) or "calm"
    return "-".join(("rk4" if c.integrator else "euler", "shared" if c.shared else "flat", ext, switches))


def samples(c):
    """the S of the case's form"""
    return S_SHARED if c.shared else S_FLAT


def group(c):
    """what the restatement's flights depend on: the wrench and score variants of one group share them"""
    return c.integrator, c.shared, c.limits, c.models


# ---- the kernel of a case, by its symbol (the Itanium mangling of the template arguments: Li<int>E, Lb<0|1>E, J<types>E for the pack)

_PACK = {(False, False): "", (True, False): "NS_13ControlLimitsE", (False, True): "NS_11BatchModelsE",
         (True, True): "NS_13ControlLimitsENS_11BatchModelsE"}  # (ControlLimits first: launch_ext.h, with_extensions)


def kernel_name(c):
    """the symbol of the kernel a call of the case launches: k_closed_loop<INTEG, SHARED, Lim...> without a wrench and a score
    (launch_closed_loop_scored hands those to launch_closed_loop), else k_closed_loop_scored<INTEG, SHARED, WRENCH, SCORE, Lim...>"""
    pack = "J%sE" % _PACK[(c.limits, c.models)]
    if not (c.wrench or c.score):
        return "_ZN5qilqr13k_closed_loopILi%dELb%dE%sEEvNS_11ModelConstsIdEENS_14ClosedLoopArgsEDpT1_" % (c.integrator, c.shared, pack)
    return ("_ZN5qilqr20k_closed_loop_scoredILi%dELb%dELb%dELb%dE%sEEvNS_11ModelConstsIdEENS_14ClosedLoopArgsENS_19ClosedLoopScoreArgsEDpT3_"
            % (c.integrator, c.shared, c.wrench, c.score, pack))


_SYMBOL = re.compile(r"^_ZN5qilqr(?:13k_closed_loopILi([01])ELb([01])E|20k_closed_loop_scoredILi([01])ELb([01])ELb([01])ELb([01])E)J((?:NS_\d+[A-Za-z]+E)*)EEEv")


def case_of(symbol):
    """the case whose template arguments the symbol of a built kernel spells, read from the mangled name alone; None: not one of the family"""
    m = _SYMBOL.match(symbol)
    if not m:
        return None
    types = re.findall(r"NS_\d+([A-Za-z]+)E", m.group(7))
    if not set(types) <= {"ControlLimits", "BatchModels"} or len(set(types)) != len(types):
        return None
    lim, mod = "ControlLimits" in types, "BatchModels" in types
    if m.group(1) is not None:
        return Case(int(m.group(1)), m.group(2) == "1", False, False, lim, mod)
    return Case(int(m.group(3)), m.group(4) == "1", m.group(5) == "1", m.group(6) == "1", lim, mod)


# ---- the inputs the cases share

def spheres_about(plan, x0, seed, n_shared=8, K=2, counts=None, aim=(), aim_at=(0.08, 0.16)):
    """(shared (n_shared, 5), own (B, K, 8), counts): spheres about the plans' paths in the style of
    tests/test_gpu_scored_flight.py's spheres_on_the_way -- shared ones beside plan knots, moving ones per problem -- and, so that small
    sets of samples hold flights that hit, one sphere per entry of `aim` beside a sample's start: ("shared", j, b, sample) or
    ("own", j, b, sample) puts sphere j (of problem b's own table, at rest) aim_at[0] m from the start of sample (b, sample) with radius
    aim_at[1]"""
    Bp, n = plan.shape[0], plan.shape[1]
    r = np.random.default_rng(seed)
    shared = np.zeros((n_shared, 5))
    for j in range(n_shared):
        b, i = j % Bp, (1 + 2 * j) % n
        shared[j, :3] = plan[b, i, 1:4] + 0.45 * (2.0 * r.random(3) - 1.0)
        shared[j, 3] = 0.12 + 0.04 * (j % 3)
        shared[j, 4] = 20.0 + 5.0 * (j % 9)
    own = np.zeros((Bp, K, 8))
    for b in range(Bp):
        for j in range(K):
            own[b, j, :3] = plan[b, (2 + j) % n, 1:4] + 0.4 * (2.0 * r.random(3) - 1.0)
            own[b, j, 3:6] = 0.5 * (2.0 * r.random(3) - 1.0)
            own[b, j, 6:8] = (0.14 + 0.03 * (j % 3), 30.0 + 2.0 * (j % 7))
    for kind, j, b, sample in aim:
        d = r.standard_normal(3)
        at = x0[b, sample, 0:3] + aim_at[0] * d / np.linalg.norm(d)
        if kind == "shared":
            shared[j, :4] = (*at, aim_at[1])
        else:
            own[b, j, :3], own[b, j, 3:6], own[b, j, 6] = at, 0.0, aim_at[1]
    counts = np.full(Bp, K, dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    return shared, own, counts


def device_gains(cfg, plan):
    """(B, n, 52): the backward pass of a plain handle about the plans (needs the device)"""
    from quadrotorilqr_amd import capi
    gains, _ = capi.from_config(cfg).backwards_pass(plan)
    return gains


@functools.lru_cache(maxsize=None)
def inputs(gains_of=device_gains):
    """the inputs of the 64 cases, built once and read-only: plans (B = 2, n = 6), the gains of the handle's backward pass (gains_of:
    tests on the CPU pass closed_loop_numpy.oracle_gains), 63 sampled start states per plan -- sample 1 starts where sample 0 does, so that
    two models show on one state -- per-knot gusts and the two sphere tables.  The flattened form's S = 5 takes the first five samples."""
    cfg, plan = cn.plans(B, N, SEED)
    gains = np.ascontiguousarray(gains_of(cfg, plan))
    x0 = cn.sample_states(plan, S_SHARED, 0, SEED + 1)
    x0[:, 1] = x0[:, 0]
    gust = pb.gust_wrenches(B, S_SHARED, N, SEED + 2, 1.5, 0.05)
    shared, own, counts = spheres_about(plan, x0, SEED + 3, counts=(2, 1), aim=(("shared", 0, 0, 2), ("own", 0, 1, 3)))
    x = dict(cfg=cfg, plan=plan, gains=gains, x0=x0, gust=gust, shared=shared, own=own, counts=counts)
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def models_for(Bp, S):
    """B S models cycled from MODELS3: model b S + j flies sample (b, j), so neighbouring samples never share one"""
    return [MODELS3[r % 3] for r in range(Bp * S)]


def configure(s, c, x, Bp=B):
    """the case's switches on a handle: the integrator, the thrust limits, the per-sample models, and with a score both sphere tables"""
    s.set_integrator(c.integrator)
    if c.limits:
        s.set_control_limits(*LIMITS)
    if c.models:
        s.set_models(models_for(Bp, samples(c)))
    if c.score:
        s.set_obstacles(x["shared"])
        s.set_batch_obstacles(x["own"], x["counts"])
    return s


def own_rows(own, counts):
    """the rows in use of every problem's own table, as the restatement takes them"""
    return [own[b, :counts[b]] for b in range(len(own))]


# ---- tables at capacity: B = 3, n = 6, 64 shared spheres and K = 64 spheres per problem with counts 64, 0 and 37

CAP_B, CAP_K, CAP_COUNTS = 3, 64, (64, 0, 37)
CAP_AIMED = (("shared", 63, 1, 4), ("own", 63, 0, 3), ("own", 36, 2, 2))  # the last sphere in use of each table, beside a sample < S_FLAT
CAP_NEAR = 8  # the shared spheres the reduced tables keep (and sphere 0 of every problem's own)


def unused_rows(own, counts, plan):
    """rows at and beyond counts[b]: a sphere at rest centred on a plan knot, radius 1, weight 1e6 -- finite, and ruinous if it were read"""
    own = own.copy()
    for b in range(len(own)):
        for j in range(counts[b], own.shape[1]):
            own[b, j] = (*plan[b, j % plan.shape[1], 1:4], 0.0, 0.0, 0.0, 1.0, 1e6)
    return own


@functools.lru_cache(maxsize=None)
def capacity_inputs(gains_of=device_gains):
    """plans, gains, 63 start states and gusts per plan, and two placements of full tables.  "full": spheres about the paths, the last one
    in use of each table deepest in a sample's way (CAP_AIMED).  "far": the first CAP_NEAR shared spheres and every problem's own sphere 0
    as in "full", every other sphere in use 5 m and more off the paths -- never within 1 m of a flight, so a call with only the near ones
    computes the same."""
    cfg, plan = cn.plans(CAP_B, N, SEED + 10)
    gains = np.ascontiguousarray(gains_of(cfg, plan))
    x0 = cn.sample_states(plan, S_SHARED, 0, SEED + 11)
    gust = pb.gust_wrenches(CAP_B, S_SHARED, N, SEED + 12, 1.5, 0.05)
    counts = np.array(CAP_COUNTS, dtype=np.int32)
    # (the aimed spheres: 0.02 m from the start, radius 0.3 -- a clearance of -0.28 where no other sphere's radius reaches 0.21)
    shared, own, _ = spheres_about(plan, x0, SEED + 13, n_shared=OB_MAX, K=CAP_K, aim=CAP_AIMED, aim_at=(0.02, 0.3))
    far_shared, far_own = shared.copy(), own.copy()
    r = np.random.default_rng(SEED + 14)
    away = lambda k: np.array([5.0, -6.0, 7.0]) * r.choice([-1.0, 1.0], (k, 3)) + r.random((k, 3))  # noqa: E731
    far_shared[CAP_NEAR:, :3] += away(OB_MAX - CAP_NEAR)
    for b in range(CAP_B):
        far_own[b, 1:, :3] += away(CAP_K - 1)
        far_own[b, 1:, 3:6] *= 0.1
    x = dict(cfg=cfg, plan=plan, gains=gains, x0=x0, gust=gust, counts=counts, shared=shared, own=unused_rows(own, counts, plan),
             far_shared=far_shared, far_own=unused_rows(far_own, counts, plan))
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


# ---- a second tile of the per-problem table: B = 70, n = 4, K = 3

TILE_B, TILE_N, TILE_K, TILE_ROWS = 70, 4, 3, (0, 63, 64, 69)


@functools.lru_cache(maxsize=None)
def tile_inputs(gains_of=device_gains):
    """70 plans of 4 knots, 63 start states and gusts per plan, 4 shared spheres and 3 own spheres per problem with counts[b] = (b + 1) % 4
    -- 1 for rows 0 and 64, 0 for row 63, 2 for row 69 -- sphere 0 of every problem that has one deepest in the way of its sample 0"""
    cfg, plan = cn.plans(TILE_B, TILE_N, SEED + 20)
    gains = np.ascontiguousarray(gains_of(cfg, plan))
    x0 = cn.sample_states(plan, S_SHARED, 0, SEED + 21)
    gust = pb.gust_wrenches(TILE_B, S_SHARED, TILE_N, SEED + 22, 1.5, 0.05)
    counts = ((np.arange(TILE_B) + 1) % 4).astype(np.int32)
    shared, own, _ = spheres_about(plan, x0, SEED + 23, n_shared=4, K=TILE_K, aim=tuple(("own", 0, b, 0) for b in range(TILE_B) if counts[b]),
                                   aim_at=(0.02, 0.3))
    x = dict(cfg=cfg, plan=plan, gains=gains, x0=x0, gust=gust, counts=counts, shared=shared, own=unused_rows(own, counts, plan))
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


# ---- what the exact comparisons are conditioned on, from the restatement's own flights

def commanded(plan, gains, traj):
    """(B, S, n, 4): the thrusts the law commands at the flown states of traj (B, S, n, 18), before any clamp: u_i + K_i (x (-) plan_i), the
    restatement's own operations on its own states"""
    _, K = orc.gains_to_kK(np.asarray(gains, dtype=np.float64))
    u = np.empty(traj.shape[:3] + (4,))
    for b, j, i in np.ndindex(*traj.shape[:3]):
        u[b, j, i] = plan[b, i, 14:18] + K[b, i] @ orc.state_minus(traj[b, j, i, 1:14], plan[b, i, 1:14])
    return u


def limit_margin(u, limits=LIMITS):
    """the least distance of a commanded thrust from either bound"""
    return float(min(np.abs(u - limits[0]).min(), np.abs(u - limits[1]).min()))


def clearances(traj, dt, shared, own):
    """(S, n, n_shared + K_b): the clearance |p - c| - radius of every flown knot of one plan's flights traj (S, n, 18) to every shared
    sphere and then every one of the plan's own spheres own (K_b, 8), at the knot's time"""
    out = np.empty(traj.shape[:2] + (len(shared) + len(own),))
    for i in range(traj.shape[1]):
        sp = np.vstack([np.asarray(shared, dtype=np.float64).reshape(-1, 5), mov.at_time(np.asarray(own, dtype=np.float64).reshape(-1, 8), i * dt)])
        out[:, i] = np.linalg.norm(traj[:, i, None, 1:4] - sp[None, :, 0:3], axis=2) - sp[None, :, 3]
    return out


def nearest_sphere(traj, dt, shared, own):
    """(S,): the sphere of the smallest clearance over each flight (an index into the shared table followed by the plan's own)"""
    c = clearances(traj, dt, shared, own)
    return c.min(axis=1).argmin(axis=1)


def over(got, want, rtol, atol):
    """the largest error over its bound"""
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


# ---- device calls on plain buffers with guarded outputs

def scored_device(hip, s, plan, gains, x0, wrench=None, score=True):
    """one call of qilqr_closed_loop_scored_device over all knots on 0xFF-prefilled outputs with a guard behind each: (traj, stats, score or
    None, whether every guard kept its bits).  Without a wrench and a score the three new arguments are NULL."""
    from quadrotorilqr_amd import capi
    Bp, n, S = plan.shape[0], plan.shape[1], x0.shape[1]
    lib = capi.load()
    d = [hip.upload(a) for a in (plan, gains, x0)]
    d_w = hip.upload(wrench) if wrench is not None else None
    shapes = [(Bp, S, n, 18), (Bp, S, 4)] + ([(Bp, S, 4)] if score else [])
    outs = [hip.alloc(8 * int(np.prod(sh)) + GUARD) for sh in shapes]
    rc = lib.qilqr_closed_loop_scored_device(s._h, d[0], d[1], d[2], d_w, 1 if wrench is None else wrench.shape[2], None, Bp, n, S, 0, n - 1,
                                             outs[0], outs[1], outs[2] if score else None)
    assert rc == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    got, kept = [], True
    for ptr, sh in zip(outs, shapes):
        nbytes = 8 * int(np.prod(sh))
        raw = hip.download(ptr, (nbytes + GUARD,), dtype=np.uint8)
        got.append(raw[:nbytes].view(np.float64).reshape(sh))
        kept = kept and bool((raw[nbytes:] == 0xFF).all())
    return got[0], got[1], got[2] if score else None, kept
