"""The cases of tests/test_gpu_linearize_keys.py: one handle per reachable k_linearize instantiation (route.h, lin_instantiated), and
what tests/test_linearize_cases_cpu.py needs to prove that the table covers them -- the weights of each kind, the restatement of what
qilqr_create, qilqr_set_integrator and qilqr_set_state_weight_schedule make of a handle for the route (host/api_handle.h: four bit-exact
predicates on Q and R and two fields of the device configuration), the inputs of a case and its restatement.  Test infrastructure only."""
import collections
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np

from quadrotorilqr_amd import problems as pb
from tests import schedule_cases as sc
from tests.composed_numpy_ilqr import ComposedILQR, ComposedLimitedILQR
from tests.independent_numpy_ilqr import Model, knot_from_state
from tests.test_gpu_batch_obstacles import moving_on
from tests.test_gpu_obstacles import spheres_on
from tests.test_gpu_parity import random_cfg

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = ("diag", "block", "sym", "qsym", "nonsym", "block_qsym")
FORCE_GENERAL = (0, 1, 2, 5, 7, 8)  # the values qilqr_create accepts in the product build
LIMITS = (0.5, 4.5)
COUNTS = np.array([3, 1, 0])  # per-problem spheres in use: one problem has none
# the extension forms of k_linearize (route.h, LIN_*): (models, shared spheres, per-problem spheres) -> the key's ext field
FORMS = {"none": (0, 0, 0), "models": (1, 0, 0), "shared": (0, 1, 0), "models+shared": (1, 1, 0), "problem": (0, 0, 1),
         "models+problem": (1, 0, 1)}
EXT = {"none": 0, "models": 1, "shared": 2, "models+shared": 3, "problem": 6, "models+problem": 7}
BW_FOUR, BW_TWO, BW_ONE, BW_FUSED = range(4)  # route.h, BackwardKind

# weights: one of WEIGHTS; schedule: None, "terminal", "dense" (every Q_i symmetric) or "nonsym" ("dense" with one non-symmetric entry)
Case = collections.namedtuple("Case", "weights integrator f32 force_general dense_weights limits models shared problem schedule")


def case(weights, form="none", integrator=0, f32=0, force_general=0, dense_weights=0, limits=0, schedule=None):
    m, s, p = FORMS[form]
    return Case(weights, integrator, f32, force_general, dense_weights, limits, m, s, p, schedule)


def name(c):
    form = "+".join(k for k, on in (("models", c.models), ("shared", c.shared), ("problem", c.problem)) if on) or "none"
    return "-".join(x for x in (c.weights, "rk4" if c.integrator else "euler", "f32" if c.f32 else "f64", form, f"fg{c.force_general}",
                                "dense_weights" if c.dense_weights else "", "limits" if c.limits else "",
                                f"sched_{c.schedule}" if c.schedule else "") if x)


# ---- the weights

def block_weights(seed, r_symmetric=True):
    """dense symmetric 6 x 6 pose and velocity blocks, an exactly zero coupling block; R dense, symmetric or not"""
    r = np.random.default_rng(70000 + seed)
    Q = np.zeros((12, 12))
    for k, scale in ((0, 4.0), (6, 0.5)):
        A = r.uniform(-1, 1, (6, 6))
        M = A @ A.T + 6 * np.eye(6)
        Q[k:k + 6, k:k + 6] = scale * 0.5 * (M + M.T)  # (M + M^T) / 2: the product's rounding is not symmetric by contract
    R = r.uniform(-0.3, 0.3, (4, 4))
    R = (R + R.T if r_symmetric else R) + 2 * np.eye(4)
    return Q, R


def config(weights, seed, n=12, B=3):
    """random_cfg's problem (model, trajectories, desired trajectory) with the weights of the kind"""
    dense = {"diag": False, "block": False, "block_qsym": False, "sym": "sym", "qsym": "qsym", "nonsym": True}[weights]
    cfg = random_cfg(seed, n=n, dense=dense, B=B)
    if weights in ("block", "block_qsym"):
        cfg["Q"], cfg["R"] = block_weights(seed, weights == "block")
    return cfg


def predicates(Q, R):
    """the four bit-exact predicates of qilqr_create: Q == Q^T, R == R^T, Q's upper-right 6 x 6 block zero, Q diagonal"""
    Q, R = np.asarray(Q), np.asarray(R)
    return dict(q_sym=bool(np.array_equal(Q, Q.T)), r_sym=bool(np.array_equal(R, R.T)), ur_zero=not Q[:6, 6:].any(),
                q_diag=not (Q - np.diag(np.diag(Q))).any())


@functools.lru_cache(maxsize=None)
def kind_predicates(weights):
    cfg = config(weights, 1, n=2, B=1)
    return predicates(cfg["Q"], cfg["R"])


def route_inputs(c, B=3):
    """what route_inputs (host/launches.h) reads of the handle the case makes, in hr_lin_route's order"""
    p, fg = kind_predicates(c.weights), c.force_general
    symmetric = p["q_sym"] and p["r_sym"] and fg != 1                  # qilqr_create
    layout_sym = p["q_sym"] and fg != 1
    layout_kind = 0 if not layout_sym else (2 if p["ur_zero"] else 1)  # make_layout, layout_kind (set_integrator keeps both flags)
    q_diag = p["q_diag"] and c.dense_weights == 0
    if c.schedule:                                                     # qilqr_set_state_weight_schedule
        symmetric = c.schedule != "nonsym" and p["r_sym"] and fg != 1
        q_diag, layout_kind = False, 0
    return [int(x) for x in (symmetric, q_diag, layout_kind, c.f32, c.integrator, c.limits, c.models, c.shared or c.problem, c.problem,
                             c.schedule is not None, fg, B)]


def accepted(c):
    """the setters' refusals (host/api_handle.h): every extension on fp32; limits on non-symmetric weights, or beside a non-symmetric
    schedule (with a symmetric schedule the handle's own Q need not be symmetric, R must)"""
    if c.f32 and (c.integrator or c.limits or c.models or c.shared or c.problem or c.schedule):
        return False
    if c.limits:
        p = kind_predicates(c.weights)
        if c.schedule:
            return c.schedule != "nonsym" and p["r_sym"] and c.force_general != 1
        return p["q_sym"] and p["r_sym"] and c.force_general != 1
    return True


def every_input():
    """the whole public input space of the route of k_linearize"""
    for w, fg, dw, integ, f32, lim, (m, s, p), sched in itertools.product(WEIGHTS, FORCE_GENERAL, (0, 1), (0, 1), (0, 1), (0, 1),
                                                                          itertools.product((0, 1), repeat=3), (None, "dense", "nonsym")):
        c = Case(w, integ, f32, fg, dw, lim, m, s, p, sched)
        if accepted(c):
            yield c


@functools.lru_cache(maxsize=None)
def harness():
    so, src = os.path.join(HERE, "libhost_route_harness.so"), os.path.join(HERE, "host_route_harness.cpp")
    deps = [src, os.path.join(HERE, "..", "quadrotorilqr_amd", "csrc", "route.h"), os.path.join(HERE, "..", "include", "quadrotor_ilqr.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hr_lin_route.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    return lib


def route(c, B=3):
    """(key {lin_kind, integrator, tiled, f32, ext}, backward kind, admitted) of a call of B problems on the case's handle"""
    inp, out = np.array(route_inputs(c, B), dtype=np.int64), np.zeros(7, dtype=np.int64)
    assert harness().hr_lin_route(inp.ctypes.data_as(C.POINTER(C.c_long)), out.ctypes.data_as(C.POINTER(C.c_long))) == 7
    return tuple(out[:5].tolist()), int(out[5]), bool(out[6])


# ---- what qilqr_describe says of the route, from the case's own fields (no route.h: tests/test_linearize_cases_cpu.py compares)

def general(c):
    """the reference's own forms: the general kernel"""
    return c.weights in ("qsym", "nonsym", "block_qsym") or c.force_general == 1 or c.schedule == "nonsym"


def one_wavefront(c):
    return bool(general(c) or c.integrator or c.limits or c.models or c.schedule or c.force_general == 2)


def expected_text(c, B=3):
    """the parts of qilqr_describe(B) the GPU tests assert: the arithmetic form, the backward kernel, the precision"""
    arith = "arithmetic: the reference's own forms" if general(c) else "arithmetic: symmetric-weight forms"
    sym = "false>" if general(c) else "true>"
    if not one_wavefront(c):
        kernel = "backward: k_backward4, fused" if c.force_general in (0, 5) and B <= 4096 else "backward: k_backward4, six wavefronts"
    elif c.models:
        kernel = "backward: k_backward_models<" + sym + (" box form" if c.limits else "") + ", one wavefront per trajectory"
    elif c.limits:
        kernel = "backward: k_backward<true> box form, one wavefront per trajectory"
    else:
        kernel = "backward: k_backward<" + sym + ", one wavefront per trajectory"
    return arith, kernel, "; mixed precision" if c.f32 else "; fp64; "


def text_from_route(c, B=3):
    """the same parts as host/describe.h derives them from the route: from the harness's backward kind and the restated `symmetric`"""
    _, bw, _ = route(c, B)
    symmetric = bool(route_inputs(c, B)[0])
    arith = "arithmetic: the reference's own forms" if bw == BW_ONE and not symmetric else "arithmetic: symmetric-weight forms"
    sym = "true>" if symmetric else "false>"
    kernel = "backward: " + ("k_backward4, fused" if bw == BW_FUSED else "k_backward4, six wavefronts" if bw == BW_FOUR else "k_backward2" if bw == BW_TWO
                             else "k_backward_models<" + sym + (" box form" if c.limits else "") + ", one wavefront per trajectory" if c.models
                             else "k_backward<true> box form, one wavefront per trajectory" if c.limits
                             else "k_backward<" + sym + ", one wavefront per trajectory")
    return arith, kernel, "; mixed precision" if c.f32 else "; fp64; "


def recursion(c):
    """the restatement's recursion of the case: 0 (the reference's forms) for the general kernel, 1 otherwise"""
    return 0 if general(c) else 1


# ---- the table

def _table():
    t = []
    for form in FORMS:
        for integ in (0, 1):
            # the one-wavefront kernels' plain records: every kind, either integrator, every form
            for w in ("diag", "block", "sym", "nonsym"):
                t.append(case(w, form, integ, force_general=2))
            if integ == 0 and FORMS[form][0] == 0:  # tiled records: the symmetric kinds without models
                for w in ("diag", "block", "sym"):
                    t.append(case(w, form, 0))
        # kind 2 through dense_weights = 1 on a diagonal Q, and kinds 0, 1 and 2 through the other roads to them
        t.append(case("diag", form, 0, dense_weights=1, force_general=2))
    t += [case("qsym", "shared"), case("block_qsym", "problem"), case("block_qsym", "models", 1), case("sym", "models+shared", force_general=1),
          case("block", "shared", force_general=5), case("sym", "problem", force_general=8), case("block", "none", force_general=7),
          case("diag", "none", dense_weights=1)]
    # thrust limits: the box form reads the same records (kinds 1, 2 and 3, plain)
    t += [case("sym", "shared", limits=1), case("block", "problem", limits=1), case("diag", "models+problem", limits=1),
          case("block", "models+shared", 1, limits=1)]
    # a schedule: dense records of kind 0 whatever the weights, every extension form
    t += [case("diag", "none", schedule="dense"), case("block", "models", schedule="terminal"), case("sym", "shared", 1, schedule="dense"),
          case("block", "models+shared", schedule="nonsym"), case("diag", "problem", schedule="terminal"),
          case("block_qsym", "models+problem", 1, schedule="dense"), case("sym", "problem", schedule="dense", limits=1)]
    # the mixed mode: kinds 0, 1 and 2 (a diagonal Q takes kind 2 there), both placements where both exist
    t += [case("diag", f32=1, force_general=2), case("block", f32=1), case("sym", f32=1), case("sym", f32=1, force_general=2),
          case("nonsym", f32=1)]
    assert len(set(t)) == len(t)
    return tuple(t)


TABLE = _table()
F64 = tuple(c for c in TABLE if not c.f32)
F32 = tuple(c for c in TABLE if c.f32)


# ---- the inputs of a case and its restatement

def seed_of(c):
    return 4000 + TABLE.index(c)


def past_the_first(trajs, table, counts, dt):
    """every problem with spheres of its own has a knot from the third on inside one of them.  (A sphere's term at knot i changes the
    position block of V_xx(i) alone, and the Euler step's J_u has no position rows: it enters the gains of the knots up to i - 2.  One that
    reaches knots 0 and 1 only moves the cost and no gain, and the comparison of the gains would not see whose sphere it was.)"""
    for b in range(len(trajs)):
        own = np.asarray(table[b, :counts[b]], dtype=float)
        hit = any((np.linalg.norm(trajs[b, i, 1:4] - (own[:, :3] + i * dt * own[:, 3:6]), axis=1) < own[:, 6]).any() for i in range(2, trajs.shape[1]))
        if counts[b] and not hit:
            return False
    return True


def inputs(c, n=12, B=3, seed=None):
    """the fp64 cases' problem: random_cfg's trajectories and desired trajectory, and whatever the case sets on the handle"""
    seed = seed_of(c) if seed is None else seed
    cfg = config(c.weights, seed, n=n, B=B)
    trajs = cfg["init"]
    x = dict(cfg=cfg, trajs=trajs, limits=LIMITS if c.limits else None, mods=None, shared=None, table=None, counts=None, Qs=None)
    if c.models:
        x["mods"] = [dict(cfg["model"], mass_kg=cfg["model"]["mass_kg"] * (0.8 + 0.1 * (b % 7)), arm_length_m=0.7 - 0.02 * (b % 5)) for b in range(B)]
    for attempt in range(50):  # (the first draw that puts a knot from the third on into one of the problem's own spheres: see past_the_first)
        r = np.random.default_rng(90000 + seed + 1000 * attempt)
        if c.shared:
            x["shared"] = spheres_on(trajs, r)
        if c.problem:
            x["table"] = moving_on(trajs, cfg["dt"], r)
            x["counts"] = np.resize(COUNTS, B)
        if not c.problem or n < 3 or past_the_first(trajs, x["table"], x["counts"], cfg["dt"]):
            break
    else:
        raise AssertionError("no draw of the spheres meets the condition")
    if c.schedule:
        x["Qs"] = sc.schedule("terminal" if c.schedule == "terminal" else "dense", n)
        if c.schedule == "nonsym":
            x["Qs"] = sc.one_nonsymmetric(x["Qs"])
    return x


def restatement(c, x, b, cfg=None):
    """the composed restatement of problem b of the case's inputs"""
    cfg = cfg or x["cfg"]
    m = Model(**(x["mods"][b] if x["mods"] else cfg["model"]))
    if x["limits"] is None:
        o = ComposedILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), integrator=c.integrator, recursion=recursion(c))
    else:  # (the box form is the symmetric recursion)
        o = ComposedLimitedILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), *x["limits"], integrator=c.integrator)
    if x["shared"] is not None:
        o.set_obstacles(x["shared"])
    if x["table"] is not None:
        o.set_problem_obstacles(x["table"][b, :x["counts"][b]])
    o.set_state_weight_schedule(x["Qs"])
    return o


def handle(capi, c, x, cfg=None, rows=None, **kw):
    """the device handle of the case (rows: the problems of x it holds, all by default)"""
    cfg = cfg or x["cfg"]
    rows = np.arange(len(x["trajs"])) if rows is None else np.asarray(rows)
    s = capi.from_config(cfg, force_general=c.force_general, dense_weights=c.dense_weights, precision="f32" if c.f32 else "f64", **kw)
    s.set_integrator(c.integrator)
    if x["limits"]:
        s.set_control_limits(*x["limits"])
    if x["mods"]:
        s.set_models([x["mods"][b] for b in rows])
    if x["shared"] is not None:
        s.set_obstacles(x["shared"])
    if x["table"] is not None:
        s.set_batch_obstacles(x["table"][rows], x["counts"][rows])
    if x["Qs"] is not None:
        s.set_state_weight_schedule(x["Qs"])
    return s


def compare_passes(s, c, x, rows=None, trajs=None, restated=None):
    """cost_trajectory, backwards_pass and line_search of the handle against the composed restatement, problem by problem, at the bars of the
    suite's pass tests.  rows: the problems to compare (all by default); restated(b): the restatement of problem b (restatement(c, x, b) by
    default).  Every figure is printed before it is asserted."""
    from tests.test_gpu_obstacles import split_gains
    trajs = x["trajs"] if trajs is None else trajs
    opt = x["cfg"]["options"]
    cost = s.cost_trajectory(trajs)
    gains, terms = s.backwards_pass(trajs)
    ls = s.line_search(trajs, cost, gains, terms)
    for b in (range(len(trajs)) if rows is None else rows):
        o = restated(b) if restated else restatement(c, x, b)
        pts = o.unpack(trajs[b])
        want = o.cost_trajectory(pts)
        ks, Ks, t = o.backwards_pass(pts)
        ks, Ks, t = np.array(ks), np.array(Ks), np.array(t)
        k_dev, K_dev = split_gains(gains[b])
        scale = max(np.abs(ks).max(), np.abs(Ks).max())
        print("%s problem %d: cost rel %.2e, gains abs/scale %.2e, terms rel %.2e" %
              (name(c), b, abs(cost[b] - want) / abs(want), max(np.abs(k_dev - ks).max(), np.abs(K_dev - Ks).max()) / scale,
               np.max(np.abs(terms[b] - t) / np.maximum(np.abs(t), 1e-300))))
        np.testing.assert_allclose(cost[b], want, rtol=1e-10)
        np.testing.assert_allclose(k_dev, ks, rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(K_dev, Ks, rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(terms[b], t, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(t).max()))
        # the line search: the step and the cost of the accepted candidate against the restatement's search with the device's gains
        step, found = 1.0, False
        for _ in range(opt["ls_max_iters"]):
            cand = o.cost_trajectory(o.forward_sim(pts, list(k_dev), list(K_dev), step))
            if cand - cost[b] < opt["desired_reduction_frac"] * (step * terms[b][0] + step * step * terms[b][1] / 2.0):
                found = True
                break
            step *= opt["step_update"]
        assert (ls["status"][b] == 0) == found, b
        if found:
            assert ls["step"][b] == step, b
            np.testing.assert_allclose(ls["cost"][b], cand, rtol=1e-9)
    return cost, gains, terms


# ---- the mixed mode: config3's problems with the case's weights, and how far fp32 inputs move the fp64 restatement

MIXED_BARS = dict(cost=2e-5, terms=2e-3, gains=1e-3)  # test_config3_mixed_precision_reduced's per-pass bars
# the new cases' weights: (seed of config()'s weights, scale of their off-diagonal part), chosen on the CPU among seeds 3 ... 8 and scales
# +-0.5 with the restatement alone, for a margin no smaller than config3's own (mixed_config; tests/test_linearize_cases_cpu.py)
MIXED_WEIGHTS = {"block": (3, 0.5), "sym": (6, -0.5), "nonsym": (6, -0.5)}


def mixed_config(c, B=3, N=20):
    """pb.config3(B, N) with the case's weights put in (None: its own).  The weights keep config3's diagonal and take the off-diagonal
    structure of the kind's weights (config(); MIXED_WEIGHTS has the seed and the scale s): entry (i, k) is s w_ik sqrt(d_i d_k / (w_ii w_kk)) with d config3's diagonal,
    a congruence that keeps symmetry, zeros and definiteness; then every entry is rounded to fp32, as config3's own weights are fp32
    numbers.  That brings the deviation of the fp32-rounded restatement, relative to the bars, to config3's own
    (tests/test_linearize_cases_cpu.py asserts it; DESIGN.md section 6 has the ratios)."""
    cfg = pb.config3(B=B, N=N)
    if c is not None and c.weights != "diag":
        seed, off = MIXED_WEIGHTS[c.weights]
        w = config(c.weights, seed, n=2, B=1)
        for k in ("Q", "R"):
            d, wd = np.diag(cfg[k]), np.diag(w[k])
            scale = np.sqrt(np.outer(d, d) / np.outer(wd, wd))
            m = np.diag(d) + off * (w[k] - np.diag(wd)) * scale
            cfg[k] = m.astype(np.float32).astype(np.float64)  # (elementwise: symmetry and zeros stay)
        assert predicates(cfg["Q"], cfg["R"]) == kind_predicates(c.weights)
    return cfg


def mixed_restatement(c, cfg):
    o = ComposedILQR(Model(**cfg["model"]), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]),
                     recursion=recursion(c) if c is not None else 1)
    return o


def f32_rounded(cfg):
    """the config as the mixed mode stores it: weights, model, desired trajectory and trajectories rounded to fp32"""
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    out = dict(cfg, Q=rd(cfg["Q"]), R=rd(cfg["R"]), desired=rd(cfg["desired"]), init=rd(cfg["init"]))
    out["model"] = {k: (rd(v) if k == "inertia" else float(np.float32(v))) for k, v in cfg["model"].items()}
    return out


def mixed_trajs(c, cfg):
    """the trajectories of the mixed-mode passes: every problem rolled out from its start with zero gains, as
    test_config3_mixed_precision_reduced takes them (config3's initial trajectories sit on the desired one from knot 1 on: every gain term
    is zero there), by the fp64 restatement"""
    o = mixed_restatement(c, cfg)
    n = cfg["init"].shape[1]
    out = []
    for t in cfg["init"]:
        pts = o.forward_sim(o.unpack(t), [np.zeros(4)] * n, [np.zeros((4, 12))] * n, 1.0)
        out.append([knot_from_state(t[j, 0], T, v, u) for j, (T, v, u) in enumerate(pts)])
    return np.array(out)


def mixed_passes(c, cfg, traj):
    """(cost, gains as one array, terms) of a trajectory by the fp64 restatement"""
    o = mixed_restatement(c, cfg)
    pts = o.unpack(traj)
    ks, Ks, t = o.backwards_pass(pts)
    return o.cost_trajectory(pts), np.concatenate([np.array(ks).ravel(), np.array(Ks).ravel()]), np.array(t)


def mixed_margins(c, B=3, N=20):
    """bar / deviation for cost, terms and gains: the deviation of the restatement under fp32-rounded inputs, in each bar's own measure,
    the worst of the B problems"""
    cfg = mixed_config(c, B, N)
    low, trajs = f32_rounded(cfg), mixed_trajs(c, cfg)
    dev = dict(cost=0.0, terms=0.0, gains=0.0)
    for b in range(B):
        c64, g64, t64 = mixed_passes(c, cfg, trajs[b])
        c32, g32, t32 = mixed_passes(c, low, trajs[b].astype(np.float32).astype(np.float64))
        dev["cost"] = max(dev["cost"], abs(c32 - c64) / abs(c64))
        dev["terms"] = max(dev["terms"], np.max(np.abs(t32 - t64) / np.abs(t64)))
        dev["gains"] = max(dev["gains"], np.max(np.abs(g32 - g64)) / np.max(np.abs(g64)))
    return {k: MIXED_BARS[k] / dev[k] for k in dev}
