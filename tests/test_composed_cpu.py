"""The composed restatement (tests/composed_numpy_ilqr.py: schedule, shared spheres and the problem's own moving spheres in one knot cost)
without a device: it is each of the restatements it composes when the other table is empty, bit for bit; its differentials against central
differences of its own cost; and the inputs of the GPU comparisons (tests/test_gpu_linearize_keys.py, tests/test_gpu_composed.py) tell the
right index from each wrong one by a thousand times the comparison's tolerance."""
import numpy as np
import pytest

from tests import composed_cases as cc, linearize_cases as lc, schedule_cases as sc
from tests.composed_numpy_ilqr import ComposedILQR, ComposedLimitedILQR
from tests.independent_numpy_ilqr import Model, se3_exp
from tests.moving_obstacle_numpy_ilqr import MovingObstacleILQR, MovingObstacleLimitedILQR, at_time
from tests.schedule_numpy_ilqr import ScheduleILQR, ScheduleLimitedILQR
from tests.test_gpu_batch_obstacles import reached
from tests.test_gpu_obstacles import spheres_on

COST_TOL, GAIN_TOL = 1e-10, 1e-8  # the GPU comparison's relative bars: the cost, and the gains against their largest entry
FACTOR = 1000.0


def same_bits(a, b):
    for k in ("status", "iters", "n_bwd", "n_fwd", "cost"):
        assert a[k] == b[k], k
    assert np.array_equal(a["traj"], b["traj"]) and np.array_equal(a["cost_hist"], b["cost_hist"])


def same_passes(a, b, pts):
    assert a.cost_trajectory(pts) == b.cost_trajectory(pts)
    for x, y in zip(a.backwards_pass(pts), b.backwards_pass(pts)):
        assert np.array_equal(np.array(x), np.array(y))
    for i in (0, len(pts) // 2, len(pts) - 1):
        (ca, Ca), (cb, Cb) = a.cost_knot_diffs(*pts[i], i), b.cost_knot_diffs(*pts[i], i)
        assert ca == cb and all(np.array_equal(Ca[k], Cb[k]) for k in Ca)


# ---- reductions

@pytest.mark.parametrize("recursion,integrator,limits", [(0, 0, None), (1, 0, None), (1, 1, None), (1, 0, (0.5, 4.5)), (1, 1, (0.5, 4.5))])
def test_without_spheres_of_its_own_it_is_the_schedule_restatement(recursion, integrator, limits):
    N = 12
    cfg = sc.config(N)
    Qs = sc.schedule("dense", N) if recursion else sc.one_nonsymmetric(sc.schedule("dense", N))
    shared = spheres_on(cfg["init"], np.random.default_rng(3), 2)
    m = Model(**cfg["model"])
    args = (m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]))
    if limits:
        ref, o = ScheduleLimitedILQR(*args, *limits, integrator=integrator), ComposedLimitedILQR(*args, *limits, integrator=integrator)
    else:
        ref, o = (cls(*args, integrator=integrator, recursion=recursion) for cls in (ScheduleILQR, ComposedILQR))
    for x in (ref, o):
        x.set_obstacles(shared)
        x.set_state_weight_schedule(Qs)
    same_passes(ref, o, ref.unpack(cfg["init"][1]))
    same_bits(ref.solve(cfg["init"][0]), o.solve(cfg["init"][0]))


@pytest.mark.parametrize("limits", [None, (0.5, 4.5)])
@pytest.mark.parametrize("integrator", [0, 1])
def test_without_a_schedule_it_is_the_moving_sphere_restatement(integrator, limits):
    x = cc.solve_inputs(12, False)
    cfg = x["cfg"]
    shared = spheres_on(cfg["init"], np.random.default_rng(4), 2)
    args = (Model(**cfg["model"]), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]))
    if limits:
        ref, o = MovingObstacleLimitedILQR(*args, *limits, integrator=integrator), ComposedLimitedILQR(*args, *limits, integrator=integrator)
    else:
        ref, o = MovingObstacleILQR(*args, integrator=integrator), ComposedILQR(*args, integrator=integrator)
    for y in (ref, o):
        y.set_obstacles(shared)
        y.set_problem_obstacles(x["table"][0])
    assert o.Qs is None
    same_passes(ref, o, ref.unpack(cfg["init"][0]))
    same_bits(ref.solve(cfg["init"][0]), o.solve(cfg["init"][0]))


# ---- differences

def test_the_differentials_are_those_of_the_composed_cost():
    """C_x of knot i against central differences of the composed knot cost along X Exp(delta) and v + delta, at knots inside a moving
    sphere of the problem's and outside every one: the step and the bound of tests/test_batch_obstacles_cpu.py's check of the sphere term
    (1e-6; rtol 1e-6, atol 1e-7 max(1, |g|))."""
    x = cc.window_inputs(6)
    sl = slice(cc.K0, cc.K0 + cc.N)
    b = 0
    o = cc.window_restatement(x, b, x["cfg"]["desired"][sl], x["Qs"][sl])
    pts = o.unpack(x["init"][b])
    own = x["table"][b, :x["counts"][b]]
    inside = [i for i in range(cc.N) if (np.linalg.norm(pts[i][0][:3, 3] - at_time(own, i * o.dt)[:, :3], axis=1) < at_time(own, i * o.dt)[:, 3]).any()]
    outside = [i for i in range(cc.N) if i not in inside]
    assert inside and outside
    eps = 1e-6
    r = np.random.default_rng(8)
    for i in inside[:2] + outside[:2]:
        T, v, u = pts[i]
        if i in outside:  # (off the desired pose: the tracking term's gradient is not zero there)
            T, v = T @ se3_exp(0.05 * r.standard_normal(6)), v + 0.1 * r.standard_normal(6)
            assert not (np.linalg.norm(T[:3, 3] - at_time(own, i * o.dt)[:, :3], axis=1) < at_time(own, i * o.dt)[:, 3]).any()
        c, C = o.cost_knot_diffs(T, v, u, i)
        one = cc.window_restatement(x, b, x["cfg"]["desired"][sl][i:i + 1], x["Qs"][sl][i:i + 1], own=cc.later(own, i * o.dt))
        assert one.cost_trajectory([(T, v, u)]) == pytest.approx(c, rel=1e-14)  # (the knot's cost alone, its spheres moved to t_i)
        fd = np.empty(12)
        for k in range(12):
            d = np.zeros(12)
            d[k] = eps
            fd[k] = (one.cost_trajectory([(T @ se3_exp(d[:6]), v + d[6:], u)]) - one.cost_trajectory([(T @ se3_exp(-d[:6]), v - d[6:], u)])) / (2 * eps)
        np.testing.assert_allclose(C["x"], fd, rtol=1e-6, atol=1e-7 * max(1.0, np.abs(C["x"]).max()))
        _, plain = cc.window_restatement(x, b, x["cfg"]["desired"][sl], x["Qs"][sl], own=own[:0]).cost_knot_diffs(T, v, u, i)
        assert (i in inside) == (not np.array_equal(plain["xx"], C["xx"]))  # the Gauss-Newton term is there exactly where a sphere is


# ---- discriminating inputs

def moved(right, wrong, pts):
    """how far the wrong restatement is from the right one in the GPU comparison's own measures: (cost, relative; largest gain, against
    the right one's largest)"""
    c0, c1 = right.cost_trajectory(pts), wrong.cost_trajectory(pts)
    (k0, K0, _), (k1, K1, _) = right.backwards_pass(pts), wrong.backwards_pass(pts)
    g0, g1 = np.concatenate([np.ravel(k0), np.ravel(K0)]), np.concatenate([np.ravel(k1), np.ravel(K1)])
    return abs(c1 - c0) / abs(c0), np.abs(g1 - g0).max() / np.abs(g0).max()


def assert_discriminates(right, wrong, pts, what, cost=True):
    dc_, dg = moved(right, wrong, pts)
    print("%s: cost moves by %.2e, the largest gain by %.2e" % (what, dc_, dg))
    if cost:
        assert dc_ >= FACTOR * COST_TOL, (what, dc_)
    assert dg >= FACTOR * GAIN_TOL, (what, dg)


@pytest.mark.parametrize("B", [6, 70])
def test_the_horizon_start_inputs_tell_the_right_index_from_the_wrong_ones(B):
    x = cc.window_inputs(B)
    des, Qs, dt = x["cfg"]["desired"], x["Qs"], x["cfg"]["dt"]
    sl = slice(cc.K0, cc.K0 + cc.N)
    assert all(reached(x["init"][b:b + 1], x["table"][b:b + 1], x["counts"][b:b + 1], dt) > 0 for b in range(B) if x["counts"][b])
    for b in (0, 1, 2, 4) if B == 6 else (64, 68):
        assert x["counts"][b] > 0
        right = cc.window_restatement(x, b, des[sl], Qs[sl])
        pts = right.unpack(x["init"][b])
        own = x["table"][b, :x["counts"][b]]
        assert_discriminates(right, cc.window_restatement(x, b, des[sl], Qs[sl], own=cc.later(own, cc.K0 * dt)), pts, "sphere time (k0 + i) dt")
        assert_discriminates(right, cc.window_restatement(x, b, des[sl], Qs[:cc.N]), pts, "Qs[i] for Qs[k0 + i]")
        assert_discriminates(right, cc.window_restatement(x, b, des[sl], None), pts, "the handle's Q for Qs[k0 + i]")
        assert_discriminates(right, cc.window_restatement(x, b, des[:cc.N], Qs[sl]), pts, "desired[i] for desired[k0 + i]")
        nxt = (b + 1) % B
        assert_discriminates(right, cc.window_restatement(x, b, des[sl], Qs[sl], own=x["table"][nxt, :max(x["counts"][nxt], 1)]), pts,
                             "the next problem's spheres")


def wrong_alternatives(c, x, b):
    """(what, restatement, whether the cost moves) for each wrong index of a case's inputs"""
    B = len(x["trajs"])
    nxt = (b + 1) % B
    out = []
    if x["Qs"] is not None:
        out.append(("the handle's Q for Qs[i]", lc.restatement(c, dict(x, Qs=None), b), True))
        out.append(("Qs[i + 1] for Qs[i]", lc.restatement(c, dict(x, Qs=np.roll(x["Qs"], -1, axis=0)), b), True))
    if x["table"] is not None and x["counts"][b]:  # (a problem without spheres of its own need not be near its neighbour's)
        swapped = dict(x, table=np.roll(x["table"], -1, axis=0), counts=np.roll(x["counts"], -1))
        out.append(("the next problem's spheres", lc.restatement(c, swapped, b), True))
    if x["mods"]:  # (the cost does not depend on the model: the gains tell)
        out.append(("the next problem's model", lc.restatement(c, dict(x, mods=list(np.roll(np.array(x["mods"], dtype=object), -1))), b), False))
    return out


def check_case(c, x):
    if x["table"] is not None:
        for b in range(len(x["trajs"])):
            if x["counts"][b]:
                assert reached(x["trajs"][b:b + 1], x["table"][b:b + 1], x["counts"][b:b + 1], x["cfg"]["dt"]) > 0, (lc.name(c), b)
    for b in range(len(x["trajs"])):
        right = lc.restatement(c, x, b)
        pts = right.unpack(x["trajs"][b])
        for what, wrong, cost in wrong_alternatives(c, x, b):
            assert_discriminates(right, wrong, pts, "%s, problem %d: %s" % (lc.name(c), b, what), cost)


def test_the_composed_pass_inputs_tell_the_right_index_from_the_wrong_ones():
    for c in cc.PASS_CASES:
        check_case(c, lc.inputs(c, seed=cc.pass_seed(c)))


def test_the_key_table_inputs_tell_the_right_problem_and_knot_from_the_wrong_ones():
    """every fp64 case of tests/linearize_cases.py that has something per problem or per knot"""
    n = 0
    for c in lc.F64:
        if c.models or c.problem or c.schedule:
            check_case(c, lc.inputs(c))
            n += 1
    assert n >= 30


def test_the_block_weights_tell_their_entries_apart():
    """the block-diagonal kind's records hold one triangle of each 6 x 6 block.  Transposing a symmetric block changes no number, so no
    comparison can see that; an entry taken from the wrong place shows when the 15 off-diagonal pairs of a block are all different."""
    Q, _ = lc.block_weights(lc.seed_of(lc.F64[1]))
    V = Q[6:, 6:]
    off = V[np.tril_indices(6, -1)]
    assert len(set(off.tolist())) == 15 and np.abs(off).min() > 1e-3


def test_the_solve_inputs_keep_their_counts_when_the_spheres_move_by_1e_13():
    """the rule tests/test_gpu_batch_obstacles.py states for its limits case: counts that change with such a perturbation are counts no two
    implementations need agree on"""
    for N in cc.SIZES:
        for models in (False, True):
            x = cc.solve_inputs(N, models)
            assert reached(x["cfg"]["init"], x["table"], x["counts"], x["cfg"]["dt"]) > 0
            for b in cc.PROBLEMS:
                ref = cc.compute(N, models, b)
                assert ref["status"] in (0, 1) and ref["iters"] >= 2, (N, models, b, ref["status"])
                for nudge in (1e-13, -1e-13):
                    got = cc.compute(N, models, b, nudge)
                    assert [got[k] for k in cc.COUNTS] == [ref[k] for k in cc.COUNTS], (N, models, b, nudge)
                    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-10)
