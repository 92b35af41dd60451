"""The spherical obstacles (qilqr_set_obstacles) on the CPU: the penalty of quadrotorilqr_amd/csrc/obstacles.h compiled with g++
(tests/host_obstacles_harness.cpp) against finite differences through the SE(3) retraction and against the NumPy restatement
(tests/obstacle_numpy_ilqr.py), the rules for inactive spheres and a knot at a sphere's center, and the public interface."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from quadrotorilqr_amd import capi
from tests import obstacle_numpy_ilqr as obs
from tests.independent_numpy_ilqr import pose_from_knot, se3_exp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def harness():
    d = tempfile.mkdtemp(prefix="host_obstacles_harness_")
    so = os.path.join(d, "libhost_obstacles_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_obstacles_harness.cpp"), "-lm"])
    return C.CDLL(so)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def run(harness, pt, spheres, cost=0.0, g=None, H=None):
    """the header's penalty at knot pt: (cost, g[3], H[3 x 3], active, loader calls) starting from the given accumulators"""
    pt = np.ascontiguousarray(pt, dtype=np.float64)
    sp = np.ascontiguousarray(np.asarray(spheres, dtype=np.float64).reshape(-1, 5))
    c = C.c_double(cost)
    g = np.zeros(3) if g is None else np.array(g, dtype=np.float64)
    H = np.zeros(9) if H is None else np.array(H, dtype=np.float64).reshape(9)
    began = C.c_int(0)
    active = harness.ho_add_obstacles(_dp(pt), _dp(sp), C.c_int(len(sp)), C.byref(c), _dp(g), _dp(H), C.byref(began))
    return c.value, g, H.reshape(3, 3), bool(active), began.value


def random_knot(r):
    q = Rotation.random(random_state=int(r.integers(1 << 30))).as_quat()  # x, y, z, w
    p = r.normal(size=3)
    return np.concatenate([[0.0], p, [q[3], q[0], q[1], q[2]], r.normal(size=6), r.normal(size=4)])


def spheres_around(r, p, k):
    """k spheres, each containing p (random centers within 0.6 of p, radii beyond the distance) with random weights"""
    c = p + r.normal(size=(k, 3)) * 0.3
    d = np.linalg.norm(c - p, axis=1)
    return np.column_stack([c, d + r.uniform(0.05, 0.5, size=k), r.uniform(0.1, 20.0, size=k)])


def test_penalty_and_gradient_match_finite_differences_through_the_retraction(harness):
    r = np.random.default_rng(11)
    for _ in range(40):
        pt = random_knot(r)
        sp = spheres_around(r, pt[1:4], int(r.integers(1, 5)))
        sp = np.vstack([sp, [[pt[1] + 50.0, pt[2], pt[3], 1.0, 3.0]]])  # and one far away
        cost, g, H, active, began = run(harness, pt, sp)
        assert active and began == 1
        T = pose_from_knot(pt)
        np.testing.assert_allclose(cost, obs.penalty(sp, T), rtol=1e-13)
        eps = 1e-6
        fd = np.empty(6)
        for k in range(6):
            e = np.zeros(6)
            e[k] = eps
            fd[k] = (obs.penalty(sp, T @ se3_exp(e)) - obs.penalty(sp, T @ se3_exp(-e))) / (2 * eps)
        np.testing.assert_allclose(g, fd[:3], rtol=1e-6, atol=1e-7 * max(1.0, np.abs(g).max()))
        np.testing.assert_allclose(fd[3:], 0.0, atol=1e-7 * max(1.0, np.abs(g).max()))  # theta moves no position


def test_gauss_newton_block_is_2_w_m_m_transposed(harness):
    r = np.random.default_rng(12)
    for _ in range(40):
        pt = random_knot(r)
        sp = spheres_around(r, pt[1:4], 1)
        _, g, H, _, _ = run(harness, pt, sp)
        R = pose_from_knot(pt)[:3, :3]
        e = pt[1:4] - sp[0, :3]
        m = R.T @ (e / np.linalg.norm(e))
        np.testing.assert_allclose(H, 2 * sp[0, 4] * np.outer(m, m), rtol=1e-13, atol=1e-14 * sp[0, 4])
        assert np.array_equal(H, H.T)  # one increment per pair, in both triangles
        h = sp[0, 3] - np.linalg.norm(e)
        np.testing.assert_allclose(g, -2 * sp[0, 4] * h * m, rtol=1e-13, atol=1e-15)


def test_restatement_matches_the_header(harness):
    r = np.random.default_rng(13)
    for _ in range(40):
        pt = random_knot(r)
        sp = np.vstack([spheres_around(r, pt[1:4], 3), [[9.0, 9.0, 9.0, 0.5, 1.0]]])[r.permutation(4)]
        c0, g0, H0 = r.normal(), r.normal(size=3), r.normal(size=(3, 3))
        H0 = H0 + H0.T
        cost, g, H, _, _ = run(harness, pt, sp, c0, g0, H0)
        pc, pg, pH = obs.penalty(sp, pose_from_knot(pt), diffs=True)
        np.testing.assert_allclose(cost, c0 + pc, rtol=1e-13)
        np.testing.assert_allclose(g, g0 + pg, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(H, H0 + pH, rtol=1e-12, atol=1e-13)


def test_an_inactive_sphere_adds_nothing_bit_for_bit(harness):
    r = np.random.default_rng(14)
    for _ in range(20):
        pt = random_knot(r)
        p = pt[1:4]
        d = r.uniform(0.5, 3.0)
        u = r.normal(size=3)
        u /= np.linalg.norm(u)
        sp = [[*(p + d * u), d * 0.999, 5.0],        # just outside
              [*(p + 100.0 * u), 1.0, 1e6],          # far away
              [*(p - d * u), d, 2.0]]                # touching: h = 0 (or a rounding off it)
        c0, g0, H0 = r.normal(), r.normal(size=3), r.normal(size=(3, 3))
        cost, g, H, active, began = run(harness, pt, sp[:2], c0, g0, H0)
        assert not active and began == 0
        assert cost == c0 and np.array_equal(g, g0) and np.array_equal(H, H0)
        # a sphere exactly on the knot's surface: h is 0 or a rounding error away; if inactive, nothing moves
        cost, g, H, active, _ = run(harness, pt, sp[2:], c0, g0, H0)
        if not active:
            assert cost == c0 and np.array_equal(g, g0) and np.array_equal(H, H0)


def test_a_knot_at_the_center_pays_w_r_squared_and_gets_no_differentials(harness):
    r = np.random.default_rng(15)
    pt = random_knot(r)
    sp = [[pt[1], pt[2], pt[3], 0.7, 3.0]]
    g0, H0 = r.normal(size=3), r.normal(size=(3, 3))
    cost, g, H, active, began = run(harness, pt, sp, 1.25, g0, H0)
    assert active and began == 1
    assert cost == 1.25 + 3.0 * 0.7 * 0.7
    assert np.array_equal(g, g0) and np.array_equal(H, H0)
    pc, pg, pH = obs.penalty(sp, pose_from_knot(pt), diffs=True)
    assert pc == 3.0 * 0.7 * 0.7 and not pg.any() and not pH.any()


def test_restatement_cost_and_differentials_add_to_the_tracking_cost():
    from quadrotorilqr_amd import problems as pb
    from tests.independent_numpy_ilqr import Model
    cfg = pb.config2(B=2, N=12, seed=3)
    o = obs.ObstacleILQR(Model(**cfg["model"]), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]))
    pts = o.unpack(cfg["init"][0])
    base = o.cost_trajectory(pts)
    p = pts[5][0][:3, 3]
    o.set_obstacles([[*p, 0.3, 10.0], [*(p + 100.0), 0.3, 10.0]])
    with_obs = o.cost_trajectory(pts)
    assert with_obs >= base + 10.0 * 0.3 * 0.3 * (1 - 1e-12)
    _, C = o.cost_knot_diffs(*pts[5], 5)  # the knot at the first sphere's center: cost term only
    _, C0 = obs.cost_knot(o.Q, o.R, *pts[5], *o.des[5], diffs=True)
    assert np.array_equal(C["x"], C0["x"]) and np.array_equal(C["xx"], C0["xx"])


def test_header_and_python_expose_the_entry_points():
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    assert re.search(r"int qilqr_set_obstacles\(qilqr_solver \*s, const double \*spheres, int32_t count\);", header)
    assert re.search(r"int qilqr_sharded_set_obstacles\(qilqr_sharded \*h, const double \*spheres, int32_t count\);", header)
    assert re.search(r"#define QILQR_MAX_OBSTACLES 64\b", header)
    assert re.search(r"#define QILQR_ABI_VERSION 7\b", header)
    assert {"qilqr_set_obstacles", "qilqr_sharded_set_obstacles"} <= set(capi.EXPORTS)
    assert capi.MAX_OBSTACLES == 64
    for cls in (capi.QuadrotorILQRBatch, capi.QuadrotorILQRSharded):
        assert callable(getattr(cls, "set_obstacles", None)) and callable(getattr(cls, "clear_obstacles", None))
    assert capi.obstacle_array([[0, 0, 0, 1, 1]]).shape == (1, 5)
    for bad in ([], [[0, 0, 0, 1]], np.zeros((2, 3, 5))):
        with pytest.raises(TypeError):
            capi.obstacle_array(bad)


def test_library_exports_the_setters():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = capi.load()
    assert hasattr(lib, "qilqr_set_obstacles") and hasattr(lib, "qilqr_sharded_set_obstacles")
    assert lib.qilqr_set_obstacles(None, None, 0) == capi.ERR_INVALID_ARG  # a null handle is refused, nothing touched
