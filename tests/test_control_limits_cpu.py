"""The per-rotor thrust limits (qilqr_set_control_limits) on the CPU: the box QP of quadrotorilqr_amd/csrc/box_qp.h -- its NumPy
restatement against the KKT conditions, the header compiled for the host (tests/host_box_harness.cpp) against the restatement -- and
the restatement of the whole extension (tests/limited_numpy_ilqr.py) against the unconstrained restatement and on the reference's demo."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from quadrotorilqr_amd import problems as pb
from tests import limited_numpy_ilqr as lim
from tests.independent_numpy_ilqr import ILQR, Model

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "oracle_golden.npz"))


def random_problems(count, seed=7):
    """SPD H of spread conditioning, g, and boxes with no, some or every bound active, some sides infinite; Q_ux"""
    r = np.random.default_rng(seed)
    out = []
    for t in range(count):
        A = r.normal(size=(4, 4))
        H = A @ A.T + 10.0 ** r.uniform(-2, 1) * np.eye(4)
        H = 0.5 * (H + H.T)
        g = r.normal(size=4) * 10.0 ** r.uniform(-1, 2)
        x_free = np.linalg.solve(H, -g)
        kind = t % 4  # 0: boxes wide of the free optimum, 1: some rotors cut, 2: every rotor cut, 3: random boxes
        l, h = np.empty(4), np.empty(4)
        for a in range(4):
            s = abs(x_free[a]) + 1.0
            if kind == 0 or (kind == 1 and r.random() < 0.5):
                l[a], h[a] = x_free[a] - r.uniform(0.1, 2) * s, x_free[a] + r.uniform(0.1, 2) * s
            elif kind == 3:
                l[a] = r.uniform(-2, 1) * s
                h[a] = l[a] + r.uniform(0.01, 3) * s
            elif r.random() < 0.5:
                l[a], h[a] = -np.inf, x_free[a] - r.uniform(0.05, 1) * s
            else:
                l[a], h[a] = x_free[a] + r.uniform(0.05, 1) * s, np.inf
            if r.random() < 0.15:
                l[a] = -np.inf
            if r.random() < 0.15:
                h[a] = np.inf
        out.append((H, g, l, h, r.normal(size=(4, 12))))
    return out


PROBLEMS = random_problems(2000)


def test_numpy_box_qp_meets_the_kkt_conditions():
    seen_clamped = set()
    for H, g, l, h, _ in PROBLEMS:
        x, c, _, ok = lim.box_qp(H, g, l, h)
        assert ok
        assert np.all(x >= l) and np.all(x <= h)
        grad = g + H @ x
        scale = np.abs(g).max() + np.abs(H).max() * np.abs(x).max() + 1e-300
        free = ~c
        assert np.all(np.abs(grad[free]) <= 1e-10 * scale), (grad, c, x, l, h)
        assert np.all(grad[c & (x == l)] > 0) and np.all(grad[c & (x == h)] < 0)
        # a clamped rotor sits on its bound, a free one inside the box or on a bound with a zero gradient
        assert np.all((x[c] == l[c]) | (x[c] == h[c]))
        seen_clamped.add(int(c.sum()))
        if not c.any() and np.all((x > l) & (x < h)):
            np.testing.assert_allclose(x, np.linalg.solve(H, -g), rtol=1e-10, atol=1e-12 * np.abs(x).max())
    assert seen_clamped == {0, 1, 2, 3, 4}


def test_numpy_box_qp_without_bounds_is_the_newton_step():
    for H, g, _, _, _ in PROBLEMS[:200]:
        inf = np.full(4, np.inf)
        x, c, _, ok = lim.box_qp(H, g, -inf, inf)
        assert ok and not c.any()
        np.testing.assert_allclose(x, np.linalg.solve(H, -g), rtol=1e-10, atol=1e-13 * np.abs(x).max())


def test_numpy_box_qp_reports_an_indefinite_matrix():
    H = np.diag([1.0, -1.0, 2.0, 3.0])
    inf = np.full(4, np.inf)
    assert not lim.box_qp(H, np.ones(4), -inf, inf)[3]


@pytest.fixture(scope="module")
def hb():
    d = tempfile.mkdtemp(prefix="host_box_harness_")
    so = os.path.join(d, "libhost_box_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_box_harness.cpp"), "-lm"])
    return C.CDLL(so)


def P(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_box_qp_header_matches_the_restatement(hb):
    for H, g, l, h, Qux in PROBLEMS:
        H, g, l, h, Qux = (np.ascontiguousarray(a, dtype=float) for a in (H, g, l, h, Qux))
        k, K, cm = np.zeros(4), np.zeros((4, 12)), C.c_int()
        assert hb.hb_box_qp(P(H), P(g), P(l), P(h), P(Qux), P(k), P(K), C.byref(cm)) == 1
        x, c, factor, ok = lim.box_qp(H, g, l, h)
        assert ok
        assert [(cm.value >> a) & 1 for a in range(4)] == [int(v) for v in c]
        np.testing.assert_allclose(k, x, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(x).max()))
        Kr = lim.box_gain(factor, c, Qux)
        np.testing.assert_allclose(K, Kr, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(Kr).max()))
        assert np.all(K[c] == 0.0)


def test_box_qp_header_reports_an_indefinite_matrix(hb):
    H = np.ascontiguousarray(np.diag([1.0, -1.0, 2.0, 3.0]))
    inf = np.full(4, np.inf)
    k, K, cm = np.zeros(4), np.zeros((4, 12)), C.c_int()
    assert hb.hb_box_qp(P(H), P(np.ones(4)), P(-inf), P(inf), P(np.zeros((4, 12))), P(k), P(K), C.byref(cm)) == 0


def restatements(cfg, lo, hi, integrator=0):
    m = Model(**cfg["model"])
    o = dict(cfg["options"])
    plain = ILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], o, integrator=integrator, recursion=1)
    box = lim.LimitedILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], o, lo, hi, integrator=integrator)
    return plain, box


@pytest.mark.parametrize("integrator", [0, 1])
def test_restatement_with_infinite_limits_is_the_unconstrained_one(integrator):
    cfg = pb.config2(B=2, N=12, seed=3)
    cfg["options"] = dict(cfg["options"], rtol=1e-9, atol=1e-9)
    plain, box = restatements(cfg, -np.inf, np.inf, integrator)
    for t in cfg["init"]:
        pts = plain.unpack(t)
        k0, K0, t0 = plain.backwards_pass(pts)
        k1, K1, t1 = box.backwards_pass(pts)
        assert not box.qp_failed and not box.clamped.any()
        sk = max(np.abs(np.array(k0)).max(), 1.0)
        sK = max(np.abs(np.array(K0)).max(), 1.0)
        np.testing.assert_allclose(np.array(k1), np.array(k0), rtol=1e-12, atol=1e-12 * sk)
        np.testing.assert_allclose(np.array(K1), np.array(K0), rtol=1e-12, atol=1e-12 * sK)
        np.testing.assert_allclose(t1, t0, rtol=1e-12, atol=1e-12 * np.abs(t0).max())
        for alpha in (1.0, 0.5):
            f0 = plain.forward_sim(pts, k0, K0, alpha)
            f1 = box.forward_sim(pts, k0, K0, alpha)
            for (Ta, va, ua), (Tb, vb, ub) in zip(f0, f1):
                assert np.array_equal(Ta, Tb) and np.array_equal(va, vb) and np.array_equal(ua, ub)
        a, b = plain.solve(t), box.solve(t)
        for key in ("status", "iters", "n_bwd", "n_fwd"):
            assert a[key] == b[key], key
        np.testing.assert_allclose(b["cost"], a["cost"], rtol=1e-9)
        np.testing.assert_allclose(b["traj"], a["traj"], atol=1e-6)


def test_restatement_on_the_reference_demo_keeps_the_thrusts_in_the_box():
    d = pb.box_climb_desired(4.0)
    np.testing.assert_array_equal(d, G["demo40_desired"])
    opts = dict(pb.OPTIONS_DEMO, populate_debug=False)
    box = lim.LimitedILQR(Model(**pb.MODEL_D), pb.Q_DEMO, pb.R_DEMO, d, pb.DT_DEMO, opts, 0.0, 9.81)
    out = box.solve(d)
    assert out["status"] in (0, 1), out["status"]
    u = out["traj"][:, 14:18]
    assert u.min() >= 0.0 and u.max() <= 9.81
    unconstrained = G["demo40_traj"][:, 14:18]
    assert unconstrained.min() < 0.0  # the limits were active
    assert np.isclose(u, 0.0).any()
    assert out["cost"] >= G["demo40_cost_hist"][-1]
