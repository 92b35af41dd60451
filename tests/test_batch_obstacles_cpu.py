"""The per-problem, moving spheres (qilqr_set_batch_obstacles) on the CPU: the routines of quadrotorilqr_amd/csrc/obstacles.h compiled
with g++ (tests/host_batch_obstacles_harness.cpp) against finite differences through the SE(3) retraction and the NumPy restatement
(tests/moving_obstacle_numpy_ilqr.py); the bits of a static sphere against the shared table's; unused rows; the device layout; the
setter's checks; and the public interface."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from quadrotorilqr_amd import capi
from tests import moving_obstacle_numpy_ilqr as mob
from tests.independent_numpy_ilqr import pose_from_knot, se3_exp
from tests.test_obstacles_cpu import random_knot, spheres_around

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def hb():
    d = tempfile.mkdtemp(prefix="host_batch_obstacles_harness_")
    so = os.path.join(d, "libhost_batch_obstacles_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "host_batch_obstacles_harness.cpp"),
                           "-lm"])
    lib = C.CDLL(so)
    lib.hb_count.restype = C.c_long
    lib.hb_count.argtypes = [C.c_long, C.c_int]
    lib.hb_index.restype = C.c_long
    lib.hb_index.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int]
    lib.hb_relayout.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p]
    lib.hb_knot.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_int, C.c_int, C.c_double,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hb_moving_sphere.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hb_shared.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hb_check.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return lib


def _v(a):
    return a.ctypes.data_as(C.c_void_p)


def relayout(hb, spheres):
    sp = np.ascontiguousarray(spheres, dtype=np.float64)
    B, K = sp.shape[:2]
    out = np.full(hb.hb_count(B, K), np.nan)
    hb.hb_relayout(_v(sp), B, K, _v(out))
    return out


def knot(hb, pt, shared, tab, K, row, count, jend, t, cost=0.0, g=None, H=None):
    """k_linearize's obstacle terms of one knot (the shared spheres, then problem row's): (cost, g, H, active, loader calls)"""
    pt = np.ascontiguousarray(pt, dtype=np.float64)
    sh = np.ascontiguousarray(np.asarray(shared, dtype=np.float64).reshape(-1, 5))
    c = C.c_double(cost)
    g = np.zeros(3) if g is None else np.array(g, dtype=np.float64)
    H = np.zeros(9) if H is None else np.array(H, dtype=np.float64).reshape(9)
    began = C.c_int(0)
    active = hb.hb_knot(_v(pt), _v(sh), len(sh), _v(tab), K, row, count, jend, C.c_double(t), C.byref(c), _v(g), _v(H), C.byref(began))
    return c.value, g, H.reshape(3, 3), bool(active), began.value


def moving(hb, pt, row8, t):
    pt = np.ascontiguousarray(pt, dtype=np.float64)
    sp = np.ascontiguousarray(row8, dtype=np.float64)
    c, g, H = C.c_double(0.0), np.zeros(3), np.zeros(9)
    active = hb.hb_moving_sphere(_v(pt), _v(sp), C.c_double(t), C.byref(c), _v(g), _v(H))
    return c.value, g, H.reshape(3, 3), bool(active)


def moving_around(r, p, t, k):
    """k moving spheres, each containing p at time t"""
    s5 = spheres_around(r, p, k)
    v = r.normal(size=(k, 3))
    return np.column_stack([s5[:, :3] - t * v, v, s5[:, 3:]])


def test_moving_term_and_gradient_match_finite_differences_through_the_retraction(hb):
    r = np.random.default_rng(21)
    for _ in range(40):
        pt = random_knot(r)
        t = r.uniform(0.0, 3.0)
        row = moving_around(r, pt[1:4], t, 1)[0]
        cost, g, H, active = moving(hb, pt, row, t)
        assert active
        T = pose_from_knot(pt)
        np.testing.assert_allclose(cost, mob.moving_penalty(row, t, T), rtol=1e-12)
        eps = 1e-6
        fd = np.empty(6)
        for k in range(6):
            e = np.zeros(6)
            e[k] = eps
            fd[k] = (mob.moving_penalty(row, t, T @ se3_exp(e)) - mob.moving_penalty(row, t, T @ se3_exp(-e))) / (2 * eps)
        np.testing.assert_allclose(g, fd[:3], rtol=1e-6, atol=1e-7 * max(1.0, np.abs(g).max()))
        np.testing.assert_allclose(fd[3:], 0.0, atol=1e-7 * max(1.0, np.abs(g).max()))
        assert np.array_equal(H, H.T)


def test_knot_terms_match_the_restatement(hb):
    r = np.random.default_rng(22)
    for trial in range(40):
        pt = random_knot(r)
        i, dt = int(r.integers(0, 60)), 0.05
        t = i * dt
        K = int(r.integers(1, 6))
        B = int(r.integers(1, 140))
        row = int(r.integers(0, B))
        own = np.vstack([moving_around(r, pt[1:4], t, K - 1), [[40.0, 0, 0, 1.0, 0, 0, 0.5, 3.0]]])[r.permutation(K)]
        table = r.normal(size=(B, K, 8)) * 50.0
        table[..., 6] = np.abs(table[..., 6]) + 0.1
        table[row] = own
        shared = spheres_around(r, pt[1:4], int(r.integers(0, 3)))
        c0, g0, H0 = r.normal(), r.normal(size=3), r.normal(size=(3, 3))
        H0 = H0 + H0.T
        cost, g, H, _, _ = knot(hb, pt, shared, relayout(hb, table), K, row, K, K, t, c0, g0, H0)
        o = mob._MovingObstacles()
        o.dt = dt
        o.set_obstacles(shared)
        o.set_problem_obstacles(own)
        pc, pg, pH = mob.obs.penalty(o.knot_spheres(i), pose_from_knot(pt), diffs=True)
        np.testing.assert_allclose(cost, c0 + pc, rtol=1e-12)
        np.testing.assert_allclose(g, g0 + pg, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(H, H0 + pH, rtol=1e-12, atol=1e-12)


def test_a_static_problem_sphere_gives_the_bits_of_the_shared_one(hb):
    r = np.random.default_rng(23)
    for _ in range(40):
        pt = random_knot(r)
        s5 = np.vstack([spheres_around(r, pt[1:4], 3), [[5.0, 5.0, 5.0, 0.5, 1.0]]])[r.permutation(4)]
        c = C.c_double(0.25)
        g, H = np.full(3, 0.5), np.full(9, 0.125)
        hb.hb_shared(_v(np.ascontiguousarray(pt)), _v(np.ascontiguousarray(s5)), len(s5), C.byref(c), _v(g), _v(H))
        B, row = 70, int(r.integers(0, 70))
        table = np.zeros((B, 4, 8))
        table[:, :, 6] = 1.0
        table[row] = mob.static_rows(s5)
        for t in (0.0, 0.35, 4.75):  # any time: c + t 0 = c exactly
            cost, g2, H2, _, _ = knot(hb, pt, [], relayout(hb, table), 4, row, 4, 4, t, 0.25, np.full(3, 0.5), np.full(9, 0.125))
            assert cost == c.value and np.array_equal(g2, g) and np.array_equal(H2.reshape(9), H)
            # shared and per-problem halves of the same list: the bits of the whole list shared
            t2 = table.copy()
            t2[row, :2] = t2[row, 2:]
            cost, g2, H2, _, _ = knot(hb, pt, s5[:2], relayout(hb, t2), 4, row, 2, 2, t, 0.25, np.full(3, 0.5), np.full(9, 0.125))
            assert cost == c.value and np.array_equal(g2, g) and np.array_equal(H2.reshape(9), H)


def test_rows_beyond_the_count_change_no_bit(hb):
    r = np.random.default_rng(24)
    for _ in range(30):
        pt = random_knot(r)
        t = r.uniform(0.0, 2.0)
        K, cnt = 6, int(r.integers(0, 4))
        B, row = 130, int(r.integers(0, 130))
        clean = np.zeros((B, K, 8))
        clean[:, :, 6] = 1.0
        clean[row, :cnt] = moving_around(r, pt[1:4], t, cnt) if cnt else clean[row, :0]
        nan = clean.copy()
        nan[row, cnt:] = np.nan
        reached = clean.copy()
        if K - cnt:
            reached[row, cnt:] = moving_around(r, pt[1:4], t, K - cnt)
        c0, g0, H0 = r.normal(), r.normal(size=3), r.normal(size=(3, 3))
        base = knot(hb, pt, [], relayout(hb, clean), K, row, cnt, cnt, t, c0, g0, H0)
        for tab in (nan, reached):
            for jend in (cnt, K):  # the wavefront's largest count may be any of them
                out = knot(hb, pt, [], relayout(hb, tab), K, row, cnt, jend, t, c0, g0, H0)
                assert out[0] == base[0] and np.array_equal(out[1], base[1]) and np.array_equal(out[2], base[2])
                assert out[3:] == base[3:]
        if cnt == 0:
            assert base[0] == c0 and np.array_equal(base[1], g0) and base[4] == 0


@pytest.mark.parametrize("B,K", [(1, 1), (63, 3), (64, 2), (65, 5), (130, 64), (200, 7)])
def test_device_layout_round_trips(hb, B, K):
    r = np.random.default_rng(B * 100 + K)
    sp = r.normal(size=(B, K, 8))
    out = relayout(hb, sp)
    tiles = (B + 63) // 64
    assert len(out) == tiles * K * 8 * 64
    tiled = out.reshape(tiles, K, 8, 64)
    back = np.transpose(tiled, (0, 3, 1, 2)).reshape(tiles * 64, K, 8)
    assert np.array_equal(back[:B], sp)
    assert not back[B:].any()  # the padding rows of the last tile: zeros
    for b, j, w in ((0, 0, 0), (B - 1, K - 1, 7), (B // 2, K // 2, 3)):
        assert out[hb.hb_index(b, K, j, w)] == sp[b, j, w]
    if B >= 64:  # word w of sphere j for 64 consecutive problems: one contiguous run
        idx = [hb.hb_index(b, K, K - 1, 5) for b in range(64)]
        assert idx == list(range(idx[0], idx[0] + 64))


def check(hb, spheres, counts, B, K):
    b, j = C.c_long(), C.c_int()
    why = C.create_string_buffer(256)
    sp = None if spheres is None else np.ascontiguousarray(spheres, dtype=np.float64)
    cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
    rc = hb.hb_check(None if sp is None else _v(sp), None if cn is None else _v(cn), B, K, C.byref(b), C.byref(j), why, 256)
    return rc, why.value.decode(), b.value, j.value


def test_the_setters_checks(hb):
    ok = np.zeros((3, 4, 8))
    ok[..., 6] = 1.0
    assert check(hb, ok, None, 3, 4)[0] == 0
    assert check(hb, None, None, 0, 0)[0] == 0  # the clear
    assert check(hb, np.zeros((1, 64, 8)) + [0, 0, 0, 0, 0, 0, 1, 0], None, 1, 64)[0] == 0  # 64 spheres, weight 0: allowed
    for K in (0, 65, -1):
        rc, why, _, _ = check(hb, np.ones((1, max(K, 1), 8)), None, 1, K)
        assert rc == 1 and "K" in why
    rc, why, _, _ = check(hb, None, None, 3, 4)
    assert rc == 1 and "clear" in why
    for counts, b in (([4, 5, 0], 1), ([0, 0, -1], 2)):
        rc, why, bb, _ = check(hb, ok, counts, 3, 4)
        assert (rc, bb) == (1, b) and "count" in why
    for (b, j, w, v), what in (((2, 1, 4, np.nan), "non-finite"), ((0, 3, 0, np.inf), "non-finite"), ((1, 2, 6, 0.0), "radius"),
                               ((1, 0, 6, -1.0), "radius"), ((2, 3, 7, -1e-9), "weight")):
        bad = ok.copy()
        bad[b, j, w] = v
        rc, why, bb, jj = check(hb, bad, None, 3, 4)
        assert (rc, bb, jj) == (1, b, j) and what in why, (why, bb, jj)
    # an unused row is never looked at
    bad = ok.copy()
    bad[1, 2:] = np.nan
    bad[1, 3, 6] = -5.0
    assert check(hb, bad, [4, 2, 4], 3, 4)[0] == 0
    assert check(hb, bad, [4, 3, 4], 3, 4)[:4] == (1, "a non-finite value", 1, 2)


def test_header_and_python_expose_the_entry_points():
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    assert re.search(r"int qilqr_set_batch_obstacles\(qilqr_solver \*s, const double \*spheres, const int32_t \*counts, int32_t B, "
                     r"int32_t K\);", header)
    assert re.search(r"int qilqr_sharded_set_batch_obstacles\(qilqr_sharded \*h, const double \*spheres, const int32_t \*counts, "
                     r"int32_t B, int32_t K\);", header)
    assert re.search(r"#define QILQR_OBSTACLE_WORDS 8\b", header)
    assert re.search(r"#define QILQR_ABI_VERSION 7\b", header)
    assert {"qilqr_set_batch_obstacles", "qilqr_sharded_set_batch_obstacles"} <= set(capi.EXPORTS)
    assert capi.OBSTACLE_WORDS == 8
    for cls in (capi.QuadrotorILQRBatch, capi.QuadrotorILQRSharded):
        assert callable(getattr(cls, "set_batch_obstacles", None)) and callable(getattr(cls, "clear_batch_obstacles", None))
    arr, cnt = capi.batch_obstacle_arrays([[[1, 2, 3, 0.5, 7]]])  # (B, K, 5): static
    assert arr.shape == (1, 1, 8) and list(arr[0, 0]) == [1, 2, 3, 0, 0, 0, 0.5, 7] and cnt is None
    arr, cnt = capi.batch_obstacle_arrays(np.zeros((2, 3, 8)), [1, 3])
    assert cnt.dtype == np.int32 and list(cnt) == [1, 3]
    for bad in ([], np.zeros((2, 5)), np.zeros((2, 3, 6)), np.zeros((0, 3, 8)), np.zeros((2, 0, 8))):
        with pytest.raises(TypeError):
            capi.batch_obstacle_arrays(bad)
    with pytest.raises(TypeError):
        capi.batch_obstacle_arrays(np.zeros((2, 3, 8)), [1, 2, 3])
    with pytest.raises(TypeError):
        capi.batch_obstacle_arrays(np.zeros((2, 3, 8)), [1.0, 2.0])


def test_library_exports_the_setters():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = capi.load()
    assert hasattr(lib, "qilqr_set_batch_obstacles") and hasattr(lib, "qilqr_sharded_set_batch_obstacles")
    assert lib.qilqr_set_batch_obstacles(None, None, None, 0, 0) == capi.ERR_INVALID_ARG  # a null handle is refused, nothing touched
    assert lib.qilqr_sharded_set_batch_obstacles(None, None, None, 0, 0) == capi.ERR_INVALID_ARG
