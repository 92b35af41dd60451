"""The per-knot state-weight schedule without a device (qilqr_set_state_weight_schedule): the NumPy restatement
(tests/schedule_numpy_ilqr.py) against itself -- its two recursions on the inputs of tests/schedule_cases.py, its C_x against central
differences, a constant schedule against the plain restatement --, the route a scheduled handle takes (route.h through
tests/host_schedule_harness.cpp), the setter's check of a schedule (schedule.h), and what of the ABI runs without a GPU."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

from quadrotorilqr_amd import capi, problems as pb
from tests import schedule_cases as sc
from tests.independent_numpy_ilqr import ILQR, Model, se3_exp
from tests.obstacle_numpy_ilqr import ObstacleILQR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "quadrotorilqr_amd", "csrc")
IN = ("symmetric", "layout_kind", "q_diag", "integrator", "limited", "modeled", "obstacles", "problem_obstacles", "force_general",
      "persistent", "compaction", "streams", "single_wave_rollout", "round_launch", "B", "scheduled")
OUT = ("backward", "tiled", "combined", "fuse_kinds", "round_kernel", "late_tail", "persistent", "lin_kind", "key", "admitted", "rollout",
       "compact", "parts")
BW_ONE = 2


def _build(name, deps, flags=()):
    so, src = os.path.join(HERE, f"lib{name}.so"), os.path.join(HERE, f"{name}.cpp")
    deps = [src] + deps
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", *flags, "-o", so, src])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hs():
    # (-DQILQR_WITH_SOLVE4: the diagnostics build's rule, in which persistent = 1 selects k_solve4 where nothing forbids it)
    lib = _build("host_schedule_harness", [os.path.join(CSRC, "route.h"), os.path.join(CSRC, "schedule.h"),
                                           os.path.join(HERE, "..", "include", "quadrotor_ilqr.h")], ["-DQILQR_WITH_SOLVE4"])
    lib.hs_route.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.hs_check.argtypes = [C.POINTER(C.c_double), C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    return lib


def route(hs, **kw):
    row = dict.fromkeys(IN, 0)
    row.update(kw)
    inp = np.array([row[k] for k in IN], dtype=np.int64)
    out = np.zeros(len(OUT), dtype=np.int64)
    assert hs.hs_route(inp.ctypes.data_as(C.POINTER(C.c_long)), out.ctypes.data_as(C.POINTER(C.c_long))) == len(OUT)
    return dict(zip(OUT, out.tolist()))


# ---- the restatement

@pytest.mark.parametrize("N", sc.SIZES)
@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_two_recursions_agree_on_the_committed_inputs(N, kind):
    """The reference-form recursion and the symmetrised one take the same decisions on every input the GPU tests compare against: equal
    counts are then attainable for either backward kernel, and the project's bars (cost 1e-9 relative, trajectory 1e-6) with them."""
    assert np.array_equal(sc.schedule(kind, N), np.transpose(sc.schedule(kind, N), (0, 2, 1)))
    for b in sc.PROBLEMS:
        r0, r1 = sc.compute(N, kind, b, 0), sc.compute(N, kind, b, 1)
        counts = [[r[k] for k in sc.COUNTS] for r in (r0, r1)]
        assert counts[0] == counts[1], (N, kind, b, counts)
        assert r0["status"] == 0 and 2 <= r0["iters"] <= 30, (N, kind, b, counts)
        np.testing.assert_allclose(r1["cost"], r0["cost"], rtol=1e-12)
        np.testing.assert_allclose(r1["traj"], r0["traj"], rtol=0, atol=1e-10)
        # ... and the record the GPU tests read is this computation (another BLAS may round differently: the same bars)
        g = sc.solved(N, kind, b)
        assert [g[k] for k in sc.COUNTS] == counts[1], (N, kind, b)
        np.testing.assert_allclose(g["cost"], r1["cost"], rtol=1e-12)
        np.testing.assert_allclose(g["traj"], r1["traj"], rtol=0, atol=1e-10)
        np.testing.assert_allclose(g["cost_hist"], r1["cost_hist"], rtol=1e-12)


@pytest.mark.parametrize("kind", sc.KINDS)
def test_c_x_is_the_gradient_of_the_scheduled_cost(kind):
    """C_x of knot i against central differences of the knot cost along X Exp(delta) (pose) and v + delta (velocity).  Step 1e-5 on a cost
    of order 1e3 with third derivatives of the same order: truncation ~ 1e-7, rounding ~ 1e-16 * 1e3 / 1e-5 = 1e-8: 1e-6 of the scale."""
    N = 12
    cfg = sc.config(N)
    o = sc.restatement(cfg, sc.schedule(kind, N), 0)  # (symmetric: cost.hh's C_x = 2 dx^T Q J is the gradient only then)
    r = np.random.default_rng(5)
    pts = o.unpack(cfg["init"][1])
    h = 1e-5
    for i in (0, N // 3, N // 2, N - 1):
        T, v, u = pts[i]
        T = T @ se3_exp(0.3 * r.standard_normal(6))  # off the desired pose (every knot but the first starts on it)
        v = v + 0.2 * r.standard_normal(6)
        _, Cd = o.cost_knot_diffs(T, v, u, i)
        num = np.zeros(12)
        for k in range(12):
            d = np.zeros(12)
            d[k] = h

            def at(sign):
                one = [(T @ se3_exp(sign * d[:6]), v + sign * d[6:], u)]
                single = sc.restatement(dict(cfg, desired=cfg["desired"][i:i + 1]), o.Qs[i:i + 1], 0)
                return single.cost_trajectory(one)
            num[k] = (at(1.0) - at(-1.0)) / (2 * h)
        scale = np.abs(Cd["x"]).max()
        assert scale > 0
        np.testing.assert_allclose(Cd["x"], num, rtol=0, atol=1e-6 * scale)
        # ... and C_xx = 2 J^T Qs[i] J is this knot's: linear in the knot's matrix (doubling is exact in binary)
        twice = sc.restatement(dict(cfg, desired=cfg["desired"][i:i + 1]), 2.0 * o.Qs[i:i + 1], 0).cost_knot_diffs(T, v, u, 0)[1]
        assert np.array_equal(twice["xx"], 2.0 * Cd["xx"]) and np.abs(Cd["xx"]).max() > 0


@pytest.mark.parametrize("recursion", [0, 1])
def test_a_constant_schedule_is_the_plain_restatement(recursion):
    N = 12
    cfg = sc.config(N)
    # the plain restatement of either form: ILQR's symmetrised recursion; the reference's forms with Q_uu read as Eigen's LDL^T reads it
    # (ObstacleILQR without spheres, the comparand of the general kernel elsewhere in the suite)
    plain = (ILQR if recursion == 1 else ObstacleILQR)(Model(**cfg["model"]), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"],
                                                        dict(cfg["options"]), recursion=recursion)
    o = sc.restatement(cfg, sc.schedule("constant", N), recursion)
    a, b = plain.solve(cfg["init"][0]), o.solve(cfg["init"][0])
    for k in ("status", "iters", "n_bwd", "n_fwd", "cost"):
        assert a[k] == b[k], k
    assert np.array_equal(a["traj"], b["traj"]) and np.array_equal(a["cost_hist"], b["cost_hist"])
    pts = plain.unpack(cfg["init"][2])
    assert plain.cost_trajectory(pts) == o.cost_trajectory(pts)
    for x, y in zip(plain.backwards_pass(pts), o.backwards_pass(pts)):
        assert np.array_equal(np.array(x), np.array(y))


def test_the_helpers_of_problems_py():
    Q, Qf = 0.01 * pb.Q_DEMO, 10 * pb.Q_DEMO
    t = pb.terminal_schedule(Q, Qf, 5)
    assert t.shape == (5, 12, 12) and all(np.array_equal(t[i], Q) for i in range(4)) and np.array_equal(t[4], Qf)
    assert np.array_equal(pb.terminal_schedule(Q, Qf, 1), Qf[None])
    w = pb.waypoint_schedule(Q, Qf, 6, (2, 5))
    assert [bool(np.array_equal(w[i], Qf)) for i in range(6)] == [False, False, True, False, False, True]
    assert all(np.array_equal(w[i], Q) for i in (0, 1, 3, 4))
    with pytest.raises(ValueError):
        pb.waypoint_schedule(Q, Qf, 6, (6,))
    with pytest.raises(ValueError):
        pb.terminal_schedule(Q, Qf, 0)


# ---- the route

EXTENSIONS = [dict(integrator=i, limited=l, modeled=m, obstacles=o, problem_obstacles=p)
              for i, l, m, (o, p) in itertools.product((0, 1), (0, 1), (0, 1), ((0, 0), (1, 0), (0, 1), (1, 1)))]


def test_a_scheduled_handle_takes_the_route_of_non_symmetric_weights(hs):
    with open(os.path.join(HERE, "golden", "linearize_keys.json")) as f:
        recorded = {tuple(r) for r in json.load(f)["rows"]}
    assert len(recorded) == 58
    seen_keys = set()
    for ext in EXTENSIONS:
        for own in (dict(symmetric=1, layout_kind=2, q_diag=1), dict(symmetric=1, layout_kind=1), dict(symmetric=0, layout_kind=0),
                    dict(symmetric=1, layout_kind=0)):  # (the last: what the setter makes of the handle for a symmetric schedule)
            for B in (1, 64, 1024, 1025, 4096, 4097, 65536):
                for dev in (dict(), dict(force_general=2), dict(force_general=5), dict(force_general=8), dict(persistent=1), dict(compaction=1),
                            dict(streams=2), dict(single_wave_rollout=3), dict(round_launch=2)):
                    kw = dict(ext, **own, **dev, B=B)
                    got = route(hs, scheduled=1, **kw)
                    assert got["backward"] == BW_ONE and not got["tiled"], (kw, got)
                    assert not (got["combined"] or got["fuse_kinds"] or got["round_kernel"] or got["late_tail"] or got["persistent"]), (kw, got)
                    assert got["lin_kind"] == 0 and got["admitted"] == 1, (kw, got)
                    ext_bits = 1 * ext["modeled"] + 2 * (ext["obstacles"] or ext["problem_obstacles"]) + 4 * ext["problem_obstacles"]
                    assert (0, ext["integrator"], 0, 0, ext_bits) in recorded, kw
                    seen_keys.add(got["key"])
                    # the rollout rule and the compaction are those of the same handle with non-symmetric weights and no schedule
                    ref = route(hs, scheduled=0, **dict(kw, symmetric=0, layout_kind=0, q_diag=0))
                    for k in ("rollout", "compact", "parts", "key", "backward", "tiled", "lin_kind"):
                        assert got[k] == ref[k], (k, kw, got, ref)
                    assert got["compact"] == (1 if dev.get("compaction") == 1 and not ext["modeled"] else 0), (kw, got)
    assert len(seen_keys) == 2 * 6  # either integrator x {plain, models, spheres, both, per-problem spheres, those with models}


def test_without_a_schedule_the_routes_are_the_recorded_ones():
    """tests/golden/routes.json through the unchanged tests/host_route_harness.cpp, whose aggregate never names the new field"""
    lib = _build("host_route_harness", [os.path.join(CSRC, "route.h"), os.path.join(HERE, "..", "include", "quadrotor_ilqr.h")])
    lib.hr_route.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    with open(os.path.join(HERE, "golden", "routes.json")) as f:
        golden = json.load(f)
    n_in, n_out = len(golden["inputs"]), len(golden["outputs"])
    out = np.zeros(n_out, dtype=np.int64)
    for row in np.array(golden["rows"], dtype=np.int64):
        inp = np.ascontiguousarray(row[:n_in])
        assert lib.hr_route(inp.ctypes.data_as(C.POINTER(C.c_long)), out.ctypes.data_as(C.POINTER(C.c_long))) == n_out
        assert np.array_equal(out, row[n_in:]), dict(zip(golden["inputs"], inp.tolist()))


def test_the_default_handle_keeps_its_route_when_the_flag_is_off(hs):
    got = route(hs, symmetric=1, layout_kind=2, q_diag=1, B=1024)
    assert got["combined"] and got["round_kernel"] and got["lin_kind"] == 3 and got["tiled"] and got["backward"] != BW_ONE


# ---- the setter's checks

def check(hs, Qs, n=None):
    sym, where = C.c_int(-1), (C.c_long * 3)(0, 0, 0)
    if Qs is None:
        rc = hs.hs_check(None, 0 if n is None else n, C.byref(sym), where)
    else:
        Qs = np.ascontiguousarray(Qs, dtype=np.float64)
        rc = hs.hs_check(Qs.ctypes.data_as(C.POINTER(C.c_double)), len(Qs) if n is None else n, C.byref(sym), where)
    return rc, sym.value, tuple(where)


def test_the_check_of_a_schedule(hs):
    Qs = sc.schedule("dense", 7)
    assert check(hs, Qs) == (0, 1, (-1, -1, -1))
    assert check(hs, sc.one_nonsymmetric(Qs)) == (0, 0, (-1, -1, -1))
    assert check(hs, None) == (0, 1, (-1, -1, -1))       # NULL, 0 clears
    assert check(hs, None, 3)[0] == 1                     # NULL with a count
    assert check(hs, Qs, 0)[0] == 1 and check(hs, Qs, -2)[0] == 1
    for bad in (np.nan, np.inf, -np.inf):
        for knot, row, col in ((0, 0, 0), (3, 11, 2), (6, 5, 11)):
            q = Qs.copy()
            q[knot, row, col] = bad
            q[6, 11, 11] = np.nan  # (a later one: the first is named)
            rc, _, where = check(hs, q)
            assert rc == 1 and where == (knot, row, col), (bad, where)
    semi = pb.waypoint_schedule(np.zeros((12, 12)), -pb.Q_DEMO, 4, (1,))  # definiteness is not checked
    assert check(hs, semi)[:2] == (0, 1)


def test_the_abi_without_a_device():
    lib = capi.load()
    Qs = sc.schedule("terminal", 4)
    p = Qs.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.qilqr_set_state_weight_schedule(None, p, C.c_int32(4)) == capi.ERR_INVALID_ARG
    assert b"null" in lib.qilqr_last_error()
    assert lib.qilqr_sharded_set_state_weight_schedule(None, p, C.c_int32(4)) == capi.ERR_INVALID_ARG
    assert {"qilqr_set_state_weight_schedule", "qilqr_sharded_set_state_weight_schedule"} <= set(capi.EXPORTS)
    for bad in (np.zeros((12, 12)), np.zeros((0, 12, 12)), np.zeros((3, 12, 11)), np.zeros((3, 144))):
        with pytest.raises(TypeError, match="state-weight schedule"):
            capi.schedule_array(bad)
    assert capi.schedule_array(list(Qs)).shape == (4, 12, 12)
