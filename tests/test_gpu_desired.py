"""Batch solves against desired trajectories that change from knot to knot and from problem to problem (tests/desired_cases.py), on every
route that reads the desired trajectory: k_linearize's cost half (plain and tiled), k_round's linearisation of its candidates (linearize_block
and round_follow, chunks of sixteen knots x four rows, or sixty-four knots of a lone trajectory), k_solve4 (diagnostics build), the tiling of
per-problem desired trajectories in begin_batch (fp64 and fp32) and the sub-batch part's view of them.  Each case is compared problem by
problem with an oracle built on that problem's own desired trajectory (tests/test_desired_cases_cpu.py shows that a wrong knot, problem or
column moves the oracle's solution far beyond these bars), and says from describe() which route it was written for.

fp64 bars: status, iterations, backward passes and rollouts equal -- or a near-tie the oracle's own decisions excuse
(tests/exit_paths.py) --, cost within 1e-9 relative, trajectory within 1e-6.  Mixed precision: test_config3_mixed_precision_reduced's bars
(cost 1e-3, trajectory 1e-2, every status 0 or 1).  Batches beyond a few hundred problems are compared on a fixed sample of rows (first and
last tile, both sides of every sub-batch boundary, the ragged tail); the rest is covered by the bit-identity properties below."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests.desired_cases import tracking_case  # noqa: E402
from tests.exit_paths import assert_same_exit_paths, batch_bound  # noqa: E402
from tests.observed import observed  # noqa: E402

KEYS = ("traj", "cost", "status", "iters", "n_bwd", "n_fwd")
COUNTS = KEYS[2:]
MIXED = dict(rtol=1e-5, atol=1e-5)  # config3's convergence tolerances


def oracle_for(cfg, desired, model=None, integrator=0):
    o = orc.OracleSolver(orc.model_params(**(model or cfg["model"])), cfg["Q"], cfg["R"], desired, cfg["dt"], orc.options(**cfg["options"]))
    if integrator:
        o.set_integrator(integrator)
    return o


def oracle_rows(cfg, des, rows, init=None, models=None, integrator=0):
    """the oracle of each row's own desired trajectory (and model), and its solution; at most 16 threads (ctypes releases the GIL)"""
    init = cfg["init"] if init is None else init

    def one(b):
        o = oracle_for(cfg, des[b], None if models is None else models[b], integrator)
        return o, o.solve(init[b])

    with ThreadPoolExecutor(max_workers=min(16, len(rows))) as ex:
        res = list(ex.map(one, rows))
    return [o for o, _ in res], {k: np.array([r[k] for _, r in res]) for k in KEYS}


def sample_rows(B, parts=1):
    """all rows up to 400; beyond, ~64 fixed rows: the first and last tile, both sides of every 64-row tile edge that is a sub-batch
    boundary (ilqr_capi.hip: part p starts at tile tiles * p / parts), a few tile edges inside the parts, and the ragged tail"""
    if B <= 400:
        return np.arange(B)
    tiles = (B + 63) // 64
    rows = {0, 1, 2, 31, 62, 63, 64, 65, B - 1, B - 2, ((B - 1) // 64) * 64, ((B - 1) // 64) * 64 - 1}
    for p in range(1, parts):
        e = (tiles * p // parts) * 64
        rows |= {e - 2, e - 1, e, e + 1}
    rows |= set(range(64 * 5 - 1, B - 64, max(64, (B // 40) // 64 * 64)))  # tile edges through the batch
    rows |= set(np.linspace(0, B - 1, 24).astype(int).tolist())
    return np.array(sorted(r for r in rows if 0 <= r < B))


def parts_of(text):
    return int(text.split("sub-batch streams: ")[1].split(";")[0]) if "sub-batch streams: " in text else 1


def check(out, cfg, des, rows, label, route, init=None, models=None, integrator=0, mixed=False):
    """rows of a device result against the oracle of each row's own desired trajectory.
    fp64: a row whose counts differ from the oracle's must be excused by tests/exit_paths.py (a comparison of the oracle's path decided
    by less than the rounding of either side); its cost is held to the bar, its trajectory -- one line-search step or iteration away
    from the oracle's by that decision -- is not.
    Mixed precision: the bars of test_config3_mixed_precision_reduced (cost 1e-3, every status 0 or 1, iteration counts within 3) for
    every row, and the trajectory bar of 1e-2 for every row whose counts are the oracle's.  fp32 rounding can flip an Armijo test of
    the last iterations (one line-search trial more or less, seen at 130 x 40: rows 4 and 68, counts (1, 10, 10, 12) against
    (1, 10, 10, 11)); the solve then ends on another step length along a direction in which this family's cost is flat -- 2.6e-2 in a
    control, 1.4e-6 of the cost --, which the trajectory bar is not about.  Such rows must stay a small minority (at most 1 in 10)."""
    init = cfg["init"] if init is None else init
    oracles, ref = oracle_rows(cfg, des, rows, init, models, integrator)
    got = {k: np.asarray(out[k])[rows] for k in KEYS}
    msg = f"{label}\nroute: {route}"
    if mixed:
        assert np.isin(got["status"], [0, 1]).all() and np.isin(ref["status"], [0, 1]).all(), (msg, got["status"], ref["status"])
        assert np.abs(got["iters"].astype(int) - ref["iters"]).max() <= 3, (msg, got["iters"], ref["iters"])
        np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-3, err_msg=msg)
        same = np.ones(len(rows), dtype=bool)
        for k in COUNTS:
            same &= got[k] == ref[k]
        assert (~same).sum() <= len(rows) // 10, (msg, np.nonzero(~same)[0])
        observed(f"desired trajectories, {label} ({int((~same).sum())} of {len(rows)} rows with other counts)",
                 {k: got[k][same] for k in KEYS}, {k: ref[k][same] for k in KEYS})
        np.testing.assert_allclose(got["traj"][same], ref["traj"][same], atol=1e-2, err_msg=msg)
        return
    same = np.ones(len(rows), dtype=bool)
    for k in COUNTS:
        same &= got[k] == ref[k]
    bound = batch_bound(got, ref, same)
    for j in np.nonzero(~same)[0]:  # a near-tie of the oracle's own decisions, problem by problem
        one = {k: got[k][j:j + 1] for k in KEYS}
        assert_same_exit_paths(one, {k: ref[k][j:j + 1] for k in KEYS}, oracles[j], init[rows[j]:rows[j] + 1], bound=bound,
                               label=f"{label}, batch row {rows[j]} (checked alone as")
    if same.any():
        observed(f"desired trajectories, {label} ({int((~same).sum())} of {len(rows)} rows excused)",
                 {k: got[k][same] for k in KEYS}, {k: ref[k][same] for k in KEYS})
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, err_msg=msg)
    np.testing.assert_allclose(got["traj"][same], ref["traj"][same], atol=1e-6, err_msg=msg)
    return ref


def assert_bits(a, b, what):
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{what}: {k}")


def assert_route(text, *parts, absent=()):
    for p in parts:
        assert p in text, f"route is not the one this case was written for: {p!r} missing from\n{text}"
    for p in absent:
        assert p not in text, f"route is not the one this case was written for: {p!r} in\n{text}"


# ------------------------------------------------------------------ one trajectory: k_round with one row per block (round_follow's 64-knot tasks)
@pytest.mark.parametrize("N", [16, 17, 100])
def test_one_trajectory_through_solve_and_solve_batch(N):
    cfg, des = tracking_case(1, N, seed=100 + N)
    s = capi.from_config(cfg)
    route = s.describe(1)
    assert_route(route, "k_round", "compaction: off")
    out = s.solve_batch(cfg["init"], des)
    check(out, cfg, des, np.arange(1), f"1 x {N}, solve_batch", route)
    own = capi.from_config(dict(cfg, desired=des[0]))  # qilqr_solve: the handle's own desired trajectory is this problem's
    traj, info = own.solve(cfg["init"][0])
    single = dict(traj=traj[None], cost=np.array([info["cost"]]), status=np.array([info["status"]]), iters=np.array([info["iters"]]))
    for k in ("traj", "cost", "status", "iters"):
        np.testing.assert_array_equal(single[k], out[k], err_msg=f"qilqr_solve against qilqr_solve_batch, {k}")
    assert_bits(own.solve_batch(cfg["init"]), out, "the handle's desired trajectory against desired_batch")


# ------------------------------------------------------------------ ragged blocks, horizons about round_follow's chunks of sixteen knots
@pytest.mark.parametrize("B", [6, 7, 9, 64])
def test_ragged_blocks_and_chunk_edges(B):
    for N in (15, 16, 17, 33, 65):
        cfg, des = tracking_case(B, N, seed=200 + B + N)
        s = capi.from_config(cfg)
        route = s.describe(B)
        assert_route(route, "k_round", "k_backward4, fused")
        check(s.solve_batch(cfg["init"], des), cfg, des, np.arange(B), f"{B} x {N}", route)


# ------------------------------------------------------------------ the batch sizes of the other launch forms
def profiled_solve(cfg, des, **kw):
    s = capi.from_config(cfg, profile=2, **kw)
    out = s.solve_batch(cfg["init"], des)
    return s, out, s.profile_get()


def test_headline_shape_k_round():
    cfg, des = tracking_case(1024, 100, seed=300)
    s, out, p = profiled_solve(cfg, des)
    route = s.describe(1024)
    assert_route(route, "k_round", "4 rounds per launch", "k_backward4, fused", "compaction: off")
    assert p["rollout_launches"] == 0 and p["backward_launches"] > 0, (p, route)  # every round a k_round launch
    assert np.isin(out["status"], [0, 1]).all()
    check(out, cfg, des, sample_rows(1024), "1024 x 100 (k_round)", route)


def test_three_launches_with_the_fused_backward_pass():
    cfg, des = tracking_case(2048, 40, seed=301)
    s, out, p = profiled_solve(cfg, des)
    route = s.describe(2048)
    assert_route(route, "k_backward4, fused", "k_rollout16", "sub-batch streams: 1")
    # desired_batch turns the compaction off (route.h: per-problem desired trajectories would have to move along), and with it the
    # change-over to k_round: the rounds stay three launches
    assert s.compaction_moves() == 0 and p["rollout_launches"] > 0 and p["linearize_launches"] > 0, (p, route)
    check(out, cfg, des, sample_rows(2048), "2048 x 40 (three launches, fused backward)", route)


def test_gradient_wavefront_factors_q_uu():
    cfg, des = tracking_case(3584, 40, seed=302)
    s, out, p = profiled_solve(cfg, des)
    route = s.describe(3584)
    assert_route(route, "k_backward4, fused", "six wavefronts, Q_uu factored by the gradient wavefront", "sub-batch streams: 1")
    assert s.compaction_moves() == 0 and p["rollout_launches"] > 0, (p, route)
    check(out, cfg, des, sample_rows(3584), "3584 x 40 (six-wavefront form while 3072 or more run)", route)


def test_beyond_the_regime_two_parts():
    B = 4352
    cfg, des = tracking_case(B, 40, seed=303)
    s, out, p = profiled_solve(cfg, des)
    route = s.describe(B)
    assert_route(route, "k_backward4, six wavefronts", "k_rollout3 for a trajectory's first 16 rollouts, k_rollout16 from there on",
                 "sub-batch streams: 2")
    assert s.compaction_moves() == 0 and p["rollout_launches"] > 0, (p, route)
    rows = sample_rows(B, parts_of(route))
    assert {2175, 2176} <= set(rows.tolist())  # (68 tiles in two parts: the second part starts at row 2176 -- the b0 offset)
    check(out, cfg, des, rows, f"{B} x 40 (k_backward4 six wavefronts, k_rollout3 then k_rollout16, two parts)", route)


def test_sub_batch_streams_keep_each_part_s_desired_rows():
    cfg, des = tracking_case(400, 40, seed=304)
    s = capi.from_config(cfg, streams=3)
    route = s.describe(400)
    assert_route(route, "sub-batch streams: 3")
    out = s.solve_batch(cfg["init"], des)
    check(out, cfg, des, sample_rows(400), "400 x 40, streams = 3", route)
    assert_bits(capi.from_config(cfg, streams=1).solve_batch(cfg["init"], des), out, "one stream against three")


@pytest.mark.parametrize("B,N", [(130, 40), (1024, 100)])
def test_mixed_precision(B, N):
    cfg, des = tracking_case(B, N, seed=305 + B, options=MIXED)
    s = capi.from_config(cfg, precision="f32")
    route = s.describe(B)
    assert_route(route, "mixed precision")
    check(s.solve_batch(cfg["init"], des), cfg, des, sample_rows(B), f"{B} x {N}, mixed precision", route, mixed=True)


def test_runge_kutta_plain_records():
    cfg, des = tracking_case(16, 30, seed=306)
    s = capi.from_config(cfg)
    s.set_integrator(1)
    route = s.describe(16)
    assert_route(route, "Runge-Kutta step", "k_rollout;")
    check(s.solve_batch(cfg["init"], des), cfg, des, np.arange(16), "16 x 30, Runge-Kutta", route, integrator=1)


def test_general_weights_one_wavefront_backward():
    # (the reference's forms model the cost with Q as given while the cost sees only its symmetric part: the last iteration's line search
    # backs off to steps whose Armijo tests compare differences of ~1e-13 of the cost, so most rows end on an excused near-tie)
    cfg, des = tracking_case(16, 30, seed=307)
    U = np.random.default_rng(307).uniform(-1, 1, (12, 12))
    cfg["Q"] = cfg["Q"] + 0.05 * U  # not symmetric: the reference's own forms
    assert not np.array_equal(cfg["Q"], cfg["Q"].T)
    s = capi.from_config(cfg, force_general=1)
    route = s.describe(16)
    assert_route(route, "the reference's own forms", "general kernel")
    check(s.solve_batch(cfg["init"], des), cfg, des, np.arange(16), "16 x 30, non-symmetric Q (general kernel)", route)


@pytest.mark.parametrize("B,streams", [(16, 0), (400, 3)])
def test_per_problem_models_and_desired_trajectories_stay_paired(B, streams):
    from tests.test_gpu_batch_models import random_models
    models = random_models(B, 308 + B)
    cfg, des = tracking_case(B, 30, seed=308, model=models)
    s = capi.from_config(cfg, streams=streams)
    s.set_models(models)
    route = s.describe(B)
    assert_route(route, "per-problem models", f"sub-batch streams: {max(streams, 1)}")
    out = s.solve_batch(cfg["init"], des)
    check(out, cfg, des, sample_rows(B), f"{B} x 30, per-problem models, streams = {streams}", route, models=models)
    if streams:
        one = capi.from_config(cfg, streams=1)
        one.set_models(models)
        assert_bits(one.solve_batch(cfg["init"], des), out, "per-problem models, one stream against three")


def test_thrust_limits_against_the_restatement():
    from tests import limited_numpy_ilqr as lim
    from tests.independent_numpy_ilqr import Model, pose_from_knot
    cfg, des = tracking_case(8, 30, seed=309)
    lo, hi = 2.1, 2.8  # the desired controls (hover 2.45 N +- 20 %) lie inside the box and outside it on both sides
    assert (des[:, :, 14:18] < lo).any() and (des[:, :, 14:18] > hi).any() and ((des[:, :, 14:18] > lo) & (des[:, :, 14:18] < hi)).any()
    s = capi.from_config(cfg)
    s.set_control_limits(lo, hi)
    route = s.describe(8)
    assert_route(route, "control limits", "box form")
    out = s.solve_batch(cfg["init"], des)
    for b in range(8):
        o = lim.LimitedILQR(Model(**cfg["model"]), cfg["Q"], cfg["R"], des[b], cfg["dt"], dict(cfg["options"]), lo, hi)
        ref = o.solve(cfg["init"][b])
        msg = f"problem {b}\nroute: {route}"
        assert [out[k][b] for k in COUNTS] == [ref[k] for k in COUNTS], msg
        np.testing.assert_allclose(out["cost"][b], ref["cost"], rtol=1e-9, err_msg=msg)
        for i in range(30):
            np.testing.assert_allclose(pose_from_knot(out["traj"][b, i]), pose_from_knot(ref["traj"][i]), atol=1e-6, err_msg=msg)
        np.testing.assert_allclose(out["traj"][b, :, 8:18], ref["traj"][:, 8:18], atol=1e-6, err_msg=msg)
    u = out["traj"][:, :, 14:18]
    assert u.min() >= lo and u.max() <= hi and ((u == lo).any() or (u == hi).any())


def test_obstacles_on_a_moving_desired_path():
    from tests import obstacle_numpy_ilqr as obs
    from tests.independent_numpy_ilqr import Model, pose_from_knot
    cfg, des = tracking_case(8, 30, seed=310)
    r = np.random.default_rng(310)
    spheres = np.array([[*(des[b, i, 1:4] + r.normal(size=3) * 0.05), 0.35, 20.0] for b, i in zip(range(8), r.integers(5, 25, 8))])
    s = capi.from_config(cfg)
    s.set_obstacles(spheres)
    route = s.describe(8)
    assert_route(route, "obstacles (extension)")
    out = s.solve_batch(cfg["init"], des)
    p = out["traj"][:, :, None, 1:4] - spheres[None, None, :, :3]
    assert (np.linalg.norm(des[:, :, None, 1:4] - spheres[None, None, :, :3], axis=-1) < spheres[:, 3]).any()
    assert (np.linalg.norm(p, axis=-1) < spheres[:, 3]).any()  # the solutions press against the spheres
    for b in range(8):
        o = obs.ObstacleILQR(Model(**cfg["model"]), cfg["Q"], cfg["R"], des[b], cfg["dt"], dict(cfg["options"]))
        o.set_obstacles(spheres)
        ref = o.solve(cfg["init"][b])
        msg = f"problem {b}\nroute: {route}"
        assert [out[k][b] for k in COUNTS] == [ref[k] for k in COUNTS], msg
        np.testing.assert_allclose(out["cost"][b], ref["cost"], rtol=1e-9, err_msg=msg)
        for i in range(30):
            np.testing.assert_allclose(pose_from_knot(out["traj"][b, i]), pose_from_knot(ref["traj"][i]), atol=1e-6, err_msg=msg)
        np.testing.assert_allclose(out["traj"][b, :, 8:18], ref["traj"][:, 8:18], atol=1e-6, err_msg=msg)


def test_sharded_is_the_single_handle_problem_by_problem():
    cfg, des = tracking_case(203, 40, seed=311)
    one = capi.from_config(cfg)
    a = one.solve_batch(cfg["init"], des)
    check(a, cfg, des, np.arange(203), "203 x 40, one handle", one.describe(203))
    many = capi.sharded_from_config(cfg, devices=[0, 0, 0])
    assert [c for _, c in many.shard_ranges(203)] != [203]
    assert_bits(many.solve_batch(cfg["init"], des), a, "three shards against one handle")


def solve_device(s, init, des):
    """qilqr_solve_batch_device with the initial and the desired trajectories in device buffers (the HIP runtime this process already
    runs on: tests/test_gpu_sharded._Hip)"""
    from tests.test_gpu_sharded import _Hip
    hip = _Hip()
    try:
        B, n = init.shape[0], init.shape[1]

        def upload(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            p = hip.alloc(a.nbytes)
            assert hip.lib.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), C.c_int(1)) == 0
            return p

        d_init, d_des = upload(init), upload(des)
        shapes = dict(traj=(init.shape, np.float64), cost=((B,), np.float64), **{k: ((B,), np.int32) for k in COUNTS})
        ptrs = {k: hip.alloc(int(np.prod(sh)) * np.dtype(dt).itemsize) for k, (sh, dt) in shapes.items()}
        rc = capi.load().qilqr_solve_batch_device(s._h, C.c_void_p(d_init), C.c_void_p(d_des), C.c_int32(B), C.c_int32(n),
                                                   *[C.c_void_p(ptrs[k]) for k in KEYS])
        assert rc == 0, capi.load().qilqr_last_error()
        assert hip.lib.hipDeviceSynchronize() == 0
        return {k: hip.download(ptrs[k], *shapes[k]) for k in KEYS}
    finally:
        hip.close()


def test_device_entry_point_with_a_device_desired_batch():
    cfg, des = tracking_case(777, 60, seed=312)
    s = capi.from_config(cfg)
    a = s.solve_batch(cfg["init"], des)
    d = solve_device(s, cfg["init"], des)
    assert_bits(d, a, "qilqr_solve_batch_device against qilqr_solve_batch")
    check(d, cfg, des, sample_rows(777), "777 x 60, device entry point", s.describe(777))


def test_persistent_solve():
    from tests.diag_lib import capi_diag
    cfg, des = tracking_case(203, 60, seed=313)
    s = capi_diag().from_config(cfg, persistent=1, profile=1)
    route = s.describe(203)
    assert_route(route, "k_solve4")
    s.profile_reset()
    out = s.solve_batch(cfg["init"], des)
    p = s.profile_get()
    assert p["solve_launches"] == 1 and p["backward_launches"] == 0 and p["rollout_launches"] == 0, (p, route)
    check(out, cfg, des, np.arange(203), "203 x 60, persistent (k_solve4)", route)


# ------------------------------------------------------------------ properties, bit for bit
ROUTES = [dict(B=7, N=17), dict(B=64, N=33), dict(B=1024, N=100), dict(B=2048, N=40), dict(B=400, N=40, streams=3),
          dict(B=130, N=40, precision="f32"), dict(B=1024, N=100, precision="f32"), dict(B=16, N=30, integrator=1),
          dict(B=16, N=30, force_general=1)]


def route_id(r):
    return "-".join(f"{k}{v}" for k, v in r.items())


def handle(cfg, r):
    kw = {k: v for k, v in r.items() if k in ("streams", "precision", "force_general")}
    s = capi.from_config(cfg, **kw)
    if r.get("integrator"):
        s.set_integrator(r["integrator"])
    return s


@pytest.mark.parametrize("r", ROUTES, ids=route_id)
def test_rows_equal_to_the_shared_trajectory_give_the_shared_call_s_bits(r):
    cfg, des = tracking_case(r["B"], r["N"], seed=400 + r["N"], shared=True, options=MIXED if r.get("precision") else None)
    s = handle(cfg, r)
    shared = s.solve_batch(cfg["init"])
    assert_bits(s.solve_batch(cfg["init"], des), shared, f"{route_id(r)}, desired_batch of the shared trajectory\nroute: {s.describe(r['B'])}")
    assert np.isin(shared["status"], [0, 1]).all()


@pytest.mark.parametrize("r", ROUTES, ids=route_id)
def test_the_time_column_changes_no_bit(r):
    cfg, des = tracking_case(r["B"], r["N"], seed=500 + r["N"], options=MIXED if r.get("precision") else None)
    s = handle(cfg, r)
    a = s.solve_batch(cfg["init"], des)
    other = des.copy()
    other[:, :, 0] = 1e6 - 3.0 * np.arange(r["N"])[None, :] - np.arange(r["B"])[:, None]
    assert_bits(s.solve_batch(cfg["init"], other), a, f"{route_id(r)}, desired_batch with another time column")
    # ... and of the handle's shared desired trajectory
    d2 = cfg["desired"].copy()
    d2[:, 0] = -7.0 * np.arange(r["N"])
    s2 = handle(dict(cfg, desired=d2), r)
    assert_bits(s2.solve_batch(cfg["init"]), s.solve_batch(cfg["init"]), f"{route_id(r)}, shared desired trajectory with another time column")


@pytest.mark.parametrize("n", [1, 2, 17, 40, 99])
def test_initial_trajectories_shorter_than_the_desired_one(n):
    """a handle of N_d = 100 desired knots solves n-knot problems against the first n knots (cost.hh:39-40), with the bits of a handle made
    with desired[:n] -- qilqr_solve, qilqr_solve_batch at B = 6 and 1024, qilqr_cost_trajectory, the reference's Python surface -- and the
    oracle's results"""
    cfg, _ = tracking_case(1024, 100, seed=600, shared=True)
    init = np.ascontiguousarray(cfg["init"][:, :n])
    long_, short = capi.from_config(cfg), capi.from_config(dict(cfg, desired=cfg["desired"][:n]))
    for B in (6, 1024):
        a, b = long_.solve_batch(init[:B]), short.solve_batch(init[:B])
        assert_bits(a, b, f"n = {n}, B = {B}\nroute: {long_.describe(B)}")
    des = np.broadcast_to(cfg["desired"][:n], init.shape)
    check(a, dict(cfg, init=init), des, sample_rows(1024), f"1024 x {n} against a 100-knot desired trajectory", long_.describe(1024), init=init)
    for b in range(3):
        t1, i1 = long_.solve(init[b])
        t2, i2 = short.solve(init[b])
        np.testing.assert_array_equal(t1, t2)
        assert (i1["cost"], i1["status"], i1["iters"]) == (i2["cost"], i2["status"], i2["iters"])
        np.testing.assert_array_equal(t1, a["traj"][b])
    np.testing.assert_array_equal(long_.cost_trajectory(init[:64]), short.cost_trajectory(init[:64]))
    from src.demo import extract_traj_array, options_message, trajectory_message
    from src.quadrotor_ilqr_binding import QuadrotorILQR
    m = cfg["model"]

    def binding(desired):
        return QuadrotorILQR(m["mass_kg"], m["inertia"], m["arm_length_m"], m["torque_to_thrust_ratio_m"], m["g_mpss"], cfg["Q"], cfg["R"],
                             trajectory_message(desired), cfg["dt"], options_message(cfg["options"]))

    t1, _ = binding(cfg["desired"]).solve(trajectory_message(init[0]))
    t2, _ = binding(cfg["desired"][:n]).solve(trajectory_message(init[0]))
    np.testing.assert_array_equal(extract_traj_array(t1), extract_traj_array(t2))
    np.testing.assert_array_equal(extract_traj_array(t1), a["traj"][0])


def test_a_desired_batch_longer_than_the_handle_s_desired_trajectory_is_accepted():
    """begin_batch checks the length against the handle's desired trajectory only when no desired_batch is given"""
    cfg, des = tracking_case(64, 60, seed=700)
    s = capi.from_config(dict(cfg, desired=cfg["desired"][:20]))
    with pytest.raises(IndexError):
        s.solve_batch(cfg["init"])
    out = s.solve_batch(cfg["init"], des)
    check(out, cfg, des, np.arange(64), "64 x 60 on a handle of 20 desired knots", s.describe(64))
    assert_bits(capi.from_config(cfg).solve_batch(cfg["init"], des), out, "the handle's own length against a shorter one")
