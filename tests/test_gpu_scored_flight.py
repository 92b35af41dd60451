"""The scored closed-loop flight on the device (qilqr_closed_loop_scored[_device], k_closed_loop_scored): with nothing new asked for, the
bits of qilqr_closed_loop_device, and of qilqr_closed_loop in the host form; under gusts against the restatement from the oracle's primitives (tests/scored_flight_numpy.py); the
score against qilqr_cost_trajectory on the flights themselves; across the kernel's two forms bit for bit (S = 64 and 126 share a plan's
operands through LDS -- the score's among them -- S = 70, 5 and 1 do not); over a window of knots; through the device form's stream
ordering; and through quadrotorilqr_amd.mpc.RecedingHorizon.evaluate.  n = 24 on closed_loop_numpy.plans."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc, scored_flight_numpy as sn  # noqa: E402
from tests.test_gpu_closed_loop import Hip, MODELS3  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 24, 21
N_DES, K0 = 40, 7


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


def case(B, **kw):
    cfg, plan = cn.plans(B, N, SEED)
    s = capi.from_config(cfg, **kw)
    gains, _ = s.backwards_pass(plan)
    return cfg, plan, s, gains


def spheres_on_the_way(plan):
    """8 shared spheres and one moving sphere per problem about the plans' paths (tests/test_scored_flight_cpu.py's placement)"""
    B = plan.shape[0]
    r = np.random.default_rng(SEED + 9)
    shared = np.zeros((8, 5))
    for j in range(8):
        b, i = j % B, 2 + 3 * (j % 7)
        shared[j, :3] = plan[b, i, 1:4] + 0.45 * (2.0 * r.random(3) - 1.0)
        shared[j, 3] = 0.12 + 0.04 * (j % 3)
        shared[j, 4] = 20.0 + 5.0 * j
    own = np.zeros((B, 2, 8))
    for b in range(B):
        own[b, 0, :3] = plan[b, 10, 1:4] + 0.25
        own[b, 0, 3:6] = (0.5, -0.4, 0.3)
        own[b, 0, 6:8] = (0.2, 40.0)
    return shared, own, np.ones(B, dtype=np.int32)


def scheduled_case(B):
    """(cfg, plan, solver, gains, Qs): a handle whose desired trajectory has 40 knots, a waypoint schedule with no two knots alike and the
    horizon start at 7; the plans start about desired[7:31]"""
    cfg, _ = dc.tracking_case(B, N_DES, SEED, shared=True)
    plan = dc.start_from(np.repeat(cfg["desired"][None, K0:K0 + N], B, axis=0), np.arange(B), SEED)
    s = capi.from_config(cfg)
    Qs = pb.waypoint_schedule(0.01 * pb.Q_DEMO, 10 * pb.Q_DEMO, N_DES, (3, 12, 19, 30, 39))
    for k in range(N_DES):
        Qs[k] = Qs[k] * (1.0 + 0.01 * k)
    s.set_state_weight_schedule(Qs)
    s.set_horizon_start(K0)
    gains, _ = s.backwards_pass(plan)
    return cfg, plan, s, gains, Qs


def scored_device(hip, s, plan, gains, x0, wrench=None, desired=None, i0=0, i1=N - 1, traj=True, stats=True, score=True):
    """one call of qilqr_closed_loop_scored_device through ctypes on 0xFF-prefilled outputs: (rc, traj, stats, score) as raw downloads"""
    B, S = x0.shape[0], x0.shape[1]
    lib = capi.load()
    d = [hip.upload(a) for a in (plan, gains, x0)]
    d_w = hip.upload(wrench) if wrench is not None else None
    d_des = hip.upload(desired) if desired is not None else None
    d_traj = hip.alloc(8 * B * S * N * 18) if traj else None
    d_stats = hip.alloc(8 * B * S * 4) if stats else None
    d_score = hip.alloc(8 * B * S * 4) if score else None
    rc = lib.qilqr_closed_loop_scored_device(s._h, d[0], d[1], d[2], d_w, 1 if wrench is None else wrench.shape[2], d_des, B, N, S, i0, i1, d_traj, d_stats, d_score)
    assert rc == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    return (hip.download(d_traj, (B, S, N, 18)) if traj else None, hip.download(d_stats, (B, S, 4)) if stats else None,
            hip.download(d_score, (B, S, 4)) if score else None)


# ------------------------------------------------------------------------------------------------ 1. nothing new asked for: the parent's bits

@pytest.mark.parametrize("S", [64, 70])
def test_with_the_three_new_arguments_null_it_has_the_bits_of_closed_loop_device(hip, S):
    B = 3
    cfg, plan, s, gains = case(B)
    s.set_control_limits(0.5, 5.0)
    x0 = cn.sample_states(plan, S, 0, SEED + 1)
    lib = capi.load()
    d = [hip.upload(a) for a in (plan, gains, x0)]
    d_traj, d_stats = hip.alloc(8 * B * S * N * 18), hip.alloc(8 * B * S * 4)
    assert lib.qilqr_closed_loop_device(s._h, d[0], d[1], d[2], B, N, S, 0, N - 1, d_traj, d_stats) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    want_traj, want_stats = hip.download(d_traj, (B, S, N, 18)), hip.download(d_stats, (B, S, 4))
    got_traj, got_stats, _ = scored_device(hip, s, plan, gains, x0, score=False)
    assert not np.isnan(want_traj).any() and got_traj.tobytes() == want_traj.tobytes() and got_stats.tobytes() == want_stats.tobytes()
    # ... and so through capi
    host = s.closed_loop(plan, gains, x0)
    assert host["traj"].tobytes() == want_traj.tobytes() and host["stats"].tobytes() == want_stats.tobytes() and sorted(host) == ["stats", "traj"]


def test_the_plain_host_form_is_the_scored_one_with_the_three_new_arguments_null():
    """qilqr_closed_loop and qilqr_closed_loop_scored(wrench = desired = out_score = NULL) through ctypes, on a handle with thrust limits:
    the same bytes in 0xFF-prefilled outputs in both forms of the kernel, over all knots and over a window, and the same refusals"""
    B = 3
    cfg, plan, s, gains = case(B)
    s.set_control_limits(0.5, 5.0)
    lib = capi.load()
    plan, gains = capi._d16(plan), capi._d16(gains)

    def both(handle, x0, i0, i1):
        """[(rc, the last error, out_traj, out_stats)] of the plain and of the scored entry point"""
        S, out = x0.shape[1], []
        for scored in (False, True):
            traj, stats = capi._d16(np.empty((B, S, N, 18))), capi._d16(np.empty((B, S, 4)))
            traj.view(np.uint8)[...] = 0xFF
            stats.view(np.uint8)[...] = 0xFF
            head, tail = (handle._h, plan.ctypes.data, gains.ctypes.data, x0.ctypes.data), (B, N, S, i0, i1, traj.ctypes.data, stats.ctypes.data)
            rc = lib.qilqr_closed_loop_scored(*head, None, 0, None, *tail, None) if scored else lib.qilqr_closed_loop(*head, *tail)
            out.append((rc, lib.qilqr_last_error().decode() if rc else "", traj, stats))
        return out

    for S in (5, 64):  # the flattened and the shared-operand form
        for i0, i1 in ((0, N - 1), (3, 17)):
            x0 = capi._d16(cn.sample_states(plan, S, i0, SEED + 11 + i0))
            (rc_p, _, traj_p, stats_p), (rc_s, _, traj_s, stats_s) = both(s, x0, i0, i1)
            assert rc_p == 0 and rc_s == 0, (S, i0, i1, lib.qilqr_last_error())
            assert traj_p.tobytes() == traj_s.tobytes() and stats_p.tobytes() == stats_s.tobytes(), (S, i0, i1)
            raw = traj_p.view(np.uint8).reshape(B, S, N, 18 * 8)
            assert (raw[:, :, :i0] == 0xFF).all() and (raw[:, :, i1 + 1:] == 0xFF).all(), (S, i0, i1)
            assert not np.isnan(traj_p[:, :, i0:i1 + 1]).any() and not np.isnan(stats_p).any() and np.array_equal(traj_p[:, :, i0, 1:14], x0), (S, i0, i1)
    # what a handle makes both refuse: the same code, the same words
    x0 = capi._d16(cn.sample_states(plan, 5, 0, SEED + 11))
    other_count = capi.from_config(cfg)
    other_count.set_models([MODELS3[b % 3] for b in range(B)])  # (B models, and B * S = 15 samples)
    for handle, why in ((capi.from_config(cfg, precision="f32"), "precision 0"), (other_count, "they were set for 3, this call has B * S = 15")):
        (rc_p, text_p, traj_p, _), (rc_s, text_s, traj_s, _) = both(handle, x0, 0, N - 1)
        assert rc_p == rc_s == capi.ERR_INVALID_ARG and text_p == text_s and why in text_p, (rc_p, rc_s, text_p, text_s)
        assert (traj_p.view(np.uint8) == 0xFF).all() and (traj_s.view(np.uint8) == 0xFF).all()


# ------------------------------------------------------------------------------------------------ 2. the restatement

@pytest.fixture(scope="module")
def gusty():
    """B = 3, S = 70: plans, gains, sampled states, per-knot gusts and spheres (computed once, never written to)"""
    B, S = 3, 70
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 1)
    gust = pb.gust_wrenches(B, S, N, SEED + 2, 1.5, 0.05)
    shared, own, counts = spheres_on_the_way(plan)
    for a in (plan, gains, x0, gust, shared, own, counts):
        a.setflags(write=False)
    return cfg, plan, gains, x0, gust, shared, own, counts


@pytest.mark.parametrize("integrator, ext", [(0, "plain"), (1, "plain"), (0, "limits"), (1, "models")])
def test_gusty_flights_against_the_restatement(gusty, integrator, ext):
    cfg, plan, gains, x0, gust, shared, own, counts = gusty
    B, S = x0.shape[0], x0.shape[1]
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    s.set_obstacles(shared)
    s.set_batch_obstacles(own, counts)
    limits = models = None
    if ext == "limits":
        limits = (1.0, 4.0)
        s.set_control_limits(*limits)
    if ext == "models":
        models = [MODELS3[(r + 1) % 3] for r in range(B * S)]
        s.set_models(models)
    want_traj, want_stats, want_score, clear = sn.scored_flight(plan, gains, x0, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], cfg["desired"], integrator=integrator,
                                                                models=models, limits=limits, wrench=gust, shared=shared,
                                                                own=[own[b, :counts[b]] for b in range(B)])
    got = s.closed_loop(plan, gains, x0, wrench=gust, score=True)
    over = lambda g, w: float((np.abs(g - w) / (sn.ATOL + sn.RTOL * np.abs(w))).max())
    print("[observed] integrator %d, %s: largest error over its bound %.3g (trajectories), %.3g (statistics), %.3g (cost), %.3g (clearance)" % (
        integrator, ext, over(got["traj"], want_traj), over(got["stats"], want_stats), over(got["score"][..., 0], want_score[..., 0]),
        over(got["score"][..., 1], want_score[..., 1])))
    np.testing.assert_allclose(got["traj"], want_traj, rtol=sn.RTOL, atol=sn.ATOL)
    np.testing.assert_allclose(got["stats"][..., :3], want_stats[..., :3], rtol=sn.RTOL, atol=sn.ATOL)
    assert np.array_equal(got["stats"][..., 3], want_stats[..., 3])
    gap, zero = sn.margins(clear)
    assert gap > 1e-6 and zero > 1e-6, (gap, zero)  # (neither the knot nor the count can flip inside the bound)
    np.testing.assert_allclose(got["score"][..., :2], want_score[..., :2], rtol=sn.RTOL, atol=sn.ATOL)
    assert np.array_equal(got["score"][..., 2:], want_score[..., 2:])
    assert (got["score"][..., 3] > 0).any() and (got["score"][..., 3] == 0).any()
    if ext == "limits":
        assert (got["stats"][..., 3] > 0).any()
    # the gusts are felt
    calm = s.closed_loop(plan, gains, x0)
    assert (np.abs(calm["traj"][:, :, -1, 1:4] - got["traj"][:, :, -1, 1:4]).max(axis=2) > 1e-6).all()


# ------------------------------------------------------------------------------------------------ 3. the score alone, against qilqr_cost_trajectory

@pytest.mark.parametrize("S", [5, 64])
def test_a_score_only_call_charges_what_cost_trajectory_charges_the_flights(hip, S):
    B = 3
    cfg, plan, s, gains, Qs = scheduled_case(B)
    shared, own, counts = spheres_on_the_way(plan)
    s.set_obstacles(shared)
    s.set_batch_obstacles(own, counts)
    x0 = cn.sample_states(plan, S, 0, SEED + 4)
    gust = pb.gust_wrenches(B, S, N, SEED + 5, 1.5, 0.05)
    _, _, score = scored_device(hip, s, plan, gains, x0, wrench=gust, traj=False, stats=False)
    flights = s.closed_loop(plan, gains, x0, wrench=gust, score=True)  # a second call wrote the flights
    assert flights["score"].tobytes() == score.tobytes()
    # cost_trajectory reads row b of the per-problem table for trajectory b: sample j of every plan is one batch of B trajectories
    want = np.stack([s.cost_trajectory(np.ascontiguousarray(flights["traj"][:, j])) for j in range(S)], axis=1)
    print("[observed] S = %d: cost against cost_trajectory, largest error over its bound %.3g" % (
        S, float((np.abs(score[..., 0] - want) / (sn.ATOL + sn.RTOL * np.abs(want))).max())))
    np.testing.assert_allclose(score[..., 0], want, rtol=1e-10, atol=1e-10)
    assert (score[..., 3] > 0).any()  # (spheres were charged)
    # the schedule and the start are read: another start, another cost
    s.set_horizon_start(K0 + 1)
    assert (s.closed_loop(plan, gains, x0, traj=False, stats=False, wrench=gust, score=True)["score"][..., 0] != score[..., 0]).all()
    # ... and a desired trajectory per plan is taken whatever the start: the handle's own window gives the cost of start 7 again
    per_plan = np.ascontiguousarray(np.repeat(cfg["desired"][None, K0:K0 + N], B, axis=0))
    s.clear_state_weight_schedule()
    s.set_horizon_start(K0)
    at7 = s.closed_loop(plan, gains, x0, traj=False, stats=False, wrench=gust, score=True)["score"]
    s.set_horizon_start(0)
    assert s.closed_loop(plan, gains, x0, traj=False, stats=False, wrench=gust, score=True, desired=per_plan)["score"].tobytes() == at7.tobytes()


# ------------------------------------------------------------------------------------------------ 4. one arithmetic across the forms

@pytest.mark.parametrize("kind", ["handle", "schedule"])
@pytest.mark.parametrize("integrator", [0, 1])
def test_a_samples_bits_do_not_depend_on_the_form_that_carried_it(gusty, integrator, kind):
    cfg, plan, gains, x0, gust, shared, own, counts = gusty
    if kind == "schedule":  # (a knot's Q changes with the knot: the double-buffered half of the LDS image)
        cfg, plan, s, gains, _ = scheduled_case(3)
        x0 = cn.sample_states(plan, 70, 0, SEED + 1)
        shared, own, counts = spheres_on_the_way(plan)
    else:
        s = capi.from_config(cfg)
    s.set_integrator(integrator)
    s.set_control_limits(0.5, 5.0)
    s.set_obstacles(shared)
    s.set_batch_obstacles(own, counts)
    fly = lambda idx, **kw: s.closed_loop(plan, gains, x0[:, idx], wrench=gust[:, idx], score=True, **kw)
    same = lambda a, b, idx: all(a[k].tobytes() == b[k][:, idx].tobytes() for k in ("traj", "stats", "score"))
    whole = fly(list(range(70)))  # S = 70: the flattened form
    assert np.isfinite(whole["score"]).all() and (whole["score"][..., 2] >= 0).all() and (whole["stats"][..., 3] > 0).any()
    if kind == "handle":
        assert (whole["score"][..., 3] > 0).any()
    for j in (0, 63, 64, 69):  # S = 1
        assert same(fly([j]), whole, [j]), j
    pick = [69, 0, 64, 7, 63]  # S = 5
    assert same(fly(pick), whole, pick)
    first = list(range(64))  # S = 64: the shared-operand form, one wavefront per plan: the score's operands come out of LDS
    assert same(fly(first), whole, first)
    again = list(range(70)) + list(range(56))  # S = 126: two wavefronts per plan, two idle lanes in the second
    assert same(fly(again), whole, again)
    # the switches alone: the wrench without a score, the score without a wrench, in both forms
    for idx in (first, pick):
        assert s.closed_loop(plan, gains, x0[:, idx], wrench=gust[:, idx])["traj"].tobytes() == whole["traj"][:, idx].tobytes()
    calm70, calm64 = s.closed_loop(plan, gains, x0, score=True), s.closed_loop(plan, gains, x0[:, first], score=True)
    assert calm64["score"].tobytes() == calm70["score"][:, first].tobytes() and calm64["traj"].tobytes() == s.closed_loop(plan, gains, x0[:, first])["traj"].tobytes()
    # a constant wrench is the repeated row
    one = np.ascontiguousarray(gust[:, :, 3:4])
    for idx in (first, pick):
        a = s.closed_loop(plan, gains, x0[:, idx], wrench=one[:, idx], score=True)
        b = s.closed_loop(plan, gains, x0[:, idx], wrench=np.ascontiguousarray(np.repeat(one[:, idx], N, axis=2)), score=True)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ------------------------------------------------------------------------------------------------ 5. a window, 6. stream ordering

@pytest.mark.parametrize("S", [5, 64])
def test_a_window_of_knots(hip, gusty, S):
    cfg, plan, gains, x0, gust, shared, own, counts = gusty
    B = 3
    s = capi.from_config(cfg)
    s.set_obstacles(shared)
    s.set_batch_obstacles(own, counts)
    x3 = cn.sample_states(plan, S, 3, SEED + 6)
    w = np.ascontiguousarray(gust[:, :S])
    traj, stats, score = scored_device(hip, s, plan, gains, x3, wrench=w, i0=3, i1=17)
    raw = traj.view(np.uint8).reshape(B, S, N, 18 * 8)
    assert (raw[:, :, :3] == 0xFF).all() and (raw[:, :, 18:] == 0xFF).all() and not np.isnan(traj[:, :, 3:18]).any()
    # the score covers the window only: the restatement's over the same knots (rows of the wrench outside it are never read)
    w_nan = w.copy()
    w_nan[:, :, :3] = np.nan
    w_nan[:, :, 17:] = np.nan
    _, _, again = scored_device(hip, s, plan, gains, x3, wrench=w_nan, i0=3, i1=17, traj=False, stats=False)
    assert again.tobytes() == score.tobytes()
    want = sn.scored_flight(plan, gains, x3, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], cfg["desired"], i0=3, i1=17, wrench=w, shared=shared,
                            own=[own[b, :counts[b]] for b in range(B)])
    gap, zero = sn.margins(want[3])
    assert gap > 1e-6 and zero > 1e-6
    np.testing.assert_allclose(score[..., :2], want[2][..., :2], rtol=sn.RTOL, atol=sn.ATOL)
    assert np.array_equal(score[..., 2:], want[2][..., 2:]) and ((score[..., 2] >= 3) & (score[..., 2] <= 17)).all()
    whole = s.closed_loop(plan, gains, x3, 3, N - 1, wrench=w, score=True)
    assert whole["traj"][:, :, 3:18].tobytes() == traj[:, :, 3:18].tobytes() and (whole["score"][..., 0] > score[..., 0]).all()


@pytest.mark.parametrize("S", [1, 64, 70])
def test_the_device_forms_in_a_row_and_one_synchronise(hip, S):
    B = 6
    cfg, plan, s, gains = case(B)
    shared, own, counts = spheres_on_the_way(plan)
    s.set_obstacles(shared)
    s.set_batch_obstacles(own, counts)
    x0 = cn.sample_states(plan, S, 0, SEED + 7)
    gust = pb.gust_wrenches(B, S, N, SEED + 8, 1.5, 0.05)
    want = s.closed_loop(plan, gains, x0, wrench=gust, score=True)
    lib = capi.load()
    d_plan, d_x0, d_w = hip.upload(plan), hip.upload(x0), hip.upload(gust)
    d_gains, d_traj, d_stats, d_score, d_only = (hip.alloc(a.nbytes) for a in (gains, want["traj"], want["stats"], want["score"], want["score"]))
    assert lib.qilqr_backwards_pass_device(s._h, d_plan, B, N, d_gains, None) == 0, lib.qilqr_last_error()
    assert lib.qilqr_closed_loop_scored_device(s._h, d_plan, d_gains, d_x0, d_w, N, None, B, N, S, 0, N - 1, d_traj, d_stats, d_score) == 0, lib.qilqr_last_error()
    assert lib.qilqr_closed_loop_scored_device(s._h, d_plan, d_gains, d_x0, d_w, N, None, B, N, S, 0, N - 1, None, None, d_only) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    for ptr, k in ((d_traj, "traj"), (d_stats, "stats"), (d_score, "score"), (d_only, "score")):
        assert hip.download(ptr, want[k].shape).tobytes() == want[k].tobytes(), k


def test_what_a_scored_call_refuses_on_a_handle():
    B, S = 3, 5
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 6)
    gust = pb.gust_wrenches(B, S, N, SEED, 1.0, 0.01)
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").closed_loop(plan, gains, x0, score=True)
    with pytest.raises(TypeError, match="n_w must be 1"):
        s.closed_loop(plan, gains, x0, wrench=gust[:, :, :2])
    bad = gust.copy()
    bad[2, 3, 11, 4] = np.inf
    with pytest.raises(TypeError, match="non-finite value at problem 2, sample 3, knot 11"):
        s.closed_loop(plan, gains, x0, wrench=bad)
    s.set_batch_obstacles(np.array([[[0.0, 0, 0, 0, 0, 0, 0.1, 1.0]]] * (B + 1)))
    with pytest.raises(TypeError, match="per-problem obstacles were set for another B"):
        s.closed_loop(plan, gains, x0, score=True)
    assert sorted(s.closed_loop(plan, gains, x0, wrench=gust)) == ["stats", "traj"]  # (without a score the table plays no part)
    s.clear_batch_obstacles()
    short = capi.from_config(dict(cfg, desired=cfg["desired"][:N - 2]))
    with pytest.raises(IndexError, match="beyond the handle's desired trajectory"):
        short.closed_loop(plan, gains, x0, score=True)
    assert short.closed_loop(plan, gains, x0, 0, N - 3, score=True)["score"].shape == (B, S, 4)
    assert short.closed_loop(plan, gains, x0, score=True, desired=plan)["score"].shape == (B, S, 4)
    s.set_state_weight_schedule(np.repeat(np.asarray(cfg["Q"], dtype=np.float64)[None], N - 1, axis=0))
    with pytest.raises(IndexError, match="beyond the state-weight schedule"):
        s.closed_loop(plan, gains, x0, score=True)
    for shape_error in (lambda: s.closed_loop(plan, gains, x0, wrench=gust[:, :, :, :5]), lambda: s.closed_loop(plan, gains, x0, wrench=gust[:, :4]),
                        lambda: s.closed_loop(plan, gains, x0, score=True, desired=plan[:, :-1])):
        with pytest.raises(TypeError):
            shape_error()
    out = s.closed_loop(plan, gains, x0, 0, N - 2, traj=False, stats=False, score=True)
    assert sorted(out) == ["score"] and np.isposinf(out["score"][..., 1]).all() and (out["score"][..., 2] == -1).all() and (out["score"][..., 3] == 0).all()


# ------------------------------------------------------------------------------------------------ 7. RecedingHorizon.evaluate

@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/scored_flight_torch_child.py, once (PyTorch's ROCm runtime has to be the first a process initialises).  The arrays it recorded."""
    out = str(tmp_path_factory.mktemp("scored_flight_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.scored_flight_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_receding_horizon_evaluate_against_closed_loop_scored(torch_forms):
    r = torch_forms
    for tick in range(2):
        tag = "tick%d_" % tick
        assert r[tag + "keys"].tolist() == ["score", "stats"]
        assert r[tag + "stats"].shape == (6, 70, 4) and r[tag + "score"].shape == (6, 70, 4) and np.isfinite(r[tag + "score"][..., 0]).all()
        assert r[tag + "stats"].tobytes() == r[tag + "host_stats"].tobytes() and r[tag + "score"].tobytes() == r[tag + "host_score"].tobytes()
        assert r[tag + "calm_score"].tobytes() == r[tag + "host_calm_score"].tobytes() and (r[tag + "calm_score"][..., 0] != r[tag + "score"][..., 0]).all()
        assert np.isfinite(r[tag + "score"][..., 1]).all() and (r[tag + "score"][..., 2] >= 0).all()  # (the handle's spheres are seen)
    said = {k[len("refusal_"):]: str(v) for k, v in r.items() if k.startswith("refusal_")}
    assert said["fine"] == "accepted", said["fine"]
    for k, kind, text in (("evaluate_without_gains", "RuntimeError", "gains=True"), ("x0_shape", "TypeError", "x0 must be"),
                          ("wrench_shape", "TypeError", "wrench must be"), ("score_shape", "TypeError", "out_score must have shape"),
                          ("wrench_float32", "TypeError", "float64"), ("wrench_rows", "TypeError", "n_w must be 1"),
                          ("desired_host", "TypeError", "CUDA tensor")):
        assert said[k].startswith(kind) and text in said[k], (k, said[k])
