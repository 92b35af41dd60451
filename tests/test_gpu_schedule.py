"""The per-knot state-weight schedule on the device (qilqr_set_state_weight_schedule: the cost half of k_linearize takes knot i's Q
from the schedule, and the handle the route of non-symmetric weights) against the NumPy restatement (tests/schedule_numpy_ilqr.py):
every pass with either one-wavefront backward kernel and each extension, whole solves, the knot index, bits equal to a handle without a
schedule where the schedule repeats the handle's Q, independence of batch, order, compaction, streams and shards, a terminal weight
doing what it is for, the route's text, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import schedule_cases as sc  # noqa: E402
from tests.independent_numpy_ilqr import pose_from_knot  # noqa: E402
from tests.test_gpu_obstacles import KEYS, device_solve, split_gains  # noqa: E402
from tests.test_gpu_parity import random_cfg  # noqa: E402

# (schedule, one non-symmetric Q_i, integrator, thrust limits, per-problem models, a shared sphere)
PASS_CASES = [
    ("terminal", False, 0, None, False, False),   # symmetric: k_backward<true> on dense records, against recursion 1
    ("waypoint", False, 0, None, False, False),   # ... semi-definite Q_i
    ("dense", False, 0, None, False, False),
    ("dense", True, 0, None, False, False),       # one non-symmetric Q_i: the general kernel, against recursion 0
    ("terminal", True, 0, None, False, False),
    ("dense", False, 1, None, False, False),      # Runge-Kutta
    ("terminal", False, 0, (0.5, 4.5), False, False),  # thrust limits: the box form
    ("waypoint", False, 0, None, True, False),    # per-problem models
    ("dense", True, 0, None, False, True),        # a shared sphere on the path, the general kernel
    ("terminal", False, 1, None, True, True),     # Runge-Kutta, models and the sphere together
]


@pytest.mark.parametrize("case", range(len(PASS_CASES)))
def test_passes_match_the_restatement(case):
    kind, nonsym, integrator, limits, models, sphere = PASS_CASES[case]
    n = 12
    cfg = random_cfg(300 + case, n=n, dense=False, B=3)
    trajs = cfg["init"]
    Qs = sc.schedule(kind, n)
    if nonsym:
        Qs = sc.one_nonsymmetric(Qs)
    spheres = np.array([[*(trajs[0, 5, 1:4] + [0.1, -0.05, 0.08]), 0.7, 15.0]]) if sphere else None
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    if limits:
        s.set_control_limits(*limits)
    mods = [dict(cfg["model"], mass_kg=cfg["model"]["mass_kg"] * (0.8 + 0.1 * b)) for b in range(len(trajs))] if models else None
    if models:
        s.set_models(mods)
    if sphere:
        s.set_obstacles(spheres)
    s.set_state_weight_schedule(Qs)
    text = s.describe(len(trajs))
    assert ("k_backward_models<" if models else "k_backward<") + ("false>" if nonsym else "true>") in text, text
    cost = s.cost_trajectory(trajs)
    gains, terms = s.backwards_pass(trajs)
    ls = s.line_search(trajs, cost, gains, terms)
    for b in range(len(trajs)):
        o = sc.restatement(cfg, Qs, 0 if nonsym else 1, mods[b] if models else None, limits, integrator, spheres)
        pts = o.unpack(trajs[b])
        np.testing.assert_allclose(cost[b], o.cost_trajectory(pts), rtol=1e-10)
        ks, Ks, t = o.backwards_pass(pts)
        k_dev, K_dev = split_gains(gains[b])
        scale = max(np.abs(np.array(ks)).max(), np.abs(np.array(Ks)).max())
        np.testing.assert_allclose(k_dev, np.array(ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(K_dev, np.array(Ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(terms[b], t, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(t).max()))
        # the line search: the step and the cost of the accepted candidate against the restatement's search with the device's gains
        step, found = 1.0, False
        for _ in range(cfg["options"]["ls_max_iters"]):
            c = o.cost_trajectory(o.forward_sim(pts, list(k_dev), list(K_dev), step))
            if c - cost[b] < cfg["options"]["desired_reduction_frac"] * (step * terms[b][0] + step * step * terms[b][1] / 2.0):
                found = True
                break
            step *= cfg["options"]["step_update"]
        assert (ls["status"][b] == 0) == found, b
        if found:
            assert ls["step"][b] == step, b
            np.testing.assert_allclose(ls["cost"][b], c, rtol=1e-9)


def assert_solve_matches(out, b, ref, row=None):
    row = b if row is None else row
    assert [out["status"][row], out["iters"][row], out["n_bwd"][row], out["n_fwd"][row]] == \
        [ref["status"], ref["iters"], ref["n_bwd"], ref["n_fwd"]], b
    np.testing.assert_allclose(out["cost"][row], ref["cost"], rtol=1e-9)
    for i in range(len(ref["traj"])):
        np.testing.assert_allclose(pose_from_knot(out["traj"][row, i]), pose_from_knot(ref["traj"][i]), atol=1e-6)
    np.testing.assert_allclose(out["traj"][row, :, 8:18], ref["traj"][:, 8:18], atol=1e-6)


@pytest.mark.parametrize("N", sc.SIZES)
@pytest.mark.parametrize("kind", sc.KINDS)
def test_solves_match_the_restatement(N, kind):
    """B = 6; the restatement solves problems 0-2 (tests/schedule_cases.py), symmetric schedules: k_backward<true> against recursion 1"""
    cfg = sc.config(N)
    s = capi.from_config(cfg)
    s.set_state_weight_schedule(sc.schedule(kind, N))
    out = s.solve_batch(cfg["init"])
    for b in sc.PROBLEMS:
        assert_solve_matches(out, b, sc.solved(N, kind, b))


@pytest.mark.parametrize("kind", sc.KINDS)
def test_the_single_solve_and_its_history(kind):
    N = 12
    cfg = sc.config(N)
    cfg["options"] = dict(cfg["options"], populate_debug=True)
    s = capi.from_config(cfg)
    s.set_state_weight_schedule(sc.schedule(kind, N))
    for b in sc.PROBLEMS[:2]:
        ref = sc.solved(N, kind, b)
        traj, info = s.solve(cfg["init"][b])
        assert [info["status"], info["iters"]] == [ref["status"], ref["iters"]]  # (qilqr_solve returns no pass counts: the batch solve below)
        assert len(info["debug_costs"]) == info["iters"] == len(ref["cost_hist"])
        np.testing.assert_allclose(info["debug_costs"], ref["cost_hist"], rtol=1e-9)
        np.testing.assert_allclose(info["cost"], ref["cost"], rtol=1e-9)
        np.testing.assert_allclose(traj[:, 8:18], ref["traj"][:, 8:18], atol=1e-6)
    out = s.solve_batch(cfg["init"][:2])  # ... and the batch solve's cost history
    hist = s.cost_history(2)
    for b in range(2):
        ref = sc.solved(N, kind, b)
        assert [out[k][b] for k in sc.COUNTS] == [ref[k] for k in sc.COUNTS]
        np.testing.assert_allclose(hist[b, :ref["iters"]], ref["cost_hist"], rtol=1e-9)


def test_the_knot_index_over_tiles_and_two_knots():
    """B = 70 (a partly empty second tile of 64), n = 2, every Q_i different"""
    n, B = 2, 70
    cfg = random_cfg(411, n=n, dense=False, B=B)
    Qs = sc.schedule("dense", 5)[3:5]
    assert not np.array_equal(Qs[0], Qs[1])
    s = capi.from_config(cfg)
    s.set_state_weight_schedule(Qs)
    cost = s.cost_trajectory(cfg["init"])
    gains, terms = s.backwards_pass(cfg["init"])
    for b in (0, 1, 63, 64, 69):
        o = sc.restatement(cfg, Qs, 1)
        pts = o.unpack(cfg["init"][b])
        np.testing.assert_allclose(cost[b], o.cost_trajectory(pts), rtol=1e-10)
        ks, Ks, t = o.backwards_pass(pts)
        k_dev, K_dev = split_gains(gains[b])
        scale = max(np.abs(np.array(ks)).max(), np.abs(np.array(Ks)).max())
        np.testing.assert_allclose(k_dev, np.array(ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(K_dev, np.array(Ks), rtol=1e-8, atol=1e-9 * scale)
        swapped = sc.restatement(cfg, Qs[::-1], 1).cost_trajectory(pts)  # (the comparison tells the knots apart)
        assert abs(swapped - cost[b]) > 1e-6 * abs(cost[b])


def test_longer_schedules_shorter_calls_and_the_refusal_of_longer_ones():
    n = 12
    cfg = random_cfg(412, n=n, dense=False, B=3)
    Qs20 = sc.schedule("dense", 20)
    s, t = capi.from_config(cfg), capi.from_config(cfg)
    s.set_state_weight_schedule(Qs20)       # n_knots = 20: the first 12 are used
    t.set_state_weight_schedule(Qs20[:n])
    assert np.array_equal(s.cost_trajectory(cfg["init"]), t.cost_trajectory(cfg["init"]))
    for x, y in zip(s.backwards_pass(cfg["init"]), t.backwards_pass(cfg["init"])):
        assert np.array_equal(x, y)
    a, b = s.solve_batch(cfg["init"]), t.solve_batch(cfg["init"])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    s.set_state_weight_schedule(Qs20[:8])   # n_knots = 8 < n
    for call in (lambda: s.cost_trajectory(cfg["init"]), lambda: s.solve_batch(cfg["init"]), lambda: s.backwards_pass(cfg["init"])):
        with pytest.raises(IndexError, match="state-weight schedule"):
            call()
    # ... while a call of 8 knots is accepted, and its cost is not the unscheduled handle's
    assert not np.array_equal(s.cost_trajectory(cfg["init"][:, :8]), capi.from_config(cfg).cost_trajectory(cfg["init"][:, :8]))
    gains = t.backwards_pass(cfg["init"])[0]
    assert s.forward_sim(cfg["init"], gains).shape == cfg["init"].shape  # (evaluates no cost: takes any length)
    # an initial trajectory shorter than the desired one: the absolute knot index, as for the desired trajectory
    long_cfg = sc.config(24, B=3)
    u = capi.from_config(long_cfg)
    u.set_state_weight_schedule(sc.schedule("dense", 24))
    short = long_cfg["init"][:, :n]
    out = u.solve_batch(short)
    o = sc.restatement(long_cfg, sc.schedule("dense", 24), 1)
    np.testing.assert_allclose(u.cost_trajectory(short)[1], o.cost_trajectory(o.unpack(short[1])), rtol=1e-10)
    assert_solve_matches(out, 1, o.solve(short[1]))


@pytest.mark.parametrize("B", [64, 300])
def test_a_schedule_of_the_handles_own_q_gives_its_bits(B):
    """a handle with a non-symmetric Q already takes the dense records and the general kernel: Qs[i] = Q changes where Q is read, and no bit"""
    N = 20
    cfg = pb.config2(B=B, N=N, seed=41)
    Q = cfg["Q"].copy()
    Q[1, 8] += 0.5
    Q[4, 2] -= 0.25
    cfg["Q"] = Q
    plain = capi.from_config(cfg)
    want = device_solve(plain, cfg["init"])
    s = capi.from_config(cfg)
    assert s.describe(B) == plain.describe(B)
    s.set_state_weight_schedule(np.broadcast_to(Q, (N, 12, 12)))
    text = s.describe(B)
    assert "state-weight schedule" in text and text.replace(text[text.index("; state-weight schedule"):text.index("; fp64")], "") == plain.describe(B)
    got, host = device_solve(s, cfg["init"]), s.solve_batch(cfg["init"])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (B, k)
        assert np.array_equal(host[k], want[k]), (B, "host", k)
    assert np.array_equal(s.cost_trajectory(cfg["init"]), plain.cost_trajectory(cfg["init"]))


def test_a_cleared_handle_is_one_that_never_had_a_schedule():
    B, N = 64, 20
    cfg = pb.config2(B=B, N=N, seed=42)
    never = capi.from_config(cfg)
    want = device_solve(never, cfg["init"])
    s = capi.from_config(cfg)
    before = s.describe(B)
    assert "k_round" in before
    s.set_state_weight_schedule(sc.schedule("terminal", N))
    assert "k_round" not in s.describe(B)
    changed = device_solve(s, cfg["init"])
    assert not np.array_equal(changed["traj"], want["traj"])
    s.clear_state_weight_schedule()
    assert s.describe(B) == before and "k_round" in s.describe(B)
    again, host = device_solve(s, cfg["init"]), s.solve_batch(cfg["init"])
    for k in KEYS:
        assert np.array_equal(again[k], want[k]), k
        assert np.array_equal(host[k], want[k]), ("host", k)
    s.clear_state_weight_schedule()  # (clearing twice is allowed)


def test_results_do_not_depend_on_batch_order_compaction_streams_or_shards():
    N = 20
    cfg = pb.config2(B=16, N=N, seed=43)
    init, Qs = cfg["init"], sc.schedule("terminal", N)

    def handle(**kw):
        s = capi.from_config(cfg, **capi.PIN_ARITHMETIC, **kw)
        s.set_state_weight_schedule(Qs)
        return s

    def same(out, copies, what):
        for k in KEYS:
            assert np.array_equal(out[k].reshape((copies, 16) + out[k].shape[1:]), np.broadcast_to(base[k], (copies,) + base[k].shape)), (what, k)

    base = handle().solve_batch(init)
    assert len(set(base["iters"].tolist())) > 1  # (the problems finish in different rounds)
    big = np.concatenate([init] * 17)
    same(handle().solve_batch(big), 17, "B = 272")
    perm = np.random.default_rng(3).permutation(16)
    out = handle().solve_batch(init[perm])
    for k in KEYS:
        assert np.array_equal(out[k], base[k][perm]), ("permuted", k)
    packed = handle(compaction=1)
    same(device_solve(packed, big), 17, "compaction = 1")
    assert packed.compaction_moves() > 0
    loose = handle(compaction=-1)
    same(device_solve(loose, big), 17, "compaction = -1")
    assert loose.compaction_moves() == 0
    same(handle(streams=2).solve_batch(big[:256]), 16, "streams = 2")
    same(device_solve(handle(streams=2), big[:256]), 16, "streams = 2, device-resident")
    sh = capi.sharded_from_config(cfg, devices=(0, 0), **capi.PIN_ARITHMETIC)
    sh.set_state_weight_schedule(Qs)
    out = sh.solve_batch(init)
    for k in KEYS:
        assert np.array_equal(out[k], base[k]), ("sharded", k)
    sh.clear_state_weight_schedule()
    free = capi.from_config(cfg, **capi.PIN_ARITHMETIC).solve_batch(init)
    out = sh.solve_batch(init)
    for k in KEYS:
        assert np.array_equal(out[k], free[k]), ("sharded, cleared", k)


def test_a_terminal_weight_brings_the_end_of_the_demo_closer_to_its_target():
    d = pb.box_climb_desired(4.0)  # config1's demo shortened to 40 knots
    assert len(d) == 40
    cfg = dict(model=pb.MODEL_D, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=pb.DT_DEMO, desired=d, init=d[None], options=dict(pb.OPTIONS_DEMO, populate_debug=False))
    s = capi.from_config(cfg)
    s.set_state_weight_schedule(pb.terminal_schedule(0.01 * pb.Q_DEMO, 0.01 * pb.Q_DEMO, 40))
    loose = s.solve_batch(d[None])
    s.set_state_weight_schedule(pb.terminal_schedule(0.01 * pb.Q_DEMO, 10.0 * pb.Q_DEMO, 40))
    tight = s.solve_batch(d[None])
    # (either convergence test: which of the two ends a solve is not what the comparison is about, an exhausted search or iteration count is)
    assert loose["status"][0] in (0, 1) and tight["status"][0] in (0, 1), (loose["status"], tight["status"])
    err = lambda out: np.linalg.norm(out["traj"][0, -1, 1:4] - d[-1, 1:4])  # noqa: E731
    print("final-knot position error: constant %.4g m, terminal %.4g m" % (err(loose), err(tight)))
    assert err(tight) < err(loose)


def test_describe_names_the_schedule_and_the_route():
    N = 12
    cfg = sc.config(N)
    s = capi.from_config(cfg)
    s.set_state_weight_schedule(sc.schedule("waypoint", N))
    for B in (1, 64, 1024, 4096, 8192, 65536):
        text = s.describe(B)
        assert "state-weight schedule (extension): n_knots = 12, every Q_i symmetric" in text, text
        assert "k_backward<true>, one wavefront per trajectory" in text and "round: three launches" in text, text
        assert "k_round" not in text and "k_backward4" not in text and "k_backward_rollout" not in text and "k_solve4" not in text, text
        assert "symmetric-weight forms" in text
    s.set_state_weight_schedule(sc.one_nonsymmetric(sc.schedule("waypoint", N)))
    text = s.describe(64)
    assert "not every Q_i symmetric" in text and "k_backward<false>" in text and "the reference's own forms" in text, text
    for kw in (dict(force_general=8), dict(force_general=5), dict(force_general=2), dict(single_wave_rollout=3), dict(streams=3), dict(round_launch=2)):
        t = capi.from_config(cfg, **kw)
        t.set_state_weight_schedule(sc.schedule("terminal", N))
        for B in (64, 1024, 8192):
            text = t.describe(B)
            assert "k_round" not in text and "k_backward4" not in text and "k_backward<true>" in text, (kw, B, text)
    g = capi.from_config(cfg, force_general=1)   # force_general = 1: the general kernel whatever the schedule
    g.set_state_weight_schedule(sc.schedule("terminal", N))
    assert "k_backward<false>" in g.describe(64) and "every Q_i symmetric" in g.describe(64)
    c = capi.from_config(cfg, compaction=1)
    c.set_state_weight_schedule(sc.schedule("terminal", N))
    assert "compaction of the running trajectories: on" in c.describe(1024)
    assert "compaction: off" in s.describe(8192)


def test_refusals():
    N = 12
    cfg = sc.config(N)
    Qs = sc.schedule("dense", N)
    s = capi.from_config(cfg)
    plain_text = s.describe(6)
    for bad in (np.nan, np.inf):
        q = Qs.copy()
        q[3, 11, 2] = bad
        q[7, 0, 0] = bad
        with pytest.raises(TypeError, match=r"non-finite entry \(knot 3, row 11, column 2\)"):
            s.set_state_weight_schedule(q)
    assert s.describe(6) == plain_text  # a refused schedule changes nothing
    with pytest.raises(TypeError, match="state-weight schedule"):
        s.set_state_weight_schedule(np.zeros((0, 12, 12)))
    lib = capi.load()
    import ctypes as C
    assert lib.qilqr_set_state_weight_schedule(s._h, Qs.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(0)) == capi.ERR_INVALID_ARG
    assert lib.qilqr_set_state_weight_schedule(s._h, Qs.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(-1)) == capi.ERR_INVALID_ARG
    assert lib.qilqr_set_state_weight_schedule(s._h, None, C.c_int32(2)) == capi.ERR_INVALID_ARG
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").set_state_weight_schedule(Qs)
    capi.from_config(cfg, precision="f32").clear_state_weight_schedule()  # (nothing to clear: allowed)
    lim = capi.from_config(cfg)
    lim.set_control_limits(0.5, 4.5)
    with pytest.raises(TypeError, match="control limits"):
        lim.set_state_weight_schedule(sc.one_nonsymmetric(Qs))
    lim.set_state_weight_schedule(Qs)
    other = capi.from_config(cfg)
    other.set_state_weight_schedule(sc.one_nonsymmetric(Qs))
    with pytest.raises(TypeError, match="control limits"):
        other.set_control_limits(0.5, 4.5)
    # limits on a handle whose own Q is not symmetric, under a symmetric schedule: the schedule stays until the limits are cleared
    tilted = dict(cfg, Q=cfg["Q"] + 0.5 * np.eye(12, k=3))
    own = capi.from_config(tilted)
    with pytest.raises(TypeError, match="control limits"):
        own.set_control_limits(0.5, 4.5)
    own.set_state_weight_schedule(Qs)
    own.set_control_limits(0.5, 4.5)
    with pytest.raises(TypeError, match="clear the limits"):
        own.clear_state_weight_schedule()
    assert "state-weight schedule" in own.describe(6) and "box form" in own.describe(6)
    own.clear_control_limits()
    own.clear_state_weight_schedule()
    assert own.describe(6) == capi.from_config(tilted).describe(6)
    sh = capi.sharded_from_config(cfg, devices=(0, 0))
    free = sh.solve_batch(cfg["init"])
    sh.set_state_weight_schedule(Qs)
    q = Qs.copy()
    q[5, 1, 1] = np.nan
    with pytest.raises(TypeError, match="knot 5, row 1, column 1"):
        sh.set_state_weight_schedule(q)
    out = sh.solve_batch(cfg["init"])  # a refused schedule leaves every shard cleared
    for k in KEYS:
        assert np.array_equal(out[k], free[k]), k
    from tests.diag_lib import capi_diag
    p = capi_diag().from_config(cfg, persistent=1)
    p.set_state_weight_schedule(Qs)
    with pytest.raises(TypeError, match="persistent"):
        p.solve_batch(cfg["init"])
