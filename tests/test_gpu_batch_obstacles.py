"""Per-problem, moving spheres on the device (qilqr_set_batch_obstacles: k_linearize's cost half reads each problem's spheres by its row)
against the NumPy restatement (tests/moving_obstacle_numpy_ilqr.py): every pass with each backward form, whole solves, the bits of a shared
table and of a handle without obstacles, independence of the batch, the order, the compaction, the streams and the shards, the demo kept
clear of a moving sphere, the route, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import moving_obstacle_numpy_ilqr as mob  # noqa: E402
from tests.independent_numpy_ilqr import Model, pose_from_knot  # noqa: E402
from tests.test_gpu_obstacles import KEYS, PASS_CASES, PATH_SPHERES, device_solve, spheres_on, split_gains  # noqa: E402
from tests.test_gpu_parity import random_cfg  # noqa: E402


def moving_on(trajs, dt, r, K=3):
    """(B, K, 8) spheres per problem: each problem's first spheres contain one of its own knots at that knot's time (moving), the last
    moves far from everything"""
    B, n = trajs.shape[:2]
    out = np.zeros((B, K, 8))
    for b in range(B):
        for j in range(K - 1):
            i = int(r.integers(0, n))
            v = r.normal(size=3) * 0.8
            c = trajs[b, i, 1:4] + r.normal(size=3) * 0.15
            out[b, j] = [*(c - i * dt * v), *v, np.linalg.norm(c - trajs[b, i, 1:4]) + r.uniform(0.3, 0.8), r.uniform(5.0, 40.0)]
        out[b, K - 1] = [900.0 + b, -700.0, 5.0, 1.0, 0.5, 0.0, 1.5, 1e4]
    return out


def restatement(cfg, own, shared=None, model=None, limits=None, integrator=0):
    m = Model(**(model or cfg["model"]))
    if limits is None:
        o = mob.MovingObstacleILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), integrator=integrator)
    else:
        o = mob.MovingObstacleLimitedILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), *limits,
                                          integrator=integrator)
    if shared is not None:
        o.set_obstacles(shared)
    o.set_problem_obstacles(own)
    return o


def reached(trajs, table, counts, dt):
    """knots inside one of their own problem's spheres"""
    n = trajs.shape[1]
    hits = 0
    for b in range(len(trajs)):
        for i in range(n):
            s = mob.at_time(table[b, :counts[b]], i * dt)
            hits += int((np.linalg.norm(trajs[b, i, 1:4] - s[:, :3], axis=1) < s[:, 3]).sum())
    return hits


@pytest.mark.parametrize("case", range(len(PASS_CASES)))
def test_passes_match_the_restatement(case):
    dense, integrator, limits, models, kw, copies = PASS_CASES[case]
    cfg = random_cfg(150 + case, n=20, dense=dense, B=6)
    r = np.random.default_rng(1900 + case)
    trajs = cfg["init"]
    table = moving_on(trajs, cfg["dt"], r)
    counts = np.array([3, 2, 3, 1, 3, 0])
    assert reached(trajs, table, counts, cfg["dt"]) > 0
    shared = spheres_on(trajs, r, 2) if case % 2 else None  # both tables in every other case
    B = len(trajs) * copies
    big = np.concatenate([trajs] * copies)
    s = capi.from_config(cfg, **kw)
    s.set_integrator(integrator)
    if limits:
        s.set_control_limits(*limits)
    mods = [dict(cfg["model"], mass_kg=cfg["model"]["mass_kg"] * (0.8 + 0.1 * b)) for b in range(len(trajs))] if models else None
    if models:
        s.set_models(mods * copies)
    if shared is not None:
        s.set_obstacles(shared)
    s.set_batch_obstacles(np.concatenate([table] * copies), np.tile(counts, copies))
    cost = s.cost_trajectory(big)
    gains, terms = s.backwards_pass(big)
    for b in range(len(trajs)):
        o = restatement(cfg, table[b, :counts[b]], shared, mods[b] if models else None, limits, integrator)
        pts = o.unpack(trajs[b])
        np.testing.assert_allclose(cost[b], o.cost_trajectory(pts), rtol=1e-10)
        ks, Ks, t = o.backwards_pass(pts)
        k_dev, K_dev = split_gains(gains[b])
        scale = max(np.abs(np.array(ks)).max(), np.abs(np.array(Ks)).max())
        np.testing.assert_allclose(k_dev, np.array(ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(K_dev, np.array(Ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(terms[b], t, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(t).max()))
        if not models and b < 2:  # qilqr_forward_sim evaluates no cost: any B
            fwd = s.forward_sim(big[b:b + 1], gains[b:b + 1], 0.5)[0]
            ref = o.forward_sim(pts, list(k_dev), list(K_dev), 0.5)
            for i, (T, v, u) in enumerate(ref):
                np.testing.assert_allclose(pose_from_knot(fwd[i]), T, rtol=0, atol=1e-9)
    for c in range(1, copies):  # every copy of a problem: the same bits
        assert np.array_equal(cost[c * 6:(c + 1) * 6], cost[:6]) and np.array_equal(gains[c * 6:(c + 1) * 6], gains[:6])
    ls = s.line_search(big, cost, gains, terms)
    for b in range(len(trajs)):
        o = restatement(cfg, table[b, :counts[b]], shared, mods[b] if models else None, limits, integrator)
        pts = o.unpack(trajs[b])
        k_dev, K_dev = split_gains(gains[b])
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


def path_table(cfg, r, B):
    """moving spheres across each problem's initial path (timed to be at a knot when the trajectory is), distinct per problem"""
    return moving_on(cfg["init"][:B], cfg["dt"], r, K=3)


# (the thrust-limit case takes a seed whose restatement keeps its counts when the spheres move by 1e-13: seed 3's line search
# counts change with such a perturbation, so no two implementations need agree on them)
@pytest.mark.parametrize("seed,integrator,limits,shared", [(0, 0, None, False), (1, 0, None, True), (2, 1, None, False),
                                                           (4, 0, (0.0, 6.0), False)])
def test_solves_match_the_restatement(seed, integrator, limits, shared):
    r = np.random.default_rng(18000 + seed)
    cfg = pb.config2(B=8, N=int(r.integers(15, 41)), seed=180 + seed)
    cfg["options"] = dict(cfg["options"], rtol=1e-10, atol=1e-10)
    table = path_table(cfg, r, 8)
    counts = np.array([3, 2, 3, 1, 3, 2, 0, 3])
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    if limits:
        s.set_control_limits(*limits)
        s.set_regularisation(1.0, 4.0, 1e6)
    if shared:
        s.set_obstacles(PATH_SPHERES)
    s.set_batch_obstacles(table, counts)
    out = s.solve_batch(cfg["init"])
    assert reached(cfg["init"], table, counts, cfg["dt"]) > 0
    for b, t in enumerate(cfg["init"]):
        o = restatement(cfg, table[b, :counts[b]], PATH_SPHERES if shared else None, limits=limits, integrator=integrator)
        if limits:
            o.set_regularisation(1.0, 4.0, 1e6)
        ref = o.solve(t)
        assert [out["status"][b], out["iters"][b], out["n_bwd"][b], out["n_fwd"][b]] == \
            [ref["status"], ref["iters"], ref["n_bwd"], ref["n_fwd"]], b
        np.testing.assert_allclose(out["cost"][b], ref["cost"], rtol=1e-9)
        for i in range(len(t)):
            np.testing.assert_allclose(pose_from_knot(out["traj"][b, i]), pose_from_knot(ref["traj"][i]), atol=1e-6)
        np.testing.assert_allclose(out["traj"][b, :, 8:18], ref["traj"][:, 8:18], atol=1e-6)


def equal(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("B", [64, 1024, 5000])
def test_static_rows_give_the_bits_of_the_shared_table(B):
    cfg = pb.config2(B=B, N=60, seed=31)
    shared = capi.from_config(cfg)
    shared.set_obstacles(PATH_SPHERES)
    ref = device_solve(shared, cfg["init"])
    s = capi.from_config(cfg)
    s.set_batch_obstacles(np.broadcast_to(PATH_SPHERES, (B,) + PATH_SPHERES.shape))  # (B, K, 5): v = 0
    assert "batch obstacles (extension)" in s.describe(B) and "none moving" in s.describe(B)
    equal(device_solve(s, cfg["init"]), ref, (B, "device"))
    equal(s.solve_batch(cfg["init"]), ref, (B, "host"))


def test_unreached_rows_give_the_bits_of_a_handle_without_them_and_a_cleared_handle_the_default_route():
    B = 1024
    cfg = pb.config2(B=B, N=60, seed=31)
    plain = device_solve(capi.from_config(cfg), cfg["init"])
    s = capi.from_config(cfg)
    far = np.zeros((B, 2, 8))
    far[:, 0] = [1000.0, 0.0, 0.0, 0.0, 2.0, 0.0, 1.0, 50.0]
    far[:, 1] = [0.0, -800.0, 5.0, 1.0, 0.0, 0.0, 2.5, 1e4]
    s.set_batch_obstacles(far, np.arange(B) % 3)
    equal(device_solve(s, cfg["init"]), plain, "unreached")
    equal(s.solve_batch(cfg["init"]), plain, "unreached, host")
    s.set_batch_obstacles(path_table(cfg, np.random.default_rng(5), 64))
    device_solve(s, cfg["init"][:64])
    s.clear_batch_obstacles()
    assert "batch obstacles" not in s.describe(B) and "k_round" in s.describe(B)
    equal(device_solve(s, cfg["init"]), plain, "cleared")


def test_results_do_not_depend_on_the_batch_the_order_the_compaction_the_streams_or_the_shards():
    cfg = pb.config2(B=16, N=30, seed=33)
    init = cfg["init"]
    table = path_table(cfg, np.random.default_rng(34), 16)
    counts = np.array([3, 2, 1, 0] * 4)

    def handle(rows, cnt, **kw):
        s = capi.from_config(cfg, **capi.PIN_ARITHMETIC, **kw)
        s.set_batch_obstacles(rows, cnt)
        return s

    def tiled(B):
        return np.concatenate([init] * (B // 16)), np.concatenate([table] * (B // 16)), np.tile(counts, B // 16)

    def same_as_base(out, B, what):
        for k in KEYS:
            assert np.array_equal(out[k].reshape((B // 16, 16) + out[k].shape[1:]), np.broadcast_to(base[k], (B // 16,) + base[k].shape)), \
                (what, B, k)

    base = handle(table, counts).solve_batch(init)
    assert reached(base["traj"], table, counts, cfg["dt"]) > 0
    for B in (1024, 5008):
        big, rows, cnt = tiled(B)
        same_as_base(handle(rows, cnt).solve_batch(big), B, "batch")
        same_as_base(device_solve(handle(rows, cnt), big), B, "batch, device")
    perm = np.random.default_rng(35).permutation(16)
    out = handle(table[perm], counts[perm]).solve_batch(init[perm])
    for k in KEYS:
        assert np.array_equal(out[k], base[k][perm]), ("permutation", k)
    big, rows, cnt = tiled(5008)
    big, rows, cnt = big[:5000], rows[:5000], cnt[:5000]
    on = handle(rows, cnt, compaction=1)
    moved = device_solve(on, big)
    assert on.compaction_moves() > 0
    equal(moved, device_solve(handle(rows, cnt, compaction=-1), big), "compaction")
    same_as_base({k: v[:4992] for k, v in moved.items()}, 4992, "compaction")
    big, rows, cnt = tiled(8192)
    one = device_solve(handle(rows, cnt, streams=1), big)
    same_as_base(one, 8192, "one stream")
    equal(device_solve(handle(rows, cnt, streams=4), big), one, "four streams")
    sh = capi.sharded_from_config(cfg, devices=(0, 0), **capi.PIN_ARITHMETIC)
    sh.set_batch_obstacles(table, counts)
    equal(sh.solve_batch(init), base, "sharded")
    sh.clear_batch_obstacles()
    equal(sh.solve_batch(init), capi.from_config(cfg, **capi.PIN_ARITHMETIC).solve_batch(init), "sharded, cleared")


def test_the_demo_keeps_clear_of_a_sphere_that_moves_across_its_path():
    d = pb.box_climb_desired(4.0)
    cfg = dict(model=pb.MODEL_D, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=pb.DT_DEMO, desired=d, init=d[None],
               options=dict(pb.OPTIONS_DEMO, populate_debug=False))
    free = capi.from_config(cfg).solve_batch(d[None])
    i0, radius = 6, 0.8
    p0 = free["traj"][0, i0, 1:4] + [0.0, -0.06, -0.05]
    v = np.array([0.0, 1.5, 0.5])  # across the path: at p0 when the free solution is at knot i0
    c0 = p0 - i0 * pb.DT_DEMO * v
    sphere = np.array([[[*c0, *v, radius, 1e6]]])
    s = capi.from_config(cfg)
    s.set_batch_obstacles(sphere)
    out = s.solve_batch(d[None])
    assert out["status"][0] in (0, 1), out["status"]
    n = d.shape[0]
    centre = c0 + np.arange(n)[:, None] * pb.DT_DEMO * v

    def dist(t):
        return np.linalg.norm(t[0, :, 1:4] - centre, axis=1)

    assert dist(out["traj"]).min() > radius - 1e-3, dist(out["traj"]).min()
    assert dist(free["traj"]).min() < radius  # without the sphere the solution passes through it
    frozen = capi.from_config(cfg)
    frozen.set_batch_obstacles(np.array([[[*c0, 0.0, 0.0, 0.0, radius, 1e6]]]))
    assert not np.array_equal(frozen.solve_batch(d[None])["traj"], out["traj"])


def test_the_route_and_the_refusals():
    cfg = pb.config2(B=16, N=20)
    table = path_table(cfg, np.random.default_rng(7), 16)
    for B in (1, 16, 64, 1024, 2048, 4096, 8192, 65536):
        s = capi.from_config(cfg)
        s.set_batch_obstacles(np.concatenate([table] * (B // 16 + 1))[:B], np.arange(B) % 3)
        text = s.describe(B)
        assert f"batch obstacles (extension): per-problem spheres for B = {B} problems, K = 3, at most {min(B - 1, 2)} used" in text, text
        assert ("some moving" if B > 1 else "none moving") in text
        assert "k_round" not in text and "k_solve4" not in text, (B, text)
    for kw in (dict(force_general=8), dict(force_general=5), dict(compaction=1), dict(single_wave_rollout=3), dict(streams=3)):
        t = capi.from_config(cfg, **kw)
        t.set_batch_obstacles(np.concatenate([table] * 64))
        assert "k_round" not in t.describe(1024), kw
    s = capi.from_config(cfg)
    s.set_batch_obstacles(table)
    init = cfg["init"]
    gains, terms = s.backwards_pass(init)
    cost = s.cost_trajectory(init)
    for call in (lambda: s.cost_trajectory(init[:8]), lambda: s.backwards_pass(init[:8]),
                 lambda: s.line_search(init[:8], cost[:8], gains[:8], terms[:8]), lambda: s.solve_batch(init[:8]),
                 lambda: s.solve(init[0])):
        with pytest.raises(TypeError, match="batch obstacles were set for B = 16"):
            call()
    with pytest.raises(AssertionError, match="batch obstacles were set for B = 16"):  # (device_solve asserts rc == 0 with the error)
        device_solve(s, init[:8])
    s.forward_sim(init[:3], gains[:3], 1.0)  # evaluates no cost: any B
    one = capi.from_config(cfg)
    one.set_batch_obstacles(table[:1])
    one.solve(init[0])  # qilqr_solve counts as B = 1
    for args, what in (((np.ones((16, 65, 8)),), "K must be"), ((table, [4] * 16), "count"), ((table, [-1] + [0] * 15), "count")):
        with pytest.raises(TypeError, match=what):
            s.set_batch_obstacles(*args)
    for (b, j, w, v), what in (((3, 1, 2, np.nan), "non-finite"), ((5, 0, 4, np.inf), "non-finite"), ((7, 2, 6, 0.0), "radius"),
                               ((9, 1, 7, -1.0), "weight")):
        bad = table.copy()
        bad[b, j, w] = v
        with pytest.raises(TypeError, match=rf"{what}.*\(problem {b}, sphere {j}\)"):
            s.set_batch_obstacles(bad)
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").set_batch_obstacles(table)
    sh = capi.sharded_from_config(cfg, devices=(0, 0))
    sh.set_batch_obstacles(table)
    bad = table.copy()
    bad[12, 0, 6] = -1.0
    with pytest.raises(TypeError, match=r"radius.*\(problem 12, sphere 0\)"):
        sh.set_batch_obstacles(bad)
    sh.solve_batch(init[:8])  # the failure left every shard cleared: any B
    sh.set_batch_obstacles(table)
    with pytest.raises(TypeError, match="batch obstacles were set for B = 16"):
        sh.solve_batch(init[:8])
    from tests.diag_lib import capi_diag
    p = capi_diag().from_config(cfg, persistent=1)
    p.set_batch_obstacles(table)
    with pytest.raises(TypeError, match="persistent"):
        p.solve_batch(init)
