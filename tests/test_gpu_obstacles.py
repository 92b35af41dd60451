"""Spherical obstacles on the device (qilqr_set_obstacles: k_linearize adds the penalties of obstacles.h to the cost half of every
knot record) against the NumPy restatement (tests/obstacle_numpy_ilqr.py): every pass with each backward form, whole solves, bits
equal to a handle without obstacles when no knot reaches them, batch-size and sharding independence, the demo kept clear of a
sphere, the route, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import obstacle_numpy_ilqr as obs  # noqa: E402
from tests.independent_numpy_ilqr import Model, pose_from_knot  # noqa: E402
from tests.test_gpu_parity import random_cfg  # noqa: E402

KEYS = ("traj", "cost", "status", "iters", "n_bwd", "n_fwd")
FAR = np.array([[1000.0, 0.0, 0.0, 1.0, 50.0], [0.0, -800.0, 5.0, 2.5, 1e4]])  # no trajectory here comes near


def split_gains(g):
    """[n][52] device gains -> k [n][4], K [n][4][12] (K column-major after k)"""
    return g[:, :4], np.transpose(g[:, 4:].reshape(-1, 12, 4), (0, 2, 1))


def spheres_on(trajs, r, count=4):
    """spheres around knots of the first problems (each containing its knot, off-center), and one far away"""
    out = []
    for j in range(count):
        b, i = j % len(trajs), int(r.integers(0, trajs.shape[1]))
        c = trajs[b, i, 1:4] + r.normal(size=3) * 0.15
        out.append([*c, np.linalg.norm(c - trajs[b, i, 1:4]) + r.uniform(0.3, 0.8), r.uniform(5.0, 40.0)])
    return np.vstack([out, FAR[:1]])


def restatement(cfg, spheres, model=None, limits=None, integrator=0):
    m = Model(**(model or cfg["model"]))
    if limits is None:
        o = obs.ObstacleILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), integrator=integrator)
    else:
        o = obs.ObstacleLimitedILQR(m, cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), *limits, integrator=integrator)
    o.set_obstacles(spheres)
    return o


def active_knots(trajs, spheres):
    p = trajs[:, :, None, 1:4] - spheres[None, None, :, :3]
    return int((np.linalg.norm(p, axis=-1) < spheres[None, None, :, 3]).sum())


# (dense weights, integrator, thrust limits, per-problem models, handle options, batch copies)
PASS_CASES = [
    (False, 0, None, False, {}, 1),                          # diagonal Q: the fused k_backward4, tiled records of kind 3
    ("sym", 0, None, False, {}, 1),                          # dense symmetric: kind 1
    (True, 0, None, False, {}, 1),                           # non-symmetric: the reference's forms, dense kind 0
    (False, 1, None, False, {}, 1),                          # Runge-Kutta
    ("sym", 1, (0.5, 4.5), False, {}, 1),                    # Runge-Kutta with limits
    (False, 0, (0.5, 4.5), False, {}, 1),                    # limits
    (False, 0, None, True, {}, 1),                           # per-problem models
    (False, 1, (0.5, 4.5), True, {}, 1),                     # models, limits, Runge-Kutta
    (False, 0, None, False, dict(force_general=2), 1),       # the one-wavefront symmetric kernel
    ("sym", 0, None, False, dict(force_general=1), 1),       # the general kernel on symmetric weights
    (False, 0, None, False, {}, 700),                        # B = 4200: the six-wavefront k_backward4
]


@pytest.mark.parametrize("case", range(len(PASS_CASES)))
def test_passes_match_the_restatement(case):
    dense, integrator, limits, models, kw, copies = PASS_CASES[case]
    cfg = random_cfg(50 + case, n=20, dense=dense, B=6)
    r = np.random.default_rng(900 + case)
    trajs = cfg["init"]
    spheres = spheres_on(trajs, r)
    assert active_knots(trajs, spheres) > 0
    B = len(trajs) * copies
    big = np.concatenate([trajs] * copies)
    s = capi.from_config(cfg, **kw)
    s.set_integrator(integrator)
    if limits:
        s.set_control_limits(*limits)
    mods = [dict(cfg["model"], mass_kg=cfg["model"]["mass_kg"] * (0.8 + 0.1 * b)) for b in range(len(trajs))] if models else None
    if models:
        s.set_models(mods * copies)
    s.set_obstacles(spheres)
    cost = s.cost_trajectory(big)
    gains, terms = s.backwards_pass(big)
    for b in range(len(trajs)):
        o = restatement(cfg, spheres, mods[b] if models else None, limits, integrator)
        pts = o.unpack(trajs[b])
        np.testing.assert_allclose(cost[b], o.cost_trajectory(pts), rtol=1e-10)
        ks, Ks, t = o.backwards_pass(pts)
        k_dev, K_dev = split_gains(gains[b])
        scale = max(np.abs(np.array(ks)).max(), np.abs(np.array(Ks)).max())
        np.testing.assert_allclose(k_dev, np.array(ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(K_dev, np.array(Ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(terms[b], t, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(t).max()))
        for alpha in ((1.0, 0.25) if not models else ()):  # (a handle with models takes calls of their B only)
            fwd = s.forward_sim(big[b:b + 1], gains[b:b + 1], alpha)[0]
            ref = o.forward_sim(pts, list(k_dev), list(K_dev), alpha)
            for i, (T, v, u) in enumerate(ref):
                np.testing.assert_allclose(pose_from_knot(fwd[i]), T, rtol=0, atol=1e-9)
                np.testing.assert_allclose(fwd[i, 8:18], np.concatenate([v, u]), rtol=0, atol=1e-9)
    for c in range(1, copies):  # every copy of a problem: the same bits
        assert np.array_equal(cost[c * 6:(c + 1) * 6], cost[:6]) and np.array_equal(gains[c * 6:(c + 1) * 6], gains[:6])
    # the line search: the step and the cost of the accepted candidate against the restatement's search with the device's gains
    ls = s.line_search(big, cost, gains, terms)
    for b in range(len(trajs)):
        o = restatement(cfg, spheres, mods[b] if models else None, limits, integrator)
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


def solve_cfg(seed):
    r = np.random.default_rng(8000 + seed)
    cfg = pb.config2(B=4, N=int(r.integers(15, 41)), seed=80 + seed)
    cfg["options"] = dict(cfg["options"], rtol=1e-10, atol=1e-10)
    return cfg


# spheres on the desired path (config2 hovers at the origin: every knot's target is inside the first sphere) and one beside it
PATH_SPHERES = np.array([[0.25, 0.0, 0.1, 0.6, 20.0], [-0.4, 0.5, 0.0, 0.5, 5.0], *FAR])


@pytest.mark.parametrize("seed,integrator,limits", [(0, 0, None), (1, 0, None), (2, 1, None), (3, 0, (0.0, 6.0))])
def test_solves_match_the_restatement(seed, integrator, limits):
    cfg = solve_cfg(seed)
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    if limits:
        s.set_control_limits(*limits)
        s.set_regularisation(1.0, 4.0, 1e6)
    s.set_obstacles(PATH_SPHERES)
    o = restatement(cfg, PATH_SPHERES, limits=limits, integrator=integrator)
    if limits:
        o.set_regularisation(1.0, 4.0, 1e6)
    out = s.solve_batch(cfg["init"])
    assert active_knots(out["traj"], PATH_SPHERES) > 0  # the solutions press against the spheres
    for b, t in enumerate(cfg["init"]):
        ref = o.solve(t)
        assert [out["status"][b], out["iters"][b], out["n_bwd"][b], out["n_fwd"][b]] == \
            [ref["status"], ref["iters"], ref["n_bwd"], ref["n_fwd"]], b
        np.testing.assert_allclose(out["cost"][b], ref["cost"], rtol=1e-9)
        for i in range(len(t)):
            np.testing.assert_allclose(pose_from_knot(out["traj"][b, i]), pose_from_knot(ref["traj"][i]), atol=1e-6)
        np.testing.assert_allclose(out["traj"][b, :, 8:18], ref["traj"][:, 8:18], atol=1e-6)


def device_solve(s, init):
    """qilqr_solve_batch_device on buffers from the HIP runtime this process already runs on (no torch: test_gpu_sharded._Hip), results
    back as a dict of NumPy arrays"""
    import ctypes as C
    from tests.test_gpu_sharded import _Hip
    hip = _Hip()
    try:
        init = np.ascontiguousarray(init, dtype=np.float64)
        B, n = init.shape[0], init.shape[1]
        d_init = hip.alloc(init.nbytes)
        assert hip.lib.hipMemcpy(C.c_void_p(d_init), init.ctypes.data_as(C.c_void_p), C.c_size_t(init.nbytes), C.c_int(1)) == 0
        shapes = dict(traj=(init.shape, np.float64), cost=((B,), np.float64), **{k: ((B,), np.int32) for k in KEYS[2:]})
        ptrs = {k: hip.alloc(int(np.prod(sh)) * np.dtype(dt).itemsize) for k, (sh, dt) in shapes.items()}
        rc = capi.load().qilqr_solve_batch_device(s._h, C.c_void_p(d_init), None, C.c_int32(B), C.c_int32(n),
                                                   *[C.c_void_p(ptrs[k]) for k in KEYS])
        assert rc == 0, capi.load().qilqr_last_error()
        assert hip.lib.hipDeviceSynchronize() == 0
        return {k: hip.download(ptrs[k], *shapes[k]) for k in KEYS}
    finally:
        hip.close()


@pytest.mark.parametrize("B", [64, 1024, 5000])
def test_unreached_obstacles_give_the_bits_of_a_handle_without_them(B):
    cfg = pb.config2(B=B, N=60, seed=31)
    plain = device_solve(capi.from_config(cfg), cfg["init"])
    s = capi.from_config(cfg)
    s.set_obstacles(FAR)
    assert "obstacles" in s.describe(B)
    far = device_solve(s, cfg["init"])
    host = s.solve_batch(cfg["init"])
    for k in KEYS:
        assert np.array_equal(far[k], plain[k]), (B, k)
        assert np.array_equal(host[k], plain[k]), (B, "host", k)
    if B == 1024:  # a cleared handle: the default route again, the same bits
        s.set_obstacles(PATH_SPHERES)
        device_solve(s, cfg["init"][:64])
        s.clear_obstacles()
        assert "obstacles" not in s.describe(B)
        again = device_solve(s, cfg["init"])
        for k in KEYS:
            assert np.array_equal(again[k], plain[k]), ("cleared", k)


def test_results_do_not_depend_on_the_batch_or_the_shards():
    cfg = pb.config2(B=16, N=30, seed=33)
    init = cfg["init"]

    def handle(**kw):
        s = capi.from_config(cfg, **capi.PIN_ARITHMETIC, **kw)
        s.set_obstacles(PATH_SPHERES)
        return s

    base = handle().solve_batch(init)
    assert active_knots(base["traj"], PATH_SPHERES) > 0
    for B in (1024, 5008):
        big = np.concatenate([init] * (B // 16))
        for out in (handle().solve_batch(big), device_solve(handle(), big)):
            for k in KEYS:
                assert np.array_equal(out[k].reshape((B // 16, 16) + out[k].shape[1:]), np.broadcast_to(base[k], (B // 16,) + base[k].shape)), (B, k)
    sh = capi.sharded_from_config(cfg, devices=(0, 0), **capi.PIN_ARITHMETIC)
    sh.set_obstacles(PATH_SPHERES)
    out = sh.solve_batch(init)
    for k in KEYS:
        assert np.array_equal(out[k], base[k]), ("sharded", k)
    sh.clear_obstacles()
    free = capi.from_config(cfg, **capi.PIN_ARITHMETIC).solve_batch(init)
    out = sh.solve_batch(init)
    for k in KEYS:
        assert np.array_equal(out[k], free[k]), ("sharded, cleared", k)


def test_the_demo_keeps_clear_of_a_sphere_on_its_path():
    d = pb.box_climb_desired(4.0)
    cfg = dict(model=pb.MODEL_D, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=pb.DT_DEMO, desired=d, init=d[None],
               options=dict(pb.OPTIONS_DEMO, populate_debug=False))
    free = capi.from_config(cfg).solve_batch(d[None])
    # a sphere around the free solution's seventh knot (which cuts the desired path's first corner), slightly off its center
    sphere = np.array([[*(free["traj"][0, 6, 1:4] + [0.0, -0.06, -0.05]), 0.8, 1e6]])
    s = capi.from_config(cfg)
    s.set_obstacles(sphere)
    out = s.solve_batch(d[None])
    assert out["status"][0] in (0, 1), out["status"]
    dist = lambda t: np.linalg.norm(t[0, :, 1:4] - sphere[0, :3], axis=1)  # noqa: E731
    assert dist(out["traj"]).min() > 0.8 - 1e-3, dist(out["traj"]).min()
    assert dist(free["traj"]).min() < 0.8  # without the sphere the solution passes through it
    assert out["cost"][0] > free["cost"][0]


def test_the_route_takes_no_kernel_that_linearises_inside_itself():
    cfg = pb.config2(B=16, N=20)
    s = capi.from_config(cfg)
    plain = capi.from_config(cfg)
    assert "k_round" in plain.describe(1024)  # (what the default route takes at this size)
    s.set_obstacles(FAR)
    for B in (1, 16, 64, 1024, 2048, 4096, 8192, 65536):
        text = s.describe(B)
        assert "obstacles (extension): 2 sphere(s)" in text
        assert "k_round" not in text and "k_solve4" not in text, (B, text)
    for kw in (dict(force_general=8), dict(force_general=5), dict(compaction=1), dict(single_wave_rollout=3), dict(streams=3)):
        t = capi.from_config(cfg, **kw)
        t.set_obstacles(FAR)
        for B in (64, 1024, 8192):
            assert "k_round" not in t.describe(B), (kw, B)


def test_refusals():
    cfg = pb.config2(B=2, N=8)
    s = capi.from_config(cfg)
    with pytest.raises(TypeError, match="obstacles"):
        s.set_obstacles(np.tile([0.0, 0.0, 0.0, 1.0, 1.0], (65, 1)))
    for bad, what in (([0.0, np.nan, 0.0, 1.0, 1.0], "non-finite"), ([0.0, 0.0, np.inf, 1.0, 1.0], "non-finite"),
                      ([0.0, 0.0, 0.0, 0.0, 1.0], "radius"), ([0.0, 0.0, 0.0, -1.0, 1.0], "radius"),
                      ([0.0, 0.0, 0.0, 1.0, -1e-9], "weight")):
        with pytest.raises(TypeError, match=what):
            s.set_obstacles([[1.0, 1.0, 1.0, 0.5, 1.0], bad])
    assert "obstacles" not in s.describe(2)  # a refused table changes nothing
    s.set_obstacles(np.tile([0.0, 0.0, 0.0, 1.0, 0.0], (64, 1)))  # 64 spheres, weight 0: allowed
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").set_obstacles(FAR)
    sh = capi.sharded_from_config(cfg, devices=(0, 0))
    with pytest.raises(TypeError, match="radius"):
        sh.set_obstacles([[0.0, 0.0, 0.0, 0.0, 1.0]])
    from tests.diag_lib import capi_diag
    p = capi_diag().from_config(cfg, persistent=1)
    p.set_obstacles(FAR)
    with pytest.raises(TypeError, match="persistent"):
        p.solve_batch(cfg["init"])
