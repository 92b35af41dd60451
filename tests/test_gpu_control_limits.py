"""The per-rotor thrust limits on the device (qilqr_set_control_limits: the box form of k_backward<true> and k_rollout with the
controls clamped) against the NumPy restatement of the extension (tests/limited_numpy_ilqr.py): every pass, whole solves, batch-size
independence, the handle without limits, the reference's demo with physical thrusts, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import limited_numpy_ilqr as lim  # noqa: E402
from tests.independent_numpy_ilqr import Model, pose_from_knot  # noqa: E402
from tests.test_gpu_parity import random_cfg  # noqa: E402


def restatement(cfg, lo, hi, integrator=0):
    return lim.LimitedILQR(Model(**cfg["model"]), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), lo, hi,
                           integrator=integrator)


def split_gains(g):
    """[n][52] device gains -> k [n][4], K [n][4][12] (K column-major after k)"""
    return g[:, :4], np.transpose(g[:, 4:].reshape(-1, 12, 4), (0, 2, 1))


def percentile_limits(trajs):
    u = trajs[:, :, 14:18].reshape(-1, 4)
    return np.percentile(u, 20, axis=0), np.percentile(u, 80, axis=0)


@pytest.mark.parametrize("seed,dense,integrator", [(41, False, 0), (42, "sym", 0), (43, False, 1), (44, "sym", 1)])
def test_passes_match_the_restatement(seed, dense, integrator):
    cfg = random_cfg(seed, n=25, dense=dense, B=6)
    trajs = cfg["init"]
    lo, hi = percentile_limits(trajs)
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    s.set_control_limits(lo, hi)
    o = restatement(cfg, lo, hi, integrator)
    gains, terms = s.backwards_pass(trajs)
    r = np.random.default_rng(seed)
    clamped_any = 0
    for b in range(len(trajs)):
        pts = o.unpack(trajs[b])
        ks, Ks, t = o.backwards_pass(pts)
        assert not o.qp_failed
        k_dev, K_dev = split_gains(gains[b])
        scale = max(np.abs(np.array(ks)).max(), np.abs(np.array(Ks)).max())
        np.testing.assert_allclose(k_dev, np.array(ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(K_dev, np.array(Ks), rtol=1e-8, atol=1e-9 * scale)
        np.testing.assert_allclose(terms[b], t, rtol=1e-8, atol=1e-10 * max(1.0, np.abs(t).max()))
        assert np.all(K_dev[o.clamped] == 0.0)  # the clamped rotors' rows of K are exactly zero
        clamped_any += int(o.clamped.sum())
        # forward_sim with the device's gains at three step sizes: the clamped controls and the states they lead to
        for alpha in (1.0, 0.5, 0.5 ** int(r.integers(2, 5))):
            fwd = s.forward_sim(trajs[b:b + 1], gains[b:b + 1], alpha)[0]
            ref = o.forward_sim(pts, list(k_dev), list(K_dev), alpha)
            assert np.all(fwd[:, 14:18] >= lo) and np.all(fwd[:, 14:18] <= hi)
            for i, (T, v, u) in enumerate(ref):
                np.testing.assert_allclose(pose_from_knot(fwd[i]), T, rtol=0, atol=1e-9)
                np.testing.assert_allclose(fwd[i, 8:14], v, rtol=0, atol=1e-9)
                np.testing.assert_allclose(fwd[i, 14:18], u, rtol=0, atol=1e-9)
    assert clamped_any > 0  # some bounds were active


SOLVE_SEEDS = [0, 1, 2, 3]


def solve_cfg(seed):
    r = np.random.default_rng(7000 + seed)
    cfg = pb.config2(B=4, N=int(r.integers(15, 41)), seed=60 + seed)
    cfg["options"] = dict(cfg["options"], rtol=1e-10, atol=1e-10)
    if seed == 3:
        cfg["options"]["ls_max_iters"] = 1  # with Levenberg-Marquardt restarts below: every rejected full step restarts
    return cfg


@pytest.mark.parametrize("seed", SOLVE_SEEDS)
def test_solves_match_the_restatement(seed):
    cfg = solve_cfg(seed)
    lo, hi = 0.0, 6.0
    s = capi.from_config(cfg)
    s.set_control_limits(lo, hi)
    o = restatement(cfg, lo, hi)
    if seed == 3:
        s.set_regularisation(1.0, 4.0, 1e6)
        o.set_regularisation(1.0, 4.0, 1e6)
    out = s.solve_batch(cfg["init"])
    for b, t in enumerate(cfg["init"]):
        ref = o.solve(t)
        assert [out["status"][b], out["iters"][b], out["n_bwd"][b], out["n_fwd"][b]] == \
            [ref["status"], ref["iters"], ref["n_bwd"], ref["n_fwd"]], b
        np.testing.assert_allclose(out["cost"][b], ref["cost"], rtol=1e-9)
        for i in range(len(t)):
            np.testing.assert_allclose(pose_from_knot(out["traj"][b, i]), pose_from_knot(ref["traj"][i]), atol=1e-6)
        np.testing.assert_allclose(out["traj"][b, :, 8:18], ref["traj"][:, 8:18], atol=1e-6)
    u = out["traj"][:, :, 14:18]
    assert np.all(u >= lo) and np.all(u <= hi)
    assert np.any(u == lo) or np.any(u == hi)


def test_results_do_not_depend_on_the_batch():
    cfg = pb.config2(B=16, N=20, seed=71)
    lo, hi = 0.0, 6.0
    init = cfg["init"]

    def limited(**kw):
        s = capi.from_config(cfg, **kw)
        s.set_control_limits(lo, hi)
        return s

    s = limited()
    base = s.solve_batch(init)
    assert np.all(base["traj"][:, :, 14:18] >= lo) and np.all(base["traj"][:, :, 14:18] <= hi)
    for b in range(16):  # one at a time through qilqr_solve
        traj, info = s.solve(init[b])
        assert np.array_equal(traj, base["traj"][b]) and info["cost"] == base["cost"][b]
        assert info["status"] == base["status"][b] and info["iters"] == base["iters"][b]
    keys = ("traj", "cost", "status", "iters", "n_bwd", "n_fwd")
    for B in (1024, 4352):
        big = np.concatenate([init] * (B // 16))
        for compaction in (-1, 1):
            out = limited(compaction=compaction).solve_batch(big)
            for k in keys:
                assert np.array_equal(out[k].reshape((B // 16, 16) + out[k].shape[1:]), np.broadcast_to(base[k], (B // 16,) + base[k].shape)), (B, compaction, k)
    sh = capi.sharded_from_config(cfg, devices=(0, 0))
    sh.set_control_limits(lo, hi)
    out = sh.solve_batch(init)
    for k in keys:
        assert np.array_equal(out[k], base[k]), ("sharded", k)


def test_a_cleared_handle_is_today_s_and_infinite_limits_are_the_one_wavefront_route():
    cfg = pb.config2(B=1024, N=100)
    fresh = capi.from_config(cfg).solve_batch(cfg["init"])
    s = capi.from_config(cfg)
    s.set_control_limits(0.0, 6.0)
    assert "control limits" in s.describe(1024)
    s.solve_batch(cfg["init"][:64])
    s.clear_control_limits()
    assert "control limits" not in s.describe(1024)
    again = s.solve_batch(cfg["init"])
    for k in ("traj", "cost", "status", "iters", "n_bwd", "n_fwd"):
        assert np.array_equal(again[k], fresh[k]), k
    small = pb.config2(B=64, N=50, seed=5)
    box = capi.from_config(small)
    box.set_control_limits(-np.inf, np.inf)
    a = box.solve_batch(small["init"])
    b = capi.from_config(small, force_general=2, single_wave_rollout=1).solve_batch(small["init"])
    np.testing.assert_allclose(a["cost"], b["cost"], rtol=1e-9)
    np.testing.assert_allclose(a["traj"], b["traj"], atol=1e-6)


def test_the_demo_flies_with_physical_thrusts():
    d = pb.box_climb_desired(4.0)
    cfg = dict(model=pb.MODEL_D, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=pb.DT_DEMO, desired=d, init=d[None],
               options=dict(pb.OPTIONS_DEMO, populate_debug=False))
    free = capi.from_config(cfg).solve_batch(d[None])
    s = capi.from_config(cfg)
    s.set_control_limits(0.0, 9.81)
    out = s.solve_batch(d[None])
    assert out["status"][0] in (0, 1), out["status"]
    u = out["traj"][0, :, 14:18]
    assert u.min() >= 0.0 and u.max() <= 9.81
    assert free["traj"][0, :, 14:18].min() < 0.0  # the limits were active
    assert out["cost"][0] >= free["cost"][0]


def test_refusals():
    cfg = pb.config2(B=2, N=8)
    s = capi.from_config(cfg)
    with pytest.raises(TypeError, match="lo < hi"):
        s.set_control_limits([0, 0, 0, 1], [1, 1, 1, 1])
    with pytest.raises(TypeError, match="lo < hi"):
        s.set_control_limits([0, np.nan, 0, 0], 1.0)
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").set_control_limits(0.0, 6.0)
    with pytest.raises(TypeError, match="symmetric"):
        capi.from_config(random_cfg(45, n=8, dense=True, B=2)).set_control_limits(0.0, 6.0)
    with pytest.raises(TypeError, match="symmetric"):
        capi.from_config(cfg, force_general=1).set_control_limits(0.0, 6.0)
    with pytest.raises(TypeError, match="positive definite"):
        capi.from_config(dict(cfg, R=np.diag([1.0, 1.0, 1.0, 0.0]))).set_control_limits(0.0, 6.0)
    s.set_control_limits(-np.inf, np.inf)  # open sides are allowed
    from tests.diag_lib import capi_diag
    p = capi_diag().from_config(cfg, persistent=1)
    p.set_control_limits(0.0, 6.0)
    with pytest.raises(TypeError, match="persistent"):
        p.solve_batch(cfg["init"])
