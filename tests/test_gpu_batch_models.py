"""Per-problem models on the device (qilqr_set_batch_models: k_linearize, k_backward_models and k_rollout reading each problem's record)
against the oracle built with each problem's own model, against the product itself (a fresh handle per model on the same general
kernels), across batch sizes, orderings, compaction settings and shards; the physics (hover thrust m g / 4 per problem); a handle
without models or with them cleared; thrust limits; and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import limited_numpy_ilqr as lim  # noqa: E402
from tests.independent_numpy_ilqr import Model, pose_from_knot  # noqa: E402

KEYS = ("traj", "cost", "status", "iters", "n_bwd", "n_fwd")


def random_models(count, seed):
    """as tests/test_gpu_parity.py::randomised_cfg draws a model: mass 0.5..3 kg, random SPD inertia, arm, torque ratio, g"""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        A = r.uniform(-0.3, 0.3, (3, 3))
        out.append(dict(mass_kg=r.uniform(0.5, 3.0), inertia=A @ A.T + np.diag(r.uniform(0.5, 2.0, 3)),
                        arm_length_m=r.uniform(0.2, 1.2), torque_to_thrust_ratio_m=r.uniform(0.05, 0.5), g_mpss=r.uniform(3.0, 12.0)))
    return out


def models_cfg(seed, B=48, n=40, weights="diag", max_iters=30, ls_max_iters=20):
    """B problems, each with its own model, towards one hover pose; the handle's own model is configs[1]'s (never any problem's)"""
    r = np.random.default_rng(5000 + seed)
    dt = float(r.uniform(0.04, 0.1))
    Q = np.diag(np.concatenate([r.uniform(10, 200, 6), r.uniform(0.5, 5, 6)]))
    R = np.diag(r.uniform(0.5, 3.0, 4))
    if weights == "sym":
        G = r.uniform(-1, 1, (12, 12))
        Q = Q + 0.3 * (G @ G.T)
        G = r.uniform(-0.3, 0.3, (4, 4))
        R = R + G @ G.T
    elif weights == "nonsym":
        Q = Q + 0.3 * r.uniform(-1, 1, (12, 12))
        R = R + 0.1 * r.uniform(-1, 1, (4, 4))
    models = random_models(B, 900 + seed)
    desired = pb.hover_desired(n, dt, np.mean([pb.hover_thrust(m) for m in models]))
    desired[:, 1:8] = orc.se3_exp(np.concatenate([r.uniform(-1, 1, 3), r.uniform(-0.3, 0.3, 3)]))
    init = pb.random_start_batch(np.arange(B), desired, 77 + seed, pos_m=0.8, ang_rad=0.6, vel_sigma=0.4)
    opts = dict(step_update=0.5, desired_reduction_frac=0.1, ls_max_iters=ls_max_iters, rtol=1e-10, atol=1e-10, max_iters=max_iters,
                populate_debug=False)
    return dict(model=pb.MODEL_A, Q=Q, R=R, dt=dt, desired=desired, init=init, options=opts), models


def oracle_of(cfg, model, integrator=0, reg=None):
    o = orc.OracleSolver(orc.model_params(**model), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], orc.options(**cfg["options"]))
    o.set_integrator(integrator)
    if reg:
        o.set_regularisation(*reg)
    return o


def solver(cfg, models=None, integrator=0, reg=None, limits=None, **kw):
    s = capi.from_config(cfg, **kw)
    s.set_integrator(integrator)
    if reg:
        s.set_regularisation(*reg)
    if limits:
        s.set_control_limits(*limits)
    if models is not None:
        s.set_models(models)
    return s


def assert_same(a, b, label=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (label, k)


CASES = [  # seed, n, integrator, weights, restarts
    (1, 40, 0, "diag", None),
    (2, 100, 0, "sym", None),
    (3, 40, 1, "diag", None),
    (4, 100, 1, "sym", None),
    (5, 12, 0, "nonsym", None),
    (6, 40, 0, "diag", (1.0, 4.0, 1e6)),
]


@pytest.mark.parametrize("seed,n,integrator,weights,reg", CASES)
def test_solves_match_the_oracle_with_each_problem_s_model(seed, n, integrator, weights, reg):
    cfg, models = models_cfg(seed, n=n, weights=weights, ls_max_iters=2 if reg else 20)
    out = solver(cfg, models, integrator, reg).solve_batch(cfg["init"])
    for b, m in enumerate(models):
        ref = oracle_of(cfg, m, integrator, reg).solve_batch(cfg["init"][b:b + 1])
        assert [int(out[k][b]) for k in KEYS[2:]] == [int(ref[k][0]) for k in KEYS[2:]], b
        np.testing.assert_allclose(out["cost"][b], ref["cost"][0], rtol=1e-9)
        np.testing.assert_allclose(out["traj"][b], ref["traj"][0], atol=1e-6)
    assert len(set(out["cost"].tolist())) > len(models) // 2


@pytest.mark.parametrize("integrator", [0, 1])
def test_passes_match_the_oracle_problem_by_problem(integrator):
    """backwards_pass, forward_sim and cost_trajectory on the random starts, then line_search from the rolled-out trajectory (a
    dynamically consistent one, where the searches accept), problem by problem against the oracle with that problem's model"""
    cfg, models = models_cfg(11 + integrator, B=16, n=30)
    s = solver(cfg, models, integrator)
    trajs = cfg["init"]
    gains, terms = s.backwards_pass(trajs)
    fwd = s.forward_sim(trajs, gains, 0.5)
    cost = s.cost_trajectory(trajs)
    gains2, terms2 = s.backwards_pass(fwd)
    cost2 = s.cost_trajectory(fwd)
    ls = s.line_search(fwd, cost2, gains2, terms2)
    accepted = 0
    for b, m in enumerate(models):
        o = oracle_of(cfg, m, integrator)
        for tr, g, t in ((trajs[b], gains[b], terms[b]), (fwd[b], gains2[b], terms2[b])):
            g_ref, t_ref = o.backwards_pass(tr)
            np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-10 * np.abs(g_ref).max())
            np.testing.assert_allclose(t, t_ref, rtol=1e-9, atol=1e-10 * np.abs(t_ref).max())
        np.testing.assert_allclose(fwd[b], o.forward_sim(trajs[b], gains[b], 0.5), atol=1e-9)
        np.testing.assert_allclose(cost[b], o.cost_trajectory(trajs[b]), rtol=1e-12)
        r = o.line_search(fwd[b], cost2[b], gains2[b], terms2[b])
        assert ls["status"][b] == r["status"], b
        if r["status"] == 0:  # (an exhausted search reports no step of its own)
            assert ls["step"][b] == r["step"], b
            np.testing.assert_allclose(ls["cost"][b], r["cost"], rtol=1e-10)
            np.testing.assert_allclose(ls["traj"][b], r["traj"], atol=1e-9)
        accepted += r["status"] == 0
    assert accepted >= len(models) // 2


@pytest.mark.parametrize("integrator,limited,reg", [(0, False, None), (1, False, None), (0, True, (1.0, 4.0, 1e6)), (1, True, None)])
def test_problem_b_is_a_fresh_handle_with_model_b_bit_for_bit(integrator, limited, reg):
    """The product as its own comparand: problem b of the batch equals a handle created with models[b] on the same general kernels
    (force_general = 2, single_wave_rollout = 1), the same integrator, limits and restarts, solving init[b] alone."""
    cfg, models = models_cfg(20 + integrator + 2 * limited, B=40, n=50, ls_max_iters=2 if reg else 20)
    limits = (0.0, 12.0) if limited else None
    out = solver(cfg, models, integrator, reg, limits).solve_batch(cfg["init"])
    for b in (0, 7, 22, 39):
        one = solver(dict(cfg, model=models[b]), None, integrator, reg, limits, force_general=2, single_wave_rollout=1)
        ref = one.solve_batch(cfg["init"][b:b + 1])
        for k in KEYS:
            assert np.array_equal(out[k][b], ref[k][0]), (b, k)


def test_permuting_problems_permutes_every_output_bit_for_bit():
    cfg, models = models_cfg(30, B=64, n=40)
    B = len(models)
    r = np.random.default_rng(3)
    desired = np.repeat(cfg["desired"][None], B, axis=0)
    desired[:, :, 1:4] += r.uniform(-0.5, 0.5, (B, 1, 3))
    base = solver(cfg, models).solve_batch(cfg["init"], desired)
    perm = r.permutation(B)
    out = solver(cfg, [models[p] for p in perm]).solve_batch(cfg["init"][perm], desired[perm])
    for k in KEYS:
        assert np.array_equal(out[k], base[k][perm]), k


def test_rows_above_the_regime_boundary_and_with_compaction_are_the_small_batches_bits():
    cfg, models = models_cfg(31, B=5000, n=30, max_iters=12)
    big = solver(cfg, models).solve_batch(cfg["init"])
    for lo in (0, 2048, 4096, 4936):
        part = solver(cfg, models[lo:lo + 64]).solve_batch(cfg["init"][lo:lo + 64])
        for k in KEYS:
            assert np.array_equal(big[k][lo:lo + 64], part[k]), (lo, k)
    B = 2048
    on = solver(cfg, models[:B], compaction=1).solve_batch(cfg["init"][:B])
    off = solver(cfg, models[:B], compaction=-1).solve_batch(cfg["init"][:B])
    assert_same(on, off, "compaction")
    for k in KEYS:
        assert np.array_equal(on[k], big[k][:B]), k


def test_hover_thrust_is_each_problem_s_own():
    """Every problem is asked to hover at its own pose with its own m_b g_b / 4 as the desired thrust, from a start at 1 N per rotor:
    the solved thrust is each problem's own hover thrust (slope 1 against m_b g_b / 4).  With one model for all it is not."""
    B, n = 32, 40
    models = random_models(B, 77)
    dt = 0.05
    r = np.random.default_rng(9)
    want = np.array([pb.hover_thrust(m) for m in models])
    desired = np.repeat(pb.hover_desired(n, dt, 0.0)[None], B, axis=0)
    for b in range(B):
        desired[b, :, 1:8] = orc.se3_exp(np.concatenate([r.uniform(-1, 1, 3), r.uniform(-0.5, 0.5, 3)]))
        desired[b, :, 14:18] = want[b]
    init = desired.copy()
    init[:, :, 14:18] = 1.0
    cfg = dict(model=pb.MODEL_A, Q=pb.Q_DEMO, R=pb.R_DEMO, dt=dt, desired=desired[0], init=init,
               options=dict(pb.OPTIONS_DEMO, populate_debug=False, rtol=1e-10, atol=1e-10))
    out = solver(cfg, models).solve_batch(init, desired)
    # (the mean over the knots whose control acts within the horizon; the solves stop a little short of exact hover -- status 0, the
    # oracle with each problem's model stops at the same place: 7.5 % at most, slope 0.97 -- and with one model for all the slope is 0.14)
    got = out["traj"][:, :-1, 14:18].mean(axis=(1, 2))
    np.testing.assert_allclose(got, want, rtol=0.1)
    slope = np.polyfit(want, got, 1)[0]
    assert abs(slope - 1.0) < 0.05, slope
    shared = solver(cfg).solve_batch(init, desired)["traj"][:, :-1, 14:18].mean(axis=(1, 2))
    assert abs(np.polyfit(want, shared, 1)[0] - 1.0) > 0.5


def test_off_means_off():
    cfg, _ = models_cfg(40, B=96, n=40)
    same = [cfg["model"]] * 96
    general = dict(force_general=2, single_wave_rollout=1)
    assert_same(solver(cfg, same, **general).solve_batch(cfg["init"]), solver(cfg, **general).solve_batch(cfg["init"]), "handle's model")
    big = pb.config2(B=1024, N=100)
    fresh = capi.from_config(big).solve_batch(big["init"])
    s = capi.from_config(big)
    s.set_models(random_models(64, 5))
    assert "per-problem models" in s.describe(64)
    s.solve_batch(big["init"][:64])
    s.clear_models()
    assert "per-problem models" not in s.describe(1024)
    assert_same(s.solve_batch(big["init"]), fresh, "cleared")
    assert_same(capi.from_config(big).solve_batch(big["init"]), fresh, "never set")


def test_thrust_limits_with_models_match_the_restatement():
    cfg, models = models_cfg(50, B=4, n=25)
    lo, hi = 0.0, 10.0
    out = solver(cfg, models, limits=(lo, hi)).solve_batch(cfg["init"])
    for b, m in enumerate(models):
        ref = lim.LimitedILQR(Model(**m), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], dict(cfg["options"]), lo, hi).solve(cfg["init"][b])
        assert [out["status"][b], out["iters"][b], out["n_bwd"][b], out["n_fwd"][b]] == \
            [ref["status"], ref["iters"], ref["n_bwd"], ref["n_fwd"]], b
        np.testing.assert_allclose(out["cost"][b], ref["cost"], rtol=1e-9)
        for i in range(cfg["init"].shape[1]):
            np.testing.assert_allclose(pose_from_knot(out["traj"][b, i]), pose_from_knot(ref["traj"][i]), atol=1e-6)
        np.testing.assert_allclose(out["traj"][b, :, 8:18], ref["traj"][:, 8:18], atol=1e-6)
    u = out["traj"][:, :, 14:18]
    assert np.all(u >= lo) and np.all(u <= hi)


def test_sharded_equals_the_single_handle_bit_for_bit():
    cfg, models = models_cfg(60, B=101, n=30)
    single = solver(cfg, models).solve_batch(cfg["init"])
    sh = capi.sharded_from_config(cfg, devices=[0] * 3)
    sh.set_models(models)
    assert_same(sh.solve_batch(cfg["init"]), single, "sharded")
    with pytest.raises(TypeError, match="B = 101"):
        sh.solve_batch(cfg["init"][:100])
    sh.clear_models()
    assert_same(sh.solve_batch(cfg["init"]), capi.from_config(cfg).solve_batch(cfg["init"]), "sharded, cleared")


def test_refusals():
    cfg, models = models_cfg(70, B=8, n=10)
    s = capi.from_config(cfg)
    s.set_models(models)
    with pytest.raises(TypeError, match="B = 8"):
        s.solve_batch(cfg["init"][:7])
    with pytest.raises(TypeError, match="B = 8"):
        s.backwards_pass(cfg["init"][:4])
    with pytest.raises(TypeError, match="qilqr_solve"):
        s.solve(cfg["init"][0])
    s.cost_trajectory(cfg["init"][:3])  # (model-free: any B)
    bad = list(models)
    bad[5] = dict(bad[5], inertia=np.diag([1.0, -1.0, 1.0]))
    with pytest.raises(RuntimeError, match=r"Inertia matrix is not positive definite!.*problem 5"):
        s.set_models(bad)
    with pytest.raises(RuntimeError, match="problem 5"):
        capi.sharded_from_config(cfg, devices=[0, 0]).set_models(bad)
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").set_models(models)
    from tests.diag_lib import capi_diag
    p = capi_diag().from_config(cfg, persistent=1)
    p.set_models(models)
    with pytest.raises(TypeError, match="persistent"):
        p.solve_batch(cfg["init"])
