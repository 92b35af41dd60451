"""The sampling planner on the device (k_mppi_flight, k_mppi_update: mppi_kernels.h) through the C ABI on plain device buffers: every
instantiation of the flight against the restatement (tests/mppi_numpy.py) with the CPU suite's bars, the update against the host program
(tests/host_mppi_harness.cpp) over the same scores within tests/mppi_numpy.py's update_bound, the known answers, containment and
independence of the batch, what follows it (qilqr_reduce_scores_device, qilqr_cost_trajectory, qilqr_solve_batch_device); and
RecedingHorizon's explore, in a torch process of its own.  n = 12 (6 at S = 4096)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import monte_carlo_numpy as mn, mppi_cases as mc, mppi_numpy as mp, scored_flight_numpy as sn  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402
from tests.test_mppi_cpu import PLANNED_COSTS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, SEED = mc.B, mc.N, 77
FLIGHT_SEED = 79  # of the draws of the eight-kernel test: the restatement's own margins (knot gap, |clearance|, thrust to limit > 1e-6) hold in all sixteen cases
GUARD = 64  # bytes behind the end of every output, prefilled with 0xFF like the output


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def harness():
    return mc.build_harness(["-O2"], "host_mppi_harness")


def guarded(hip, shape):
    return hip.alloc(8 * int(np.prod(shape)) + GUARD)


def fetch(hip, ptr, shape):
    """the output, raw, and whether the guard behind it kept its bits"""
    words = int(np.prod(shape))
    raw = hip.download(ptr, (8 * words + GUARD,), dtype=np.uint8)
    return raw[:8 * words].view(np.float64).reshape(shape), bool((raw[8 * words:] == 0xFF).all())


def rule_of(sigma, lambda_=1.0, tau_s=0.0, collision_cost=0.0, first_is_nominal=False):
    return capi.mppi_rule(sigma, lambda_, tau_s, collision_cost, first_is_nominal)


def solver_for(cfg, integrator=0, limits=None, models=None, shared=None, own=None, counts=None, Qs=None, k0=0, handle_desired=None):
    s = capi.from_config(cfg if handle_desired is None else dict(cfg, desired=handle_desired))
    s.set_integrator(integrator)
    if limits is not None:
        s.set_control_limits(*limits)
    if models is not None:
        s.set_models(models)
    if shared is not None:
        s.set_obstacles(shared)
    if own is not None:
        s.set_batch_obstacles(own, np.asarray(counts, dtype=np.int32))
    if Qs is not None:
        s.set_state_weight_schedule(np.asarray(Qs).reshape(-1, 12, 12))
        s.set_horizon_start(k0)
    return s


def dev_flight(hip, s, plan, S, seed, rule, x0=None, desired=None, b0=0):
    lib = capi.load()
    b, n = plan.shape[:2]
    d_plan, d_x0, d_des = hip.upload(plan), (hip.upload(x0) if x0 is not None else None), (hip.upload(desired) if desired is not None else None)
    d_score = guarded(hip, (b, S, 4))
    assert lib.qilqr_mppi_flight_device(s._h, C.byref(rule), seed, d_plan, d_x0, d_des, b, n, S, b0, d_score) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    score, kept = fetch(hip, d_score, (b, S, 4))
    assert kept, "k_mppi_flight wrote behind the end of d_score"
    return score


def dev_update(hip, s, plan, score, seed, rule, x0=None, desired=None, b0=0):
    lib = capi.load()
    b, n, S = plan.shape[0], plan.shape[1], score.shape[1]
    d_plan, d_x0, d_des = hip.upload(plan), (hip.upload(x0) if x0 is not None else None), (hip.upload(desired) if desired is not None else None)
    d_score, d_out, d_info = hip.upload(score), guarded(hip, (b, n, 18)), guarded(hip, (b, 8))
    assert lib.qilqr_mppi_update_device(s._h, C.byref(rule), seed, d_plan, d_x0, d_des, d_score, b, n, S, b0, d_out, d_info) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    (out, kept_out), (info, kept_info) = fetch(hip, d_out, (b, n, 18)), fetch(hip, d_info, (b, 8))
    assert kept_out and kept_info, "the update wrote behind the end of an output"
    assert not np.isnan(out).any(), "a word of d_out_plan was left unwritten"
    return out, info


# ------------------------------------------------------------------------------------------------ 1. the eight kernels of the flight

@pytest.fixture(scope="module")
def two_plans():
    """B = 2 of the standard case with every operand of the score; the limits and the spheres are tests/mppi_cases.py's"""
    host, rest, cfg, plan, x0, _ = mc.everything(5, SEED)
    cut = lambda v: v[:2] if isinstance(v, (list, np.ndarray)) and len(v) == B else v
    return {k: cut(v) for k, v in host.items()}, {k: (v if k in ("limits", "desired", "Qs", "shared") else cut(v)) for k, v in rest.items()}, cfg, plan[:2], x0[:2]


@pytest.mark.parametrize("ext", ["plain", "limits", "models", "both"])
@pytest.mark.parametrize("integrator", [0, 1])
def test_every_flight_kernel_against_the_restatement(hip, two_plans, integrator, ext):
    host, rest, cfg, plan, x0 = two_plans
    limits = host["limits"] if ext in ("limits", "both") else None
    models = host["models"] if ext in ("models", "both") else None
    s = solver_for(cfg, integrator, limits, models, host["shared"], host["own"], host["counts"], host["Qs"], host["k0"], host["handle_desired"])
    rest = dict(rest, limits=limits, models=models)
    rule = rule_of(mc.SIGMA, tau_s=0.3)
    for S in (63, 130):  # one idle lane; three blocks per plan, the last mostly idle
        eps = mp.perturbations(FLIGHT_SEED, 2, S, N, cfg["dt"], mc.SIGMA, tau_s=0.3)
        want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], integrator=integrator, **rest)
        gaps = sn.margins(clear)
        assert np.isfinite(want).all() and gap > 1e-6 and gaps[0] > 1e-6 and gaps[1] > 1e-6, (S, gap, gaps)
        got = dev_flight(hip, s, plan, S, FLIGHT_SEED, rule, x0=x0)
        over = lambda g, w: float((np.abs(g - w) / (sn.ATOL + sn.RTOL * np.abs(w))).max())
        print("[observed] integrator %d, %s, S = %d: error over its bar %.3g (cost), %.3g (clearance)" % (
            integrator, ext, S, over(got[..., 0], want[..., 0]), over(got[..., 1], want[..., 1])))
        np.testing.assert_allclose(got[..., :2], want[..., :2], rtol=sn.RTOL, atol=sn.ATOL)
        assert np.array_equal(got[..., 2:], want[..., 2:])
        assert (got[..., 3] > 0).any() and (got[..., 3] == 0).any()  # some samples hit
        if limits is not None:  # some thrusts clamp: the flight without limits scores otherwise
            u = plan[:, None, :, 14:18] + eps
            assert ((u < limits[0]) | (u > limits[1])).any()
    if models is not None:  # the two models part: plan 1 under the handle's model scores otherwise, plan 0 (whose model is the handle's) the same
        s.clear_models()
        same = dev_flight(hip, s, plan, 130, FLIGHT_SEED, rule, x0=x0)
        assert same[0].tobytes() == got[0].tobytes() and (same[1, :, 0] != got[1, :, 0]).all()


# ------------------------------------------------------------------------------------------------ 2. the batch plays no part, 3. containment

@pytest.fixture(scope="module")
def three_plans():
    host, rest, cfg, plan, x0, _ = mc.everything(5, SEED)
    s = solver_for(cfg, 1, host["limits"], host["models"], host["shared"], host["own"], host["counts"], host["Qs"], host["k0"], host["handle_desired"])
    return host, rest, cfg, plan, x0, s


@pytest.mark.parametrize("S", [1, 5, 64, 65])
def test_a_plans_bits_do_not_depend_on_the_batch(hip, three_plans, S):
    host, _, cfg, plan, x0, s = three_plans
    rule = rule_of(mc.SIGMA, lambda_=300.0, tau_s=0.3, collision_cost=10.0)
    whole = dev_flight(hip, s, plan, S, SEED, rule, x0=x0)
    out, info = dev_update(hip, s, plan, whole, SEED, rule, x0=x0)
    longer = dev_flight(hip, s, plan, 130, SEED, rule, x0=x0)
    assert longer[:, :S].tobytes() == whole.tobytes()  # (a sample's bits do not depend on S)
    # plans 1 .. 2 with b0 = 1 (their models and their rows of the per-problem table set for those two)
    s2 = solver_for(cfg, 1, host["limits"], host["models"][1:], host["shared"], host["own"][1:], host["counts"][1:], host["Qs"], host["k0"], host["handle_desired"])
    part = dev_flight(hip, s2, plan[1:], S, SEED, rule, x0=x0[1:], b0=1)
    assert part.tobytes() == whole[1:].tobytes()
    out2, info2 = dev_update(hip, s2, plan[1:], part, SEED, rule, x0=x0[1:], b0=1)
    assert out2.tobytes() == out[1:].tobytes() and info2.tobytes() == info[1:].tobytes()
    # plan 0 alone
    s1 = solver_for(cfg, 1, host["limits"], host["models"][:1], host["shared"], host["own"][:1], host["counts"][:1], host["Qs"], host["k0"], host["handle_desired"])
    alone = dev_flight(hip, s1, plan[:1], S, SEED, rule, x0=x0[:1])
    assert alone.tobytes() == whole[:1].tobytes()
    out1, info1 = dev_update(hip, s1, plan[:1], alone, SEED, rule, x0=x0[:1])
    assert out1.tobytes() == out[:1].tobytes() and info1.tobytes() == info[:1].tobytes()


def test_a_refused_call_on_a_live_handle_writes_nothing(hip, three_plans):
    _, _, _, plan, x0, s = three_plans
    lib = capi.load()
    S = 5
    d_plan, d_x0 = hip.upload(plan), hip.upload(x0)
    d_score, d_out, d_info = guarded(hip, (B, S, 4)), guarded(hip, (B, N, 18)), guarded(hip, (B, 8))
    bad = [rule_of(mc.SIGMA, lambda_=0.0), rule_of([0.1, -0.1, 0.1, 0.1]), rule_of(mc.SIGMA, tau_s=float("nan"))]
    flagged = rule_of(mc.SIGMA)
    flagged.flags = 2
    for r in bad + [flagged]:
        assert lib.qilqr_mppi_flight_device(s._h, C.byref(r), SEED, d_plan, d_x0, None, B, N, S, 0, d_score) == capi.ERR_INVALID_ARG
        assert lib.qilqr_mppi_update_device(s._h, C.byref(r), SEED, d_plan, d_x0, None, d_score, B, N, S, 0, d_out, d_info) == capi.ERR_INVALID_ARG
    ok = rule_of(mc.SIGMA)
    assert lib.qilqr_mppi_flight_device(s._h, C.byref(ok), SEED, d_plan, d_x0, None, B, N, 4097, 0, d_score) == capi.ERR_INVALID_ARG
    assert lib.qilqr_mppi_flight_device(s._h, C.byref(ok), SEED, d_plan, d_x0, None, B - 1, N, S, 0, d_score) == capi.ERR_INVALID_ARG  # models for B
    assert "set for B plans" in lib.qilqr_last_error().decode()
    assert lib.qilqr_mppi_update_device(s._h, C.byref(ok), SEED, d_plan, d_x0, None, d_score, B, N, S, 0, d_plan, d_info) == capi.ERR_INVALID_ARG
    assert lib.qilqr_mppi_flight_device(s._h, C.byref(ok), SEED, d_plan, d_x0, None, B, N + 9, S, 0, d_score) == capi.ERR_LENGTH_MISMATCH  # past the schedule
    hip.synchronize(lib.qilqr_stream(s._h))
    for ptr, shape in ((d_score, (B, S, 4)), (d_out, (B, N, 18)), (d_info, (B, 8))):
        raw = hip.download(ptr, (8 * int(np.prod(shape)) + GUARD,), dtype=np.uint8)
        assert (raw == 0xFF).all()
    f32 = capi.from_config(three_plans[2], precision="f32")
    assert lib.qilqr_mppi_flight_device(f32._h, C.byref(ok), SEED, d_plan, d_x0, None, B, N, S, 0, d_score) == capi.ERR_INVALID_ARG
    assert "precision 0" in lib.qilqr_last_error().decode()


# ------------------------------------------------------------------------------------------------ 4. the update against the host program

@pytest.mark.parametrize("S, n", [(5, N), (64, N), (70, N), (1024, N), (4096, 6)])
def test_the_update_against_the_host_program_over_the_same_scores(hip, harness, S, n):
    """one sample per lane up to S = 1024, four per lane at 4096; the scores are the device's own flight's, handed to both, so that the
    flight's rounding is not in the comparison.  J_min, its sample and the count must match exactly, the controls within update_bound."""
    host, rest, cfg, plan, x0, _ = mc.everything(5, SEED)
    plan, b = np.ascontiguousarray(plan[:2, :n]), 2
    cut = dict(x0=x0[:b], models=host["models"][:b], own=host["own"][:b], counts=host["counts"][:b])
    s = solver_for(cfg, 0, host["limits"], cut["models"], host["shared"], cut["own"], cut["counts"], host["Qs"], host["k0"], host["handle_desired"])
    kw = dict(tau_s=0.3, collision_cost=30.0, first_is_nominal=True)
    rule = rule_of(mc.SIGMA, lambda_=400.0, **kw)
    score = dev_flight(hip, s, plan, S, SEED, rule, x0=cut["x0"])
    assert np.isfinite(score).all()
    got, info = dev_update(hip, s, plan, score, SEED, rule, x0=cut["x0"])
    want, want_info = mc.host_update(harness, cfg, plan, score, SEED, mc.SIGMA, 400.0, **dict(host, **cut), **{k: v for k, v in kw.items() if k != "tau_s"})
    _, eps = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, first_is_nominal=True, **dict(host, **cut))
    _, _, scale = mp.update(plan, score, eps, 400.0, 30.0, host["limits"])
    bound = mp.update_bound(scale, S, mc.SIGMA)
    err = np.abs(got[:, :, 14:18] - want[:, :, 14:18])
    print("[observed] S = %d: control error %.3g of its bound (largest %.3g); effective samples %s" % (S, (err / bound).max(), err.max(), info[:, 2].tolist()))
    assert (err <= bound).all()
    assert np.array_equal(info[:, [0, 1, 3]], want_info[:, [0, 1, 3]])
    np.testing.assert_allclose(info[:, 2], want_info[:, 2], rtol=1e-12)
    assert got[:, :, 0].tobytes() == plan[:, :, 0].tobytes() and np.array_equal(got[:, 0, 1:14], cut["x0"])
    # the new plan's states and its score: the host program's flight of ITS controls, within the flight's bar
    np.testing.assert_allclose(got, want, rtol=sn.RTOL, atol=sn.ATOL)
    np.testing.assert_allclose(info[:, 4:6], want_info[:, 4:6], rtol=sn.RTOL, atol=sn.ATOL)


# ------------------------------------------------------------------------------------------------ 5. what follows it

def test_the_new_plan_is_a_trajectory_the_solver_takes(hip):
    """no sphere is set: word 4 of info is what qilqr_cost_trajectory charges d_out_plan (1e-10), and a solve from it does not end higher"""
    cfg, plan, x0 = mc.standard()
    s = solver_for(cfg)
    rule = rule_of(mc.SIGMA, lambda_=100.0, tau_s=0.3, first_is_nominal=True)
    score = dev_flight(hip, s, plan, 70, SEED, rule, x0=x0)
    out, info = dev_update(hip, s, plan, score, SEED, rule, x0=x0)
    cost = s.cost_trajectory(out)
    np.testing.assert_allclose(info[:, 4], cost, rtol=1e-10, atol=1e-10)
    assert np.isposinf(info[:, 5]).all() and (info[:, 6] == -1).all() and not info[:, 7].any()
    lib = capi.load()
    d_init, d_traj, d_cost = hip.upload(out), hip.alloc(8 * B * N * 18), hip.alloc(8 * B)
    d_int = [hip.alloc(4 * B) for _ in range(4)]
    vp = C.c_void_p
    rc = lib.qilqr_solve_batch_device(s._h, vp(d_init), None, C.c_int32(B), C.c_int32(N), vp(d_traj), vp(d_cost), *(vp(p) for p in d_int))
    assert rc == 0, lib.qilqr_last_error()
    solved = hip.download(d_cost, (B,))
    assert (solved <= cost).all() and (solved < cost).any(), (solved, cost)


def test_the_known_answers_on_the_device(hip):
    cfg, plan, x0 = mc.standard()
    s = solver_for(cfg)
    S = 70
    still = rule_of(0.0, lambda_=5.0)
    score = dev_flight(hip, s, plan, S, SEED, still, x0=x0)
    assert (score == score[:, :1]).all()
    out, info = dev_update(hip, s, plan, score, SEED, still, x0=x0)
    assert out[:, :, 14:18].tobytes() == plan[:, :, 14:18].tobytes() and info[:, 4:].tobytes() == score[:, 0].tobytes()
    assert np.array_equal(info[:, :4], np.stack([score[:, 0, 0], np.zeros(B), np.full(B, float(S)), np.full(B, float(S))], axis=1))
    lam = 1e-6
    cold = rule_of(mc.SIGMA, lambda_=lam, tau_s=0.3)
    score = dev_flight(hip, s, plan, S, SEED, cold, x0=x0)
    J = np.sort(score[..., 0], axis=1)
    assert ((J[:, 1] - J[:, 0]) / lam > 745).all()
    out, info = dev_update(hip, s, plan, score, SEED, cold, x0=x0)
    best = score[..., 0].argmin(axis=1)
    assert np.array_equal(info[:, 1], best) and (info[:, 2] == 1.0).all()
    assert np.array_equal(info[:, 4:], score[np.arange(B), best])  # the new plan flies what the best sample flew, bit for bit
    eps = mp.perturbations(SEED, B, S, N, cfg["dt"], mc.SIGMA, tau_s=0.3)
    assert np.abs(out[:, :, 14:18] - (plan[:, :, 14:18] + eps[np.arange(B), best])).max() <= 2 * mp.eps_atol(mc.SIGMA)
    bad = np.full_like(score, np.nan)
    out, info = dev_update(hip, s, plan, bad, SEED, cold, x0=x0)
    assert out[:, :, 14:18].tobytes() == plan[:, :, 14:18].tobytes() and np.isnan(info[:, 0]).all() and (info[:, 1] == -1).all() and not info[:, 2:4].any()


def test_the_score_is_the_layout_the_reduction_reads(hip, three_plans):
    _, _, _, plan, x0, s = three_plans
    lib = capi.load()
    S = 70
    score = dev_flight(hip, s, plan, S, SEED, rule_of(mc.SIGMA, tau_s=0.3), x0=x0)
    d_score, d_sum = hip.upload(score), guarded(hip, (B, 8))
    assert lib.qilqr_reduce_scores_device(s._h, d_score, B, S, d_sum) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    got, kept = fetch(hip, d_sum, (B, 8))
    assert kept and mn.extremes_are_unique(score)
    mn.assert_summary(got, mn.summary(score))


# ------------------------------------------------------------------------------------------------ 6. RecedingHorizon's explore

@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/mppi_torch_child.py, once, in a fresh process (PyTorch's ROCm runtime has to be the first a process initialises)"""
    out = str(tmp_path_factory.mktemp("mppi_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.mppi_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_explore_is_the_direct_calls_between_the_shift_and_the_solve(torch_forms):
    z = torch_forms
    for step in ("start", "tick"):
        assert z[step + "_explore"].tobytes() == z[step + "_direct_info"].tobytes(), step
        assert z[step + "_traj"].tobytes() == z[step + "_direct_traj"].tobytes() and z[step + "_cost"].tobytes() == z[step + "_direct_cost"].tobytes(), step
        assert sorted(z[step + "_keys"]) == sorted(["u0", "traj", "cost", "status", "iters", "explore"]), step
        assert z[step + "_explore"].shape == (3, 8) and (z[step + "_explore"][:, 3] == 70).all(), step
    assert "S, seed, sigma, lambda_" in str(z["refusal_missing"]) and "S, seed, sigma, lambda_" in str(z["refusal_unknown"])


def test_without_explore_the_calls_are_what_they_were(torch_forms):
    z = torch_forms
    for step in ("start", "tick"):
        assert list(z[step + "_none_keys"]) == list(z[step + "_plain_keys"]) and "explore" not in list(z[step + "_plain_keys"]), step
        for k in ("traj", "cost", "status", "iters", "u0"):
            assert z["%s_none_%s" % (step, k)].tobytes() == z["%s_plain_%s" % (step, k)].tobytes(), (step, k)


def test_it_plans_on_the_device_as_on_the_host(torch_forms):
    cost = torch_forms["planning_info"][:, :, 4]
    print("[observed] nominal cost per round on the device:", cost.tolist())
    np.testing.assert_allclose(cost, PLANNED_COSTS, rtol=sn.RTOL, atol=sn.ATOL)
    assert (np.diff(cost, axis=0) < 0).all()
