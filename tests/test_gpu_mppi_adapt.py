"""The planner's adapted spread on the device (k_mppi_flight_spread, k_mppi_adapt: mppi_adapt_kernels.h) through the C ABI on plain
device buffers: every instantiation of the flight against the restatement (tests/mppi_adapt_numpy.py) with the CPU suite's bars, the
adaptation against the host program (tests/host_mppi_adapt_harness.cpp) over the same scores within the CPU suite's bounds, the
bit-equalities with the existing planner, containment and independence of the batch, what follows it; and RecedingHorizon's
explore["adapt"], in a torch process of its own.  n = 12 (6 at S = 4096)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import mppi_adapt_cases as ac, mppi_adapt_numpy as ma, mppi_cases as mc, mppi_numpy as mp, scored_flight_numpy as sn  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402
from tests.test_gpu_mppi import GUARD, dev_flight, dev_update, fetch, guarded, rule_of, solver_for  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, SEED = mc.B, mc.N, 77
FLIGHT_SEED = 80  # of the draws of the eight-kernel test: the restatement's own margins (knot gap, |clearance|, thrust to limit > 1e-6) hold in all sixteen cases


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def harness():
    return ac.build_harness(["-O2"], "host_mppi_adapt_harness")


def adapt_rule(floor=ac.FLOOR, cap=ac.CAP, rate=ac.RATE):
    return capi.mppi_adapt_rule(floor, cap, rate)


def dev_flight_spread(hip, s, plan, spread, S, seed, rule, x0=None, b0=0):
    lib = capi.load()
    b, n = plan.shape[:2]
    d_plan, d_x0, d_spread = hip.upload(plan), (hip.upload(x0) if x0 is not None else None), hip.upload(spread)
    d_score = guarded(hip, (b, S, 4))
    assert lib.qilqr_mppi_flight_spread_device(s._h, C.byref(rule), seed, d_plan, d_x0, None, d_spread, b, n, S, b0, d_score) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    score, kept = fetch(hip, d_score, (b, S, 4))
    assert kept, "k_mppi_flight_spread wrote behind the end of d_score"
    return score


def dev_adapt(hip, s, plan, spread, score, seed, rule, adapt, x0=None, b0=0, mean_only=False):
    lib = capi.load()
    b, n, S = plan.shape[0], plan.shape[1], score.shape[1]
    d_plan, d_x0, d_spread = hip.upload(plan), (hip.upload(x0) if x0 is not None else None), hip.upload(spread)
    d_score, d_out, d_new, d_info = hip.upload(score), guarded(hip, (b, n, 18)), guarded(hip, (b, n, 4)), guarded(hip, (b, 8))
    rc = lib.qilqr_mppi_adapt_device(s._h, C.byref(rule), C.byref(adapt), seed, d_plan, d_x0, None, d_spread, d_score, b, n, S, b0, d_out,
                                     None if mean_only else d_new, d_info)
    assert rc == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    (out, k0), (new, k1), (info, k2) = fetch(hip, d_out, (b, n, 18)), fetch(hip, d_new, (b, n, 4)), fetch(hip, d_info, (b, 8))
    assert k0 and k1 and k2, "the adaptation wrote behind the end of an output"
    assert not np.isnan(out).any(), "a word of d_out_plan was left unwritten"
    if mean_only:
        assert (new.view(np.uint8) == 0xFF).all()
    else:
        assert not np.isnan(new).any(), "a word of d_out_spread was left unwritten"
    return out, info, new


# ------------------------------------------------------------------------------------------------ 1. the eight kernels of the flight

@pytest.fixture(scope="module")
def two_plans():
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
    spread = ac.spread_field(2)
    assert (np.diff(spread, axis=1) != 0).any(axis=(0, 2)).all()  # the spread varies along the horizon
    for S in (63, 130):  # one idle lane; three blocks per plan, the last mostly idle
        eps = ma.perturbations(FLIGHT_SEED, spread, S, cfg["dt"], tau_s=0.3)
        want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], integrator=integrator, **rest)
        gaps = sn.margins(clear)
        assert np.isfinite(want).all() and gap > 1e-6 and gaps[0] > 1e-6 and gaps[1] > 1e-6, (S, gap, gaps)
        got = dev_flight_spread(hip, s, plan, spread, S, FLIGHT_SEED, rule, x0=x0)
        over = lambda g, w: float((np.abs(g - w) / (sn.ATOL + sn.RTOL * np.abs(w))).max())
        print("[observed] integrator %d, %s, S = %d: error over its bar %.3g (cost), %.3g (clearance)" % (
            integrator, ext, S, over(got[..., 0], want[..., 0]), over(got[..., 1], want[..., 1])))
        np.testing.assert_allclose(got[..., :2], want[..., :2], rtol=sn.RTOL, atol=sn.ATOL)
        assert np.array_equal(got[..., 2:], want[..., 2:])
        assert (got[..., 3] > 0).any() and (got[..., 3] == 0).any()  # some samples hit
        if limits is not None:
            u = plan[:, None, :, 14:18] + eps
            assert ((u < limits[0]) | (u > limits[1])).any()
    if models is not None:  # the two models part
        s.clear_models()
        same = dev_flight_spread(hip, s, plan, spread, 130, FLIGHT_SEED, rule, x0=x0)
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
    rule, adapt, spread = rule_of(mc.SIGMA, lambda_=300.0, tau_s=0.3, collision_cost=10.0), adapt_rule(), ac.spread_field()
    whole = dev_flight_spread(hip, s, plan, spread, S, SEED, rule, x0=x0)
    outs = dev_adapt(hip, s, plan, spread, whole, SEED, rule, adapt, x0=x0)
    # plans 1 .. 2 with b0 = 1 (their models and their rows of the per-problem table set for those two)
    s2 = solver_for(cfg, 1, host["limits"], host["models"][1:], host["shared"], host["own"][1:], host["counts"][1:], host["Qs"], host["k0"], host["handle_desired"])
    part = dev_flight_spread(hip, s2, plan[1:], spread[1:], S, SEED, rule, x0=x0[1:], b0=1)
    assert part.tobytes() == whole[1:].tobytes()
    for one, every in zip(dev_adapt(hip, s2, plan[1:], spread[1:], part, SEED, rule, adapt, x0=x0[1:], b0=1), outs):
        assert one.tobytes() == every[1:].tobytes()
    # plan 0 alone
    s1 = solver_for(cfg, 1, host["limits"], host["models"][:1], host["shared"], host["own"][:1], host["counts"][:1], host["Qs"], host["k0"], host["handle_desired"])
    alone = dev_flight_spread(hip, s1, plan[:1], spread[:1], S, SEED, rule, x0=x0[:1])
    assert alone.tobytes() == whole[:1].tobytes()
    for one, every in zip(dev_adapt(hip, s1, plan[:1], spread[:1], alone, SEED, rule, adapt, x0=x0[:1]), outs):
        assert one.tobytes() == every[:1].tobytes()


def test_a_refused_call_on_a_live_handle_writes_nothing(hip, three_plans):
    _, _, _, plan, x0, s = three_plans
    lib = capi.load()
    S = 5
    d_plan, d_x0, d_spread = hip.upload(plan), hip.upload(x0), hip.upload(ac.spread_field())
    d_score, d_out, d_new, d_info = guarded(hip, (B, S, 4)), guarded(hip, (B, N, 18)), guarded(hip, (B, N, 4)), guarded(hip, (B, 8))
    ok, fine = rule_of(mc.SIGMA), adapt_rule()
    flight = lambda r, spread=d_spread, score=d_score, b=B, n=N: lib.qilqr_mppi_flight_spread_device(s._h, C.byref(r), SEED, d_plan, d_x0, None, spread, b, n, S, 0, score)
    adapt = lambda r, a, spread=d_spread, out=d_out, new=d_new: lib.qilqr_mppi_adapt_device(s._h, C.byref(r), C.byref(a) if a is not None else None, SEED, d_plan,
                                                                                             d_x0, None, spread, d_score, B, N, S, 0, out, new, d_info)
    for r in (rule_of(mc.SIGMA, lambda_=0.0), rule_of([0.1, -0.1, 0.1, 0.1])):
        assert flight(r) == capi.ERR_INVALID_ARG and adapt(r, fine) == capi.ERR_INVALID_ARG
    assert flight(ok, spread=None) == capi.ERR_INVALID_ARG and flight(ok, spread=d_spread + 8) == capi.ERR_INVALID_ARG
    assert flight(ok, score=d_spread) == capi.ERR_INVALID_ARG and "d_score overlaps d_spread" in lib.qilqr_last_error().decode()
    assert flight(ok, b=B - 1) == capi.ERR_INVALID_ARG and "set for B plans" in lib.qilqr_last_error().decode()
    assert flight(ok, n=N + 9) == capi.ERR_LENGTH_MISMATCH
    for a in (None, adapt_rule(floor=-1.0), adapt_rule(cap=float("inf")), adapt_rule(floor=0.5, cap=0.4), adapt_rule(rate=0.0), adapt_rule(rate=1.5)):
        assert adapt(ok, a) == capi.ERR_INVALID_ARG, lib.qilqr_last_error()
    reserved = adapt_rule()
    reserved.reserved[2] = 1.0
    assert adapt(ok, reserved) == capi.ERR_INVALID_ARG
    assert adapt(ok, fine, new=d_spread) == capi.ERR_INVALID_ARG and "not work in place" in lib.qilqr_last_error().decode()
    assert adapt(ok, fine, new=d_out) == capi.ERR_INVALID_ARG and adapt(ok, fine, out=d_spread) == capi.ERR_INVALID_ARG
    hip.synchronize(lib.qilqr_stream(s._h))
    for ptr, shape in ((d_score, (B, S, 4)), (d_out, (B, N, 18)), (d_new, (B, N, 4)), (d_info, (B, 8))):
        raw = hip.download(ptr, (8 * int(np.prod(shape)) + GUARD,), dtype=np.uint8)
        assert (raw == 0xFF).all()
    assert np.array_equal(hip.download(d_spread, (B, N, 4)), ac.spread_field())


# ------------------------------------------------------------------------------------------------ 4. the adaptation against the host program

@pytest.mark.parametrize("S, n", [(5, N), (64, N), (70, N), (1024, N), (4096, 6)])
def test_the_adaptation_against_the_host_program_over_the_same_scores(hip, harness, S, n):
    """one sample per lane up to S = 1024, four per lane at 4096; the scores are the device's own flight's, handed to both.  J_min, its
    sample and the count must match exactly, the controls within update_bound, the spreads within adapt_bound / (s_dev + s_ref)."""
    host, rest, cfg, plan, x0, _ = mc.everything(5, SEED)
    plan, b = np.ascontiguousarray(plan[:2, :n]), 2
    spread = np.ascontiguousarray(ac.spread_field()[:2, :n])
    cut = dict(x0=x0[:b], models=host["models"][:b], own=host["own"][:b], counts=host["counts"][:b])
    s = solver_for(cfg, 0, host["limits"], cut["models"], host["shared"], cut["own"], cut["counts"], host["Qs"], host["k0"], host["handle_desired"])
    kw = dict(tau_s=0.3, collision_cost=30.0, first_is_nominal=True)
    rule = rule_of(mc.SIGMA, lambda_=400.0, **kw)
    score = dev_flight_spread(hip, s, plan, spread, S, SEED, rule, x0=cut["x0"])
    assert np.isfinite(score).all()
    got, info, new = dev_adapt(hip, s, plan, spread, score, SEED, rule, adapt_rule(), x0=cut["x0"])
    hkw = dict(dict(host, **cut), collision_cost=30.0, first_is_nominal=True)
    want, want_info, want_new, _ = ac.host_adapt(harness, cfg, plan, score, SEED, spread, 400.0, **hkw)
    _, eps = ac.host_fly(harness, cfg, plan, S, SEED, spread, **{k: v for k, v in hkw.items() if k != "collision_cost"})
    ref = ma.adapt(plan, score, eps, spread, 400.0, ac.FLOOR, ac.CAP, ac.RATE, 30.0, host["limits"])
    bound = mp.update_bound(ref["scale"], S, spread)
    err = np.abs(got[:, :, 14:18] - want[:, :, 14:18])
    assert (err <= bound).all()
    assert np.array_equal(info[:, [0, 1, 3]], want_info[:, [0, 1, 3]])
    np.testing.assert_allclose(info[:, 2], want_info[:, 2], rtol=1e-12)
    worst, near, either = ac.compare_spreads(new, dict(ref, spread=want_new), ma.adapt_bound(ref["scale"], ref["scale2"], S, spread, ref["v"], ac.RATE))
    print("[observed] S = %d: control error %.3g, spread error %.3g of their bounds; %.3g of the entries near floor or cap" % (S, (err / bound).max(), worst, near))
    assert worst <= 1.0 and either and near <= 0.05
    np.testing.assert_allclose(got, want, rtol=sn.RTOL, atol=sn.ATOL)
    np.testing.assert_allclose(info[:, 4:6], want_info[:, 4:6], rtol=sn.RTOL, atol=sn.ATOL)
    # d_out_spread = NULL: the mean only, the same bits
    mean, mean_info, _ = dev_adapt(hip, s, plan, spread, score, SEED, rule, adapt_rule(), x0=cut["x0"], mean_only=True)
    assert mean.tobytes() == got.tobytes() and mean_info.tobytes() == info.tobytes()


# ------------------------------------------------------------------------------------------------ 5. the existing planner's bits, what follows

@pytest.mark.parametrize("integrator", [0, 1])
def test_a_constant_spread_without_correlation_is_the_existing_planner(hip, three_plans, integrator):
    host, _, cfg, plan, x0, _ = three_plans
    s = solver_for(cfg, integrator, host["limits"], host["models"], host["shared"], host["own"], host["counts"], host["Qs"], host["k0"], host["handle_desired"])
    rule = rule_of(mc.SIGMA, lambda_=150.0, collision_cost=30.0, first_is_nominal=True)
    for S in (70, 1500):
        want = dev_flight(hip, s, plan, S, SEED, rule, x0=x0)
        got = dev_flight_spread(hip, s, plan, ac.constant_spread(mc.SIGMA), S, SEED, rule, x0=x0)
        assert got.tobytes() == want.tobytes(), S
        want_out, want_info = dev_update(hip, s, plan, want, SEED, rule, x0=x0)
        out, info, new = dev_adapt(hip, s, plan, ac.constant_spread(mc.SIGMA), got, SEED, rule, adapt_rule(), x0=x0)
        assert out[:, :, 14:18].tobytes() == want_out[:, :, 14:18].tobytes() and info[:, :4].tobytes() == want_info[:, :4].tobytes(), S
        assert out.tobytes() == want_out.tobytes() and info.tobytes() == want_info.tobytes(), S
        assert (new != mc.SIGMA).any()


def test_the_known_answers_on_the_device_and_the_solver_takes_the_plan(hip):
    cfg, plan, x0 = mc.standard()
    s = solver_for(cfg)
    S, lam, spread = 70, 1e-6, ac.spread_field()
    cold = rule_of(mc.SIGMA, lambda_=lam, tau_s=0.3)
    score = dev_flight_spread(hip, s, plan, spread, S, SEED, cold, x0=x0)
    J = np.sort(score[..., 0], axis=1)
    assert ((J[:, 1] - J[:, 0]) / lam > 745).all()
    out, info, new = dev_adapt(hip, s, plan, spread, score, SEED, cold, adapt_rule(rate=1.0), x0=x0)
    assert (info[:, 2] == 1.0).all() and (new == ac.FLOOR).all()  # var = 0 exactly
    bad = np.full_like(score, np.nan)
    out, info, new = dev_adapt(hip, s, plan, spread, bad, SEED, cold, adapt_rule(), x0=x0)
    assert out[:, :, 14:18].tobytes() == plan[:, :, 14:18].tobytes() and new.tobytes() == spread.tobytes() and np.isnan(info[:, 0]).all()
    warm = rule_of(mc.SIGMA, lambda_=100.0, tau_s=0.3, first_is_nominal=True)
    score = dev_flight_spread(hip, s, plan, spread, S, SEED, warm, x0=x0)
    out, info, _ = dev_adapt(hip, s, plan, spread, score, SEED, warm, adapt_rule(), x0=x0)
    cost = s.cost_trajectory(out)
    np.testing.assert_allclose(info[:, 4], cost, rtol=1e-10, atol=1e-10)
    lib = capi.load()
    d_init, d_traj, d_cost = hip.upload(out), hip.alloc(8 * B * N * 18), hip.alloc(8 * B)
    d_int = [hip.alloc(4 * B) for _ in range(4)]
    vp = C.c_void_p
    rc = lib.qilqr_solve_batch_device(s._h, vp(d_init), None, C.c_int32(B), C.c_int32(N), vp(d_traj), vp(d_cost), *(vp(p) for p in d_int))
    assert rc == 0, lib.qilqr_last_error()
    solved = hip.download(d_cost, (B,))
    assert (solved <= cost).all() and (solved < cost).any(), (solved, cost)


# ------------------------------------------------------------------------------------------------ 6. RecedingHorizon's explore["adapt"]

@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/mppi_adapt_torch_child.py, once, in a fresh process (PyTorch's ROCm runtime has to be the first a process initialises)"""
    out = str(tmp_path_factory.mktemp("mppi_adapt_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.mppi_adapt_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_explore_with_adapt_is_the_direct_calls_between_the_shift_and_the_solve(torch_forms):
    z = torch_forms
    for step in ("start", "tick"):
        assert z[step + "_explore"].tobytes() == z[step + "_direct_info"].tobytes(), step
        assert z[step + "_traj"].tobytes() == z[step + "_direct_traj"].tobytes() and z[step + "_cost"].tobytes() == z[step + "_direct_cost"].tobytes(), step
        assert z[step + "_spread"].tobytes() == z[step + "_direct_spread"].tobytes(), step
        assert sorted(z[step + "_keys"]) == sorted(["u0", "traj", "cost", "status", "iters", "explore"]), step
    sigma = np.array([0.5, 0.4, 0.6, 0.5])
    assert (z["start_spread"] != sigma).any()
    # the spread a tick starts from is the last one shifted a knot, with a tail of sigma
    assert z["tick_shifted_spread"][:, :-1].tobytes() == z["start_spread"][:, 1:].tobytes() and (z["tick_shifted_spread"][:, -1] == sigma).all()
    # a refused tick rolls the spread back with the plan
    assert "rate must lie" in str(z["refusal_rate"]) and z["spread_after_refusal"].tobytes() == z["start_spread"].tobytes() and z["k0_after_refusal"] == 0
    assert "rate, floor and cap" in str(z["refusal_adapt_keys"])


def test_without_adapt_the_calls_are_what_they_were(torch_forms):
    z = torch_forms
    for step in ("start", "tick"):
        assert list(z[step + "_none_keys"]) == list(z[step + "_plain_keys"]) and "explore" not in list(z[step + "_plain_keys"]), step
        assert sorted(z[step + "_explore_keys"]) == sorted(["u0", "traj", "cost", "status", "iters", "explore"]), step
        for k in ("traj", "cost", "status", "iters", "u0"):
            assert z["%s_none_%s" % (step, k)].tobytes() == z["%s_plain_%s" % (step, k)].tobytes(), (step, k)
    assert z["spread_is_none_explore"] and z["spread_is_none_plain"] and z["spread_is_none_none"]
    # explore without adapt: the existing planner's direct calls followed by the solve, bit for bit
    assert z["start_explore_explore"].tobytes() == z["start_without_info"].tobytes()
    assert z["start_explore_traj"].tobytes() == z["start_without_traj"].tobytes() and z["start_explore_cost"].tobytes() == z["start_without_cost"].tobytes()
    assert z["start_explore_traj"].tobytes() != z["start_traj"].tobytes() or z["start_explore_explore"].tobytes() != z["start_explore"].tobytes()
