"""The sampling planner without a device: the per-lane routines of quadrotorilqr_amd/csrc/mppi_kernels.h and the rules of mppi_launch.h,
compiled with g++ into the stand-alone program tests/host_mppi_harness.cpp, against the restatement (tests/mppi_numpy.py), against answers
known without one, and against themselves; the refusals through the harness and through the C ABI; the kernels of mppi.hip by name.
B = 3, n = 12, S = 5 and 70 (one wavefront with idle lanes; two wavefronts of the update's block), with 8 shared spheres and a moving one
per problem, a schedule at horizon start 3, thrust limits and per-plan models (tests/mppi_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from quadrotorilqr_amd import capi
from tests import mppi_cases as mc, mppi_numpy as mp, scored_flight_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = mc.B, mc.N
SEED = 77
NEW_SYMBOLS = ("qilqr_mppi_flight_device", "qilqr_mppi_update_device")
# the kernels of mppi.hip: the flight's {Euler, Runge-Kutta} x {neither, limits, models, both}, the update's five block sizes
FLIGHT_KERNELS = ["_ZN5qilqr13k_mppi_flightILi%dEJ%sEEEvNS_11ModelConstsIdEENS_14MppiFlightArgsEDpT0_" % (i, e)
                  for i in (0, 1) for e in ("", "NS_13ControlLimitsE", "NS_11BatchModelsE", "NS_13ControlLimitsENS_11BatchModelsE")]
UPDATE_KERNELS = ["_ZN5qilqr13k_mppi_updateILi%dEEEvNS_14MppiUpdateArgsE" % t for t in (64, 128, 256, 512, 1024)]


@pytest.fixture(scope="module")
def harness():
    return mc.build_harness(["-O2"], "host_mppi_harness")


@pytest.fixture(scope="module")
def std():
    return mc.standard()


@pytest.fixture(scope="module")
def full():
    """S -> (host keywords, restatement keywords, cfg, plan, x0, the restatement's eps): computed once per S, never written to"""
    return {S: mc.everything(S, SEED) for S in (5, 70)}


def assert_score(got, want, clear, label=""):
    """tests/test_scored_flight_cpu.py's: cost and clearance within the bar, knot and collision count exactly -- after the restatement's own
    margins say that neither can flip inside the bar"""
    gap, zero = sn.margins(clear)
    assert gap > 1e-6 and zero > 1e-6, (label, gap, zero)
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
    np.testing.assert_allclose(got[..., 1], want[..., 1], rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
    assert np.array_equal(got[..., 2:], want[..., 2:]), label


# ------------------------------------------------------------------------------------------------ 1. the draws

@pytest.mark.parametrize("tau_s", [0.0, 0.3])
def test_the_perturbations_against_the_restatement(harness, std, tau_s):
    cfg, plan, _ = std
    _, eps = mc.host_fly(harness, cfg, plan, 70, SEED, mc.SIGMA, tau_s=tau_s, b0=4)
    want = mp.perturbations(SEED, B, 70, N, cfg["dt"], mc.SIGMA, tau_s=tau_s, b0=4)
    err = np.abs(eps - want).max()
    print("[observed] tau_s = %g: perturbation error %.3g of its bar %.3g" % (tau_s, err, mp.eps_atol(mc.SIGMA)))
    assert err <= mp.eps_atol(mc.SIGMA)
    if tau_s == 0.0:  # white noise: a knot's word is sigma times its own normal, and nothing of the knot before
        b, s, i, j = np.meshgrid(np.arange(B) + 4, np.arange(70), np.arange(N), np.arange(2), indexing="ij")
        z0, z1 = mp.mn.draws(SEED, b, s, i, mp.STREAM_CONTROLS, j)
        xi = np.stack([z0, z1], axis=-1).reshape(B, 70, N, 4)
        assert np.abs(eps - mc.SIGMA * xi).max() <= mp.eps_atol(mc.SIGMA)
    # the deviation of 3 * 70 * 12 draws per rotor: within 6 %
    assert np.abs(eps.std(axis=(0, 1, 2)) / mc.SIGMA - 1.0).max() < 0.06
    assert not np.array_equal(eps, mc.host_fly(harness, cfg, plan, 70, SEED + 1, mc.SIGMA, tau_s=tau_s, b0=4)[1])


def test_a_samples_rows_depend_on_its_indices_alone(harness, std):
    """not on B, not on S, and on b0 only through b0 + b; with the flag sample 0 -- and only sample 0 -- is zero"""
    cfg, plan, _ = std
    _, whole = mc.host_fly(harness, cfg, plan, 70, SEED, mc.SIGMA, tau_s=0.3)
    _, part = mc.host_fly(harness, cfg, plan[:1], 5, SEED, mc.SIGMA, tau_s=0.3, b0=2)
    assert part[0].tobytes() == whole[2, :5].tobytes()
    _, flagged = mc.host_fly(harness, cfg, plan, 70, SEED, mc.SIGMA, tau_s=0.3, first_is_nominal=True)
    assert not flagged[:, 0].any() and flagged[:, 1:].tobytes() == whole[:, 1:].tobytes()


# ------------------------------------------------------------------------------------------------ 2. the flight

@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("S", [5, 70])
def test_the_flight_against_the_restatement(harness, full, S, integrator):
    host, rest, cfg, plan, x0, eps = full[S]
    want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], integrator=integrator, **rest)
    label = str((S, integrator))
    assert np.isfinite(want).all(), label  # no sample is left out of the comparison
    assert gap > 1e-6, (label, gap)        # no control within the bar of a limit: the clamp cannot flip
    got, got_eps = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, integrator=integrator, **host)
    assert np.abs(got_eps - eps).max() <= mp.eps_atol(mc.SIGMA), label
    print("[observed] %s: cost error over its bar %.3g, clearance %.3g" % (
        label, (np.abs(got[..., 0] - want[..., 0]) / (sn.ATOL + sn.RTOL * np.abs(want[..., 0]))).max(),
        (np.abs(got[..., 1] - want[..., 1]) / (sn.ATOL + sn.RTOL * np.abs(want[..., 1]))).max()))
    assert_score(got, want, clear, label)
    # every switch is live: some thrusts clamp, some samples hit and some do not, the models part, the start state is read
    u = plan[:, None, :, 14:18] + eps
    assert ((u < rest["limits"][0]) | (u > rest["limits"][1])).any() and (got[..., 3] > 0).any() and (got[..., 3] == 0).any(), label
    one_model, _ = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, integrator=integrator, **dict(host, models=None))
    assert one_model[0].tobytes() == got[0].tobytes() and (one_model[1:, :, 0] != got[1:, :, 0]).all(), label  # (MODELS3[0] is the handle's)
    from_knot0, _ = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, integrator=integrator, **dict(host, x0=None))
    assert (from_knot0[..., 0] != got[..., 0]).all(), label
    at_knot0, _ = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, integrator=integrator, **dict(host, x0=np.ascontiguousarray(plan[:, 0, 1:14])))
    assert at_knot0.tobytes() == from_knot0.tobytes(), label


def test_the_flight_against_a_desired_trajectory_per_plan(harness, std):
    cfg, plan, x0 = std
    per_plan = np.ascontiguousarray(plan[::-1]) * 1.0
    eps = mp.perturbations(SEED, B, 5, N, cfg["dt"], mc.SIGMA)
    want, clear, _, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], per_plan)
    got, _ = mc.host_fly(harness, cfg, plan, 5, SEED, mc.SIGMA, x0=x0, desired=per_plan)
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=sn.RTOL, atol=sn.ATOL)
    assert np.isposinf(got[..., 1]).all() and (got[..., 2] == -1).all() and (got[..., 3] == 0).all()  # no spheres
    handles, _ = mc.host_fly(harness, cfg, plan, 5, SEED, mc.SIGMA, x0=x0)
    assert (handles[..., 0] != got[..., 0]).all()


def test_a_plans_bits_do_not_depend_on_the_batch(harness, full):
    host, _, cfg, plan, x0, _ = full[70]
    whole, _ = mc.host_fly(harness, cfg, plan, 70, SEED, mc.SIGMA, **host)
    for b in (0, B - 1):
        kw = dict(host, x0=x0[b:b + 1], models=mc.MODELS3[b:b + 1], own=host["own"][b:b + 1], counts=host["counts"][b:b + 1], b0=b)
        alone, _ = mc.host_fly(harness, cfg, plan[b:b + 1], 70, SEED, mc.SIGMA, **kw)
        assert alone[0].tobytes() == whole[b].tobytes()
        up_all = mc.host_update(harness, cfg, plan, whole, SEED, mc.SIGMA, 300.0, collision_cost=10.0, **host)
        up_one = mc.host_update(harness, cfg, plan[b:b + 1], whole[b:b + 1], SEED, mc.SIGMA, 300.0, collision_cost=10.0, **kw)
        assert up_one[0][0].tobytes() == up_all[0][b].tobytes() and up_one[1][0].tobytes() == up_all[1][b].tobytes()
    few, _ = mc.host_fly(harness, cfg, plan, 5, SEED, mc.SIGMA, **host)
    assert few.tobytes() == whole[:, :5].tobytes()


# ------------------------------------------------------------------------------------------------ 3. known answers, no restatement

def consistent_plan(cfg, plan):
    """the plans' controls rolled out from their knot 0 by the oracle's step: what forward_sim makes of them"""
    mdl = orc.model_params(**cfg["model"])
    out = np.array(plan)
    for b in range(out.shape[0]):
        for i in range(out.shape[1] - 1):
            out[b, i + 1, 1:14] = orc.discrete_step(mdl, 0, out[b, i, 1:14], out[b, i, 14:18], cfg["dt"])
    return out


def test_without_perturbations_every_sample_is_the_plan(harness, std):
    """sigma = 0.  EXACT: every sample's four score words are sample 0's; the update returns the plan's times and controls bit for bit
    (du = 0 / eta = 0 and u + 0 = u), and knot 0's state.  Within 1e-12 of the largest entry: the states of a consistent plan -- the
    library's step and the oracle's round differently."""
    cfg, plan, _ = std
    plan = consistent_plan(cfg, plan)
    score, eps = mc.host_fly(harness, cfg, plan, 70, SEED, 0.0)
    assert not eps.any() and (score == score[:, :1]).all()
    out, info = mc.host_update(harness, cfg, plan, score, SEED, 0.0, 5.0)
    assert out[:, :, 14:18].tobytes() == plan[:, :, 14:18].tobytes() and out[:, :, 0].tobytes() == plan[:, :, 0].tobytes()
    assert out[:, 0].tobytes() == plan[:, 0].tobytes()
    assert np.abs(out - plan).max() <= 1e-12 * np.abs(plan).max()
    assert np.array_equal(info[:, :4], np.stack([score[:, 0, 0], np.zeros(B), np.full(B, 70.0), np.full(B, 70.0)], axis=1))  # ties: the smaller sample
    assert info[:, 4:].tobytes() == score[:, 0].tobytes()  # the new plan is the old one: its own flight scores the same


def test_a_small_lambda_takes_the_best_sample_and_a_large_one_the_mean(harness, std):
    cfg, plan, x0 = std
    S = 70
    score, eps = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, x0=x0, tau_s=0.3)
    J = np.sort(score[..., 0], axis=1)
    lam = 1e-6
    assert ((J[:, 1] - J[:, 0]) / lam > 745).all()  # every other weight is exp(-x) with x > 745: 0 (asserted on the data)
    out, info = mc.host_update(harness, cfg, plan, score, SEED, mc.SIGMA, lam, x0=x0, tau_s=0.3)
    best = score[..., 0].argmin(axis=1)
    assert np.array_equal(info[:, 1], best) and np.array_equal(info[:, 0], J[:, 0]) and (info[:, 2] == 1.0).all()
    for b in range(B):  # EXACT: du = (1 eps_best + 0 + ...) / 1
        assert (out[b, :, 14:18] == plan[b, :, 14:18] + eps[b, best[b]]).all()
    # the new plan flies what the best sample flew: the same arithmetic on the same controls
    assert np.array_equal(info[:, 4:], score[np.arange(B), best])
    out, info = mc.host_update(harness, cfg, plan, score, SEED, mc.SIGMA, 1e300, x0=x0, tau_s=0.3)
    assert (info[:, 2] == S).all()  # every weight is 1
    bound = mp.update_bound(np.abs(eps).mean(axis=1), S, mc.SIGMA)
    assert (np.abs(out[:, :, 14:18] - (plan[:, :, 14:18] + eps.mean(axis=1))) <= bound).all()


def test_a_sample_that_diverged_has_no_weight(harness, std):
    cfg, plan, x0 = std
    S = 70
    score, eps = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, x0=x0)
    bad = np.array(score)
    best = score[..., 0].argmin(axis=1)
    bad[np.arange(B), best, 0] = np.nan
    bad[0, 3, 0] = np.inf
    out, info = mc.host_update(harness, cfg, plan, bad, SEED, mc.SIGMA, 200.0, x0=x0)
    u, info4, scale = mp.update(plan, bad, eps, 200.0)
    assert (np.abs(out[:, :, 14:18] - u) <= mp.update_bound(scale, S, mc.SIGMA)).all()
    assert np.array_equal(info[:, [0, 1, 3]], info4[:, [0, 1, 3]]) and (info[:, 1] != best).all() and info[:, 3].tolist() == [S - 2, S - 1, S - 1]
    # the samples without weight could hold anything: the update of the other 68 (69) alone, in their places, has the same bits
    junk = np.array(bad)
    junk[np.arange(B), best, 1:] = 7.0
    assert mc.host_update(harness, cfg, plan, junk, SEED, mc.SIGMA, 200.0, x0=x0)[0].tobytes() == out.tobytes()
    bad[..., 0] = np.nan
    out, info = mc.host_update(harness, cfg, plan, bad, SEED, mc.SIGMA, 200.0, x0=x0)
    assert out[:, :, 14:18].tobytes() == plan[:, :, 14:18].tobytes()  # the plan comes back
    assert np.isnan(info[:, 0]).all() and (info[:, 1] == -1).all() and not info[:, 2:4].any()


def test_with_the_nominal_sample_the_best_is_no_worse_than_the_plan(harness, full):
    host, _, cfg, plan, _, _ = full[70]
    flown, _ = mc.host_fly(harness, cfg, plan, 1, SEED, 0.0, **host)  # the old plan flown from x0
    score, eps = mc.host_fly(harness, cfg, plan, 70, SEED, mc.SIGMA, first_is_nominal=True, **host)
    assert score[:, 0].tobytes() == flown[:, 0].tobytes() and not eps[:, 0].any()
    _, info = mc.host_update(harness, cfg, plan, score, SEED, mc.SIGMA, 100.0, collision_cost=25.0, first_is_nominal=True, **host)
    assert (info[:, 0] <= mp.keys(flown, 25.0)[:, 0]).all()
    assert (info[:, 0] < mp.keys(flown, 25.0)[:, 0]).any()  # (and some perturbed sample is better)


# ------------------------------------------------------------------------------------------------ 4. it plans
PLANNED_COSTS = [[1103.3356740579316, 1116.5787116598904], [1078.1560065445262, 1094.8324776503189], [1065.9068692126941, 1074.1528140716182],
                 [1059.0967609057402, 1061.6905630291046]]


def test_it_plans(harness):
    """tests/mppi_cases.py's scenario: two vehicles hover at (0, 0, 0) and (0, 0.1, 0), the desired trajectory hovers at (1, 0, 0), two
    spheres of weight 100 stand between; S = 256, sigma 0.6 N, tau 0.4 s, lambda 20, collision cost 50, four rounds with seeds 5 .. 8.  The
    cost of the new plan's own flight (info word 4) after each round, recorded from the harness (x86-64, g++ -O2):
        round 1   1103.3356740579316   1116.5787116598904
        round 2   1078.1560065445262   1094.8324776503189
        round 3   1065.9068692126941   1074.1528140716182
        round 4   1059.0967609057402   1061.6905630291046
    from 1200 for the plans that hover where they are (12 knots x 100 x 1 m^2).  It decreases at every round, and the last plan has
    moved towards the goal."""
    plans, infos = mc.host_plan(harness)
    cost = infos[:, :, 4]
    print("[observed] nominal cost per round:", cost.tolist())
    assert (cost[0] < 1200.0).all() and (np.diff(cost, axis=0) < 0).all()
    np.testing.assert_allclose(cost, PLANNED_COSTS, rtol=1e-9)
    assert (plans[-1][:, -1, 1] > 0.3).all()
    cfg, plan, shared = mc.planning()
    hover, _ = mc.host_fly(harness, cfg, plan, 1, 0, 0.0, shared=shared)
    np.testing.assert_allclose(hover[:, 0, 0], [1200.0, 1212.0], rtol=1e-12)  # (12 knots x 100 x 1.01 m^2 for the second)


# ------------------------------------------------------------------------------------------------ 5. the update against the restatement

@pytest.mark.parametrize("S", [5, 70])
def test_the_update_against_the_restatement(harness, full, S):
    """over the harness's own scores, so that the flight's rounding is not in the comparison; the bound is tests/mppi_numpy.py's
    update_bound (4 ulp per weight in numerator and denominator, the product, one rounding per addition of the longest path, the quotient
    and the sum, doubled, times sum w |eps| / eta -- plus twice the draws' own bar)"""
    host, rest, cfg, plan, x0, eps = full[S]
    score, _ = mc.host_fly(harness, cfg, plan, S, SEED, mc.SIGMA, **host)
    for lam in (150.0, 500.0):
        out, info = mc.host_update(harness, cfg, plan, score, SEED, mc.SIGMA, lam, collision_cost=30.0, **host)
        u, info4, scale = mp.update(plan, score, eps, lam, 30.0, rest["limits"])
        bound = mp.update_bound(scale, S, mc.SIGMA)
        err = np.abs(out[:, :, 14:18] - u)
        print("[observed] S = %d, lambda = %g: control error %.3g of its bound; effective samples %s" % (S, lam, (err / bound).max(), info[:, 2].tolist()))
        assert (err <= bound).all()
        assert np.array_equal(info[:, [0, 1, 3]], info4[:, [0, 1, 3]])
        np.testing.assert_allclose(info[:, 2], info4[:, 2], rtol=1e-12)
        assert (info[:, 2] > 1.0).all() and (info[:, 2] < S).all()
        assert ((out[:, :, 14:18] >= rest["limits"][0]) & (out[:, :, 14:18] <= rest["limits"][1])).all()
        # the new plan's states are its controls flown from x0, and words 4 .. 7 that flight's score
        again, _ = mc.host_fly(harness, cfg, out, 1, SEED, 0.0, **host)
        assert again[:, 0].tobytes() == info[:, 4:].tobytes() and np.array_equal(out[:, 0, 1:14], x0)
        _, _, _, traj = mp.flight(out, x0, np.zeros((B, 1, N, 4)), cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], **rest)
        np.testing.assert_allclose(out, traj[:, 0], rtol=sn.RTOL, atol=sn.ATOL)


def test_the_grids(harness):
    grid = lambda S: [int(v) for v in subprocess.check_output([harness, "grid", str(S)]).split()]
    # blocks of a plan's flight, lanes of its update, samples per lane, and the same lanes by the rule the kernels are compiled with
    assert [grid(S) for S in (1, 5, 64, 65, 70, 130, 1024, 1025, 4096)] == [[1, 64, 1, 64], [1, 64, 1, 64], [1, 64, 1, 64], [2, 128, 1, 128], [2, 128, 1, 128],
                                                                             [3, 256, 1, 256], [16, 1024, 1, 1024], [17, 1024, 2, 1024], [64, 1024, 4, 1024]]


def test_the_harness_under_the_address_and_undefined_behaviour_sanitizers(full):
    """the stand-alone program, compiled and run once with -fsanitize=address,undefined: every operand of the score, limits, models, both
    integrators, the flight and the update"""
    exe = mc.build_harness(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "host_mppi_harness_san")
    host, _, cfg, plan, _, _ = full[70]
    for integrator in (0, 1):
        score, eps = mc.host_fly(exe, cfg, plan, 70, SEED, mc.SIGMA, integrator=integrator, first_is_nominal=True, **host)
        out, info = mc.host_update(exe, cfg, plan, score, SEED, mc.SIGMA, 100.0, collision_cost=5.0, integrator=integrator, first_is_nominal=True, **host)
        assert not np.isnan(score).any() and not np.isnan(eps).any() and not np.isnan(out).any() and not np.isnan(info).any()
    assert subprocess.check_output([exe, "refuse"] + [str(OK_CALL[k]) for k in ORDER]).decode().strip() == "ok"


# ------------------------------------------------------------------------------------------------ 6. what a call refuses
OK_CALL = dict(update=1, rule=1, sigma0=0.5, sigma1=0.5, sigma2=0.0, sigma3=0.5, tau_s=0.0, lambda_=1.0, collision_cost=0.0, flags=1, reserved=0, plan=4096,
               x0=65536, desired=131072, score=1 << 20, out_plan=1 << 21, info=1 << 22, B=2, n=4, S=3, b0=0, handle=1, f32=0, modeled=0, models_B=0, pobs_B=0,
               n_desired=10, n_sched=0, k0=0)
ORDER = tuple(OK_CALL)
# in the order of the rule (mppi_launch.h): every row is refused by its own reason, and by it still when every LATER row's fault is added
REFUSALS = [
    (dict(rule=0), "null argument"), (dict(plan=0), "null argument"), (dict(score=0), "null argument"), (dict(out_plan=0), "d_out_plan and d_info are needed"),
    (dict(info=0), "d_out_plan and d_info are needed"),
    (dict(B=0), "must be positive"), (dict(S=-1), "must be positive"), (dict(n=0), "must be positive"), (dict(n=1), "at least 2"),
    (dict(S=4097), "QILQR_RISK_MAX_SAMPLES"),
    (dict(b0=-1), "b0 must not be negative"),
    (dict(sigma2="nan"), "every sigma"), (dict(sigma0=-0.1), "every sigma"),
    (dict(lambda_=0.0), "lambda must be positive"), (dict(lambda_="nan"), "lambda must be positive"), (dict(lambda_=-1.0), "lambda must be positive"),
    (dict(tau_s=-1.0), "tau_s and collision_cost"), (dict(tau_s="nan"), "tau_s and collision_cost"), (dict(collision_cost=-1.0), "tau_s and collision_cost"),
    (dict(collision_cost="nan"), "tau_s and collision_cost"),
    (dict(flags=2), "unknown flag bits"), (dict(flags=3), "unknown flag bits"), (dict(reserved=1), "reserved word"),
    (dict(plan=4096 + 8), "16-byte aligned"), (dict(x0=65536 + 8), "16-byte aligned"), (dict(desired=131072 + 8), "16-byte aligned"),
    (dict(score=(1 << 20) + 8), "16-byte aligned"), (dict(out_plan=(1 << 21) + 8), "16-byte aligned"), (dict(info=(1 << 22) + 8), "16-byte aligned"),
    (dict(out_plan=4096 + 16), "d_out_plan overlaps an input"), (dict(out_plan=(1 << 20) + 16), "d_out_plan overlaps an input"),
    (dict(out_plan=65536 - 16), "d_out_plan overlaps an input"), (dict(out_plan=131072 + 8 * 18 * 8 - 16), "d_out_plan overlaps an input"),
    (dict(info=4096 + 32), "d_info overlaps an input"), (dict(info=(1 << 20) + 16), "d_info overlaps an input"), (dict(info=65536 + 16), "d_info overlaps an input"),
    (dict(info=(1 << 21) + 16), "d_info overlaps d_out_plan"),
    (dict(handle=0), "null handle"),
    (dict(f32=1), "precision 0"), (dict(modeled=1, models_B=6), "set for B plans"), (dict(pobs_B=3), "per-problem obstacles were set for another B"),
    (dict(desired=0, n_desired=3), "length: .*beyond the handle's desired trajectory"), (dict(desired=0, n_desired=10, k0=7), "length: .*desired trajectory"),
    (dict(n_sched=3), "length: .*beyond the state-weight schedule"), (dict(n_sched=10, k0=7), "length: .*schedule"),
]
ADMITTED = [dict(), dict(x0=0), dict(desired=0), dict(flags=0), dict(sigma0=0.0, sigma1=0.0, sigma3=0.0), dict(sigma1="inf"), dict(tau_s="inf"), dict(S=4096),
            dict(modeled=1, models_B=2), dict(pobs_B=2), dict(n_sched=4), dict(n_desired=0), dict(n_sched=11, k0=7, n_desired=11, desired=0),
            dict(out_plan=4096 + 8 * 18 * 8), dict(info=(1 << 21) + 8 * 18 * 8),
            dict(update=0, out_plan=0, info=0), dict(update=0, out_plan=8, info=8)]  # (the flight does not look at the update's outputs)
FLIGHT_REFUSALS = [(dict(score=4096 + 16), "d_score overlaps an input"), (dict(score=65536), "d_score overlaps an input"),
                   (dict(score=131072 + 32), "d_score overlaps an input"), (dict(score=0), "null argument"), (dict(handle=0), "null handle")]


def rule(exe, **change):
    call = dict(OK_CALL, **change)
    return subprocess.check_output([exe, "refuse"] + [str(call[k]) for k in ORDER]).decode().strip()


def test_the_rule_of_what_the_calls_refuse_and_its_order(harness):
    for change, why in REFUSALS:
        assert re.search(why, rule(harness, **change)), (change, rule(harness, **change))
    for change in ADMITTED:
        assert rule(harness, **change) == "ok", (change, rule(harness, **change))
    for change, why in FLIGHT_REFUSALS:
        assert re.search(why, rule(harness, update=0, **change)), (change, rule(harness, update=0, **change))
    # the order: a row's reason stands whatever comes later in the rule (every later row's fault added at once -- but for the missing
    # desired trajectory of the rows of length, which would take an overlap with it away)
    for k, (change, why) in enumerate(REFUSALS):
        later = {}
        for other, _ in REFUSALS[k + 1:]:
            later.update({key: v for key, v in other.items() if key not in change and key not in later and key != "desired"})
        got = rule(harness, **dict(later, **change))
        assert re.search(why, got), (change, later, got)


def test_the_abi_without_a_device():
    """the structure, the constants, and every refusal that needs no handle, through ctypes: the arguments are looked at before the
    handle, so a NULL handle is the last"""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi.MppiRule) == 64 and capi.MppiRule.lambda_.offset == 40 and capi.MppiRule.flags.offset == 56
    assert "#define QILQR_MPPI_INFO 8" in header and capi.MPPI_INFO == 8 and "#define QILQR_MPPI_FIRST_IS_NOMINAL 1u" in header
    assert lib.qilqr_abi_version() == 7 and "#define QILQR_ABI_VERSION 7" in header
    b, n, s = 2, 4, 3
    arrays = dict(plan=capi._d16(np.zeros((b, n, 18))), x0=capi._d16(np.zeros((b, 13))), desired=capi._d16(np.zeros((b, n, 18))),
                  score=capi._d16(np.zeros((b, s, 4))), out_plan=capi._d16(np.zeros((b, n, 18))), info=capi._d16(np.zeros((b, 8))))
    odd = capi._d16(np.zeros(b * n * 18 + 2))[1:]  # 8 bytes off a 16-byte boundary
    assert odd.ctypes.data % 16 == 8

    def call(update, rule=True, B=b, n_=n, S=s, b0=0, sigma=0.5, lambda_=1.0, tau_s=0.0, collision_cost=0.0, flags=1, reserved=0, **ptr):
        a = {k: (v.ctypes.data if v is not None else None) for k, v in dict(arrays, **ptr).items()}
        r = capi.MppiRule((C.c_double * 4)(sigma, 0.5, 0.5, 0.5), tau_s, lambda_, collision_cost, flags, reserved)
        rp = C.byref(r) if rule else None
        if update:
            rc = lib.qilqr_mppi_update_device(None, rp, 5, a["plan"], a["x0"], a["desired"], a["score"], B, n_, S, b0, a["out_plan"], a["info"])
        else:
            rc = lib.qilqr_mppi_flight_device(None, rp, 5, a["plan"], a["x0"], a["desired"], B, n_, S, b0, a["score"])
        return rc, lib.qilqr_last_error().decode()

    both = [(dict(rule=False), "null argument"), (dict(plan=None), "null argument"), (dict(score=None), "null argument"), (dict(B=0), "must be positive"),
            (dict(n_=1), "at least 2"), (dict(S=4097), "QILQR_RISK_MAX_SAMPLES"), (dict(b0=-1), "b0 must not"), (dict(sigma=float("nan")), "every sigma"),
            (dict(sigma=-1.0), "every sigma"), (dict(lambda_=0.0), "lambda must be positive"), (dict(lambda_=float("nan")), "lambda must be positive"),
            (dict(tau_s=-0.1), "tau_s and collision_cost"), (dict(collision_cost=float("nan")), "tau_s and collision_cost"), (dict(flags=4), "unknown flag bits"),
            (dict(reserved=9), "reserved word"), (dict(plan=odd), "16-byte aligned"), (dict(x0=odd), "16-byte aligned"), (dict(desired=odd), "16-byte aligned"),
            (dict(score=odd), "16-byte aligned"), (dict(), "null handle"), (dict(x0=None, desired=None), "null handle")]
    for change, why in both + [(dict(score=arrays["plan"]), "d_score overlaps an input"), (dict(score=arrays["x0"]), "d_score overlaps an input")]:
        rc, text = call(False, **change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)
    for change, why in both + [(dict(out_plan=None), "d_out_plan and d_info"), (dict(info=None), "d_out_plan and d_info"), (dict(out_plan=odd), "16-byte aligned"),
                               (dict(info=odd), "16-byte aligned"), (dict(out_plan=arrays["plan"]), "d_out_plan overlaps an input"),
                               (dict(out_plan=arrays["score"]), "d_out_plan overlaps an input"), (dict(info=arrays["score"]), "d_info overlaps an input"),
                               (dict(info=arrays["out_plan"]), "d_info overlaps d_out_plan")]:
        rc, text = call(True, **change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)


# ------------------------------------------------------------------------------------------------ 7. the kernels of the unit, by name

@pytest.mark.parametrize("defines", [[], ["-DQILQR_DIAG"]])
def test_the_kernels_of_the_unit_are_the_listed_ones(defines):
    """tests/test_kernel_symbols_cpu.py's check for mppi.hip, against the lists at the top of this file (that test's own table is closed)"""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
    asm = subprocess.check_output([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + defines +
                                  ["-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, "mppi.hip")], stderr=subprocess.DEVNULL).decode()
    got = sorted({line.split()[1] for line in asm.splitlines() if line.lstrip().startswith(".amdhsa_kernel ")})
    assert got == sorted(FLIGHT_KERNELS + UPDATE_KERNELS), got
    with open(os.path.join(csrc, "Makefile")) as f:
        assert any(ln.startswith("SRCS") and "mppi.hip" in ln.split() for ln in f)
