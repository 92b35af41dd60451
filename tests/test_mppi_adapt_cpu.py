"""The planner's adapted spread without a device: the per-lane routines of quadrotorilqr_amd/csrc/mppi_adapt_kernels.h and the rule of
mppi_adapt_launch.h, compiled with g++ into the stand-alone program tests/host_mppi_adapt_harness.cpp, against the restatement
(tests/mppi_adapt_numpy.py), against answers known without one -- the existing flight's and update's bits through tests/host_mppi_harness.cpp
among them -- and against themselves; the refusals through the harness and through the C ABI; the kernels of mppi_adapt.hip by name.
B = 3, n = 12, S = 5 and 70, with tests/mppi_cases.py's spheres, schedule at horizon start 3, limits and per-plan models."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from quadrotorilqr_amd import capi
from tests import mppi_adapt_cases as ac, mppi_adapt_numpy as ma, mppi_cases as mc, mppi_numpy as mp, scored_flight_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = mc.B, mc.N
SEED = 77
NEW_SYMBOLS = ("qilqr_mppi_flight_spread_device", "qilqr_mppi_adapt_device")
# the kernels of mppi_adapt.hip: the flight's {Euler, Runge-Kutta} x {neither, limits, models, both}, the adaptation's five block sizes
FLIGHT_KERNELS = ["_ZN5qilqr20k_mppi_flight_spreadILi%dEJ%sEEEvNS_11ModelConstsIdEENS_20MppiFlightSpreadArgsEDpT0_" % (i, e)
                  for i in (0, 1) for e in ("", "NS_13ControlLimitsE", "NS_11BatchModelsE", "NS_13ControlLimitsENS_11BatchModelsE")]
ADAPT_KERNELS = ["_ZN5qilqr12k_mppi_adaptILi%dEEEvNS_13MppiAdaptArgsE" % t for t in (64, 128, 256, 512, 1024)]


@pytest.fixture(scope="module")
def harness():
    return ac.build_harness(["-O2"], "host_mppi_adapt_harness")


@pytest.fixture(scope="module")
def old_harness():
    return mc.build_harness(["-O2"], "host_mppi_harness")


@pytest.fixture(scope="module")
def std():
    return mc.standard()


@pytest.fixture(scope="module")
def full():
    """S -> (host keywords, restatement keywords, cfg, plan, x0, spread, the restatement's eps): computed once per S, never written to"""
    return {S: ac.everything(S, SEED) for S in (5, 70)}


# ------------------------------------------------------------------------------------------------ 1. the perturbations

@pytest.mark.parametrize("tau_s", [0.0, 0.3])
def test_the_perturbations_against_the_restatement(harness, std, tau_s):
    cfg, plan, _ = std
    spread = ac.spread_field()
    _, eps = ac.host_fly(harness, cfg, plan, 70, SEED, spread, tau_s=tau_s, b0=4)
    want = ma.perturbations(SEED, spread, 70, cfg["dt"], tau_s=tau_s, b0=4)
    err = np.abs(eps - want).max()
    print("[observed] tau_s = %g: perturbation error %.3g of its bar %.3g" % (tau_s, err, ma.eps_atol(spread)))
    assert err <= ma.eps_atol(spread)
    assert len(np.unique(spread)) > 20  # (the spread varies by plan, knot and rotor)
    _, flagged = ac.host_fly(harness, cfg, plan, 70, SEED, spread, tau_s=tau_s, b0=4, first_is_nominal=True)
    assert not flagged[:, 0].any() and flagged[:, 1:].tobytes() == eps[:, 1:].tobytes()


# ------------------------------------------------------------------------------------------------ 2. the flight

@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("S", [5, 70])
def test_the_flight_against_the_restatement(harness, full, S, integrator):
    host, rest, cfg, plan, x0, spread, eps = full[S]
    want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], integrator=integrator, **rest)
    label = str((S, integrator))
    assert np.isfinite(want).all(), label
    assert gap > 1e-6, (label, gap)  # no control within the bar of a limit: the clamp cannot flip
    got, got_eps = ac.host_fly(harness, cfg, plan, S, SEED, spread, integrator=integrator, **host)
    assert np.abs(got_eps - eps).max() <= ma.eps_atol(spread), label
    zero_gap, zero = sn.margins(clear)
    assert zero_gap > 1e-6 and zero > 1e-6, label
    print("[observed] %s: cost error over its bar %.3g" % (label, (np.abs(got[..., 0] - want[..., 0]) / (sn.ATOL + sn.RTOL * np.abs(want[..., 0]))).max()))
    np.testing.assert_allclose(got[..., :2], want[..., :2], rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
    assert np.array_equal(got[..., 2:], want[..., 2:]), label
    u = plan[:, None, :, 14:18] + eps
    assert ((u < rest["limits"][0]) | (u > rest["limits"][1])).any() and (got[..., 3] > 0).any() and (got[..., 3] == 0).any(), label


# ------------------------------------------------------------------------------------------------ 3. known answers, no restatement

@pytest.mark.parametrize("integrator", [0, 1])
def test_a_constant_spread_without_correlation_is_the_existing_planner(harness, old_harness, full, integrator):
    """tau_s = 0 and spread = sigma at every knot.  EXACT: kappa_a = sigma_a and fma(0, g, k) = k, so eps, the flight's score, the new
    controls, the new states and info have the bits of the existing flight and update (tests/host_mppi_harness.cpp)."""
    host, _, cfg, plan, _, _, _ = full[70]
    host = dict(host, tau_s=0.0, integrator=integrator, first_is_nominal=True)
    want_score, want_eps = mc.host_fly(old_harness, cfg, plan, 70, SEED, mc.SIGMA, **host)
    got_score, got_eps = ac.host_fly(harness, cfg, plan, 70, SEED, ac.constant_spread(mc.SIGMA), **host)
    assert got_eps.tobytes() == want_eps.tobytes() and got_score.tobytes() == want_score.tobytes()
    want_plan, want_info = mc.host_update(old_harness, cfg, plan, want_score, SEED, mc.SIGMA, 150.0, collision_cost=30.0, **host)
    got_plan, got_info, spread, _ = ac.host_adapt(harness, cfg, plan, got_score, SEED, ac.constant_spread(mc.SIGMA), 150.0, collision_cost=30.0, **host)
    assert got_plan.tobytes() == want_plan.tobytes() and got_info.tobytes() == want_info.tobytes()
    assert (spread != mc.SIGMA).any() and ((spread >= ac.FLOOR) & (spread <= ac.CAP)).all()


def test_only_the_best_sample_weighs_and_the_spread_is_the_floor(harness, std):
    """(J_second - J_min) / lambda > 745: every other weight is 0, m1 = eps_best, m2 = eps_best^2, eta = 1 and var = e2 - du du = 0
    EXACTLY; with rate = 1 the blended variance is 0 and the new spread the floor."""
    cfg, plan, x0 = std
    spread = ac.spread_field()
    score, eps = ac.host_fly(harness, cfg, plan, 70, SEED, spread, x0=x0, tau_s=0.3)
    J = np.sort(score[..., 0], axis=1)
    lam = 1e-6
    assert ((J[:, 1] - J[:, 0]) / lam > 745).all()
    out, info, new, var = ac.host_adapt(harness, cfg, plan, score, SEED, spread, lam, rate=1.0, x0=x0, tau_s=0.3)
    best = score[..., 0].argmin(axis=1)
    assert np.array_equal(info[:, 1], best) and (info[:, 2] == 1.0).all()
    assert not var.any() and (new == ac.FLOOR).all()
    for b in range(B):
        assert (out[b, :, 14:18] == plan[b, :, 14:18] + eps[b, best[b]]).all()
    # with rate < 1 the old variance is kept in part: sqrt((1 - rate) s^2), two roundings and the root
    _, _, half, _ = ac.host_adapt(harness, cfg, plan, score, SEED, spread, lam, rate=0.5, floor=0.0, cap=10.0, x0=x0, tau_s=0.3)
    np.testing.assert_allclose(half, np.sqrt(0.5) * spread, rtol=4 * ma.EPS)


def test_without_a_finite_key_plan_and_spread_come_back(harness, std):
    cfg, plan, x0 = std
    spread = ac.spread_field()
    score, _ = ac.host_fly(harness, cfg, plan, 70, SEED, spread, x0=x0)
    bad = np.array(score)
    bad[1:, :, 0] = np.nan
    out, info, new, _ = ac.host_adapt(harness, cfg, plan, bad, SEED, spread, 100.0, x0=x0)
    assert out[1:, :, 14:18].tobytes() == plan[1:, :, 14:18].tobytes() and new[1:].tobytes() == spread[1:].tobytes()
    assert (new[0] != spread[0]).any() and (out[0, :, 14:18] != plan[0, :, 14:18]).any()
    assert np.isnan(info[1:, 0]).all() and (info[1:, 1] == -1).all() and not info[1:, 2:4].any()


def test_the_population_variance_of_four_thousand_normals(harness, std):
    """S = 4096, n = 6, lambda = 1e300 (every weight is 1), rate = 1, tau_s = 0, no nominal sample: the weighted variance is the
    population variance of S normals times s^2, whose relative deviation from s^2 has standard deviation sqrt(2 / S) = 0.022: five sigma."""
    cfg, plan, x0 = std
    s = 0.37
    plan6 = np.ascontiguousarray(plan[:, :6])
    spread = ac.constant_spread(s, B, 6)
    score, eps = ac.host_fly(harness, cfg, plan6, 4096, SEED, spread, x0=x0)
    assert np.isfinite(score[..., 0]).all()
    out, info, new, var = ac.host_adapt(harness, cfg, plan6, score, SEED, spread, 1e300, floor=0.0, cap=10.0, rate=1.0, x0=x0)
    assert (info[:, 2] == 4096).all()
    print("[observed] var / s^2 - 1: largest %.3g" % np.abs(var / s ** 2 - 1.0).max())
    assert (np.abs(var / s ** 2 - 1.0) < 0.11).all()
    # du is the plain mean and var the population variance of the eps
    np.testing.assert_allclose(out[:, :, 14:18], plan6[:, :, 14:18] + eps.mean(axis=1), rtol=0, atol=1e-13)
    np.testing.assert_allclose(var, eps.var(axis=1), rtol=1e-11)
    np.testing.assert_allclose(new, np.sqrt(var), rtol=4 * ma.EPS)


# ------------------------------------------------------------------------------------------------ 4. the adaptation against the restatement

@pytest.mark.parametrize("S", [5, 70])
def test_the_adaptation_against_the_restatement(harness, full, S):
    """over the harness's own scores; controls within tests/mppi_numpy.py's update_bound, variances within var_bound, spreads within
    adapt_bound / (s_dev + s_ref) (tests/mppi_adapt_numpy.py)"""
    host, rest, cfg, plan, x0, spread, eps = full[S]
    score, _ = ac.host_fly(harness, cfg, plan, S, SEED, spread, **host)
    for lam in (150.0, 500.0):
        out, info, new, var = ac.host_adapt(harness, cfg, plan, score, SEED, spread, lam, collision_cost=30.0, **host)
        want = ma.adapt(plan, score, eps, spread, lam, ac.FLOOR, ac.CAP, ac.RATE, 30.0, rest["limits"])
        err = np.abs(out[:, :, 14:18] - want["u"])
        assert (err <= mp.update_bound(want["scale"], S, spread)).all()
        assert np.array_equal(info[:, [0, 1, 3]], want["info"][:, [0, 1, 3]])
        vb = ma.var_bound(want["scale"], want["scale2"], S, spread)
        verr = np.abs(var - want["var"])
        assert (verr <= vb).all(), (verr / vb).max()
        worst, near, either = ac.compare_spreads(new, want, ma.adapt_bound(want["scale"], want["scale2"], S, spread, want["v"], ac.RATE))
        print("[observed] S = %d, lambda = %g: control error %.3g, variance error %.3g, spread error %.3g of their bounds; %.3g of the entries near floor or cap"
              % (S, lam, (err / mp.update_bound(want["scale"], S, spread)).max(), (verr / vb).max(), worst, near))
        assert worst <= 1.0 and either and near <= 0.05
        assert ((want["raw"] > ac.FLOOR) & (want["raw"] < ac.CAP)).all()  # floor and cap: the restatement alone stays inside
        assert (new != spread).all()
        # the new plan's states are its controls flown from x0, and words 4 .. 7 that flight's score
        again, _ = ac.host_fly(harness, cfg, out, 1, SEED, ac.constant_spread(0.0), **host)
        assert again[:, 0].tobytes() == info[:, 4:].tobytes() and np.array_equal(out[:, 0, 1:14], x0)


def test_floor_and_cap_clamp(harness, full):
    host, rest, cfg, plan, x0, spread, eps = full[70]
    score, _ = ac.host_fly(harness, cfg, plan, 70, SEED, spread, **host)
    want = ma.adapt(plan, score, eps, spread, 150.0, 0.0, 10.0, ac.RATE, 30.0, rest["limits"])
    floor, cap = np.percentile(want["raw"], 30), np.percentile(want["raw"], 70)
    _, _, new, _ = ac.host_adapt(harness, cfg, plan, score, SEED, spread, 150.0, floor=floor, cap=cap, collision_cost=30.0, **host)
    want = ma.adapt(plan, score, eps, spread, 150.0, floor, cap, ac.RATE, 30.0, rest["limits"])
    assert (new >= floor).all() and (new <= cap).all() and (new == floor).any() and (new == cap).any()
    worst, near, either = ac.compare_spreads(new, want, ma.adapt_bound(want["scale"], want["scale2"], 70, spread, want["v"], ac.RATE))
    assert worst <= 1.0 and either and near <= 0.05


def test_a_plans_bits_do_not_depend_on_the_batch(harness, full):
    host, _, cfg, plan, x0, spread, _ = full[70]
    whole, _ = ac.host_fly(harness, cfg, plan, 70, SEED, spread, **host)
    up_all = ac.host_adapt(harness, cfg, plan, whole, SEED, spread, 300.0, collision_cost=10.0, **host)
    for b in (0, B - 1):
        kw = dict(host, x0=x0[b:b + 1], models=mc.MODELS3[b:b + 1], own=host["own"][b:b + 1], counts=host["counts"][b:b + 1], b0=b)
        alone, _ = ac.host_fly(harness, cfg, plan[b:b + 1], 70, SEED, spread[b:b + 1], **kw)
        assert alone[0].tobytes() == whole[b].tobytes()
        up_one = ac.host_adapt(harness, cfg, plan[b:b + 1], whole[b:b + 1], SEED, spread[b:b + 1], 300.0, collision_cost=10.0, **kw)
        for one, every in zip(up_one, up_all):
            assert one[0].tobytes() == every[b].tobytes()


def test_the_planning_scenario_with_the_spread_adapted(harness, old_harness):
    """tests/test_mppi_cpu.py::test_it_plans' scenario with and without adaptation (rate 0.5, floor 0.05 N, cap 2 N) at equal seeds: the
    cost of the new plan's own flight after each round.  A FINDING, recorded in DESIGN.md section 8p, not an assertion of which is lower:
    asserted is only that the adapted rounds plan at all (below the hover plans' 1200 and 1212) and that the spread has moved."""
    _, infos, spreads = ac.host_plan(harness)
    _, plain = mc.host_plan(old_harness)
    print("[observed] nominal cost per round, adapted:", infos[:, :, 4].tolist())
    print("[observed] nominal cost per round, fixed sigma:", plain[:, :, 4].tolist())
    print("[observed] mean spread per knot after the last round:", spreads[-1].mean(axis=(0, 2)).round(3).tolist())
    assert np.isfinite(infos).all() and (infos[:, :, 4] < [1200.0, 1212.0]).all()
    assert (spreads[-1] != mc.PLAN_RULE["sigma"]).any() and (spreads >= 0.05).all() and (spreads <= 2.0).all()


def test_the_harness_under_the_address_and_undefined_behaviour_sanitizers(full):
    """the stand-alone program, compiled and run once with -fsanitize=address,undefined: both integrators, the flight and the adaptation"""
    exe = ac.build_harness(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "host_mppi_adapt_harness_san")
    host, _, cfg, plan, _, spread, _ = full[70]
    for integrator in (0, 1):
        score, eps = ac.host_fly(exe, cfg, plan, 70, SEED, spread, integrator=integrator, first_is_nominal=True, **host)
        outs = ac.host_adapt(exe, cfg, plan, score, SEED, spread, 100.0, collision_cost=5.0, integrator=integrator, first_is_nominal=True, **host)
        assert not np.isnan(score).any() and not np.isnan(eps).any() and not any(np.isnan(o).any() for o in outs)
    assert rule(exe) == "ok"


# ------------------------------------------------------------------------------------------------ 5. what a call refuses
OK_CALL = dict(update=1, rule=1, sigma0=0.5, sigma1=0.5, sigma2=0.0, sigma3=0.5, tau_s=0.0, lambda_=1.0, collision_cost=0.0, flags=1, reserved=0, plan=4096,
               x0=65536, desired=131072, score=1 << 20, out_plan=1 << 21, info=1 << 22, B=2, n=4, S=3, b0=0, handle=1, f32=0, modeled=0, models_B=0, pobs_B=0,
               n_desired=10, n_sched=0, k0=0, adapt=1, floor0=0.1, cap0=1.0, rate=0.5, areserved=0.0, spread=1 << 23, out_spread=1 << 24)
ORDER = tuple(OK_CALL)
SPREAD_BYTES = 2 * 4 * 4 * 8
# in the order of the rule (mppi_adapt_launch.h): the last of mppi_launch.h's argument rows, the new rows, then the handle's
REFUSALS = [
    (dict(info=(1 << 21) + 16), "d_info overlaps d_out_plan"),
    (dict(spread=0), "d_spread is needed"), (dict(adapt=0), "the adapt rule is needed"),
    (dict(floor0="nan"), "every floor"), (dict(floor0=-0.1), "every floor"),
    (dict(cap0="nan"), "every cap"), (dict(cap0="inf"), "every cap"), (dict(cap0=0.05), "every cap"),
    (dict(rate=0.0), "rate must lie"), (dict(rate=1.5), "rate must lie"), (dict(rate="nan"), "rate must lie"),
    (dict(areserved=1.0), "reserved words"),
    (dict(spread=(1 << 23) + 8), "16-byte aligned"), (dict(out_spread=(1 << 24) + 8), "16-byte aligned"),
    (dict(out_spread=4096 + 16), "d_out_spread overlaps an input"), (dict(out_spread=(1 << 20) + 16), "d_out_spread overlaps an input"),
    (dict(out_spread=(1 << 23) + 16), "d_out_spread overlaps an input"), (dict(out_spread=1 << 23), "d_out_spread overlaps an input"),
    (dict(out_spread=(1 << 21) + 32), "d_out_spread overlaps d_out_plan or d_info"), (dict(out_spread=(1 << 22) + 16), "d_out_spread overlaps d_out_plan or d_info"),
    (dict(spread=(1 << 21) + 64), "d_out_plan or d_info overlaps d_spread"), (dict(spread=(1 << 22) + 16), "d_out_plan or d_info overlaps d_spread"),
    (dict(handle=0), "null handle"),
    (dict(f32=1), "precision 0"), (dict(modeled=1, models_B=6), "set for B plans"), (dict(pobs_B=3), "per-problem obstacles were set for another B"),
    (dict(desired=0, n_desired=3), "length: .*beyond the handle's desired trajectory"), (dict(n_sched=3), "length: .*beyond the state-weight schedule"),
]
ADMITTED = [dict(), dict(out_spread=0), dict(rate=1.0), dict(floor0=0.0), dict(floor0=1.0), dict(out_spread=(1 << 23) + SPREAD_BYTES),
            dict(update=0, adapt=0, out_plan=0, info=0, out_spread=0), dict(update=0, adapt=0, floor0="nan", rate=7.0, areserved=3.0, out_spread=8)]
FLIGHT_REFUSALS = [(dict(spread=0), "d_spread is needed"), (dict(spread=(1 << 23) + 8), "16-byte aligned"), (dict(score=(1 << 23) + 16), "d_score overlaps d_spread"),
                   (dict(score=4096 + 16), "d_score overlaps an input"), (dict(handle=0), "null handle")]


def rule(exe, **change):
    call = dict(OK_CALL, **change)
    return subprocess.check_output([exe, "refuse"] + [str(call[k]) for k in ORDER]).decode().strip()


def test_the_rule_of_what_the_calls_refuse_and_its_order(harness, old_harness):
    for change, why in REFUSALS:
        assert re.search(why, rule(harness, **change)), (change, rule(harness, **change))
    for change in ADMITTED:
        assert rule(harness, **change) == "ok", (change, rule(harness, **change))
    for change, why in FLIGHT_REFUSALS:
        got = rule(harness, **dict(dict(update=0, adapt=0, out_plan=0, info=0, out_spread=0), **change))
        assert re.search(why, got), (change, got)
    # the common arguments: mppi_launch.h's rule, its order and its texts -- every row of tests/test_mppi_cpu.py's table but the handle's
    from tests import test_mppi_cpu as old
    for change, why in old.REFUSALS:
        if "handle" in change or why.startswith("length") or set(change) & {"f32", "modeled", "pobs_B"}:
            continue
        base = [str(dict(old.OK_CALL, **change)[k]) for k in old.ORDER]
        want = subprocess.check_output([old_harness, "refuse"] + base).decode().strip()
        # ... and it stands before every new row's fault, a missing handle among them
        later = dict(spread=0, adapt=0, floor0="nan", cap0="nan", rate=0.0, areserved=1.0, handle=0)
        got = rule(harness, **dict(later, **change))
        assert got == want and re.search(why, got), (change, got, want)
    # the order: a row's reason stands with every later row's fault added at once (but for the pointers a later row moves: a moved
    # pointer would take this row's own overlap or misalignment away -- and the missing desired trajectory of the rows of length)
    for k, (change, why) in enumerate(REFUSALS):
        later = {}
        for other, _ in REFUSALS[k + 1:]:
            later.update({key: v for key, v in other.items() if key not in change and key not in later and key not in ("desired", "spread", "out_spread")})
        got = rule(harness, **dict(later, **change))
        assert re.search(why, got), (change, later, got)


def test_the_abi_without_a_device():
    """the structure and every refusal that needs no handle, through ctypes: the arguments are looked at before the handle"""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi.MppiAdaptRule) == 96 and capi.MppiAdaptRule.cap.offset == 32 and capi.MppiAdaptRule.rate.offset == 64
    assert "} qilqr_mppi_adapt_rule;" in header and lib.qilqr_abi_version() == 7 and "#define QILQR_ABI_VERSION 7" in header
    r = capi.mppi_adapt_rule(0.1, [1.0, 2.0, 3.0, 4.0], 0.25)
    assert list(r.floor) == [0.1] * 4 and list(r.cap) == [1.0, 2.0, 3.0, 4.0] and r.rate == 0.25 and list(r.reserved) == [0.0] * 3
    b, n, s = 2, 4, 3
    arrays = dict(plan=capi._d16(np.zeros((b, n, 18))), x0=capi._d16(np.zeros((b, 13))), desired=capi._d16(np.zeros((b, n, 18))),
                  score=capi._d16(np.zeros((b, s, 4))), out_plan=capi._d16(np.zeros((b, n, 18))), info=capi._d16(np.zeros((b, 8))),
                  spread=capi._d16(np.zeros((b, n, 4))), out_spread=capi._d16(np.zeros((b, n, 4))))
    odd = capi._d16(np.zeros(b * n * 18 + 2))[1:]
    assert odd.ctypes.data % 16 == 8

    def call(adapting, adapt=True, sigma=0.5, lambda_=1.0, floor=0.1, cap=1.0, rate=0.5, reserved=0.0, B=b, **ptr):
        a = {k: (v.ctypes.data if v is not None else None) for k, v in dict(arrays, **ptr).items()}
        r = capi.MppiRule((C.c_double * 4)(sigma, 0.5, 0.5, 0.5), 0.0, lambda_, 0.0, 1, 0)
        ad = capi.MppiAdaptRule((C.c_double * 4)(floor, 0.1, 0.1, 0.1), (C.c_double * 4)(cap, 1.0, 1.0, 1.0), rate, (C.c_double * 3)(0.0, reserved, 0.0))
        if adapting:
            rc = lib.qilqr_mppi_adapt_device(None, C.byref(r), C.byref(ad) if adapt else None, 5, a["plan"], a["x0"], a["desired"], a["spread"], a["score"],
                                             B, n, s, 0, a["out_plan"], a["out_spread"], a["info"])
        else:
            rc = lib.qilqr_mppi_flight_spread_device(None, C.byref(r), 5, a["plan"], a["x0"], a["desired"], a["spread"], B, n, s, 0, a["score"])
        return rc, lib.qilqr_last_error().decode()

    both = [(dict(plan=None), "null argument"), (dict(B=0), "must be positive"), (dict(sigma=-1.0), "every sigma"), (dict(lambda_=0.0), "lambda must be positive"),
            (dict(plan=odd), "16-byte aligned"), (dict(spread=None), "d_spread is needed"), (dict(spread=odd), "d_spread and d_out_spread"), (dict(), "null handle")]
    for change, why in both + [(dict(score=arrays["plan"]), "d_score overlaps an input"), (dict(score=arrays["spread"]), "d_score overlaps d_spread")]:
        rc, text = call(False, **change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)
    for change, why in both + [(dict(adapt=False), "the adapt rule is needed"), (dict(floor=-1.0), "every floor"), (dict(floor=float("nan")), "every floor"),
                               (dict(cap=float("inf")), "every cap"), (dict(cap=0.01), "every cap"), (dict(rate=0.0), "rate must lie"), (dict(rate=1.01), "rate must lie"),
                               (dict(reserved=2.0), "reserved words"), (dict(out_spread=odd), "d_spread and d_out_spread"),
                               (dict(out_spread=arrays["spread"]), "d_out_spread overlaps an input"), (dict(out_spread=arrays["score"]), "d_out_spread overlaps an input"),
                               (dict(out_spread=arrays["info"]), "d_out_spread overlaps d_out_plan or d_info"),
                               (dict(spread=arrays["out_plan"]), "d_out_plan or d_info overlaps d_spread"), (dict(out_spread=None), "null handle")]:
        rc, text = call(True, **change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)


# ------------------------------------------------------------------------------------------------ 6. the kernels of the unit, by name

@pytest.mark.parametrize("defines", [[], ["-DQILQR_DIAG"]])
def test_the_kernels_of_the_unit_are_the_listed_ones(defines):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
    asm = subprocess.check_output([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + defines +
                                  ["-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, "mppi_adapt.hip")], stderr=subprocess.DEVNULL).decode()
    got = sorted({line.split()[1] for line in asm.splitlines() if line.lstrip().startswith(".amdhsa_kernel ")})
    assert got == sorted(FLIGHT_KERNELS + ADAPT_KERNELS), got
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "SRCS    += mppi_adapt.hip\n" in f.readlines()
