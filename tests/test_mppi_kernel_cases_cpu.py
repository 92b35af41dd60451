"""What tests/test_gpu_mppi_kernel_cases.py stands on, without a device.  The cases of tests/mppi_kernel_cases.py are the kernels of the
sampling planner: mppi.hip and mppi_adapt.hip cross-compiled to device assembly (the command and the keep-while-fresh files of
tests/test_kernel_symbols_cpu.py) hold 13 + 13 kernels, every one named by exactly one case, and the S of each block-size case takes its
block size by the rule the launches use (mppi_update_lanes, through tests/host_mppi_harness.cpp's `grid`).  The host programs -- the
device's comparands -- against the restatement at sample counts where their own many-wavefront and several-per-lane folds run.  And every
placement the GPU tests rely on, asserted on the restatement, so that a seed that stops satisfying one fails here and not on the device."""
import subprocess

import numpy as np
import pytest

from tests import closed_loop_cases as cc, mppi_adapt_cases as ac, mppi_adapt_numpy as ma, mppi_cases as mc, mppi_kernel_cases as kc
from tests import mppi_numpy as mp, scored_flight_numpy as sn
from tests.test_kernel_symbols_cpu import kernel_symbols

SEED = kc.SEED


@pytest.fixture(scope="module")
def harnesses():
    return mc.build_harness(["-O2"], "host_mppi_harness"), ac.build_harness(["-O2"], "host_mppi_adapt_harness")


# ------------------------------------------------------------------------------------------------ 1. the cases are the kernels

def test_the_cases_are_the_kernels_one_to_one(harnesses):
    built = {unit: kernel_symbols("product", [], unit) for unit in ("mppi", "mppi_adapt")}
    assert len(built["mppi"]) == 13 and len(built["mppi_adapt"]) == 13
    kernels = set(built["mppi"]) | set(built["mppi_adapt"])
    named = [kc.kernel_name(c) for c in kc.CASES]
    assert len(kc.CASES) == len(set(kc.CASES)) == len(set(named)) == len({kc.name(c) for c in kc.CASES}) == 26
    assert set(named) == kernels, {"built and named by no case": sorted(kernels - set(named)), "named and not built": sorted(set(named) - kernels)}
    for c in kc.CASES:
        assert kc.kernel_name(c) in built[kc.unit(c)], kc.name(c)
    # the shapes: 8 + 8 flights, {Euler, Runge-Kutta} x {plain, limits, models, both}, the eight of a unit flying every horizon of KNOT_ENDS
    for spread in (False, True):
        mine = [c for c in kc.FLIGHTS if c.spread == spread]
        assert sorted((c.integrator, c.ext) for c in mine) == sorted((i, e) for i in (0, 1) for e in kc.EXTS)
        assert {c.n for c in mine} == set(kc.KNOT_ENDS) == {2, 8, 9, 16, 17} and {c.S for c in mine} == {70}
    # 5 + 5 block sizes, each with the S that selects it: the rule of the launches, compiled for the host
    assert [(c.adapt, c.threads, c.S) for c in kc.BLOCKS] == [(a, t, s) for a in (False, True) for t, s in ((64, 64), (128, 100), (256, 200), (512, 300), (1024, 1025))]
    for c in kc.BLOCKS:
        blocks, lanes, per_lane, compiled = (int(v) for v in subprocess.check_output([harnesses[0], "grid", str(c.S)]).split())
        assert lanes == compiled == c.threads == mp.update_lanes(c.S) and per_lane == -(-c.S // c.threads), kc.name(c)
    for S in kc.RAGGED:  # more than one sample a lane, the last sweep partly filled
        _, lanes, per_lane, _ = (int(v) for v in subprocess.check_output([harnesses[0], "grid", str(S)]).split())
        assert lanes == 1024 and per_lane == -(-S // 1024) >= 2 and S % 1024 != 0


def test_the_diagnostics_build_holds_the_same_kernels():
    for unit in ("mppi", "mppi_adapt"):
        assert kernel_symbols("diag", ["-DQILQR_DIAG"], unit) == kernel_symbols("product", [], unit)


# ------------------------------------------------------------------------------------------------ 2. the host programs at the new sample counts

@pytest.mark.parametrize("S", [200, 300, 1025, 2500, 4095])
def test_the_host_programs_against_the_restatement_at_more_samples(harnesses, S):
    """tests/test_mppi_cpu.py and tests/test_mppi_adapt_cpu.py compare at S = 5 and 70: one and two wavefronts, a sample a lane.  Here the
    host programs' folds over 4, 8 and 16 wavefronts and over 2, 3 and 4 samples a lane -- the last sweep partly filled -- with those
    files' bars.  mc.everything(S, 77): B = 3, n = 12, lambda 400, collision cost 30."""
    host, rest, cfg, plan, x0, spread, eps_spread = ac.everything(S, SEED)
    eps = mp.perturbations(SEED, mc.B, S, mc.N, cfg["dt"], mc.SIGMA, tau_s=kc.TAU_S)
    score, _ = mc.host_fly(harnesses[0], cfg, plan, S, SEED, mc.SIGMA, **host)
    out, info = mc.host_update(harnesses[0], cfg, plan, score, SEED, mc.SIGMA, kc.LAMBDA, collision_cost=kc.COLLISION_COST, **host)
    u, info4, scale = mp.update(plan, score, eps, kc.LAMBDA, kc.COLLISION_COST, rest["limits"])
    bound = mp.update_bound(scale, S, mc.SIGMA)
    err = np.abs(out[:, :, 14:18] - u)
    print("[observed] S = %d: the update's control error %.3g of its bound; effective samples %s" % (S, (err / bound).max(), info[:, 2].tolist()))
    assert (err <= bound).all()
    assert np.array_equal(info[:, [0, 1, 3]], info4[:, [0, 1, 3]]) and (info[:, 3] == S).all()
    np.testing.assert_allclose(info[:, 2], info4[:, 2], rtol=1e-12)
    assert (info[:, 2] > 1.0).all() and (info[:, 2] < S).all()

    score, _ = ac.host_fly(harnesses[1], cfg, plan, S, SEED, spread, **host)
    out, info, new, var = ac.host_adapt(harnesses[1], cfg, plan, score, SEED, spread, kc.LAMBDA, collision_cost=kc.COLLISION_COST, **host)
    want = ma.adapt(plan, score, eps_spread, spread, kc.LAMBDA, ac.FLOOR, ac.CAP, ac.RATE, kc.COLLISION_COST, rest["limits"])
    bound = mp.update_bound(want["scale"], S, spread)
    err = np.abs(out[:, :, 14:18] - want["u"])
    worst, near, either = ac.compare_spreads(new, want, ma.adapt_bound(want["scale"], want["scale2"], S, spread, want["v"], ac.RATE))
    print("[observed] S = %d: the adaptation's control error %.3g, spread error %.3g of their bounds; %.3g of the entries near floor or cap" % (
        S, (err / bound).max(), worst, near))
    assert (err <= bound).all()
    assert np.array_equal(info[:, [0, 1, 3]], want["info"][:, [0, 1, 3]]) and (info[:, 3] == S).all()
    np.testing.assert_allclose(info[:, 2], want["info"][:, 2], rtol=1e-12)
    assert worst <= 1.0 and either and near <= 0.05


# ------------------------------------------------------------------------------------------------ 3. the placements the GPU tests rely on

def assert_margins(label, want, clear):
    gap, zero = sn.margins(clear)
    assert np.isfinite(want).all() and gap > 1e-6 and zero > 1e-6, (label, gap, zero)


@pytest.mark.parametrize("c", kc.FLIGHTS, ids=kc.name)
def test_the_flights_at_the_ends_of_the_knot_loops_cannot_flip(c):
    want, clear, gap = kc.flown(c)
    assert_margins(kc.name(c), want, clear)
    assert gap > 1e-6 and (np.isinf(gap) == (c.ext in ("plain", "models")))  # no control within the bar of a limit
    assert len(np.unique(want[..., 0])) == want[..., 0].size
    if c.ext in ("limits", "both"):  # some thrusts clamp
        host, _, cfg, plan, _, spread = kc.horizon(c.n)
        u = plan[:, None, :, 14:18] + kc.draws(spread if c.spread else mc.SIGMA, SEED, c.S, cfg["dt"], B=kc.KB, n=c.n)
        assert ((u < host["limits"][0]) | (u > host["limits"][1])).any() and ((u > host["limits"][0]) & (u < host["limits"][1])).any()
    assert (want[..., 3] > 0).any()  # the spheres are felt
    if c.n > 2:  # and not by every sample alike (at n = 2 the samples of a plan have hardly parted)
        assert len(np.unique(want[..., 3])) > 1


def test_the_horizons_reach_the_end_of_the_handles_trajectory():
    hd, Qs = mc.schedule()
    assert len(hd) == len(Qs) == 20 and mc.K0 == 3 and kc.N_LONG == len(hd) - mc.K0 == max(kc.KNOT_ENDS)
    assert kc.horizon(17)[3].shape == (2, 17, 18) and kc.horizon(2)[3].tobytes() == kc.horizon(17)[3][:, :2].tobytes()
    for n in kc.KNOT_ENDS:  # the spread the adaptation prefetches by the chunk differs from one chunk's row to the next chunk's
        spread = kc.horizon(n)[5]
        assert spread.shape == (2, n, 4) and (n <= 8 or (spread[:, 8:] != spread[:, :n - 8]).any(axis=2).all())


@pytest.mark.parametrize("integrator", [0, 1])
def test_the_tables_at_capacity_are_felt_to_their_last_sphere(integrator):
    x = kc.capacity_inputs(integrator)
    cfg, counts = x["cfg"], x["counts"]
    assert x["shared"].shape == (64, 5) and x["own"].shape == (3, 64, 8) and counts.tolist() == [64, 0, 37]
    for spread in (False, True):
        for S in kc.CAP_S:
            label = (integrator, spread, S)
            want, clear, traj = (a[:, :S] for a in kc.capacity_flown(spread, integrator))
            assert_margins(label, want, clear)
            assert (want[..., 3] > 0).any() and (want[..., 3] == 0).any(), label
            per_plan = [cc.clearances(traj[b], cfg["dt"], x["shared"], x["own"][b, :counts[b]]) for b in range(kc.CAP_B)]
            nearest = [c.min(axis=1).argmin(axis=1) for c in per_plan]
            assert (np.concatenate(nearest) == 63).any() and (nearest[0] == 64 + 63).any() and (nearest[2] == 64 + 36).any(), label
            # every sweep of the staging loops carries a sphere that is in some flight's cost: all five of the shared table, all eight
            # of plan 0's own, the five that plan 2's 37 spheres reach
            felt = [kc.sweeps_felt(per_plan[b], 64, int(counts[b])) for b in range(kc.CAP_B)]
            assert felt[0][0] | felt[1][0] | felt[2][0] == set(range(5)) and felt[0][1] == set(range(8)) and felt[2][1] == set(range(5)), (label, felt)
            # the other end: of the far tables only the first 8 shared spheres and own sphere 0 come within 1 m
            for b in range(kc.CAP_B):
                c = cc.clearances(traj[b], cfg["dt"], x["far_shared"], x["far_own"][b, :counts[b]])
                near = np.r_[np.arange(kc.CAP_NEAR), [64] if counts[b] else []].astype(int)
                assert np.delete(c, near, axis=2).min(initial=np.inf) > 1.0 and c[..., near].min() < 1.0, label
            short, short_clear, _ = (a[:, :S] for a in kc.capacity_flown(spread, integrator, "short"))
            assert_margins(label, short, short_clear)
            assert (short[..., 0] != want[..., 0]).any()


@pytest.mark.parametrize("integrator", [0, 1])
def test_the_second_tiles_rows_feel_their_own_spheres(integrator):
    x = kc.tile_inputs()
    counts = x["counts"]
    assert x["plan"].shape == (70, 4, 18) and x["own"].shape == (70, 3, 8) and sorted(set(counts.tolist())) == [0, 1, 2, 3]
    assert counts[63] == 0 and counts[69] > 0 and counts[64] > 0 and counts[0] > 0
    # row b - 64's spheres are others than row b's: a table read without its tile term scores otherwise
    assert (x["own"][64, 0] != x["own"][0, 0]).any() and (x["own"][69, :2] != x["own"][5, :2]).any(axis=1).all()
    for spread in (False, True):
        for S in kc.TILE_S:
            want, clear, traj = kc.tile_flown(spread, integrator, S, (64, 69))
            assert_margins((integrator, spread, S), want, clear)
            for k, b in enumerate((64, 69)):
                assert cc.nearest_sphere(traj[k], x["cfg"]["dt"], x["shared"], x["own"][b, :counts[b]])[0] == len(x["shared"])
            assert (want[:, 0, 3] > 0).all()


@pytest.mark.parametrize("first_is_nominal", [True, False])
@pytest.mark.parametrize("S", kc.RAGGED)
def test_the_ragged_sample_counts_weigh_many_samples(harnesses, S, first_is_nominal):
    """the effective sample size of the restatement lies strictly between 1 and S, and every key is finite: a dropped sweep moves both"""
    host, rest, cfg, plan, x0, spread = kc.horizon(kc.N_RAGGED)
    hkw = dict(host, integrator=1, first_is_nominal=first_is_nominal)
    for score, eps in (mc.host_fly(harnesses[0], cfg, plan, S, SEED, mc.SIGMA, **hkw), ac.host_fly(harnesses[1], cfg, plan, S, SEED, spread, **hkw)):
        _, info, _ = mp.update(plan, score, eps, kc.LAMBDA, kc.COLLISION_COST, host["limits"])
        assert (info[:, 3] == S).all() and (info[:, 2] > 1.0).all() and (info[:, 2] < S).all(), info
        # the samples of the last, partly filled sweep carry weight: without them the effective sample size is another
        cut = S // 1024 * 1024
        _, less, _ = mp.update(plan, score[:, :cut], eps[:, :cut], kc.LAMBDA, kc.COLLISION_COST, host["limits"])
        assert (np.abs(less[:, 2] - info[:, 2]) > 1e-9 * info[:, 2]).all()


@pytest.mark.parametrize("scheduled", [True, False])
def test_the_desired_trajectories_per_plan_differ_and_cannot_flip(scheduled):
    host, rest, cfg, plan, x0, spread, per_plan = kc.desired_inputs()
    assert per_plan.shape == plan.shape == (3, 12, 18) and all((per_plan[a] != per_plan[b]).any() for a in range(3) for b in range(a))
    assert all((per_plan[b] != host["handle_desired"][mc.K0:mc.K0 + 12]).any() and (per_plan[b] != cfg["desired"]).any() for b in range(3))
    knot0 = plan[:, 0, 1:14]
    assert all((knot0[a] != knot0[b]).any() for a in range(3) for b in range(a)) and (knot0 != x0).any(axis=1).all()
    rest = dict(rest, desired=per_plan) if scheduled else dict(rest, desired=per_plan, Qs=None)
    for sp in (False, True):
        eps = kc.draws(spread if sp else mc.SIGMA, SEED, kc.DES_S, cfg["dt"], first_is_nominal=True, B=kc.DES_B, n=kc.DES_N)
        want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], **rest)
        assert_margins((scheduled, sp), want, clear)
        assert gap > 1e-6
