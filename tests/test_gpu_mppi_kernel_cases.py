"""The sampling planner's 26 kernels where tests/test_gpu_mppi.py and tests/test_gpu_mppi_adapt.py do not take them (tests/mppi_kernel_cases.py
has one case per kernel and tests/test_mppi_kernel_cases_cpu.py the proof that the cases are the kernels, and that every placement relied
on here holds on the restatement): every block size of k_mppi_update and k_mppi_adapt against the host programs; sample counts that
leave the last sweep of a lane partly filled; horizons at the ends of the knot loops (n = 2, 8, 9, 16, 17), through all sixteen flight
kernels; the sphere tables of the LDS image at capacity (64 shared, 64 per problem with counts 64, 0 and 37); a second tile of the
per-problem table (B = 70); a desired trajectory per plan, and the start states read from the plan's knot 0.  Every call goes through the
C ABI on plain device buffers, every output 0xFF-prefilled with a guard behind its end; the bars are the existing files'.

What a wrong kernel would trip: a wrong stride in MppiSharedFetch::prime leaves whole sweeps of 64 words out of the image, and every sweep
holds a sphere some flight is inside (test_tables_at_capacity); bob_index without row / OB_TILE reads row b - 64's spheres for plans
64 .. 69 (test_a_second_tile_of_the_per_problem_table); a sweep dropped or a guard `j < S` misplaced moves the count of finite keys, the
effective sample size and the controls (test_ragged_sweeps...); a plan's desired trajectory or start state read at another plan's stride
scores otherwise (test_a_desired_trajectory_per_plan, test_start_states_read_from_the_plans_knot_0); a spread row prefetched from the
wrong chunk changes the controls and spreads of knots 8 and up (test_the_update_and_the_adaptation_at_the_ends_of_the_knot_loops)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import closed_loop_cases as cc, mppi_adapt_cases as ac, mppi_adapt_numpy as ma, mppi_cases as mc, mppi_kernel_cases as kc  # noqa: E402
from tests import mppi_numpy as mp, scored_flight_numpy as sn  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402
from tests.test_gpu_mppi import dev_flight, dev_update, fetch, guarded, rule_of, solver_for  # noqa: E402
from tests.test_gpu_mppi_adapt import adapt_rule, dev_adapt, dev_flight_spread  # noqa: E402

SEED = kc.SEED


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def harnesses():
    """the two host programs: (tests/host_mppi_harness.cpp, tests/host_mppi_adapt_harness.cpp)"""
    return mc.build_harness(["-O2"], "host_mppi_harness"), ac.build_harness(["-O2"], "host_mppi_adapt_harness")


def flight_rule(**kw):
    return rule_of(mc.SIGMA, tau_s=kc.TAU_S, **kw)


def update_rule(first_is_nominal=True):
    return flight_rule(lambda_=kc.LAMBDA, collision_cost=kc.COLLISION_COST, first_is_nominal=first_is_nominal)


def over(got, want):
    return cc.over(got, want, sn.RTOL, sn.ATOL)


def assert_flight(label, got, want, clear):
    """a device score (B, S, 4) against the restatement's: the `[observed]` line, cost and clearance at the flight's bar, the knot and the
    count exactly -- after the restatement's own margins have shown that it alone cannot flip them"""
    gap, zero = sn.margins(clear)
    assert np.isfinite(want).all() and gap > 1e-6 and zero > 1e-6, (label, gap, zero)
    print("[observed] %s: error over its bar %.3g (cost), %.3g (clearance)" % (label, over(got[..., 0], want[..., 0]), over(got[..., 1], want[..., 1])))
    np.testing.assert_allclose(got[..., :2], want[..., :2], rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
    assert np.array_equal(got[..., 2:], want[..., 2:]), label


# the two spread calls with a desired trajectory per plan (tests/test_gpu_mppi_adapt.py's helpers pass none)

def dev_flight_spread_towards(hip, s, plan, spread, S, seed, rule, desired, x0=None):
    lib = capi.load()
    b, n = plan.shape[:2]
    d_plan, d_x0, d_des, d_spread = hip.upload(plan), (hip.upload(x0) if x0 is not None else None), hip.upload(desired), hip.upload(spread)
    d_score = guarded(hip, (b, S, 4))
    assert lib.qilqr_mppi_flight_spread_device(s._h, C.byref(rule), seed, d_plan, d_x0, d_des, d_spread, b, n, S, 0, d_score) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    score, kept = fetch(hip, d_score, (b, S, 4))
    assert kept, "k_mppi_flight_spread wrote behind the end of d_score"
    return score


def dev_adapt_towards(hip, s, plan, spread, score, seed, rule, adapt, desired, x0=None):
    lib = capi.load()
    b, n, S = plan.shape[0], plan.shape[1], score.shape[1]
    d_plan, d_x0, d_des, d_spread = hip.upload(plan), (hip.upload(x0) if x0 is not None else None), hip.upload(desired), hip.upload(spread)
    d_score, d_out, d_new, d_info = hip.upload(score), guarded(hip, (b, n, 18)), guarded(hip, (b, n, 4)), guarded(hip, (b, 8))
    rc = lib.qilqr_mppi_adapt_device(s._h, C.byref(rule), C.byref(adapt), seed, d_plan, d_x0, d_des, d_spread, d_score, b, n, S, 0, d_out, d_new, d_info)
    assert rc == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    (out, k0), (new, k1), (info, k2) = fetch(hip, d_out, (b, n, 18)), fetch(hip, d_new, (b, n, 4)), fetch(hip, d_info, (b, 8))
    assert k0 and k1 and k2, "the adaptation wrote behind the end of an output"
    assert not np.isnan(out).any() and not np.isnan(new).any(), "a word of an output was left unwritten"
    return out, info, new


# ------------------------------------------------------------------------------------------------ the comparison with the host programs

def handle_of(n, integrator=0):
    host, _, cfg, _, _, _ = kc.horizon(n)
    return solver_for(cfg, integrator, host["limits"], host["models"], host["shared"], host["own"], host["counts"], host["Qs"], host["k0"], host["handle_desired"])


def update_against_the_host_program(hip, harnesses, n, S, first_is_nominal=True, integrator=0, label=""):
    """tests/test_gpu_mppi.py's comparison on kc.horizon(n): the device's own scores handed to both sides; J_min, its sample and the count
    exactly, the controls within update_bound, the new plan's states and score within the flight's bar -> (out_plan, info)"""
    host, rest, cfg, plan, x0, _ = kc.horizon(n)
    s, rule = handle_of(n, integrator), update_rule(first_is_nominal)
    score = dev_flight(hip, s, plan, S, SEED, rule, x0=x0)
    assert np.isfinite(score).all()
    got, info = dev_update(hip, s, plan, score, SEED, rule, x0=x0)
    hkw = dict(host, integrator=integrator, first_is_nominal=first_is_nominal)
    want, want_info = mc.host_update(harnesses[0], cfg, plan, score, SEED, mc.SIGMA, kc.LAMBDA, collision_cost=kc.COLLISION_COST, **hkw)
    _, eps = mc.host_fly(harnesses[0], cfg, plan, S, SEED, mc.SIGMA, **hkw)
    _, _, scale = mp.update(plan, score, eps, kc.LAMBDA, kc.COLLISION_COST, host["limits"])
    bound = mp.update_bound(scale, S, mc.SIGMA)
    err = np.abs(got[:, :, 14:18] - want[:, :, 14:18])
    print("[observed] update%s, n = %d, S = %d: control error %.3g of its bound, new plan %.3g of the flight's bar; effective samples %s" % (
        label, n, S, (err / bound).max(), over(got, want), info[:, 2].tolist()))
    assert (err <= bound).all()
    assert np.array_equal(info[:, [0, 1, 3]], want_info[:, [0, 1, 3]])
    np.testing.assert_allclose(info[:, 2], want_info[:, 2], rtol=1e-12)
    assert got[:, :, 0].tobytes() == plan[:, :, 0].tobytes() and np.array_equal(got[:, 0, 1:14], x0)
    np.testing.assert_allclose(got, want, rtol=sn.RTOL, atol=sn.ATOL)
    np.testing.assert_allclose(info[:, 4:6], want_info[:, 4:6], rtol=sn.RTOL, atol=sn.ATOL)
    return got, info


def adaptation_against_the_host_program(hip, harnesses, n, S, first_is_nominal=True, integrator=0, label=""):
    """tests/test_gpu_mppi_adapt.py's comparison on kc.horizon(n): the spreads within adapt_bound / (s_dev + s_ref) beside the update's
    words -> (out_plan, info, out_spread)"""
    host, rest, cfg, plan, x0, spread = kc.horizon(n)
    s, rule = handle_of(n, integrator), update_rule(first_is_nominal)
    score = dev_flight_spread(hip, s, plan, spread, S, SEED, rule, x0=x0)
    assert np.isfinite(score).all()
    got, info, new = dev_adapt(hip, s, plan, spread, score, SEED, rule, adapt_rule(), x0=x0)
    hkw = dict(host, integrator=integrator, first_is_nominal=first_is_nominal)
    want, want_info, want_new, _ = ac.host_adapt(harnesses[1], cfg, plan, score, SEED, spread, kc.LAMBDA, collision_cost=kc.COLLISION_COST, **hkw)
    _, eps = ac.host_fly(harnesses[1], cfg, plan, S, SEED, spread, **hkw)
    ref = ma.adapt(plan, score, eps, spread, kc.LAMBDA, ac.FLOOR, ac.CAP, ac.RATE, kc.COLLISION_COST, host["limits"])
    bound = mp.update_bound(ref["scale"], S, spread)
    err = np.abs(got[:, :, 14:18] - want[:, :, 14:18])
    worst, near, either = ac.compare_spreads(new, dict(ref, spread=want_new), ma.adapt_bound(ref["scale"], ref["scale2"], S, spread, ref["v"], ac.RATE))
    print("[observed] adapt%s, n = %d, S = %d: control error %.3g, spread error %.3g of their bounds, new plan %.3g of the flight's bar; %.3g of the entries "
          "near floor or cap; effective samples %s" % (label, n, S, (err / bound).max(), worst, over(got, want), near, info[:, 2].tolist()))
    assert (err <= bound).all()
    assert np.array_equal(info[:, [0, 1, 3]], want_info[:, [0, 1, 3]])
    np.testing.assert_allclose(info[:, 2], want_info[:, 2], rtol=1e-12)
    assert worst <= 1.0 and either and near <= 0.05
    assert got[:, :, 0].tobytes() == plan[:, :, 0].tobytes() and np.array_equal(got[:, 0, 1:14], x0)
    np.testing.assert_allclose(got, want, rtol=sn.RTOL, atol=sn.ATOL)
    np.testing.assert_allclose(info[:, 4:6], want_info[:, 4:6], rtol=sn.RTOL, atol=sn.ATOL)
    return got, info, new


# ------------------------------------------------------------------------------------------------ 1. every block size, by the case table

@pytest.mark.parametrize("c", kc.BLOCKS, ids=kc.name)
def test_every_block_size_against_the_host_program(hip, harnesses, c):
    """S = 64, 100, 200, 300 and 1025 launch k_mppi_update<64 .. 1024> and k_mppi_adapt<64 .. 1024> (the CPU map asserts it): one, two,
    four, eight and sixteen wavefronts whose sums combine in index order"""
    assert mp.update_lanes(c.S) == c.threads
    (adaptation_against_the_host_program if c.adapt else update_against_the_host_program)(hip, harnesses, kc.N_BLOCKS, c.S, label="<%d>" % c.threads)


# ------------------------------------------------------------------------------------------------ 2. ragged sweeps

@pytest.mark.parametrize("first_is_nominal", [True, False], ids=["nominal", "all_drawn"])
@pytest.mark.parametrize("S", kc.RAGGED)
def test_ragged_sweeps_of_the_update_and_the_adaptation(hip, harnesses, S, first_is_nominal):
    """beyond S = 1024 lane t carries samples t, t + 1024, ...: at 1025 lane 0 alone has a second, at 2500 lanes 0 .. 451 a third, at 4095
    every lane but the last a fourth.  Sample 0, the nominal one with the flag, is lane 0's first."""
    for compare in (update_against_the_host_program, adaptation_against_the_host_program):
        info = compare(hip, harnesses, kc.N_RAGGED, S, first_is_nominal=first_is_nominal, integrator=1)[1]
        assert (info[:, 3] == S).all() and (info[:, 2] > 1.0).all() and (info[:, 2] < S).all(), info[:, :4]


# ------------------------------------------------------------------------------------------------ 3. the ends of the knot loops

@pytest.mark.parametrize("c", kc.FLIGHTS, ids=kc.name)
def test_every_flight_kernel_at_the_ends_of_the_knot_loops(hip, c):
    """the sixteen flight kernels, each at one of n = 2, 8, 9, 16, 17 (the eight of a unit fly all five): the image's loads two knots
    ahead with no second knot ahead, and up to the last knot the handle's desired trajectory and schedule hold"""
    host, _, cfg, plan, x0, spread = kc.horizon(c.n)
    want, clear, gap = kc.flown(c)
    assert gap > 1e-6, (kc.name(c), gap)  # (inf without limits: no control within the bar of a limit)
    ext = kc.with_ext(host, c.ext)
    s = solver_for(cfg, c.integrator, ext["limits"], ext["models"], host["shared"], host["own"], host["counts"], host["Qs"], host["k0"], host["handle_desired"])
    if c.spread:
        got = dev_flight_spread(hip, s, plan, spread, c.S, SEED, flight_rule(), x0=x0)
    else:
        got = dev_flight(hip, s, plan, c.S, SEED, flight_rule(), x0=x0)
    assert_flight(kc.name(c), got, want, clear)
    assert len(np.unique(got[..., 0])) == got[..., 0].size  # no two samples flew alike


@pytest.mark.parametrize("n", kc.KNOT_ENDS)
def test_the_update_and_the_adaptation_at_the_ends_of_the_knot_loops(hip, harnesses, n):
    """MPPI_CHUNK = 8 knots between two combinations of the wavefronts: n = 2 is a quarter of a chunk, 8 one chunk with no next rows to
    fetch, 9 a chunk of one knot behind it, 16 two whole chunks, 17 a third of one knot.  And the nominal flight behind each stores the
    new plan's trajectory: the restatement's flight of the new controls."""
    host, rest, cfg, plan, x0, spread = kc.horizon(n)
    integrator = n % 2
    outs = (update_against_the_host_program(hip, harnesses, n, kc.S_FLIGHT, integrator=integrator)[0],
            adaptation_against_the_host_program(hip, harnesses, n, kc.S_FLIGHT, integrator=integrator)[0])
    for out in outs:
        assert (out[:, :, 14:18] != plan[:, :, 14:18]).any(axis=2).all()  # every knot's controls moved
        score, clear, _, traj = mp.flight(out, x0, np.zeros((kc.KB, 1, n, 4)), cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], integrator=integrator, **rest)
        print("[observed] n = %d: the stored trajectory of the nominal flight, error over its bar %.3g" % (n, over(out, traj[:, 0])))
        np.testing.assert_allclose(out, traj[:, 0], rtol=sn.RTOL, atol=sn.ATOL)


def test_a_horizon_beyond_the_handles_desired_trajectory_is_refused(hip):
    """mc.schedule(): 20 knots from horizon start 3 -- n = 17 is flown above, n = 18 is a reason of length for each of the four calls"""
    n, S = kc.N_LONG + 1, 5
    s, lib = handle_of(kc.N_LONG), capi.load()
    d_plan, d_x0, d_spread = hip.upload(np.zeros((kc.KB, n, 18))), hip.upload(kc.horizon(kc.N_LONG)[4]), hip.upload(np.ones((kc.KB, n, 4)))
    d_score, d_out, d_new, d_info = guarded(hip, (kc.KB, S, 4)), guarded(hip, (kc.KB, n, 18)), guarded(hip, (kc.KB, n, 4)), guarded(hip, (kc.KB, 8))
    rule, adapt = update_rule(), adapt_rule()
    for length, rc in ((n, capi.ERR_LENGTH_MISMATCH), (kc.N_LONG, 0)):
        assert lib.qilqr_mppi_flight_device(s._h, C.byref(rule), SEED, d_plan, d_x0, None, kc.KB, length, S, 0, d_score) == rc, lib.qilqr_last_error()
        if rc:
            assert lib.qilqr_mppi_update_device(s._h, C.byref(rule), SEED, d_plan, d_x0, None, d_score, kc.KB, length, S, 0, d_out, d_info) == rc
            assert lib.qilqr_mppi_flight_spread_device(s._h, C.byref(rule), SEED, d_plan, d_x0, None, d_spread, kc.KB, length, S, 0, d_score) == rc
            assert lib.qilqr_mppi_adapt_device(s._h, C.byref(rule), C.byref(adapt), SEED, d_plan, d_x0, None, d_spread, d_score, kc.KB, length, S, 0, d_out,
                                               d_new, d_info) == rc
            hip.synchronize(lib.qilqr_stream(s._h))
            for ptr, shape in ((d_score, (kc.KB, S, 4)), (d_out, (kc.KB, n, 18)), (d_new, (kc.KB, n, 4)), (d_info, (kc.KB, 8))):
                assert (hip.download(ptr, (8 * int(np.prod(shape)),), dtype=np.uint8) == 0xFF).all()  # a refused call writes nothing
    hip.synchronize(lib.qilqr_stream(s._h))


# ------------------------------------------------------------------------------------------------ 4. tables at capacity

def fly_both(hip, s, x, S, rows=slice(None), b0=0):
    """the two flights of the plans `rows` of the inputs x on the handle s: {spread: score}"""
    plan, x0, spread = (np.ascontiguousarray(x[k][rows]) for k in ("plan", "x0", "spread"))
    return {False: dev_flight(hip, s, plan, S, SEED, flight_rule(), x0=x0, b0=b0),
            True: dev_flight_spread(hip, s, plan, spread, S, SEED, flight_rule(), x0=x0, b0=b0)}


@pytest.mark.parametrize("S", kc.CAP_S)
@pytest.mark.parametrize("integrator", [0, 1])
def test_tables_at_capacity(hip, integrator, S):
    """MppiSharedFetch::prime stages 320 and 512 words 64 at a time: five and eight sweeps, and the own table's words split into sphere
    and word.  One idle lane at S = 63; three blocks per plan, each staging for itself, at S = 130."""
    x = kc.capacity_inputs(integrator)
    cfg, counts = x["cfg"], x["counts"]
    assert x["shared"].shape == (cc.OB_MAX, 5) and x["own"].shape == (kc.CAP_B, cc.OB_MAX, 8) and counts.tolist() == [64, 0, 37]
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    s.set_obstacles(x["shared"])
    s.set_batch_obstacles(x["own"], counts)
    want = {sp: tuple(a[:, :S] for a in kc.capacity_flown(sp, integrator)) for sp in (False, True)}
    for sp in (False, True):  # the placement, on the restatement, before the device is asked
        score, clear, traj = want[sp]
        nearest = [cc.nearest_sphere(traj[b], cfg["dt"], x["shared"], x["own"][b, :counts[b]]) for b in range(kc.CAP_B)]
        assert (np.concatenate(nearest) == cc.OB_MAX - 1).any() and (nearest[0] == cc.OB_MAX + 63).any() and (nearest[2] == cc.OB_MAX + 36).any()
        assert (score[..., 3] > 0).any() and (score[..., 3] == 0).any()
    full = fly_both(hip, s, x, S)
    for sp in (False, True):
        assert_flight("full tables, %s, integrator %d, S = %d" % ("spread" if sp else "sigma", integrator, S), full[sp], want[sp][0], want[sp][1])
        # (the plan with no sphere of its own is restated with the shared table alone: any of its 64 unused rows would cost 1e6 h^2)
        assert full[sp][1, :, 0].max() < 1e5
    # the other end of the loops on the same handle: full tables of which only the first 8 shared spheres and own sphere 0 ever come
    # within 1 m, then those spheres alone (8 shared, K = 1): the same bytes, and the restatement's of the short tables
    for sp in (False, True):
        for b in range(kc.CAP_B):
            c = cc.clearances(want[sp][2][b], cfg["dt"], x["far_shared"], x["far_own"][b, :counts[b]])
            near = np.r_[np.arange(kc.CAP_NEAR), [cc.OB_MAX] if counts[b] else []].astype(int)
            assert np.delete(c, near, axis=2).min(initial=np.inf) > 1.0 and c[..., near].min() < 1.0
    s.set_obstacles(x["far_shared"])
    s.set_batch_obstacles(x["far_own"], counts)
    first = fly_both(hip, s, x, S)
    s.set_obstacles(x["far_shared"][:kc.CAP_NEAR])
    s.set_batch_obstacles(x["far_own"][:, :1], np.minimum(counts, 1))
    second = fly_both(hip, s, x, S)
    for sp in (False, True):
        assert first[sp].tobytes() == second[sp].tobytes() and first[sp].tobytes() != full[sp].tobytes()
        short = tuple(a[:, :S] for a in kc.capacity_flown(sp, integrator, "short"))
        assert_flight("short tables, %s, integrator %d, S = %d" % ("spread" if sp else "sigma", integrator, S), second[sp], short[0], short[1])


# ------------------------------------------------------------------------------------------------ 5. a second tile

@pytest.mark.parametrize("S", kc.TILE_S)
@pytest.mark.parametrize("integrator", [0, 1])
def test_a_second_tile_of_the_per_problem_table(hip, integrator, S):
    """B = 70: the per-problem table is tiled by 64 problems, and plans 64 .. 69 read the second tile.  Rows 0, 63, 64 and 69 of the
    four calls against the same plan alone -- on a handle that holds that row's spheres and model, drawn as plan b0 = row."""
    x = kc.tile_inputs()
    cfg, plan, x0, spread, counts = x["cfg"], x["plan"], x["x0"], x["spread"], x["counts"]
    assert sorted(set(counts.tolist())) == [0, 1, 2, 3] and counts[69] > 0 and counts[63] == 0 and x["own"].shape == (70, 3, 8)

    def handle(rows):
        s = capi.from_config(cfg)
        s.set_integrator(integrator)
        s.set_models([x["models"][b] for b in rows])
        s.set_obstacles(x["shared"])
        s.set_batch_obstacles(x["own"][rows], counts[rows])
        return s

    def four_calls(s, rows, b0):
        p, start, sp = (np.ascontiguousarray(a[rows]) for a in (plan, x0, spread))
        score = fly_both(hip, s, x, S, rows=rows, b0=b0)
        rule = update_rule()
        return (score[False], score[True]) + dev_update(hip, s, p, score[False], SEED, rule, x0=start, b0=b0) + \
            dev_adapt(hip, s, p, sp, score[True], SEED, rule, adapt_rule(), x0=start, b0=b0)

    whole = four_calls(handle(np.arange(kc.TILE_B)), np.arange(kc.TILE_B), 0)
    assert all(np.isfinite(a).all() for a in whole)
    for b in kc.TILE_ROWS:
        alone = four_calls(handle([b]), [b], b)
        for a, w, what in zip(alone, whole, ("flight", "spread flight", "update's plan", "update's info", "adaptation's plan", "its info", "its spread")):
            assert a.tobytes() == w[b:b + 1].tobytes(), (b, what)
    rows = [64, 69]
    for sp in (False, True):
        want, clear, traj = kc.tile_flown(sp, integrator, S, tuple(rows))
        for k, b in enumerate(rows):  # the row's own spheres are felt: sphere 0 of its own is the nearest of its sample 0
            assert cc.nearest_sphere(traj[k], cfg["dt"], x["shared"], x["own"][b, :counts[b]])[0] == len(x["shared"])
        assert_flight("rows 64 and 69 of 70, %s, integrator %d, S = %d" % ("spread" if sp else "sigma", integrator, S), whole[1 if sp else 0][rows], want, clear)
        assert (whole[1 if sp else 0][rows, 0, 3] > 0).all()


# ------------------------------------------------------------------------------------------------ 6. the operands no direct call passed

def operand_handle(scheduled):
    host, rest, cfg, plan, x0, spread, per_plan = kc.desired_inputs()
    if scheduled:
        return solver_for(cfg, 0, host["limits"], host["models"], host["shared"], host["own"], host["counts"], host["Qs"], host["k0"], host["handle_desired"])
    return solver_for(cfg, 0, host["limits"], host["models"], host["shared"], host["own"], host["counts"])


@pytest.mark.parametrize("scheduled", [True, False], ids=["schedule", "handles_Q"])
def test_a_desired_trajectory_per_plan(hip, harnesses, scheduled):
    """d_desired != NULL: plan b is scored against desired + b * 18 n.  Three trajectories, none the handle's; with a schedule the state
    weights still come from the handle's horizon start, without one the handle's own desired trajectory plays no part at all."""
    host, rest, cfg, plan, x0, spread, per_plan = kc.desired_inputs()
    assert per_plan.shape == plan.shape and all((per_plan[a] != per_plan[b]).any() for a in range(3) for b in range(a))
    if not scheduled:
        host = {k: v for k, v in host.items() if k not in ("Qs", "k0", "handle_desired")}
        rest = dict(rest, Qs=None)
    s, S, rule = operand_handle(scheduled), kc.DES_S, update_rule()
    hkw = dict(host, desired=per_plan, first_is_nominal=True)
    for sp in (False, True):
        label = "per-plan desired, %s, %s" % ("spread" if sp else "sigma", "schedule" if scheduled else "the handle's Q")
        eps = kc.draws(spread if sp else mc.SIGMA, SEED, S, cfg["dt"], first_is_nominal=True, B=kc.DES_B, n=kc.DES_N)
        want, clear, gap, _ = mp.flight(plan, x0, eps, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], **dict(rest, desired=per_plan))
        assert gap > 1e-6
        if sp:
            got = dev_flight_spread_towards(hip, s, plan, spread, S, SEED, rule, per_plan, x0=x0)
            handles = dev_flight_spread(hip, s, plan, spread, S, SEED, rule, x0=x0)
        else:
            got = dev_flight(hip, s, plan, S, SEED, rule, x0=x0, desired=per_plan)
            handles = dev_flight(hip, s, plan, S, SEED, rule, x0=x0)
        assert_flight(label, got, want, clear)
        assert (handles[..., 0] != got[..., 0]).all() and handles[..., 1:].tobytes() == got[..., 1:].tobytes()  # the cost alone knows the desired trajectory
        # the update and the adaptation: the weights are the scores', so the controls are; the nominal flight behind is scored against per_plan
        if sp:
            out, info, new = dev_adapt_towards(hip, s, plan, spread, got, SEED, rule, adapt_rule(), per_plan, x0=x0)
            same, same_info, same_new = dev_adapt(hip, s, plan, spread, got, SEED, rule, adapt_rule(), x0=x0)
            want_out, want_info, _, _ = ac.host_adapt(harnesses[1], cfg, plan, got, SEED, spread, kc.LAMBDA, collision_cost=kc.COLLISION_COST, **hkw)
            assert new.tobytes() == same_new.tobytes()
        else:
            out, info = dev_update(hip, s, plan, got, SEED, rule, x0=x0, desired=per_plan)
            same, same_info = dev_update(hip, s, plan, got, SEED, rule, x0=x0)
            want_out, want_info = mc.host_update(harnesses[0], cfg, plan, got, SEED, mc.SIGMA, kc.LAMBDA, collision_cost=kc.COLLISION_COST, **hkw)
        print("[observed] %s: the new plan %.3g, its score %.3g of the flight's bar" % (label, over(out, want_out), over(info[:, 4:6], want_info[:, 4:6])))
        assert out.tobytes() == same.tobytes() and info[:, :4].tobytes() == same_info[:, :4].tobytes()
        assert (info[:, 4] != same_info[:, 4]).all() and info[:, 5:].tobytes() == same_info[:, 5:].tobytes()
        np.testing.assert_allclose(out, want_out, rtol=sn.RTOL, atol=sn.ATOL)
        assert np.array_equal(info[:, [0, 1, 3]], want_info[:, [0, 1, 3]])
        np.testing.assert_allclose(info[:, 4:6], want_info[:, 4:6], rtol=sn.RTOL, atol=sn.ATOL)


@pytest.mark.parametrize("scheduled", [True, False], ids=["schedule", "handles_Q"])
def test_start_states_read_from_the_plans_knot_0(hip, scheduled):
    """d_x0 == NULL: plan b starts at words 1 .. 13 of its own knot 0, 18 n words from plan b - 1's"""
    host, rest, cfg, plan, x0, spread, per_plan = kc.desired_inputs()
    s, S, rule = operand_handle(scheduled), kc.DES_S, update_rule()
    knot0 = np.ascontiguousarray(plan[:, 0, 1:14])
    assert all((knot0[a] != knot0[b]).any() for a in range(3) for b in range(a)) and (knot0 != x0).any(axis=1).all()
    for desired in (None, per_plan):
        fly = (lambda start: dev_flight(hip, s, plan, S, SEED, rule, x0=start, desired=desired)), \
              (lambda start: dev_flight_spread(hip, s, plan, spread, S, SEED, rule, x0=start) if desired is None else
               dev_flight_spread_towards(hip, s, plan, spread, S, SEED, rule, desired, x0=start))
        scores = [(f(None), f(knot0), f(x0)) for f in fly]
        for without, given, elsewhere in scores:
            assert without.tobytes() == given.tobytes() and (without[..., 0] != elsewhere[..., 0]).all()
        up = lambda start: dev_update(hip, s, plan, scores[0][0], SEED, rule, x0=start, desired=desired)  # noqa: E731
        ad = (lambda start: dev_adapt(hip, s, plan, spread, scores[1][0], SEED, rule, adapt_rule(), x0=start)) if desired is None else \
             (lambda start: dev_adapt_towards(hip, s, plan, spread, scores[1][0], SEED, rule, adapt_rule(), desired, x0=start))
        for call in (up, ad):
            without, given = call(None), call(knot0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(without, given))
            assert np.array_equal(without[0][:, 0, 1:14], knot0)
            assert (without[0][:, 1:, 1:14] != plan[:, 1:, 1:14]).any(axis=2).all()  # the states behind knot 0 are the nominal flight's, not the plan's
