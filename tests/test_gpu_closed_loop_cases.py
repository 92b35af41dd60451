"""Every instantiation of k_closed_loop and k_closed_loop_scored on the device (tests/closed_loop_cases.py has one case per kernel and
tests/test_closed_loop_cases_cpu.py the proof that the 64 cases are the 64 kernels), each against the restatement from the oracle's
primitives (tests/scored_flight_numpy.py, tests/closed_loop_numpy.py) at the project's bound for this chain of steps, the discrete parts
exactly; the sphere tables at capacity (64 shared spheres, 64 per problem with counts 64, 0 and 37: the staging loops of the
shared-operand form's LDS image take every trip they can); and a second tile of the per-problem table (B = 70: rows 0, 63, 64 and 69
against the same plan flown alone).  S = 63 is the shared-operand form with one idle lane, S = 5 and S = 1 the flattened form.  Every call
goes through qilqr_closed_loop_scored_device on plain device buffers, every output 0xFF-prefilled with a guard behind its end.

What a wrong kernel would trip: a missing or crossed branch of scored_switch / with_extensions launches another case's kernel, whose
flights differ (test_every_instantiation_against_the_restatement: the gusts are felt, the clamps counted, neighbouring models differ); a
wrong stride or index in ClSharedScoreFetch::prime leaves spheres 13 .. 63 (shared) or 8 .. 63 (own) out of the image or misplaced, and
the deepest sphere of each table is its last (test_tables_at_capacity); bob_index without row / OB_TILE reads row b - 64's spheres for
problems 64 .. 69 (test_a_second_tile_of_the_per_problem_table)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import closed_loop_cases as cc, closed_loop_numpy as cn, scored_flight_numpy as sn  # noqa: E402
from tests.test_gpu_closed_loop import Hip, flew_off_the_plan  # noqa: E402


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def restate(x, x0, wrench, shared, own, counts, rows=None, **kw):
    """scored_flight_numpy.scored_flight on the inputs x (of the problems `rows`), read-only: (traj, stats, score, clear)"""
    rows = list(range(len(x["plan"]))) if rows is None else list(rows)
    cfg = x["cfg"]
    return frozen(*sn.scored_flight(x["plan"][rows], x["gains"][rows], x0, cfg["model"], cfg["dt"], cfg["Q"], cfg["R"], cfg["desired"],
                                    wrench=wrench, shared=shared, own=[own[b, :counts[b]] for b in rows], **kw))


def assert_scored(label, got, want, plan, scored=True):
    """a device flight (traj, stats, score) against the restatement's (traj, stats, score, clear): the `[observed]` line, then trajectories,
    statistics, cost and clearance at the project's bound and the clamp count, the clearance knot and the hit count exactly -- after the
    restatement's own margins have shown that it alone cannot flip them"""
    traj, stats, score = got
    want_traj, want_stats, want_score, clear = want
    if scored:
        gap, zero = sn.margins(clear)
        assert gap > 1e-6 and zero > 1e-6, (label, gap, zero)  # (neither the knot nor the count can flip inside the bound)
    figures = [cc.over(traj, want_traj, sn.RTOL, sn.ATOL), cc.over(stats[..., :3], want_stats[..., :3], sn.RTOL, sn.ATOL)]
    if scored:
        figures += [cc.over(score[..., 0], want_score[..., 0], sn.RTOL, sn.ATOL), cc.over(score[..., 1], want_score[..., 1], sn.RTOL, sn.ATOL)]
    print("[observed] %s: largest error over its bound %s" % (label, ", ".join("%.3g (%s)" % (f, k) for f, k in zip(
        figures, ("trajectories", "statistics", "cost", "clearance")))))
    np.testing.assert_allclose(traj, want_traj, rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
    np.testing.assert_allclose(stats[..., :3], want_stats[..., :3], rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
    assert np.array_equal(stats[..., 3], want_stats[..., 3]), label
    assert flew_off_the_plan(traj, plan), label
    if scored:
        np.testing.assert_allclose(score[..., :2], want_score[..., :2], rtol=sn.RTOL, atol=sn.ATOL, err_msg=label)
        assert np.array_equal(score[..., 2:], want_score[..., 2:]), label
    return max(figures)


# ------------------------------------------------------------------------------------------------ 1. one case per kernel

@functools.lru_cache(maxsize=None)
def restated(group):
    """the restatement's flights of one (integrator, form, limits, models), once for its four wrench / score variants: gusty and calm with
    the spheres scored, the plain flight of closed_loop_numpy.closed_loop, and how far the commanded thrusts stay from the limits"""
    integrator, shared_form, limits, models = group
    x = cc.inputs()
    S = cc.S_SHARED if shared_form else cc.S_FLAT
    x0, gust = x["x0"][:, :S], x["gust"][:, :S]
    kw = dict(integrator=integrator, models=cc.models_for(cc.B, S) if models else None, limits=cc.LIMITS if limits else None)
    out = dict(gusty=restate(x, x0, gust, x["shared"], x["own"], x["counts"], **kw), calm=restate(x, x0, None, x["shared"], x["own"], x["counts"], **kw),
               plain=frozen(*cn.closed_loop(x["plan"], x["gains"], x0, x["cfg"]["model"], x["cfg"]["dt"], **kw)))
    out["limit_margin"] = {k: cc.limit_margin(cc.commanded(x["plan"], x["gains"], out[k][0])) for k in ("gusty", "calm")} if limits else None
    return out


@pytest.mark.parametrize("c", cc.CASES, ids=cc.name)
def test_every_instantiation_against_the_restatement(hip, c):
    x = cc.inputs()
    S = cc.samples(c)
    plan, gains = x["plan"], x["gains"]
    x0, gust = np.ascontiguousarray(x["x0"][:, :S]), np.ascontiguousarray(x["gust"][:, :S])
    r = restated(cc.group(c))
    flight = "gusty" if c.wrench else "calm"
    want = r[flight] if c.wrench or c.score else r["plain"] + (None, None)  # (without either switch: closed_loop_numpy.closed_loop)
    if c.limits:  # before the device's answer: no commanded thrust of the restatement is within 1e-6 of a bound
        assert r["limit_margin"][flight] > 1e-6, r["limit_margin"]
    s = cc.configure(capi.from_config(x["cfg"]), c, x)
    traj, stats, score, kept = cc.scored_device(hip, s, plan, gains, x0, wrench=gust if c.wrench else None, score=c.score)
    assert_scored(cc.name(c), (traj, stats, score), want, plan, scored=c.score)
    assert kept  # (S = 63: the idle lane flies a copy of sample 62 and stores nothing)
    assert np.array_equal(traj[:, :, 0, 1:14], x0)
    if c.wrench:  # the gusts are felt
        assert (np.abs(traj[:, :, -1, 1:4] - r["calm"][0][:, :, -1, 1:4]).max(axis=2) > 1e-6).all()
    u = traj[..., 14:18]
    if c.limits:  # some thrusts were clamped and some were not
        assert 0 < stats[..., 3].sum() < u.size and ((u > cc.LIMITS[0]) & (u < cc.LIMITS[1])).any()
        assert u.min() == cc.LIMITS[0] and u.max() == cc.LIMITS[1]
    else:
        assert (stats[..., 3] == 0).all() and (u < cc.LIMITS[0]).any() and (u > cc.LIMITS[1]).any()
    if c.score:
        assert (score[..., 3] > 0).any() and (score[..., 3] == 0).any()
    # samples 0 and 1 of a plan start from one state: with models they part, without they are one flight
    assert np.array_equal(x0[:, 0], x0[:, 1])
    if c.models:
        assert (np.abs(traj[:, 0, 2:, 1:14] - traj[:, 1, 2:, 1:14]).max(axis=(1, 2)) > 1e-6).all()
    elif not c.wrench:
        assert traj[:, 0].tobytes() == traj[:, 1].tobytes()


# ------------------------------------------------------------------------------------------------ 2. tables at capacity

@pytest.mark.parametrize("S", [cc.S_SHARED, cc.S_FLAT])
@pytest.mark.parametrize("integrator", [0, 1])
def test_tables_at_capacity(hip, integrator, S):
    x = cc.capacity_inputs()
    cfg, plan, gains, counts = x["cfg"], x["plan"], x["gains"], x["counts"]
    x0, gust = np.ascontiguousarray(x["x0"][:, :S]), np.ascontiguousarray(x["gust"][:, :S])
    assert x["shared"].shape == (cc.OB_MAX, 5) and x["own"].shape == (cc.CAP_B, cc.OB_MAX, 8) and counts.tolist() == [64, 0, 37]
    want = restate(x, x0, gust, x["shared"], x["own"], counts, integrator=integrator)
    # the placement, on the restatement: the last sphere in use of each table is the nearest of some flight
    nearest = [cc.nearest_sphere(want[0][b], cfg["dt"], x["shared"], x["own"][b, :counts[b]]) for b in range(cc.CAP_B)]
    assert (np.concatenate(nearest) == cc.OB_MAX - 1).any() and (nearest[0] == cc.OB_MAX + 63).any() and (nearest[2] == cc.OB_MAX + 36).any()
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    s.set_obstacles(x["shared"])
    s.set_batch_obstacles(x["own"], counts)
    traj, stats, score, kept = cc.scored_device(hip, s, plan, gains, x0, wrench=gust)
    assert_scored("full tables, integrator %d, S = %d" % (integrator, S), (traj, stats, score), want, plan)
    assert kept and (score[..., 3] > 0).any() and (score[..., 3] == 0).any()
    # (the plan with no sphere of its own is restated with the shared table alone: any of its 64 unused rows would cost 1e6 h^2)
    assert np.isfinite(score).all() and score[1, :, 0].max() < 1e5
    # the other end of the loops on the same handle: full tables of which only the first 8 shared spheres and own sphere 0 ever come
    # within 1 m, then those spheres alone (8 shared, K = 1): the same bytes, and the restatement's of the short tables
    for b in range(cc.CAP_B):
        c = cc.clearances(want[0][b], cfg["dt"], x["far_shared"], x["far_own"][b, :counts[b]])
        near = np.r_[np.arange(cc.CAP_NEAR), [cc.OB_MAX] if counts[b] else []].astype(int)
        assert np.delete(c, near, axis=2).min(initial=np.inf) > 1.0 and c[..., near].min() < 1.0
    s.set_obstacles(x["far_shared"])
    s.set_batch_obstacles(x["far_own"], counts)
    first = cc.scored_device(hip, s, plan, gains, x0, wrench=gust)
    s.set_obstacles(x["far_shared"][:cc.CAP_NEAR])
    s.set_batch_obstacles(x["far_own"][:, :1], np.minimum(counts, 1))
    second = cc.scored_device(hip, s, plan, gains, x0, wrench=gust)
    assert first[3] and second[3] and all(a.tobytes() == b.tobytes() for a, b in zip(first[:3], second[:3]))
    assert first[0].tobytes() == traj.tobytes() and first[2].tobytes() != score.tobytes()
    short = restate(x, x0, gust, x["far_shared"][:cc.CAP_NEAR], x["far_own"][:, :1], np.minimum(counts, 1), integrator=integrator)
    assert_scored("short tables, integrator %d, S = %d" % (integrator, S), second[:3], short, plan)


# ------------------------------------------------------------------------------------------------ 3. a second tile

@pytest.mark.parametrize("S", [1, cc.S_SHARED])
@pytest.mark.parametrize("integrator", [0, 1])
def test_a_second_tile_of_the_per_problem_table(hip, integrator, S):
    """S = 1: the flattened form, the problem changes from lane to lane and the tile inside the second block; S = 63: the shared-operand
    form, a block per problem, which gathers its row of the table into LDS"""
    x = cc.tile_inputs()
    cfg, plan, gains, counts = x["cfg"], x["plan"], x["gains"], x["counts"]
    x0, gust = np.ascontiguousarray(x["x0"][:, :S]), np.ascontiguousarray(x["gust"][:, :S])
    assert sorted(set(counts.tolist())) == [0, 1, 2, 3] and counts[69] > 0 and counts[63] == 0 and x["own"].shape == (70, 3, 8)

    def handle(rows):
        s = capi.from_config(cfg)
        s.set_integrator(integrator)
        s.set_obstacles(x["shared"])
        s.set_batch_obstacles(x["own"][rows], counts[rows])
        return s

    everyone = np.arange(cc.TILE_B)
    traj, stats, score, kept = cc.scored_device(hip, handle(everyone), plan, gains, x0, wrench=gust)
    assert kept and np.isfinite(traj).all() and np.isfinite(score[..., 0]).all() and flew_off_the_plan(traj, plan)
    for b in cc.TILE_ROWS:  # the same plan flown alone, on a handle whose table is that problem's rows
        one = cc.scored_device(hip, handle([b]), plan[b:b + 1], gains[b:b + 1], x0[b:b + 1], wrench=gust[b:b + 1])
        assert one[3] and one[0].tobytes() == traj[b:b + 1].tobytes() and one[1].tobytes() == stats[b:b + 1].tobytes(), b
        assert one[2].tobytes() == score[b:b + 1].tobytes(), b
    rows = [64, 69]
    want = restate(x, x0[rows], gust[rows], x["shared"], x["own"], counts, rows=rows, integrator=integrator)
    for k, b in enumerate(rows):  # the row's own spheres are felt: sphere 0 of its own is the nearest of its sample 0
        assert cc.nearest_sphere(want[0][k], cfg["dt"], x["shared"], x["own"][b, :counts[b]])[0] == len(x["shared"])
    assert_scored("rows 64 and 69 of 70, integrator %d, S = %d" % (integrator, S), (traj[rows], stats[rows], score[rows]), want, plan[rows])
    assert (score[rows, 0, 3] > 0).all()
