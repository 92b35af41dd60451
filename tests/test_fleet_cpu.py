"""Fleet deconfliction without a device: the routines of quadrotorilqr_amd/csrc/fleet_math.h and the rules of fleet_launch.h, compiled with
g++ into the stand-alone program tests/host_fleet_harness.cpp, against the restatement (tests/fleet_numpy.py, which includes none of
them), against answers known without one, and against themselves under other chunkings; the refusals through the program and through the
C ABI; the kernels of fleet.hip by name.

THE BARS.  Decided words (a partner, a knot, a count, the number in conflict) are compared exactly, on inputs whose sorted d2 lie further
apart than 1e-9 relative (asserted on the restatement alone).  Distances: 4 eps relative (three roundings of the square sum, one of the
root, on either side).  The fit: the restatement's sums are NumPy's, neither fused nor sequential, so c and the residual get
16 n eps max(1, max |p|) and v the same over (n - 1) dt; the observed error is printed, and stayed below a tenth of that bar."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from quadrotorilqr_amd import capi
from tests import fleet_cases as fc, fleet_numpy as fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
KERNELS = ["_ZN5qilqr11k_fleet_fitENS_12FleetFitArgsE", "_ZN5qilqr13k_fleet_pairsEPKdNS_14FleetPairsArgsE", "_ZN5qilqr14k_fleet_selectENS_15FleetSelectArgsE",
           "_ZN5qilqr9k_bob_setENS_10BobSetArgsE"]
KEYS = ("summary", "nbr", "spheres", "counts")


@pytest.fixture(scope="module")
def harness():
    return fc.build_harness()


def same_bytes(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in KEYS)


def compare(got, want, plan, V, K, n, label):
    """the program against the restatement: decided words exactly, distances to 4 eps, the fit words to their bar"""
    assert np.array_equal(got["counts"], want["counts"]), label
    assert np.array_equal(got["nbr"][:, :, [0, 2]], want["nbr"][:, :, [0, 2]]), label
    assert np.array_equal(got["summary"][:, [1, 2, 3, 4]], want["summary"][:, [1, 2, 3, 4]]), label
    for a, b in ((got["nbr"][:, :, 1], want["nbr"][:, :, 1]), (got["summary"][:, 0], want["summary"][:, 0])):
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin]), label
        assert (np.abs(a[fin] - b[fin]) <= 4 * EPS * np.abs(b[fin])).all(), label
    bar = 16 * n * EPS * max(1.0, np.abs(plan[:, :, 1:4]).max())
    vbar = bar / ((n - 1) * fc.DT) if n > 1 else 0.0
    ec = np.abs(got["spheres"][:, :, :3] - want["spheres"][:, :, :3]).max()
    ev = np.abs(got["spheres"][:, :, 3:6] - want["spheres"][:, :, 3:6]).max()
    er = max(np.abs(got["spheres"][:, :, 6] - want["spheres"][:, :, 6]).max(), np.abs(got["nbr"][:, :, 3] - want["nbr"][:, :, 3]).max(),
             np.abs(got["summary"][:, 5] - want["summary"][:, 5]).max())
    print("[observed] %s: c %.3g, residual %.3g of %.3g; v %.3g of %.3g" % (label, ec, er, bar, ev, vbar))
    assert ec <= bar and er <= bar and ev <= vbar, label
    assert np.array_equal(got["spheres"][:, :, 7], want["spheres"][:, :, 7]), label


# ------------------------------------------------------------------------------------------------ 1. the program against the restatement

@pytest.mark.parametrize("B, V, n, K, seed", [(12, 12, 17, 4, 1), (30, 10, 9, 3, 2), (70, 70, 5, 16, 3), (8, 4, 2, 8, 4)])
@pytest.mark.parametrize("flags", [dict(), dict(cover=True), dict(yield_to_lower=True), dict(cover=True, yield_to_lower=True, range=9.0, conflict=4.0)])
def test_the_program_against_the_restatement(harness, B, V, n, K, seed, flags):
    plan = fc.random_plans(B, n, seed)
    assert fn.gaps(plan, V) > 1e-9  # (on the restatement alone: no near-ties among an ego's sorted d2)
    want = fn.neighbours(plan, V, K, fc.DT, **fc.RULE, **flags)
    got = fc.host_run(harness, plan, V, K, **flags)
    compare(got, want, plan, V, K, n, str((B, V, n, K, flags)))
    assert got["counts"].max() > 0


def test_the_fit_is_where_a_moving_sphere_stands(harness):
    """a vehicle on an exact line c + t v with representable words is fitted exactly: residual 0, and fma(t_i, v, c) is its knot"""
    plan = fc.hover(3, 9)
    c, v = np.array([[1.0, -2.0, 0.5], [0.0, 4.0, 8.0], [-3.0, 0.25, 2.0]]), np.array([[2.0, 0.0, -1.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0]])
    t = np.arange(9) * 0.25
    plan[:, :, 1:4] = c[:, None] + t[None, :, None] * v[:, None]
    fit = fc.host_run(harness, plan, 3, 2, dt=0.25)["fit"]
    assert np.array_equal(fit[:, :3], c) and np.array_equal(fit[:, 3:6], v) and not fit[:, 6].any() and (fit[:, 7] == 1).all()


# ------------------------------------------------------------------------------------------------ 2. ties, exactly

def test_equal_distances_go_to_the_smaller_row_and_equal_knots_to_the_first(harness):
    # ego 0 at the origin; partners 1, 2, 3 at distance 2 on three axes at every knot: the list is rows 1, 2, 3, each at knot 0
    plan = fc.hover(4, 5)
    plan[1, :, 1], plan[2, :, 2], plan[3, :, 3] = 2.0, -2.0, 2.0
    got = fc.host_run(harness, plan, 4, 3)
    assert np.array_equal(got["nbr"][0, :, 0], [1, 2, 3]) and np.array_equal(got["nbr"][0, :, 2], [0, 0, 0]) and np.array_equal(got["nbr"][0, :, 1], [2, 2, 2])
    assert np.array_equal(got["summary"][0, :3], [2.0, 0.0, 1.0])
    # partner 3 comes closer at knots 2 and 4, equally: it leads the list with knot 2
    plan[3, 2, 3] = plan[3, 4, 3] = 1.0
    got = fc.host_run(harness, plan, 4, 2)
    assert np.array_equal(got["nbr"][0, :, 0], [3, 1]) and np.array_equal(got["nbr"][0, :, 2], [2, 0]) and np.array_equal(got["summary"][0, :3], [1.0, 2.0, 3.0])


@pytest.mark.parametrize("flags", [dict(), dict(yield_to_lower=True)])
def test_integer_coordinates_against_the_restatement_exactly(harness, flags):
    """on an integer grid every d2 is exact on either side, ties abound, and the decided words agree whatever the order of the sums"""
    plan = fc.integer_plans(40, 6, 7)
    want = fn.neighbours(plan, 20, 5, fc.DT, **fc.RULE, **flags)
    got = fc.host_run(harness, plan, 20, 5, **flags)
    assert np.array_equal(got["nbr"][:, :, :3], want["nbr"][:, :, :3]) and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["summary"][:, :5], want["summary"][:, :5])


# ------------------------------------------------------------------------------------------------ 3. the list does not depend on the chunks

@pytest.mark.parametrize("plans", ["random", "integer"])
def test_chunks_of_1_7_64_and_V_partners_give_the_same_bytes(harness, plans):
    V, K = 130, 16
    plan = fc.random_plans(2 * V, 4, 11) if plans == "random" else fc.integer_plans(2 * V, 4, 12, side=2)
    for flags in (dict(), dict(yield_to_lower=True, cover=True, range=6.0)):
        whole = fc.host_run(harness, plan, V, K, chunk=V, **flags)
        for chunk in (1, 7, 64):
            assert same_bytes(fc.host_run(harness, plan, V, K, chunk=chunk, **flags), whole), (plans, flags, chunk)


# ------------------------------------------------------------------------------------------------ 4. edge cases

def test_yield_to_lower_row_0_of_each_fleet_yields_to_nobody_and_the_summary_is_the_flags(harness):
    plan = fc.random_plans(18, 7, 21, spread=3.0)
    both = fc.host_run(harness, plan, 6, 4, conflict=4.0)
    low = fc.host_run(harness, plan, 6, 4, conflict=4.0, yield_to_lower=True)
    assert not low["counts"][::6].any() and (low["nbr"][::6, :, 0] == -1).all() and both["counts"][::6].all()
    assert np.array_equal(low["summary"][:, :4], both["summary"][:, :4]) and both["summary"][:, 3].any()
    for b in range(18):
        rows = low["nbr"][b, :, 0]
        assert (rows[rows >= 0] < b).all() and np.count_nonzero(rows >= 0) == min(4, b % 6)


def test_the_range_cut_and_cover(harness):
    plan = fc.random_plans(9, 12, 22, spread=4.0)
    wide = fc.host_run(harness, plan, 9, 8)
    assert (wide["counts"] == 8).all()
    cut = float(np.median(wide["nbr"][:, :, 1]))
    near = fc.host_run(harness, plan, 9, 8, range=cut)
    assert np.array_equal(near["counts"], (wide["nbr"][:, :, 1] < cut).sum(axis=1)) and np.array_equal(near["nbr"], wide["nbr"])
    for b in range(9):
        assert np.array_equal(near["spheres"][b, :near["counts"][b]], wide["spheres"][b, :near["counts"][b]]) and not near["spheres"][b, near["counts"][b]:].any()
    cover = fc.host_run(harness, plan, 9, 8, cover=True)
    assert np.array_equal(cover["spheres"][:, :, 6], fc.RULE["radius"] + wide["nbr"][:, :, 3]) and (wide["nbr"][:, :, 3] > 0).all()
    assert np.array_equal(cover["summary"][:, 5], cover["spheres"][:, :, 6].max(axis=1)) and (wide["summary"][:, 5] == fc.RULE["radius"]).all()
    assert np.array_equal(cover["spheres"][:, :, :6], wide["spheres"][:, :, :6])


def test_a_distance_on_the_boundary_of_range_and_of_conflict(harness):
    """the rule compares squares, d2 < range^2 with the square rounded once.  On the boundary itself: a partner at exactly 5 m (3, 4, 0: d2 = 25
    exactly) is no neighbour for range = 5 and not in conflict for conflict = 5, as `distance < range` says, and is both one ulp above.
    Off integers the two forms can part by an ulp of the threshold: at range = sqrt(2) rounded down, range^2 rounds to a value below 2, and a
    partner at d2 = 2 -- whose rounded root EQUALS that range -- is no neighbour by either form; the test pins what the rule does there."""
    plan = fc.hover(2, 3)
    plan[1, :, 1], plan[1, :, 2] = 3.0, 4.0
    up = float(np.nextafter(5.0, 6.0))
    at = fc.host_run(harness, plan, 2, 1, range=5.0, conflict=5.0)
    above = fc.host_run(harness, plan, 2, 1, range=up, conflict=up)
    assert not at["counts"].any() and not at["summary"][:, 3].any() and (at["nbr"][:, 0, 1] == 5.0).all()
    assert (above["counts"] == 1).all() and (above["summary"][:, 3] == 1).all()
    for r in (5.0, up):  # (here the restatement's `sqrt(d2) < range` says the same)
        assert np.array_equal(fn.neighbours(plan, 2, 1, fc.DT, **fc.RULE, range=r, conflict=r)["counts"], fc.host_run(harness, plan, 2, 1, range=r, conflict=r)["counts"])
    plan[1, :, 1], plan[1, :, 2] = 1.0, 1.0  # d2 = 2 exactly
    root = float(np.sqrt(2.0))
    assert root * root > 2.0  # (sqrt(2) rounds up: its square lies above 2)
    got = fc.host_run(harness, plan, 2, 1, range=root)
    assert (got["nbr"][:, 0, 1] == root).all() and (got["counts"] == 1).all()  # d2 = 2 < range^2, while sqrt(d2) == range: the forms part here, by the rule's statement
    assert not fc.host_run(harness, plan, 2, 1, range=float(np.nextafter(root, 0.0)))["counts"].any()


def test_more_neighbours_asked_for_than_partners_one_vehicle_and_one_knot(harness):
    plan = fc.random_plans(6, 5, 23)
    got = fc.host_run(harness, plan, 3, 8)  # K > V - 1
    assert (got["counts"] == 2).all() and (got["nbr"][:, 2:, 0] == -1).all() and np.isinf(got["nbr"][:, 2:, 1]).all() and (got["nbr"][:, 2:, 2] == -1).all()
    assert not got["nbr"][:, 2:, 3].any() and not got["spheres"][:, 2:].any()
    one = fc.host_run(harness, plan, 1, 4)  # V = 1
    assert np.isinf(one["summary"][:, 0]).all() and (one["summary"][:, 1:3] == -1).all() and not one["summary"][:, 3:].any() and not one["counts"].any()
    knot = fc.host_run(harness, plan[:, :1], 3, 2)  # n = 1: v = 0, c = p_0, residual 0
    assert not knot["fit"][:, 3:7].any() and np.array_equal(knot["fit"][:, :3], plan[:, 0, 1:4]) and (knot["nbr"][:, :, 2] == 0).all()
    assert same_bytes(knot, fc.host_run(harness, plan[:, :1], 3, 2, chunk=1))


def test_a_vehicle_that_is_nowhere_is_nobodys_neighbour_and_is_skipped_in_counts(harness):
    plan = fc.random_plans(5, 6, 24, spread=2.0)
    ref = fc.host_run(harness, plan, 5, 4)
    gone = plan.copy()
    gone[2, :, 1:4] = np.nan
    got = fc.host_run(harness, gone, 5, 4)
    others = [0, 1, 3, 4]
    assert (got["counts"][others] == 3).all() and got["counts"][2] == 0 and np.isinf(got["summary"][2, 0]) and got["summary"][2, 2] == -1
    for b in others:  # listed last, at +inf and knot -1, and no sphere
        assert got["nbr"][b, 3, 0] == 2 and np.isinf(got["nbr"][b, 3, 1]) and got["nbr"][b, 3, 2] == -1 and not got["spheres"][b, 3].any()
        assert np.array_equal(got["nbr"][b, :3, :3], ref["nbr"][b][ref["nbr"][b, :, 0] != 2][:, :3])
    # NaN at one knot only: the pair has a finite distance from the other knots, the fit is not finite, and the partner's counts skip it
    part = plan.copy()
    part[2, 3, 2] = np.nan
    got = fc.host_run(harness, part, 5, 4)
    assert (got["counts"][others] == 3).all() and got["counts"][2] == 4 and np.isfinite(got["nbr"][:, :, 1]).all() and np.isfinite(got["spheres"]).all()
    assert (got["summary"][others, 4] == 3).all()


def test_two_fleets_do_not_see_each_other(harness):
    plan = fc.random_plans(14, 6, 25)
    both = fc.host_run(harness, plan, 7, 5)
    for g in range(2):
        alone = fc.host_run(harness, plan[7 * g:7 * g + 7], 7, 5)
        shifted = dict(alone, nbr=alone["nbr"].copy(), summary=alone["summary"].copy())
        shifted["nbr"][:, :, 0] += 7 * g
        shifted["summary"][:, 2] += 7 * g
        assert same_bytes(shifted, {k: both[k][7 * g:7 * g + 7] for k in KEYS}), g


# ------------------------------------------------------------------------------------------------ 5. the row rule of the device-side setter

@pytest.mark.parametrize("B, K", [(8, 4), (70, 3), (64, 1), (129, 64)])
def test_a_table_whose_rows_all_pass_has_the_bytes_of_bob_relayout(harness, B, K):
    sp = fc.valid_spheres(B, K, B + K)
    got = fc.host_bob(harness, sp)
    assert got["tab"].tobytes() == got["relaid"].tobytes() and (got["counts"] == K).all() and got["dropped"] == 0
    counts = (np.arange(B) + 1) % (K + 1)
    zeroed = np.where(np.arange(K)[None, :, None] < counts[:, None, None], sp, 0.0)
    got = fc.host_bob(harness, sp, counts)  # (rows at or beyond a count are written as zeros whatever they held)
    assert got["tab"].tobytes() == fc.host_bob(harness, zeroed, counts)["relaid"].tobytes() and np.array_equal(got["counts"], counts) and got["dropped"] == 0


def test_dropped_rows_compact_in_order_and_are_counted(harness):
    B, K = 70, 6
    sp = fc.valid_spheres(B, K, 5)
    bad = np.zeros((B, K), dtype=bool)
    for b, j, w, value in ((0, 0, 6, 0.0), (0, 3, 7, -1.0), (1, 5, 2, np.nan), (65, 1, 4, np.inf), (65, 2, 6, -2.0), (69, 0, 0, -np.inf), (3, 4, 6, np.nan)):
        sp[b, j, w], bad[b, j] = value, True
    counts = np.full(B, K)
    counts[2], counts[3], counts[4], counts[5] = 0, 4, -3, K + 9  # (row (3, 4) lies beyond its count: not looked at, not dropped; counts are clamped)
    used = np.arange(K)[None] < np.clip(counts, 0, K)[:, None]
    want = np.zeros_like(sp)
    for b in range(B):
        rows = sp[b][used[b] & ~bad[b]]
        want[b, :len(rows)] = rows
    got = fc.host_bob(harness, sp, counts)
    assert got["dropped"] == int((used & bad).sum()) == 6
    assert np.array_equal(got["counts"], (used & ~bad).sum(axis=1))
    assert got["tab"].tobytes() == fc.host_bob(harness, want)["relaid"].tobytes()


# ------------------------------------------------------------------------------------------------ 6. what the calls refuse
OK_CALL = dict(rule=1, radius=0.8, weight=50.0, range="inf", conflict=0.8, flags=3, reserved=0, plan=1 << 20, summary=1 << 16, nbr=1 << 17, spheres=1 << 18,
               counts=1 << 19, B=4, n=6, V=2, K=3, handle=1, f32=0)
ORDER = tuple(OK_CALL)
# in the order of the rule (fleet_launch.h)
REFUSALS = [
    (dict(rule=0), "null argument"), (dict(plan=0), "null argument"),
    (dict(summary=0, nbr=0, spheres=0, counts=0), "no output"),
    (dict(B=0), "must be positive"), (dict(n=-1), "must be positive"), (dict(V=0), "must be positive"), (dict(V=3), "V must divide B"),
    (dict(K=0), "K must be 1"), (dict(K=17), "K must be 1"),
    (dict(radius=0.0), "radius"), (dict(radius="inf"), "radius"), (dict(radius="nan"), "radius"), (dict(weight=-1.0), "weight"), (dict(weight="inf"), "weight"),
    (dict(range=0.0), "range"), (dict(range="nan"), "range"), (dict(conflict=-0.5), "conflict"), (dict(conflict="inf"), "conflict"),
    (dict(flags=4), "unknown flag bits"), (dict(reserved=1), "reserved word"),
    (dict(plan=(1 << 20) + 8), "16-byte aligned"), (dict(nbr=(1 << 17) + 8), "16-byte aligned"), (dict(counts=(1 << 19) + 2), "16-byte aligned"),
    (dict(summary=(1 << 20) + 16), "an output overlaps the plan"), (dict(counts=(1 << 20) + 4 * 6 * 18 * 8 - 4), "an output overlaps the plan"),
    (dict(nbr=(1 << 16) + 16), "the outputs overlap each other"), (dict(counts=(1 << 18) + 4 * 3 * 8 * 8 - 4), "the outputs overlap each other"),
    (dict(handle=0), "null handle"), (dict(f32=1), "precision 0"),
]
ADMITTED = [dict(), dict(summary=0), dict(nbr=0, spheres=0, counts=0), dict(flags=0), dict(V=4), dict(V=1), dict(K=16), dict(range=1e-3), dict(conflict=0.0),
            dict(weight=0.0), dict(counts=(1 << 19) + 4), dict(nbr=(1 << 16) + 4 * 8 * 8), dict(counts=(1 << 18) + 4 * 3 * 8 * 8)]
MOVED = ("plan", "summary", "nbr", "spheres", "counts", "B", "n", "V", "K")

OK_BOB = dict(handle=1, f32=0, spheres=1 << 16, counts=1 << 12, dropped=1 << 10, B=8, K=4)
BOB_ORDER = tuple(OK_BOB)
BOB_REFUSALS = [(dict(handle=0), "null argument"), (dict(spheres=0), "null argument"), (dict(B=0), "B must be positive"), (dict(B=-2), "B must be positive"),
                (dict(K=0), "K must be 1"), (dict(K=65), "K must be 1"), (dict(spheres=(1 << 16) + 8), "aligned"), (dict(counts=(1 << 12) + 2), "aligned"),
                (dict(dropped=(1 << 10) + 1), "aligned"), (dict(f32=1), "precision 0")]


def rule(exe, **change):
    call = dict(OK_CALL, **change)
    return subprocess.check_output([exe, "refuse"] + [str(call[k]) for k in ORDER]).decode().strip()


def bob_rule(exe, **change):
    call = dict(OK_BOB, **change)
    return subprocess.check_output([exe, "refuse_bob"] + [str(call[k]) for k in BOB_ORDER]).decode().strip()


def test_the_rule_of_what_the_neighbours_call_refuses_and_its_order(harness):
    for change, why in REFUSALS:
        assert re.search(why, rule(harness, **change)), (change, rule(harness, **change))
    for change in ADMITTED:
        assert rule(harness, **change) == "ok", (change, rule(harness, **change))
    # the order: a row's reason stands with every later row's fault added at once (but for the pointers and shapes a later row moves)
    for k, (change, why) in enumerate(REFUSALS):
        later = {}
        for other, _ in REFUSALS[k + 1:]:
            later.update({key: v for key, v in other.items() if key not in change and key not in later and key not in MOVED})
        got = rule(harness, **dict(later, **change))
        assert re.search(why, got), (change, later, got)


def test_the_rule_of_what_the_device_setter_refuses_and_its_order(harness):
    for change, why in BOB_REFUSALS:
        assert re.search(why, bob_rule(harness, **change)), (change, bob_rule(harness, **change))
    for change in (dict(), dict(counts=0), dict(dropped=0), dict(K=64), dict(counts=(1 << 12) + 4)):
        assert bob_rule(harness, **change) == "ok", change
    for k, (change, why) in enumerate(BOB_REFUSALS):
        later = {}
        for other, _ in BOB_REFUSALS[k + 1:]:
            later.update({key: v for key, v in other.items() if key not in change and key not in later})
        assert re.search(why, bob_rule(harness, **dict(later, **change))), (change, later)


def test_the_abi_without_a_device(harness):
    """the structure and every refusal that needs no handle, through ctypes: the arguments are looked at before the handle"""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    for name in ("qilqr_fleet_neighbours_device", "qilqr_set_batch_obstacles_device"):
        assert re.search(r"\bint %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name), name
    assert C.sizeof(capi.FleetRule) == 40 and capi.FleetRule.flags.offset == 32 and capi.FleetRule.reserved.offset == 36
    assert subprocess.check_output([harness, "sizeof"]).decode().strip() == "40" and "} qilqr_fleet_rule;" in header
    assert lib.qilqr_abi_version() == 7 and "#define QILQR_ABI_VERSION 7" in header
    for name, value in (("QILQR_FLEET_MAX_NEIGHBOURS", "16"), ("QILQR_FLEET_NBR", "4"), ("QILQR_FLEET_SUMMARY", "8"), ("QILQR_FLEET_COVER", "1u"),
                        ("QILQR_FLEET_YIELD_TO_LOWER", "2u")):
        assert re.search(r"#define %s %s\b" % (name, value), header)
    assert (capi.FLEET_MAX_NEIGHBOURS, capi.FLEET_NBR, capi.FLEET_SUMMARY, capi.FLEET_COVER, capi.FLEET_YIELD_TO_LOWER) == (16, 4, 8, 1, 2)
    r = capi.fleet_rule(0.8, 50.0)
    assert (r.radius, r.weight, r.range, r.conflict, r.flags, r.reserved) == (0.8, 50.0, np.inf, 0.8, 0, 0)
    r = capi.fleet_rule(1.0, 2.0, range=5.0, conflict=0.5, cover=True, yield_to_lower=True)
    assert (r.range, r.conflict, r.flags) == (5.0, 0.5, 3)
    b, n, k = 4, 6, 3
    arrays = dict(plan=capi._d16(np.zeros((b, n, 18))), summary=capi._d16(np.zeros((b, 8))), nbr=capi._d16(np.zeros((b, k, 4))),
                  spheres=capi._d16(np.zeros((b, k, 8))), counts=np.zeros(b + 4, dtype=np.int32))
    odd = capi._d16(np.zeros(b * k * 8 + 2))[1:]
    assert odd.ctypes.data % 16 == 8

    def call(with_rule=True, radius=0.8, weight=1.0, range=np.inf, conflict=0.8, flags=0, reserved=0, B=b, V=2, K=k, **ptr):
        a = {key: (v.ctypes.data if v is not None else None) for key, v in dict(arrays, **ptr).items()}
        r = capi.FleetRule(radius, weight, range, conflict, flags, reserved)
        rc = lib.qilqr_fleet_neighbours_device(None, C.byref(r) if with_rule else None, a["plan"], B, n, V, K, a["summary"], a["nbr"], a["spheres"], a["counts"])
        return rc, lib.qilqr_last_error().decode()

    for change, why in [(dict(with_rule=False), "null argument"), (dict(plan=None), "null argument"), (dict(summary=None, nbr=None, spheres=None, counts=None), "no output"),
                        (dict(B=0), "must be positive"), (dict(V=3), "V must divide B"), (dict(K=17), "K must be 1"), (dict(radius=-1.0), "radius"),
                        (dict(weight=float("nan")), "weight"), (dict(range=0.0), "range"), (dict(conflict=float("inf")), "conflict"), (dict(flags=8), "unknown flag bits"),
                        (dict(reserved=5), "reserved word"), (dict(spheres=odd), "16-byte aligned"), (dict(nbr=arrays["plan"]), "an output overlaps the plan"),
                        (dict(summary=arrays["spheres"]), "the outputs overlap each other"), (dict(), "null handle"), (dict(summary=None, counts=None), "null handle")]:
        rc, text = call(**change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)
    rc = lib.qilqr_set_batch_obstacles_device(None, arrays["spheres"].ctypes.data, None, b, k, None)
    assert rc == capi.ERR_INVALID_ARG and "null argument" in lib.qilqr_last_error().decode()


# ------------------------------------------------------------------------------------------------ 7. the program under the sanitizers

def test_the_program_under_the_address_and_undefined_behaviour_sanitizers():
    """the stand-alone program, compiled and run once with -fsanitize=address,undefined: chunks, both flags, a NaN vehicle, the setter's rule, the rules"""
    exe = fc.build_harness(("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), "host_fleet_harness_san")
    plan = fc.random_plans(2 * 67, 5, 31)
    plan[5, :, 1:4] = np.nan
    for chunk in (1, 7, 64, 67):
        got = fc.host_run(exe, plan, 67, 16, chunk=chunk, cover=True, yield_to_lower=True, range=8.0)
        assert np.isfinite(got["spheres"]).all() and got["counts"].max() > 0
    fc.host_run(exe, plan[:3, :1], 1, 1)
    sp = fc.valid_spheres(70, 5, 32)
    sp[69, 4, 6] = -1.0
    assert fc.host_bob(exe, sp, np.arange(70) % 5 - 1)["dropped"] == 0 and fc.host_bob(exe, sp)["dropped"] == 1
    assert rule(exe) == "ok" and bob_rule(exe) == "ok"


# ------------------------------------------------------------------------------------------------ 8. the kernels of the unit, by name

@pytest.mark.parametrize("defines", [[], ["-DQILQR_DIAG"]])
def test_the_kernels_of_the_unit_are_the_listed_ones(defines):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
    asm = subprocess.check_output([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + defines +
                                  ["-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, "fleet.hip")], stderr=subprocess.DEVNULL).decode()
    got = sorted({line.split()[1] for line in asm.splitlines() if line.lstrip().startswith(".amdhsa_kernel ")})
    assert got == sorted(KERNELS), got
    # no kernel keeps anything in scratch memory (the kernel descriptors' metadata)
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm) == ["0"] * len(KERNELS)
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "SRCS    += fleet.hip\n" in f.readlines()
