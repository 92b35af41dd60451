"""The table of tests/linearize_cases.py covers every k_linearize instantiation a handle can reach: the whole public input space through
plan_route (tests/host_route_harness.cpp, hr_lin_route) gives the reachable keys; they are admitted ones (tests/golden/linearize_keys.json),
the admitted keys beyond them are the two named here, and the table's keys are the reachable set.  Also: the roads the table must hold
(thrust limits, a schedule with every extension form), the route's text each case expects, the weights of each kind, and the margins of the
mixed-mode cases against config3's own."""
import json
import os

import numpy as np
import pytest

from tests import linearize_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))

# admitted by lin_instantiated, compiled, and launched by no handle: {lin_kind, integrator, tiled, f32, ext} -> why
UNREACHABLE = {
    (0, 0, 1, 0, 0): "dense records (kind 0) placed tiled, fp64: tiled records are k_backward4's, which needs exactly symmetric Q and R, and a "
                     "symmetric Q has kind 1 at least; a schedule forces kind 0 but also the one-wavefront kernel, whose records are plain",
    (0, 0, 1, 1, 0): "its mixed-precision twin: the same, and the mixed mode takes no schedule",
}


@pytest.fixture(scope="module")
def admitted():
    with open(os.path.join(HERE, "golden", "linearize_keys.json")) as f:
        rows = {tuple(r) for r in json.load(f)["rows"]}
    assert len(rows) == 58
    return rows


@pytest.fixture(scope="module")
def reachable():
    """(qilqr_cost_trajectory ignores the models: it takes the route of the same handle without them, which the enumeration holds as well)"""
    keys = set()
    count = 0
    for c in lc.every_input():
        for B in (3, 70, 5000):  # (the key does not depend on the batch: both forms of k_backward4 read tiled records)
            key, _, ok = lc.route(c, B)
            assert ok, (c, B, key)  # a route without an instantiation would be refused at the launch
            keys.add(key)
        count += 1
    assert count == 4488  # of 13824 combinations: the setters refuse the rest
    return keys


def test_the_weights_of_each_kind_have_its_predicates():
    want = dict(diag=(1, 1, 1, 1), block=(1, 1, 1, 0), sym=(1, 1, 0, 0), qsym=(1, 0, 0, 0), nonsym=(0, 0, 0, 0), block_qsym=(1, 0, 1, 0))
    for w in lc.WEIGHTS:
        for seed in (1, 3, 4000, 4077):
            cfg = lc.config(w, seed, n=2, B=1)
            p = lc.predicates(cfg["Q"], cfg["R"])
            assert (p["q_sym"], p["r_sym"], p["ur_zero"], p["q_diag"]) == tuple(map(bool, want[w])), (w, seed, p)
            assert np.linalg.eigvalsh(0.5 * (cfg["Q"] + cfg["Q"].T)).min() > 0 and np.linalg.eigvalsh(0.5 * (cfg["R"] + cfg["R"].T)).min() > 0
    Q, _ = lc.block_weights(5)  # dense blocks, unlike each other
    assert np.count_nonzero(Q[:6, :6]) == 36 and np.count_nonzero(Q[6:, 6:]) == 36 and not np.array_equal(Q[6:, 6:], Q[:6, :6])


def test_the_reachable_keys_are_admitted_and_the_rest_is_named(admitted, reachable):
    assert reachable <= admitted, sorted(reachable - admitted)
    assert admitted - reachable == set(UNREACHABLE), {"unreached and not named": sorted(admitted - reachable - set(UNREACHABLE)),
                                                      "named but reached": sorted(set(UNREACHABLE) & reachable)}
    assert len(reachable) == 56 and sum(1 for k in reachable if k[3]) == 5


def test_the_table_covers_the_reachable_keys(reachable):
    keys = {lc.route(c)[0] for c in lc.TABLE}
    assert all(lc.accepted(c) for c in lc.TABLE)
    assert keys == reachable, {"not covered": sorted(reachable - keys), "not reachable": sorted(keys - reachable)}
    assert {lc.route(c)[0] for c in lc.F32} == {k for k in reachable if k[3]} and len(lc.F32) == 5


def test_the_table_reaches_the_plain_symmetric_kinds_through_thrust_limits():
    seen = {lc.route(c)[0][0] for c in lc.TABLE if c.limits and lc.route(c)[0][2] == 0 and not c.schedule and lc.route(c)[1] == lc.BW_ONE}
    assert {1, 2, 3} <= seen, seen


def test_the_table_has_a_scheduled_case_for_every_extension_form():
    # (the five forms with an extension argument; the table also holds the plain one)
    forms = {lc.route(c)[0][4] for c in lc.TABLE if c.schedule}
    assert forms >= {lc.EXT[f] for f in ("models", "shared", "models+shared", "problem", "models+problem")}, forms
    assert all(lc.route(c)[0][:1] == (0,) and lc.route(c)[0][2] == 0 for c in lc.TABLE if c.schedule)
    assert {c.schedule for c in lc.TABLE if c.schedule} == {"terminal", "dense", "nonsym"}


def test_the_table_reaches_kind_2_with_every_form_and_either_integrator():
    """the block-diagonal kind beside each extension form: what the suite had not run before this table"""
    got = {k[1:] for k in (lc.route(c)[0] for c in lc.TABLE if c.weights in ("block", "block_qsym")) if k[0] == 2}
    want = {(i, 0, 0, e) for i in (0, 1) for e in lc.EXT.values()} | {(0, 1, 0, e) for e in (0, 2, 6)} | {(0, 1, 1, 0)}
    assert got >= want, sorted(want - got)


@pytest.mark.parametrize("B", [3, 70])
def test_the_text_each_case_expects_follows_from_the_route(B):
    for c in lc.TABLE:
        assert lc.expected_text(c, B) == lc.text_from_route(c, B), (lc.name(c), B)
        assert (lc.recursion(c) == 0) == ("reference's own" in lc.expected_text(c, B)[0])
    assert len({lc.name(c) for c in lc.TABLE}) == len(lc.TABLE)


def test_the_mixed_cases_keep_config3s_margin_to_the_bars():
    """How far the fp64 restatement moves when its inputs, model and weights are rounded to fp32, against the per-pass bars of
    test_config3_mixed_precision_reduced: every new case leaves at least the room config3's own weights leave (bar / deviation)."""
    own = lc.mixed_margins(None)
    print("config3's own weights: bar / deviation =", {k: "%.3g" % v for k, v in own.items()})
    assert all(v > 1.0 for v in own.values()), own
    for c in lc.F32:
        got = lc.mixed_margins(c)
        print(lc.name(c), {k: "%.3g" % v for k, v in got.items()})
        for k in own:
            assert got[k] >= own[k], (lc.name(c), k, got[k], own[k])
