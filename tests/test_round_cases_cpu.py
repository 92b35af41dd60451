"""tests/round_cases.py holds what tests/test_gpu_round_instantiations.py needs it to hold -- shown without a GPU:
  names   its fifteen rows are exactly the k_round instantiations of the library (tests/golden/kernel_symbols.json);
  routes  each row's handle, through route.h itself (plan_route, round_form, round_instance: tests/host_route_harness.cpp), takes the row's own
          (LK, ROUNDS, SIX) in every launch: the batch entry and the single solve, at every count of running trajectories from B down to 1;
  inputs  the oracle's solutions of the families have the properties without which the bit comparisons would pass vacuously: iteration
          counts that differ inside a block of four, long solves, both converged statuses, backtracking, a failed search beside running
          neighbours, restarts, and the iteration cap at every position of a four-round and of a two-round launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import round_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = tuple(rc.LK_OF)


@pytest.fixture(scope="module")
def hr():
    from tests.linearize_cases import harness  # route.h built for the host: tests/host_route_harness.cpp
    lib = harness()
    lib.hr_round_form.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    return lib


def round_form(hr, kind, kw, B, several=True, seen=None, used=None, desired_batch=False, cost_hist=False, early_out=False):
    """(k_round launches, LK, ROUNDS, SIX, slot) of a launch on the handle qilqr_create makes of the kind's weights and the configuration"""
    symmetric, q_diag, layout_kind = rc.predicates(kind)
    fg = kw.get("force_general", 0)
    inp = np.array([symmetric and fg != 1, q_diag, layout_kind, fg, kw.get("round_launch", 0), kw.get("rounds_per_launch", 0), B, desired_batch,
                    cost_hist, early_out, several, B if seen is None else seen, B if used is None else used], dtype=np.int64)
    out = np.zeros(5, dtype=np.int64)
    assert hr.hr_round_form(inp.ctypes.data_as(C.POINTER(C.c_long)), out.ctypes.data_as(C.POINTER(C.c_long))) == 5
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------ names
def test_the_rows_are_the_library_s_k_round_instantiations():
    with open(os.path.join(HERE, "golden", "kernel_symbols.json")) as f:
        product = json.load(f)["product"]
    assert len(rc.ROWS) == 15 and sorted(r.slot for r in rc.ROWS) == list(range(15))
    assert sorted(rc.mangled(r) for r in rc.ROWS) == sorted(n for n in product if "k_round" in n)
    assert len({rc.row_id(r) for r in rc.ROWS}) == 15
    for r in rc.ROWS:
        assert r.slot == 5 * (r.lk - 1) + [(1, False), (1, True), (2, False), (4, False), (4, True)].index((r.rounds, r.six)), r


def test_the_weights_are_of_their_kinds():
    """qilqr_create's predicates are bit-exact: "sym" must have a non-zero coupling block, "block" exact zeros there and off-diagonal entries
    elsewhere, and all three symmetric Q and R"""
    assert rc.predicates("sym") == (True, False, 1) and rc.predicates("block") == (True, False, 2) and rc.predicates("diag") == (True, True, 2)
    (Qs, Rs), (Qb, Rb) = rc.weights("sym"), rc.weights("block")
    assert np.abs(Qs[:6, 6:]).min() > 0 and np.array_equal(Rs, Rb)
    assert np.array_equal(Qs[:6, :6], Qb[:6, :6]) and np.array_equal(Qs[6:, 6:], Qb[6:, 6:])
    for kind in KINDS:  # positive definite: the solves are well posed
        Q, R = rc.weights(kind)
        assert np.linalg.eigvalsh(Q).min() > 0 and np.linalg.eigvalsh(R).min() > 0, kind


# ------------------------------------------------------------------ routes
@pytest.mark.parametrize("row", rc.ROWS, ids=rc.row_id)
def test_each_row_s_handle_takes_the_row_s_instantiation(hr, row):
    want = (1, row.lk, row.rounds, int(row.six), row.slot)
    for B in sorted({len(p.init) for p in rc.every_bit_family()}):
        for facts in (dict(), dict(early_out=True), dict(desired_batch=True), dict(cost_hist=True), dict(desired_batch=True, early_out=True)):
            for seen in range(B, 0, -1):  # the batch entry: the launches may hold several rounds
                assert round_form(hr, row.weights, row.kw, B, seen=seen, **facts) == want, (B, facts, seen)
    # the single solve (qilqr_solve): one problem, one slot; its launches may hold several rounds as well
    assert round_form(hr, row.weights, row.kw, 1, several=True, seen=1, used=1) == want
    if row.rounds == 1:  # ... and a caller that looks at the solve round by round (several = false) gets the same launches
        assert round_form(hr, row.weights, row.kw, 1, several=False, seen=1, used=1) == want
        for B in (7, 9):
            assert round_form(hr, row.weights, row.kw, B, several=False, seen=1) == want


@pytest.mark.parametrize("kind", KINDS)
def test_the_comparand_and_the_other_configurations(hr, kind):
    lk = rc.LK_OF[kind]
    for B in (1, 7, 9):
        assert round_form(hr, kind, rc.COMPARAND, B)[0] == 0  # three launches: no k_round
        # the six-wavefront form is not instantiated for two rounds: force_general = 8 lands on (2, F)
        for seen in range(B, 0, -1):
            assert round_form(hr, kind, dict(force_general=8, rounds_per_launch=2), B, seen=seen) == (1, lk, 2, 0, rc.slot(lk, 2, False))
        # the automatic form: four fused rounds while more than half a block's trajectories run on average, the six-wavefront form from there
        got = {seen: round_form(hr, kind, dict(), B, seen=seen)[1:4] for seen in range(B, 0, -1)}
        blocks = (B + 3) // 4
        assert got == {seen: (lk, 4, int(2 * seen <= 4 * blocks)) for seen in got}, got
    assert round_form(hr, kind, dict(), 1)[1:4] == (lk, 4, 1)  # B = 1: sparse from the first launch
    assert {round_form(hr, kind, dict(), 9, seen=s)[3] for s in (9, 1)} == {0, 1}


# ------------------------------------------------------------------ inputs
def solved(kind, problem):
    return rc.oracle_solution(kind, problem)[1]


@pytest.mark.parametrize("kind", KINDS)
def test_every_family_s_solves_differ_inside_a_block(kind):
    """Every problem of every family with B >= 7 and n >= 16, under every kind of weights: at least three distinct iteration counts in the
    first block of four -- its trajectories leave the block in different rounds, and in different rounds of a launch -- and a longest solve
    of at least 17 iterations: five launches of four rounds.  (The seeds of hard and tracking were chosen for it: round_cases.HARD_SEEDS.)
    hard backtracks; plain and tracking end with status 0 and with status 1."""
    statuses = {"plain": set(), "tracking": set()}
    for p in rc.every_bit_family():
        ref = solved(kind, p)
        B, n = p.init.shape[:2]
        family = p.name.split("(")[0]
        if B >= 7 and n >= 16:
            assert len(set(ref["iters"][:4].tolist())) >= 3 and ref["iters"].max() >= 17, (p.name, ref["iters"])
        if p.options or p.mu:  # (the one-trial case and the restarts: their own conditions below)
            continue
        assert np.isfinite(ref["traj"]).all() and (ref["status"] >= 0).all(), p.name
        if family == "hard":
            assert (ref["n_fwd"] > ref["iters"]).any(), (p.name, ref["n_fwd"], ref["iters"])  # backtracking
        if family in statuses:
            statuses[family] |= set(ref["status"].tolist())
    assert {0, 1} <= statuses["plain"] and {0, 1} <= statuses["tracking"], statuses


@pytest.mark.parametrize("kind", KINDS)
def test_one_trial_fails_beside_running_neighbours_and_restarts_restart(kind):
    ref = solved(kind, rc.one_trial())
    failed = np.nonzero(ref["status"] == 3)[0]
    assert len(failed) > 0, ref["status"]
    assert any((ref["iters"][4 * (b // 4):4 * (b // 4) + 4] > ref["iters"][b]).any() for b in failed), (ref["status"], ref["iters"])
    again = solved(kind, rc.restarts())
    assert (again["n_bwd"] > again["iters"] + 1).any(), (again["n_bwd"], again["iters"])


@pytest.mark.parametrize("kind", KINDS)
def test_the_cap_falls_on_every_position_of_a_launch(kind):
    for cap in rc.CAPS:
        ref = solved(kind, rc.capped(cap))
        assert (ref["iters"] == cap).all() and (ref["status"] == 2).all(), (cap, ref["iters"], ref["status"])
    assert {c % 4 for c in rc.CAPS} == {0, 1, 2, 3} and {c % 2 for c in rc.CAPS} == {0, 1}
