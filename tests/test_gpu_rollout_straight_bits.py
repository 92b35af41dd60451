"""The sixteen-lane rollout step (rollout16_kernel.h: k_rollout16, and inlined in k_backward_rollout and k_round) writes the BITS it wrote
before its knot loop was split into a steady state -- pairs of steps that decide nothing per step: every step has a successor, operands
are read ahead on the straight line, chunk announcements are counted, a lost hand-off ends the loop behind the pair -- and the general
step for a wavefront's last one or two knots.

tests/golden/rollout16_straight_bits.npz was recorded on an MI355X by tests/golden/make_rollout16_straight_bits.py with the library of
commit a45bc01 ("Rollout step: issue independent fmac_dpp chains side by side"), the parent of that change; the fixture names the commit
it was recorded from.  The cases and their inputs are tests/rollout16_straight_cases.py: horizons around the loop's entry, its chunk
announcements and its tail of one and of two knots; rows that stay on the series throughout, rows in which a rare branch (Exp beyond its
series, Log's closed forms, Log's renormalisation) first appears in the middle of the loop and in one row of the wavefront only, and a
row that comes back onto its nominal trajectory.  (The compose's renormalisation is reached in the odd wavefront's first pose only: inside
the step loop it cannot be reached through forward_sim, see the cases' text.)  The inputs are rebuilt here and their digest is compared
with the recorded one first, so that a mismatch of the inputs is not taken for one of the kernel."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import rollout16_straight_cases as sc  # noqa: E402

PARENT = "a45bc01"


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout16_straight_bits.npz")) as z:
        fix = {k: z[k] for k in z.files}
    assert str(fix["commit"]).startswith(PARENT), fix["commit"]
    return fix


def test_the_fixture_holds_every_case(golden):
    ids = [c[0] for c in sc.cases()]
    assert len(ids) == len(set(ids)) == 2 * 8 * 2 * 5
    assert {k[4:] for k in golden if k.startswith("out:")} == set(ids) == {k[3:] for k in golden if k.startswith("in:")}


def test_the_recorded_rows_do_what_their_kinds_say(golden):
    """fp64 storage (fp32 storage rounds the nominal quaternions, so Log renormalises at every knot there): a row's rare condition is absent
    up to its knot K0 and present behind it, `plain` rows never have one"""
    seen = set()
    for cid, prec, n, kinds, alpha in sc.cases():
        if prec == "f64":
            traj, _ = sc.inputs(n, kinds)
            for r, kind in enumerate(kinds):
                sc.check_row(kind, n, traj[r], golden["out:" + cid][r])
                seen.add(kind)
    assert seen == {"plain", "kick16", "kickfar", "logleave", "logflip", "normoff", "startoff", "back", "hover", "perturbed", "spin16", "spinfar"}


@pytest.mark.parametrize("cid,prec,n,kinds,alpha", sc.cases(), ids=[c[0] for c in sc.cases()])
def test_forward_sim_writes_the_parent_commits_bits(golden, cid, prec, n, kinds, alpha):
    out, dg = sc.rollout(capi, prec, n, kinds, alpha)
    assert np.array_equal(dg, golden["in:" + cid]), "the inputs of this case are not the recorded ones"
    want = golden["out:" + cid].astype(np.float64)
    assert out.shape == want.shape == (len(kinds), n, 18)
    differ = np.argwhere(out != want)
    assert np.array_equal(out, want), f"{len(differ)} values differ, first at (row, knot, element) {differ[:4].tolist()}"
