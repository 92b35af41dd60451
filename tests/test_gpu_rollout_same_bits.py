"""The sixteen-lane rollout step (rollout16.h, rollout16_kernel.h: k_rollout16, and inlined in k_backward_rollout and k_round) writes the
BITS it wrote before its broadcast-multiply-add chains were issued side by side and its rotations by two became one hop.

tests/golden/rollout16_bits.npz was recorded on an MI355X by tests/golden/make_rollout16_bits.py with the library of commit f88abe3
("Planner: one flight block, one argument filler, one block-size dispatch"), the parent of that change; the fixture names the commit it was
recorded from.  The cases and their inputs are tests/rollout16_bits_cases.py (the smallest shapes at which each branch of the step exists);
the inputs are rebuilt here and their digest is compared with the recorded one first, so that a mismatch of the inputs is not taken for one
of the kernel."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import rollout16_bits_cases as rc  # noqa: E402

PARENT = "f88abe3"


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout16_bits.npz")) as z:
        fix = {k: z[k] for k in z.files}
    assert str(fix["commit"]).startswith(PARENT), fix["commit"]
    return fix


def test_the_fixture_holds_every_case(golden):
    ids = [c[0] for c in rc.cases()]
    assert len(ids) == len(set(ids)) == 2 * 6 * 2 * 3
    assert {k[4:] for k in golden if k.startswith("out:")} == set(ids) == {k[3:] for k in golden if k.startswith("in:")}


@pytest.mark.parametrize("cid,prec,n,kinds,alpha", rc.cases(), ids=[c[0] for c in rc.cases()])
def test_forward_sim_writes_the_parent_commits_bits(golden, cid, prec, n, kinds, alpha):
    out, dg = rc.rollout(capi, prec, n, kinds, alpha)
    assert np.array_equal(dg, golden["in:" + cid]), "the inputs of this case are not the recorded ones"
    want = golden["out:" + cid].astype(np.float64)
    assert out.shape == want.shape == (len(kinds), n, 18)
    differ = np.argwhere(out != want)
    assert np.array_equal(out, want), f"{len(differ)} values differ, first at (row, knot, element) {differ[:4].tolist()}"


@pytest.mark.parametrize("rounds_per_launch", [0, 1])
def test_a_batch_solve_through_k_round_takes_the_parent_commits_path(golden, rounds_per_launch):
    """eight problems, twelve knots, four rounds per k_round launch (0: the default) and one: status, iterations, pass counts, costs"""
    out, text = rc.solve(capi, rounds_per_launch)
    assert "k_round" in text, text
    for k in rc.SOLVE_KEYS:
        assert np.array_equal(out[k], golden[f"solve{rounds_per_launch}:{k}"]), (k, out[k], golden[f"solve{rounds_per_launch}:{k}"])
    assert (out["status"] >= 0).all() and (out["n_fwd"] >= 1).all()
