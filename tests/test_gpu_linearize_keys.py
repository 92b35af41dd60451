"""Every k_linearize instantiation a handle can reach (route.h, lin_instantiated; tests/linearize_cases.py has one case per reachable key
and tests/test_linearize_cases_cpu.py the proof that they cover them), one linearisation and one backward pass at a time against the
composed NumPy restatement (tests/composed_numpy_ilqr.py): the fp64 keys at the bars of the suite's pass tests, the mixed-mode keys at the
bars test_config3_mixed_precision_reduced asserts, the diagonal kind's bits against the block-diagonal kind's with every extension form,
and the block-diagonal kind's independence of the batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import linearize_cases as lc  # noqa: E402
from tests.test_gpu_obstacles import split_gains  # noqa: E402


def assert_route_text(s, c, B):
    text = s.describe(B)
    for part in lc.expected_text(c, B):
        assert part in text, (lc.name(c), part, text)
    assert ("mixed precision" in text) == bool(c.f32)


@pytest.mark.parametrize("c", lc.F64, ids=lc.name)
def test_fp64_passes_match_the_restatement(c):
    """B = 3, n = 12: a partly filled block of four for the tiled forms and a partly filled tile of 64 for the plain ones"""
    x = lc.inputs(c)
    s = lc.handle(capi, c, x)
    assert_route_text(s, c, 3)
    lc.compare_passes(s, c, x)


@pytest.mark.parametrize("c", lc.F32, ids=lc.name)
def test_mixed_passes_match_the_restatement(c):
    """config3(B=3, N=20) with the case's weights, its problems rolled out with zero gains: the fp32 kernels against the fp64 restatement at
    the per-pass bars of test_config3_mixed_precision_reduced (cost 2e-5, terms 2e-3 relative, gains 1e-3 of the largest).  The room the
    fp32 rounding of the inputs alone leaves below those bars is the same as for config3's own weights
    (tests/test_linearize_cases_cpu.py)."""
    cfg = lc.mixed_config(c)
    trajs = lc.mixed_trajs(c, cfg)
    s = capi.from_config(cfg, precision="f32", force_general=c.force_general)
    assert_route_text(s, c, len(trajs))
    cost = s.cost_trajectory(trajs)
    gains, terms = s.backwards_pass(trajs)
    for b in range(len(trajs)):
        c64, g64, t64 = lc.mixed_passes(c, cfg, trajs[b])
        k_dev, K_dev = split_gains(gains[b])
        g_dev = np.concatenate([k_dev.ravel(), K_dev.ravel()])
        print("%s problem %d: cost rel %.2e (bar 2e-5), terms rel %.2e (2e-3), gains abs / max %.2e (1e-3)" %
              (lc.name(c), b, abs(cost[b] - c64) / abs(c64), np.max(np.abs(terms[b] - t64) / np.abs(t64)), np.abs(g_dev - g64).max() / np.abs(g64).max()))
        np.testing.assert_allclose(cost[b], c64, rtol=lc.MIXED_BARS["cost"])
        np.testing.assert_allclose(terms[b], t64, rtol=lc.MIXED_BARS["terms"])
        np.testing.assert_allclose(g_dev, g64, rtol=0, atol=lc.MIXED_BARS["gains"] * np.abs(g64).max())


# (fg 0: the tiled records of the forms without models; fg 2: the plain ones)
DIAGONAL = [(form, fg) for form in lc.FORMS for fg in (0, 2) if fg == 2 or not lc.FORMS[form][0]]


@pytest.mark.parametrize("form,fg", DIAGONAL)
def test_a_diagonal_q_gives_the_bits_of_the_block_diagonal_kind(form, fg):
    """kind 3 against kind 2 (dense_weights = 1 on the same handle), Euler, fp64, with every extension form and on either placement"""
    c3 = lc.case("diag", form, force_general=fg)
    c2 = c3._replace(dense_weights=1)
    assert lc.route(c3)[0] == (3,) + lc.route(c2)[0][1:] and lc.route(c2)[0][0] == 2
    x = lc.inputs(c3, seed=6000 + len(form) + fg)
    a, b = lc.handle(capi, c3, x), lc.handle(capi, c2, x)
    assert a.describe(3) == b.describe(3)
    assert a.cost_trajectory(x["trajs"]).tobytes() == b.cost_trajectory(x["trajs"]).tobytes()
    for u, v in zip(a.backwards_pass(x["trajs"]), b.backwards_pass(x["trajs"])):
        assert u.tobytes() == v.tobytes()
    assert np.abs(a.backwards_pass(x["trajs"])[0]).max() > 0


# the block-diagonal kind at B = 70, n = 2: each extension form, both placements where both exist
BATCH = [(form, fg) for form in lc.FORMS for fg in (0, 2) if fg == 2 or not lc.FORMS[form][0]]
ROWS = (0, 3, 63, 64, 69)


@pytest.mark.parametrize("form,fg", BATCH)
def test_the_block_diagonal_kind_does_not_depend_on_the_batch(form, fg):
    """B = 70 (a second, partly empty tile of 64; the last block of four half full), n = 2: a row of the batch has the bytes of the same
    problem on a handle of its own, which holds that problem's model and that problem's spheres; row 69 also against the restatement"""
    c = lc.case("block", form, force_general=fg)
    assert lc.route(c, 70)[0][0] == 2 and lc.route(c, 1)[0] == lc.route(c, 70)[0]
    x = lc.inputs(c, n=2, B=70, seed=6100 + len(form) + fg)
    s = lc.handle(capi, c, x)
    assert_route_text(s, c, 70)
    cost = s.cost_trajectory(x["trajs"])
    gains, terms = s.backwards_pass(x["trajs"])
    for b in ROWS:
        own = lc.handle(capi, c, x, rows=[b])
        one = x["trajs"][b:b + 1]
        assert own.cost_trajectory(one).tobytes() == cost[b:b + 1].tobytes(), b
        g1, t1 = own.backwards_pass(one)
        assert g1.tobytes() == gains[b:b + 1].tobytes() and t1.tobytes() == terms[b:b + 1].tobytes(), b
    if x["counts"] is not None:
        assert x["counts"][69] > 0 and 0 in x["counts"]
    lc.compare_passes(s, c, x, rows=[69])
