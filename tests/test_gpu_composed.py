"""The extensions together on the device: a state-weight schedule, per-problem moving spheres, a shared sphere and per-problem models on
one handle against the composed NumPy restatement (tests/composed_numpy_ilqr.py) pass by pass and in whole solves; a horizon start beside
moving spheres (the schedule and the desired trajectory move to k0 + i, a sphere's time stays i dt from the call's first knot); and the
bits of a scheduled handle with moving spheres whatever the compaction and the streams do."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import composed_cases as cc, linearize_cases as lc, schedule_cases as sc  # noqa: E402
from tests.test_gpu_batch_obstacles import moving_on, reached  # noqa: E402
from tests.test_gpu_obstacles import KEYS, device_solve  # noqa: E402
from tests.test_gpu_schedule import assert_solve_matches  # noqa: E402


def same_bits(a, b, label=""):
    for k in KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (label, k)


@pytest.mark.parametrize("c", cc.PASS_CASES, ids=lc.name)
def test_passes_match_the_composed_restatement(c):
    """the q_sched select inside the ProblemObstacles form of the cost half, with models: B = 3, n = 12"""
    x = lc.inputs(c, seed=cc.pass_seed(c))
    s = lc.handle(capi, c, x)
    text = s.describe(3)
    for part in lc.expected_text(c, 3) + ("state-weight schedule", "batch obstacles", "per-problem models", "obstacles (extension): 5 sphere(s)"):
        assert part in text, (part, text)
    lc.compare_passes(s, c, x)


@pytest.mark.parametrize("models", [False, True], ids=["one_model", "models"])
@pytest.mark.parametrize("N", cc.SIZES)
def test_solves_match_the_composed_restatement(N, models):
    x = cc.solve_inputs(N, models)
    cfg = x["cfg"]
    s = capi.from_config(cfg)
    if models:
        s.set_models(x["mods"])
    s.set_batch_obstacles(x["table"], x["counts"])
    s.set_state_weight_schedule(x["Qs"])
    out = s.solve_batch(cfg["init"])
    assert reached(cfg["init"], x["table"], x["counts"], cfg["dt"]) > 0
    for b in cc.PROBLEMS:
        assert_solve_matches(out, b, cc.compute(N, models, b))


def window_handle(x, cfg, Qs, **kw):
    s = capi.from_config(cfg, **kw)
    s.set_state_weight_schedule(Qs)
    s.set_batch_obstacles(x["table"], x["counts"])
    return s


WINDOW = lc.Case("diag", 0, 0, 0, 0, 0, 0, 0, 1, "dense")  # (what compare_passes names the window's handle by)


@pytest.mark.parametrize("B", [6, 70])
def test_a_horizon_start_moves_the_schedule_and_not_the_spheres_time(B):
    x = cc.window_inputs(B)
    cfg, init, Qs = x["cfg"], x["init"], x["Qs"]
    sl = slice(cc.K0, cc.K0 + cc.N)
    s = window_handle(x, cfg, Qs)
    s.set_horizon_start(cc.K0)
    text = s.describe(B)
    assert "Qs[%d + i]" % cc.K0 in text and "both sphere tables are the call's own" in text and "some moving" in text, text
    # a handle created with the slices and the same, unshifted sphere table: every output, bit for bit
    sliced = window_handle(x, dict(cfg, desired=cfg["desired"][cc.K0:]), Qs[cc.K0:])
    want = sliced.solve_batch(init)
    assert (want["iters"] >= 2).all()
    same_bits(s.solve_batch(init), want, "k0 = 7")
    assert s.cost_trajectory(init).tobytes() == sliced.cost_trajectory(init).tobytes()
    for u, v in zip(s.backwards_pass(init), sliced.backwards_pass(init)):
        assert u.tobytes() == v.tobytes()
    # ... and the passes are the composed restatement's from those slices with the spheres at i dt
    rows = (0, 1, 2, 4) if B == 6 else (64, 68)
    lc.compare_passes(s, WINDOW, dict(cfg=cfg, trajs=init), rows=rows,
                      restated=lambda b: cc.window_restatement(x, b, cfg["desired"][sl], Qs[sl]))
    # k0 = 0 again: the bits of a handle that never had a start
    x0 = cc.window_inputs(B, 0)
    never = window_handle(x, cfg, Qs).solve_batch(x0["init"])
    s.set_horizon_start(0)
    same_bits(s.solve_batch(x0["init"]), never, "k0 = 0")
    if B == 6:  # the same through two shards
        sh = capi.sharded_from_config(cfg, devices=(0, 0))
        sh.set_state_weight_schedule(Qs)
        sh.set_batch_obstacles(x["table"], x["counts"])
        sh.set_horizon_start(cc.K0)
        same_bits(sh.solve_batch(init), want, "two shards")


def test_bits_do_not_depend_on_the_compaction_or_the_streams():
    """B = 300, a schedule and moving spheres: the candidate linearisation reads a problem's sphere row through the slot map"""
    B, N = 300, 20
    cfg = pb.config2(B=B, N=N, seed=44)
    init = cfg["init"]
    table = moving_on(init, cfg["dt"], np.random.default_rng(45))
    counts = np.resize([3, 2, 1, 0], B)
    Qs = sc.schedule("terminal", N)

    def handle(**kw):
        s = capi.from_config(cfg, **capi.PIN_ARITHMETIC, **kw)
        s.set_state_weight_schedule(Qs)
        s.set_batch_obstacles(table, counts)
        return s

    loose = handle(compaction=-1)
    base = device_solve(loose, init)
    assert loose.compaction_moves() == 0 and len(set(base["iters"].tolist())) > 1
    assert reached(base["traj"], table, counts, cfg["dt"]) > 0
    packed = handle(compaction=1)
    same_bits(device_solve(packed, init), base, "compaction = 1")
    assert packed.compaction_moves() > 0
    same_bits(device_solve(handle(streams=1), init), base, "streams = 1")
    same_bits(device_solve(handle(streams=2), init), base, "streams = 2")
    same_bits(handle(streams=2).solve_batch(init), base, "streams = 2, host arrays")
    same_bits(device_solve(handle(streams=2, compaction=1), init), base, "streams = 2, compaction = 1")
