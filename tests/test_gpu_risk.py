"""The risk and selection kernels on the device (k_risk_scores, k_select_plans, k_gather_plans: risk_kernels.h) through the C ABI on
plain device buffers, against the restatement in NumPy (tests/risk_numpy.py) with its bounds and against the same text run on the host
(tests/host_risk_harness.cpp), bit for bit; a plan's words do not depend on the other plans, nothing is written behind the end of an
output, a refused call writes nothing; and RecedingHorizon.evaluate_sampled with candidates and risk levels and RecedingHorizon.select,
in a torch process of their own.  B = 3, n = 24, S in {1, 5, 64, 65, 70, 128, 130, 600, 4096}."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import closed_loop_numpy as cn, risk_numpy as rn  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402
from tests.test_risk_cpu import build_harness, candidates, host_risk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 3, 24
# one slot; padding; exactly one wavefront of samples; the first size with padding behind a full wavefront; 128 and 130: the last size
# a one-wavefront block sorts (no block barrier) and the first that takes a block barrier per stage; 600: more comparators than lanes of a
# block's first wavefront, odd padding; the cap: two comparators per lane of 1024
SIZES = [1, 5, 64, 65, 70, 128, 130, 600, 4096]
LEVELS = (0.5, 0.9, 0.99)
COLUMNS = {rn.COST: "cost", rn.CLEARANCE: "clearance"}
GUARD = 64  # bytes behind the end of every output, prefilled with 0xFF like the output


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def solver():
    cfg, _ = cn.plans(B, N, 5)
    return cfg, capi.from_config(cfg)


@pytest.fixture(scope="module")
def harness():
    return build_harness(["-O2"], "host_risk_harness")


def guarded(hip, nbytes):
    return hip.alloc(nbytes + GUARD)


def fetch(hip, ptr, shape, dtype=np.float64):
    """the output and whether the guard behind it kept its bits"""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = hip.download(ptr, (nbytes + GUARD,), dtype=np.uint8)
    return raw[:nbytes].view(dtype).reshape(shape), bool((raw[nbytes:] == 0xFF).all())


def dev_risk(hip, s, score, levels, column):
    lib = capi.load()
    b, S = score.shape[:2]
    lv = np.ascontiguousarray(levels, dtype=np.float64)
    d_score, d = hip.upload(score), guarded(hip, 8 * b * len(lv) * 4)
    assert lib.qilqr_risk_scores_device(s._h, d_score, b, S, column, lv.ctypes.data, len(lv), d) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    out, kept = fetch(hip, d, (b, len(lv), 4))
    assert kept, "k_risk_scores wrote behind the end of its output"
    return out


def dev_select(hip, s, summary, risk, cands, objective="cvar", level=0, plan=None, gains=None, **thresholds):
    """choice (V,), info (V, 4) and, with plan and gains, the gathered (V, n, 18) and (V, n, 52): every output with its guard"""
    lib = capi.load()
    V = summary.shape[0] // cands
    rule = capi.SelectRule(rn.OBJECTIVES[objective], level, thresholds.get("max_collision_fraction", 1.0), thresholds.get("max_diverged_fraction", 1.0),
                           thresholds.get("min_clearance", -np.inf))
    d_sum, d_risk = hip.upload(summary), None if risk is None else hip.upload(risk)
    d_choice, d_info = guarded(hip, 4 * V), guarded(hip, 8 * 4 * V)
    n = 0 if plan is None else plan.shape[1]
    d_plan, d_gains = (None, None) if plan is None else (hip.upload(plan), hip.upload(gains))
    d_op, d_og = (None, None) if plan is None else (guarded(hip, 8 * V * n * 18), guarded(hip, 8 * V * n * 52))
    rc = lib.qilqr_select_plans_device(s._h, d_sum, d_risk, 0 if risk is None else risk.shape[1], C.byref(rule), V, cands, d_choice, d_info, d_plan, d_gains, n, d_op, d_og)
    assert rc == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    choice, kept_c = fetch(hip, d_choice, (V,), np.int32)
    info, kept_i = fetch(hip, d_info, (V, 4))
    assert kept_c and kept_i, "k_select_plans wrote behind the end of an output"
    if plan is None:
        return choice, info
    out_plan, kept_p = fetch(hip, d_op, (V, n, 18))
    out_gains, kept_g = fetch(hip, d_og, (V, n, 52))
    assert kept_p and kept_g, "k_gather_plans wrote behind the end of an output"
    return choice, info, out_plan, out_gains


# ------------------------------------------------------------------------------------------------ 1. k_risk_scores

@pytest.mark.parametrize("S", SIZES)
def test_device_risk_against_the_restatement_and_the_harness(hip, solver, harness, S):
    _, s = solver
    plain, special = rn.scores(B, S, 100 + S, special=False), rn.scores(B, S, 200 + S)
    for column in (rn.COST, rn.CLEARANCE):
        assert rn.keys_are_unique(plain, column)
        got = dev_risk(hip, s, plain, LEVELS, column)
        over = rn.assert_risk(got, plain, LEVELS, column, "S = %d, column %d" % (S, column))
        print("[observed] device risk, S = %d, column %d: error of word 1 over its bound %.3g" % (S, column, over))
        assert got.tobytes() == host_risk(harness, plain, LEVELS, column).tobytes()  # one text and one fold order produce both
        # NaN and infinite keys, and a plan without spheres
        got = dev_risk(hip, s, special, LEVELS, column)
        rn.assert_risk(got, special, LEVELS, column, "special, S = %d, column %d" % (S, column))
        assert got.tobytes() == host_risk(harness, special, LEVELS, column).tobytes()
        if column == rn.CLEARANCE:
            assert np.isposinf(got[2, :, :2]).all()
        # the plan alone (B = 1) has the bits it has among three
        for b in range(B):
            assert dev_risk(hip, s, special[b:b + 1], LEVELS, column).tobytes() == got[b:b + 1].tobytes(), b


def test_device_risk_of_ties_permutations_and_every_level(hip, solver):
    _, s = solver
    score = rn.scores(1, 130, 5, special=False)
    score[0, :, 0] = np.arange(130)
    score[0, [17, 90, 4], 0] = 64.0  # four equal keys: sorted positions 62 .. 65 hold samples {4, 17, 64, 90}
    levels = [(k + 0.5) / 130 for k in (62, 63, 64, 65)]
    got = dev_risk(hip, s, score, levels, rn.COST)
    assert list(got[0, :, 2]) == [4, 17, 64, 90] and (got[0, :, 0] == 64.0).all()
    rn.assert_risk(got, score, levels, rn.COST)
    score = rn.scores(B, 600, 77)
    perm = np.random.default_rng(1).permutation(600)
    eight = (0.0, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 0.999)  # QILQR_RISK_MAX_LEVELS of them
    for column in (rn.COST, rn.CLEARANCE):
        a, b = dev_risk(hip, s, score, eight, column), dev_risk(hip, s, np.ascontiguousarray(score[:, perm]), eight, column)
        rn.assert_risk(a, score, eight, column)
        assert a[..., [0, 1, 3]].tobytes() == b[..., [0, 1, 3]].tobytes()


def test_any_precision_mode_gives_the_same_bits(hip, solver):
    cfg, s = solver
    f32 = capi.from_config(cfg, precision="f32")
    score = rn.scores(B, 70, 3)
    assert dev_risk(hip, f32, score, LEVELS, rn.COST).tobytes() == dev_risk(hip, s, score, LEVELS, rn.COST).tobytes()
    summary, risk = candidates(3, 4, 1)
    a, b = dev_select(hip, f32, summary, risk, 4, "cvar", 1), dev_select(hip, s, summary, risk, 4, "cvar", 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------------ 2. k_select_plans and k_gather_plans

@pytest.mark.parametrize("V,cands", [(3, 4), (70, 5), (1, 1)])
def test_device_selection_and_gather_against_the_restatement(hip, solver, V, cands):
    _, s = solver
    summary, risk = candidates(V, cands, 10 * cands + V)
    r = np.random.default_rng(V)
    plan, gains = r.normal(size=(cands * V, N, 18)), r.normal(size=(cands * V, N, 52))
    seen_fallback = False
    for objective, level in (("mean", 0), ("worst", 0), ("var", 1), ("cvar", 0)):
        for kw in (dict(), dict(max_collision_fraction=0.25), dict(max_collision_fraction=0.25, max_diverged_fraction=0.0, min_clearance=0.1)):
            choice, info, out_plan, out_gains = dev_select(hip, s, summary, risk if objective in ("var", "cvar") else None, cands, objective, level, plan, gains, **kw)
            want_c, want_i = rn.select(summary, risk, cands, objective, level, **kw)
            assert np.array_equal(choice, want_c), (objective, kw, choice, want_c)
            assert np.array_equal(info.view(np.uint64), want_i.view(np.uint64)), (objective, kw, info, want_i)
            rows = choice.astype(int) * V + np.arange(V)
            assert out_plan.tobytes() == np.ascontiguousarray(plan[rows]).tobytes() and out_gains.tobytes() == np.ascontiguousarray(gains[rows]).tobytes()
            seen_fallback |= bool((info[:, 3] == 1).any())
    assert seen_fallback  # (vehicle 0's only candidate has a NaN objective when there is one candidate; vehicles 1 .. 3 else)
    # without the gather: the same choice, one launch
    choice, info = dev_select(hip, s, summary, risk, cands, "cvar", 1, max_collision_fraction=0.25)
    want_c, want_i = rn.select(summary, risk, cands, "cvar", 1, max_collision_fraction=0.25)
    assert np.array_equal(choice, want_c) and np.array_equal(info.view(np.uint64), want_i.view(np.uint64))


# ------------------------------------------------------------------------------------------------ 3. what the calls refuse on a handle

def test_what_the_calls_refuse_on_a_handle(hip, solver):
    """with a handle every refusal of the arguments still comes first and leaves every output untouched (tests/test_risk_cpu.py goes
    through every reason without one)"""
    _, s = solver
    lib = capi.load()
    V, cands, S = 3, 4, 5
    lv = np.ascontiguousarray([0.5, 0.9])
    bad_lv = np.ascontiguousarray([0.5, np.nan])
    d_score, d_risk, d_sum = hip.alloc(8 * V * cands * S * 4), hip.alloc(8 * V * cands * 2 * 4), hip.alloc(8 * V * cands * 8)
    d_choice, d_info = hip.alloc(16), hip.alloc(8 * V * 4)
    d_plan, d_gains, d_op, d_og = hip.alloc(8 * V * cands * N * 18), hip.alloc(8 * V * cands * N * 52), hip.alloc(8 * V * N * 18), hip.alloc(8 * V * N * 52)
    rule, nan_rule, bad_rule = capi.SelectRule(3, 1, 1.0, 1.0, -np.inf), capi.SelectRule(3, 1, np.nan, 1.0, -np.inf), capi.SelectRule(3, 2, 1.0, 1.0, -np.inf)
    risk_call = lambda **k: lib.qilqr_risk_scores_device(s._h, k.get("score", d_score), V * cands, k.get("S", S), k.get("column", 0), k.get("lv", lv).ctypes.data, k.get("n", 2),
                                                         k.get("risk", d_risk))
    sel = lambda r=rule, **k: lib.qilqr_select_plans_device(s._h, k.get("summary", d_sum), k.get("risk", d_risk), 2, C.byref(r), V, cands, k.get("choice", d_choice),
                                                            k.get("info", d_info), k.get("plan", d_plan), k.get("gains", d_gains), k.get("n", N), k.get("op", d_op), k.get("og", d_og))
    refused = [(lambda: risk_call(S=4097), "QILQR_RISK_MAX_SAMPLES"), (lambda: risk_call(column=2), "column must be"), (lambda: risk_call(n=9), "n_levels must be"),
               (lambda: risk_call(lv=bad_lv), "lie in [0, 1)"), (lambda: risk_call(risk=d_risk + 8), "16-byte aligned"), (lambda: risk_call(risk=d_score + 32), "d_risk overlaps d_score"),
               (lambda: sel(bad_rule), "level must be one of"), (lambda: sel(risk=None), "need d_risk"), (lambda: sel(nan_rule), "threshold is NaN"),
               (lambda: sel(gains=None), "all together or not at all"), (lambda: sel(n=0), "n must be positive"), (lambda: sel(info=d_sum + 32), "an output overlaps an input"),
               (lambda: sel(op=d_plan + 16), "an output overlaps an input"), (lambda: sel(og=d_op + 16), "two outputs overlap")]
    for call, why in refused:
        assert call() == capi.ERR_INVALID_ARG and why in lib.qilqr_last_error().decode(), (why, lib.qilqr_last_error())
    hip.synchronize(lib.qilqr_stream(s._h))
    for ptr, nbytes in ((d_risk, 8 * V * cands * 2 * 4), (d_choice, 16), (d_info, 8 * V * 4), (d_op, 8 * V * N * 18), (d_og, 8 * V * N * 52)):
        assert (hip.download(ptr, (nbytes,), dtype=np.uint8) == 0xFF).all()


# ------------------------------------------------------------------------------------------------ 4. RecedingHorizon: candidates, risk, select

@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/risk_torch_child.py, once (PyTorch's ROCm runtime has to be the first a process initialises).  The arrays it recorded."""
    out = str(tmp_path_factory.mktemp("risk_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.risk_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


V_, C_ = 3, 4  # (the child's constants, restated: importing it would initialise torch in this process)


@pytest.mark.parametrize("S", [70, 5])
def test_common_random_numbers(torch_forms, S):
    r, tag = torch_forms, "crn%d_" % S
    score, x0 = r[tag + "score"].reshape(C_, V_, S, 4), r[tag + "x0"].reshape(C_, V_, S, 13)
    assert np.isfinite(score[..., 0]).all()
    for c in range(1, C_):  # the same plan under the same samples: the same flights, bit for bit
        assert x0[c].tobytes() == x0[0].tobytes() and score[c].tobytes() == score[0].tobytes(), c
    assert not np.array_equal(score[0, 0], score[0, 1])  # (vehicles differ)
    flat = r[tag + "score"]
    assert r[tag + "risk"].shape == (V_ * C_, 2, 4)
    rn.assert_risk(r[tag + "risk"], flat, (0.5, 0.9), rn.COST, tag)
    want_c, want_i = rn.select(r[tag + "summary"], r[tag + "risk"], C_, "cvar", 1)
    assert np.array_equal(r[tag + "sel_choice"], want_c) and (want_c == 0).all() and r[tag + "sel_choice"].dtype == np.int32
    assert np.array_equal(r[tag + "sel_info"].view(np.uint64), want_i.view(np.uint64)) and (r[tag + "sel_info"][:, 1] == C_).all()
    assert r[tag + "sel_plan"].tobytes() == r["crn_plan"][:V_].tobytes() and r[tag + "sel_gains"].tobytes() == r["crn_gains"][:V_].tobytes()
    assert r[tag + "sel_u0"].tobytes() == np.ascontiguousarray(r["crn_plan"][:V_, 0, 14:18]).tobytes()


def test_a_real_choice(torch_forms):
    """candidate 2 of every vehicle flies its plan moved into a sphere: it collides, and select with max_collision_fraction = 0 does
    not choose it; the choice is the restatement's over the downloaded summary and risk"""
    r, moved = torch_forms, 2
    summary, risk = r["choice_summary"], r["choice_risk"]
    coll = summary[:, 4].reshape(C_, V_)
    assert (coll[moved] > 0).all() and (np.delete(coll, moved, axis=0) == 0).all(), coll
    rn.assert_risk(risk, r["choice_score"], (0.9,), rn.COST, "choice")
    for tag, objective in (("choice_sel_", "cvar"), ("choice_mean_sel_", "mean")):
        want_c, want_i = rn.select(summary, risk, C_, objective, 0, max_collision_fraction=0.0)
        assert np.array_equal(r[tag + "choice"], want_c) and (r[tag + "choice"] != moved).all(), (tag, r[tag + "choice"])
        assert np.array_equal(r[tag + "info"].view(np.uint64), want_i.view(np.uint64)) and (r[tag + "info"][:, 1] == C_ - 1).all() and (r[tag + "info"][:, 3] == 0).all()
        rows = r[tag + "choice"].astype(int) * V_ + np.arange(V_)
        assert r[tag + "plan"].tobytes() == np.ascontiguousarray(r["choice_plan"][rows]).tobytes()
        assert r[tag + "gains"].tobytes() == np.ascontiguousarray(r["choice_gains"][rows]).tobytes()


def test_the_defaults_return_what_the_call_returned(torch_forms):
    r = torch_forms
    assert list(r["defaults_keys_a"]) == list(r["defaults_keys_b"]) == ["score", "stats", "summary"]
    for k in ("score", "stats", "summary"):
        assert r["defaults_a_" + k].tobytes() == r["defaults_b_" + k].tobytes(), k
    assert np.isfinite(r["defaults_a_score"][..., 0]).all()


def test_the_torch_forms_check_their_arguments(torch_forms):
    said = {k[len("refusal_"):]: str(v) for k, v in torch_forms.items() if k.startswith("refusal_")}
    assert said["fine"] == "accepted" and said["select_mean_is_fine"] == "accepted", said
    for k, kind, text in (("select_without_risk", "RuntimeError", "risk_levels"), ("select_clearance_risk", "RuntimeError", "cost column"),
                          ("candidates", "TypeError", "candidates must divide"), ("select_c", "TypeError", "C must divide"), ("risk_shape", "TypeError", "out must have shape"),
                          ("risk_levels", "TypeError", "levels must be"), ("risk_column", "TypeError", "column must be"), ("risk_level_one", "TypeError", "lie in [0, 1)"),
                          ("select_choice_dtype", "TypeError", "choice must be torch.int32"), ("select_partial", "TypeError", "all together or not at all"),
                          ("select_multiple", "TypeError", "not a multiple")):
        assert said[k].startswith(kind) and text in said[k], (k, said[k])
