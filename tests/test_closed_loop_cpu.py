"""The closed-loop flight of a plan without a device: the per-sample routine of k_closed_loop (quadrotorilqr_amd/csrc/closed_loop_kernels.h,
compiled with g++ into the stand-alone program tests/host_closed_loop_harness.cpp) against the restatement from the oracle's primitives
(tests/closed_loop_numpy.py) and, from the plan's own start, against rollout_problem bit for bit; the rule of what a call refuses
(closed_loop_launch.h), through the harness and through the C ABI; and what of the ABI runs without a GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from quadrotorilqr_amd import capi, problems as pb
from tests import closed_loop_numpy as cn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B, N, S, SEED = 3, 24, 5, 5
MODELS3 = [pb.MODEL_A, dict(pb.MODEL_A, mass_kg=1.3, inertia=np.diag([1.2, 0.9, 1.5])), dict(pb.MODEL_A, mass_kg=1.1, g_mpss=9.0, arm_length_m=0.7)]
NEW_SYMBOLS = ("qilqr_backwards_pass_device", "qilqr_closed_loop", "qilqr_closed_loop_device")


def build_harness(flags, name):
    d = tempfile.mkdtemp(prefix="host_closed_loop_harness_")
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(HERE, "host_closed_loop_harness.cpp"), "-lm"])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness(["-O2"], "host_closed_loop_harness")


@pytest.fixture(scope="module")
def case():
    """B plans (perturbed desired trajectories), the oracle's gains about them, S sampled states about knot 0: computed once, never written to"""
    cfg, plan = cn.plans(B, N, SEED)
    gains = cn.oracle_gains(cfg, plan)
    x0 = cn.sample_states(plan, S, 0, SEED + 1)
    for a in (plan, gains, x0):
        a.setflags(write=False)
    return cfg, plan, gains, x0


def limits_for(u):
    """thrust limits that clamp some of the controls `u` of an unlimited flight and leave others: its 20th and 80th percentile"""
    return float(np.percentile(u, 20)), float(np.percentile(u, 80))


def model_words(m):
    return np.concatenate([[m["mass_kg"]], np.asarray(m["inertia"], dtype=np.float64).reshape(9), [m["arm_length_m"], m["torque_to_thrust_ratio_m"], m["g_mpss"]]])


def host_fly(exe, cfg, plan, gains, x0, i0=0, i1=None, integrator=0, models=None, limits=None):
    """one call on the host: (traj (B, S, n, 18), stats (B, S, 4), rollout (B, n, 18))"""
    b, n, s = plan.shape[0], plan.shape[1], x0.shape[1]
    i1 = n - 1 if i1 is None else i1
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (4,)) for v in (limits if limits is not None else (0.0, 0.0)))
    parts = [np.array([b, n, s, i0, i1, integrator, limits is not None, models is not None, cfg["dt"]], dtype=np.float64), model_words(cfg["model"]),
             np.asarray(cfg["Q"], dtype=np.float64).ravel(), np.asarray(cfg["R"], dtype=np.float64).ravel(), lo, hi]
    if models is not None:
        assert len(models) == b * s
        parts += [model_words(m) for m in models]
    parts += [plan.ravel(), gains.ravel(), x0.ravel()]
    d = tempfile.mkdtemp(prefix="closed_loop_case_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    np.concatenate(parts).tofile(fin)
    subprocess.check_call([exe, "fly", fin, fout])
    out = np.fromfile(fout)
    nt, ns = b * s * n * 18, b * s * 4
    assert out.size == nt + ns + b * n * 18
    return out[:nt].reshape(b, s, n, 18), out[nt:nt + ns].reshape(b, s, 4), out[nt + ns:].reshape(b, n, 18)


def assert_flight(got_traj, got_stats, want_traj, want_stats, label=""):
    """a flight against the restatement: the same knots written, trajectories and statistics within the bound, the clamp count exactly"""
    assert np.array_equal(np.isnan(got_traj), np.isnan(want_traj)), label
    w = ~np.isnan(want_traj)
    np.testing.assert_allclose(got_traj[w], want_traj[w], rtol=cn.RTOL, atol=cn.ATOL, err_msg=label)
    np.testing.assert_allclose(got_stats[..., :3], want_stats[..., :3], rtol=cn.RTOL, atol=cn.ATOL, err_msg=label)
    assert np.array_equal(got_stats[..., 3], want_stats[..., 3]), label


@pytest.mark.parametrize("window", [(0, N - 1), (5, 5), (3, 17)])
@pytest.mark.parametrize("ext", ["plain", "limits", "models", "both"])
@pytest.mark.parametrize("integrator", [0, 1])
def test_the_device_routine_against_the_restatement(harness, case, integrator, ext, window):
    cfg, plan, gains, _ = case
    i0, i1 = window
    x0 = cn.sample_states(plan, S, i0, SEED + 2 + i0)
    models = [MODELS3[(r + 1) % 3] for r in range(B * S)] if ext in ("models", "both") else None
    limits = None
    if ext in ("limits", "both"):
        free, _ = cn.closed_loop(plan, gains, x0, cfg["model"], cfg["dt"], i0, i1, integrator, models)
        limits = limits_for(free[:, :, i0:i1 + 1, 14:18])
    want_traj, want_stats = cn.closed_loop(plan, gains, x0, cfg["model"], cfg["dt"], i0, i1, integrator, models, limits)
    got_traj, got_stats, _ = host_fly(harness, cfg, plan, gains, x0, i0, i1, integrator, models, limits)
    label = str((integrator, ext, window))
    assert_flight(got_traj, got_stats, want_traj, want_stats, label)
    assert np.array_equal(got_traj[:, :, i0, 1:14], x0), label                                   # the state at knot i0 is x0, exactly
    assert np.array_equal(got_traj[:, :, i0:i1 + 1, 0], np.repeat(plan[:, None, i0:i1 + 1, 0], S, axis=1)), label  # the plan's times
    if i1 > i0:
        assert (got_stats[..., 2] > 1e-3).all(), label  # the plans are not feasible: the flight is off the plan at its last knot
    if limits is not None:
        count = got_stats[..., 3]
        print("[observed] %s: clamped pairs per sample %s" % (label, count.astype(int).tolist()))
        assert (count > 0).any() and ((got_traj[..., 14:18] == limits[0]) | (got_traj[..., 14:18] == limits[1])).any(), label
        w = ~np.isnan(got_traj[..., 14:18])
        assert (got_traj[..., 14:18][w] >= limits[0]).all() and (got_traj[..., 14:18][w] <= limits[1]).all(), label
    else:
        assert (got_stats[..., 3] == 0).all(), label


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("integrator", [0, 1])
def test_one_sample_from_the_plans_own_start_has_the_bits_of_rollout_problem(harness, case, integrator, limited):
    cfg, plan, gains, _ = case
    x0 = np.ascontiguousarray(plan[:, None, 0, 1:14])
    limits = None
    if limited:
        free, _, _ = host_fly(harness, cfg, plan, gains, x0, integrator=integrator)
        limits = limits_for(free[..., 14:18])
    traj, stats, rollout = host_fly(harness, cfg, plan, gains, x0, integrator=integrator, limits=limits)
    assert not np.isnan(traj).any()
    assert traj[:, 0].tobytes() == rollout.tobytes()
    assert (np.abs(traj[:, 0, 1:, 1:14] - plan[:, 1:, 1:14]).max(axis=(1, 2)) > 1e-3).all()  # dx != 0 from the second knot on
    if limited:
        assert (stats[..., 3] > 0).all()


def test_a_samples_bits_do_not_depend_on_the_others(harness, case):
    cfg, plan, gains, x0 = case
    traj, stats, _ = host_fly(harness, cfg, plan, gains, x0)
    for j in (0, S - 1):
        alone_traj, alone_stats, _ = host_fly(harness, cfg, plan, gains, np.ascontiguousarray(x0[:, j:j + 1]))
        assert alone_traj[:, 0].tobytes() == traj[:, j].tobytes() and alone_stats[:, 0].tobytes() == stats[:, j].tobytes()
    # a flight continued from its own knot is the flight
    first, _, _ = host_fly(harness, cfg, plan, gains, x0, 0, 11)
    rest, rest_stats, _ = host_fly(harness, cfg, plan, gains, np.ascontiguousarray(first[:, :, 11, 1:14]), 11, N - 1)
    assert first[:, :, :12].tobytes() == traj[:, :, :12].tobytes() and rest[:, :, 11:].tobytes() == traj[:, :, 11:].tobytes()
    assert np.isnan(first[:, :, 12:]).all() and np.isnan(rest[:, :, :11]).all()
    assert np.array_equal(rest_stats[..., 2], stats[..., 2])


def test_the_harness_under_the_address_and_undefined_behaviour_sanitizers(case):
    """the stand-alone program, compiled and run once with -fsanitize=address,undefined: a window, limits and models"""
    exe = build_harness(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "host_closed_loop_harness_san")
    cfg, plan, gains, x0 = case
    models = [MODELS3[r % 3] for r in range(B * S)]
    traj, stats, _ = host_fly(exe, cfg, plan, gains, x0, 2, N - 2, 1, models, (1.0, 4.0))
    assert not np.isnan(traj[:, :, 2:N - 1]).any() and np.isnan(traj[:, :, :2]).all() and np.isnan(traj[:, :, N - 1:]).all()
    assert not np.isnan(stats).any()


# ---- what a call refuses
OK_CALL = dict(plan=4096, gains=8192, x0=65536, out_traj=131072, out_stats=1 << 20, B=2, n=4, S=3, i0=0, i1=3, handle=1, f32=0, modeled=0, models_B=0)
REFUSALS = [
    (dict(plan=0), "null argument"), (dict(gains=0), "null argument"), (dict(x0=0), "null argument"),
    (dict(out_traj=0, out_stats=0), "no output"),
    (dict(B=0), "must be positive"), (dict(n=-1), "must be positive"), (dict(S=0), "must be positive"),
    (dict(i0=-1), "0 <= i0 <= i1 <= n - 1"), (dict(i1=4), "0 <= i0 <= i1 <= n - 1"), (dict(i0=3, i1=2), "0 <= i0 <= i1 <= n - 1"),
    (dict(plan=4096 + 8), "16-byte aligned"), (dict(x0=65536 + 8), "16-byte aligned"), (dict(out_stats=(1 << 20) + 8), "16-byte aligned"),
    (dict(out_traj=4096 + 16), "overlaps an input"), (dict(out_stats=8192 + 2 * 4 * 52 * 8 - 16), "overlaps an input"),
    (dict(out_traj=65536 - 16 * 100), "overlaps an input"), (dict(out_stats=131072 + 16), "outputs overlap"),
    (dict(handle=0), "null handle"), (dict(f32=1), "precision 0"),
    (dict(modeled=1, models_B=2), "B \\* S samples"), (dict(modeled=1, models_B=7), "B \\* S samples"),
]
ADMITTED = [dict(), dict(out_traj=0), dict(out_stats=0), dict(i0=3, i1=3), dict(modeled=1, models_B=6), dict(S=1, modeled=1, models_B=2),
            dict(out_traj=8192 + 2 * 4 * 52 * 8)]  # (an output may start where an input ends)
ORDER = ("plan", "gains", "x0", "out_traj", "out_stats", "B", "n", "S", "i0", "i1", "handle", "f32", "modeled", "models_B")


def rule(exe, **change):
    call = dict(OK_CALL, **change)
    return subprocess.check_output([exe, "refuse"] + [str(call[k]) for k in ORDER]).decode().strip()


def test_the_rule_of_what_a_call_refuses(harness):
    for change, why in REFUSALS:
        assert re.search(why, rule(harness, **change)), (change, rule(harness, **change))
    for change in ADMITTED:
        assert rule(harness, **change) == "ok", change


def test_the_abi_without_a_device():
    """the refusals come before the device is touched: every one that needs no handle, through ctypes (the arguments are looked at before
    the handle, so a NULL handle is the last of them)"""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name), name
    assert "#define QILQR_CL_STATS 4" in header and capi.CL_STATS == 4
    assert lib.qilqr_backwards_pass_device(None, None, 1, 4, None, None) == capi.ERR_INVALID_ARG and b"null" in lib.qilqr_last_error()
    b, n, s = 2, 4, 3
    arrays = dict(plan=capi._d16(np.zeros((b, n, 18))), gains=capi._d16(np.zeros((b, n, 52))), x0=capi._d16(np.zeros((b, s, 13))),
                  out_traj=capi._d16(np.zeros((b, s, n, 18))), out_stats=capi._d16(np.zeros((b, s, 4))))
    odd = capi._d16(np.zeros(b * n * 18 + 2))[1:]  # 8 bytes off a 16-byte boundary
    assert odd.ctypes.data % 16 == 8

    def call(f, B=b, n_=n, S=s, i0=0, i1=n - 1, **ptr):
        a = {k: (v.ctypes.data if v is not None else None) for k, v in dict(arrays, **ptr).items()}
        rc = f(None, a["plan"], a["gains"], a["x0"], B, n_, S, i0, i1, a["out_traj"], a["out_stats"])
        return rc, lib.qilqr_last_error().decode()

    cases = [(dict(plan=None), "null argument"), (dict(gains=None), "null argument"), (dict(x0=None), "null argument"),
             (dict(out_traj=None, out_stats=None), "no output"), (dict(B=0), "must be positive"), (dict(n_=0), "must be positive"),
             (dict(S=-2), "must be positive"), (dict(i0=-1), "i0 <= i1"), (dict(i1=n), "i0 <= i1"), (dict(i0=2, i1=1), "i0 <= i1"),
             (dict(plan=odd), "16-byte aligned"), (dict(out_traj=arrays["plan"]), "overlaps an input"),
             (dict(out_stats=arrays["x0"]), "overlaps an input"), (dict(out_stats=arrays["out_traj"]), "outputs overlap"), (dict(), "null handle")]
    for f in (lib.qilqr_closed_loop, lib.qilqr_closed_loop_device):
        for change, why in cases:
            rc, text = call(f, **change)
            assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)
