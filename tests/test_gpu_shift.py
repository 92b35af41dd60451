"""Receding-horizon stepping on the device: the horizon start (qilqr_set_horizon_start: a window into the handle's desired trajectory and
schedule, bit for bit a handle created with the slice), the shift (k_shift through qilqr_shift_batch[_device]) against its restatement
with the oracle's step (tests/shift_numpy.py) and against the solver's own rollout, its identities, its refusals, and the closed loop of
quadrotorilqr_amd/mpc.py against the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import desired_cases as dc, exit_paths, observed, shift_numpy as sn  # noqa: E402
from tests.test_gpu_sharded import _Hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KEYS = ("traj", "cost", "status", "iters", "n_bwd", "n_fwd")
N_DES, K0, N = 40, 7, 24
SEED = 21
LIMITS = (0.5, 2.2)  # hi below every model's hover thrust here: the hover tail is clamped
MODELS3 = [pb.MODEL_A, dict(pb.MODEL_A, mass_kg=1.3, inertia=np.diag([1.2, 0.9, 1.5])), dict(pb.MODEL_A, mass_kg=1.1, g_mpss=9.0, arm_length_m=0.7)]


def same_bits(a, b, label=""):
    for k in KEYS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (label, k)


# ------------------------------------------------------------------------------------------------ the horizon start

def window_case(B, k0=K0, n=N):
    """a handle's config with a time-varying shared desired trajectory of 40 knots, and initial trajectories for the window [k0, k0 + n)"""
    cfg, _ = dc.tracking_case(B, N_DES, SEED, shared=True)
    init = dc.start_from(np.repeat(cfg["desired"][None, k0:k0 + n], B, axis=0), np.arange(B), SEED)
    return cfg, init


@pytest.mark.parametrize("B", [6, 70])
def test_a_horizon_start_gives_the_bits_of_a_handle_created_with_the_slice(B):
    cfg, init = window_case(B)
    s = capi.from_config(cfg)
    never = capi.from_config(cfg).solve_batch(window_case(B, 0)[1])
    s.set_horizon_start(K0)
    text = s.describe(B)
    assert "k_round" in text and "horizon start" in text and "desired[%d + i]" % K0 in text, text
    sliced = capi.from_config(dict(cfg, desired=cfg["desired"][K0:]))
    assert "horizon start" not in sliced.describe(B)
    want = sliced.solve_batch(init)
    assert (want["iters"] >= 2).all()
    same_bits(s.solve_batch(init), want, "k0 = 7")
    # ... and differs from what the unshifted window gives (the window is read)
    assert not np.array_equal(capi.from_config(cfg).solve_batch(init)["traj"], want["traj"])
    # k0 = 0 again: the bits of a handle that never had a start
    s.set_horizon_start(0)
    assert "horizon start" not in s.describe(B)
    same_bits(s.solve_batch(window_case(B, 0)[1]), never, "k0 = 0")


@pytest.mark.parametrize("B", [6, 70])
def test_a_horizon_start_moves_the_schedule_too(B):
    cfg, init = window_case(B)
    Qs = pb.waypoint_schedule(0.01 * pb.Q_DEMO, 10 * pb.Q_DEMO, N_DES, (3, 12, 19, 30, 39))
    for k in range(N_DES):  # (no two knots alike: a wrong index shows)
        Qs[k] = Qs[k] * (1.0 + 0.01 * k)
    s = capi.from_config(cfg)
    s.set_state_weight_schedule(Qs)
    s.set_horizon_start(K0)
    assert "Qs[%d + i]" % K0 in s.describe(B)
    sliced = capi.from_config(dict(cfg, desired=cfg["desired"][K0:]))
    sliced.set_state_weight_schedule(Qs[K0:])
    want = sliced.solve_batch(init)
    same_bits(s.solve_batch(init), want, "schedule")
    assert s.cost_trajectory(init).tobytes() == sliced.cost_trajectory(init).tobytes()
    s.set_horizon_start(0)
    plain = capi.from_config(cfg)
    plain.set_state_weight_schedule(Qs)
    same_bits(s.solve_batch(window_case(B, 0)[1]), plain.solve_batch(window_case(B, 0)[1]), "schedule, k0 = 0")


def test_a_horizon_start_through_the_single_solve_and_on_two_shards():
    B = 6
    cfg, init = window_case(B)
    s = capi.from_config(cfg)
    s.set_horizon_start(K0)
    sliced = capi.from_config(dict(cfg, desired=cfg["desired"][K0:]))
    for b in (0, 3):
        ta, ia = s.solve(init[b])
        tb, ib = sliced.solve(init[b])
        assert ta.tobytes() == tb.tobytes() and (ia["cost"], ia["status"], ia["iters"]) == (ib["cost"], ib["status"], ib["iters"])
    sh = capi.sharded_from_config(cfg, devices=(0, 0))
    sh.set_horizon_start(K0)
    want = capi.sharded_from_config(dict(cfg, desired=cfg["desired"][K0:]), devices=(0, 0)).solve_batch(init)
    same_bits(sh.solve_batch(init), want, "two shards")
    same_bits(want, sliced.solve_batch(init), "shards against one device")
    with pytest.raises(TypeError, match="horizon start"):
        sh.set_horizon_start(N_DES)
    same_bits(sh.solve_batch(init), want, "a refused start leaves every shard at the start it had")


def test_the_refusals_of_a_horizon_start():
    cfg, _ = window_case(6)
    s = capi.from_config(cfg)
    s.set_horizon_start(K0)
    long_init = np.repeat(cfg["desired"][None, :34], 6, axis=0)
    with pytest.raises(IndexError, match="longer than desired"):  # 34 > 40 - 7
        s.solve_batch(long_init)
    with pytest.raises(IndexError):
        s.cost_trajectory(long_init)
    s.solve_batch(long_init[:, :33])  # (33 = 40 - 7 fits)
    s.solve_batch(long_init, desired_batch=long_init)  # a per-problem desired_batch is the caller's window
    for bad in (N_DES, -1):
        with pytest.raises(TypeError, match="horizon start"):
            s.set_horizon_start(bad)
    assert "desired[%d + i]" % K0 in s.describe(6)  # (a refused start leaves the one in force)
    with pytest.raises(TypeError, match="shorter than the horizon start"):  # ... and a schedule set now reaches beyond it
        s.set_state_weight_schedule(pb.terminal_schedule(pb.Q_DEMO, 10 * pb.Q_DEMO, K0))
    assert "state-weight schedule" not in s.describe(6)
    s.set_state_weight_schedule(pb.terminal_schedule(pb.Q_DEMO, 10 * pb.Q_DEMO, 30))
    with pytest.raises(TypeError, match="schedule"):
        s.set_horizon_start(30)
    with pytest.raises(IndexError, match="schedule"):  # 24 > 30 - 7
        s.solve_batch(long_init[:, :24])
    s.solve_batch(long_init[:, :23])
    f32 = capi.from_config(cfg, precision="f32")
    with pytest.raises(TypeError, match="precision 0"):
        f32.set_horizon_start(K0)
    f32.set_horizon_start(0)


# ------------------------------------------------------------------------------------------------ the shift

def plans(B, n):
    """(B, n, 18) plans to shift: the time-varying per-problem trajectories of tests/desired_cases.py (unit quaternions, a control of its
    own per knot and rotor, a time column unlike i dt)"""
    return dc.tracking_desired(np.arange(B), n, SEED + 1)


def measured_states(plan, steps):
    r = np.random.default_rng(5 + steps)
    x0 = plan[:, steps, 1:14] + 0.05 * r.standard_normal((plan.shape[0], 13))
    x0[:, 3:7] /= np.linalg.norm(x0[:, 3:7], axis=1, keepdims=True)
    return x0


def handle(B, integrator=0, models=False, limits=False, **kw):
    cfg = pb.config2(B=1, N=8)  # (the shift reads no desired trajectory; the passes some tests call beside it need a few knots)
    s = capi.from_config(cfg, **kw)
    s.set_integrator(integrator)
    mods = [MODELS3[b % 3] for b in range(B)] if models else None
    if models:
        s.set_models(mods)
    if limits:
        s.set_control_limits(*LIMITS)
    return s, cfg, mods


SHAPES = [(3, 12, 1), (3, 12, 11), (70, 2, 1), (70, 24, 3), (70, 24, 23)]  # (B, n, steps): (70, 2, 1) keeps one knot, on two wavefronts
VARIANTS = [("hold", 0, False, False), ("hover", 0, False, False), ("hold", 1, False, False), ("hover", 0, True, False),
            ("hold", 0, False, True), ("hover", 1, True, True)]  # (tail, integrator, per-problem models, limits)


@pytest.mark.parametrize("tail, integrator, models, limits", VARIANTS)
@pytest.mark.parametrize("B, n, steps", SHAPES)
def test_the_shift_against_the_restatement(B, n, steps, tail, integrator, models, limits):
    s, cfg, mods = handle(B, integrator, models, limits)
    plan = plans(B, n)
    for x0 in (None, measured_states(plan, steps)):
        got = s.shift(plan, x0, steps, tail)
        want = sn.shift(plan, cfg["model"], cfg["dt"], steps, tail, x0, integrator, mods, LIMITS if limits else None)
        sn.assert_shift(got, plan, want, steps, x0, label=str((B, n, steps, tail, integrator, models, limits, x0 is not None)))
        if tail == "hover":
            for b in range(B):
                u = pb.hover_thrust(mods[b] if models else cfg["model"])
                assert (got[b, n - steps:, 14:18] == (LIMITS[1] if limits else u)).all() and (not limits or u > LIMITS[1])


def test_the_shift_identities_and_independence():
    B, n = 70, 24
    s, cfg, _ = handle(B)
    plan = plans(B, n)
    assert s.shift(plan, None, 0).tobytes() == plan.tobytes()  # steps = 0 without x0: the input bit for bit
    x0 = measured_states(plan, 3)
    anchored = s.shift(plan, x0, 0)  # steps = 0 with x0: knot 0's state only
    assert np.array_equal(anchored[:, 0, 1:14], x0) and np.array_equal(anchored[:, 1:], plan[:, 1:])
    assert np.array_equal(anchored[:, 0, [0, 14, 15, 16, 17]], plan[:, 0, [0, 14, 15, 16, 17]])
    for tail in ("hold", "hover"):
        whole = s.shift(plan, x0, 3, tail)
        assert np.array_equal(whole[:, 1:n - 3], plan[:, 4:])  # kept knots
        for b in (0, 37, 63, 64, 69):  # problem b's row: the same bits in the batch of 70 and alone
            assert s.shift(plan[b:b + 1], x0[b:b + 1], 3, tail).tobytes() == whole[b].tobytes(), (tail, b)
        # the device form (buffers from the HIP runtime this process already runs on) is the host form
        dev = device_shift(s, plan, x0, 3, tail)
        assert dev.tobytes() == whole.tobytes(), tail


def device_shift(s, plan, x0, steps, tail):
    """qilqr_shift_batch_device on device buffers (no torch: test_gpu_sharded._Hip), the output back as a NumPy array"""
    hip = _Hip()
    try:
        d_in, d_out, d_x0 = hip.alloc(plan.nbytes), hip.alloc(plan.nbytes), hip.alloc(x0.nbytes)
        for d, h in ((d_in, plan), (d_x0, np.ascontiguousarray(x0))):
            assert hip.lib.hipMemcpy(C.c_void_p(d), h.ctypes.data_as(C.c_void_p), C.c_size_t(h.nbytes), C.c_int(1)) == 0
        rc = capi.load().qilqr_shift_batch_device(s._h, d_in, d_x0, plan.shape[0], plan.shape[1], steps, capi.TAILS[tail], d_out)
        assert rc == 0, capi.load().qilqr_last_error()
        # (enqueued on the handle's stream, not drained: hipMemcpy below is ordered with the null stream only, so the stream is drained here)
        assert hip.lib.hipStreamSynchronize(C.c_void_p(capi.load().qilqr_stream(s._h))) == 0
        assert hip.download(d_in, plan.shape, np.float64).tobytes() == plan.tobytes()  # the input is only read
        return hip.download(d_out, plan.shape, np.float64)
    finally:
        hip.close()


@pytest.mark.parametrize("integrator", [0, 1])
def test_the_shift_against_the_existing_rollout(integrator):
    """The tail against qilqr_forward_sim on the lane-per-trajectory kernel (single_wave_rollout = 1) with zero gains over the held
    controls, started at in[n - 1]: the same step by the same functions.  Bound: the restatement's.  Whether the bits agree is recorded,
    not asserted (the two kernels inline the step into different surroundings)."""
    B, n, steps = 70, 24, 5
    s, cfg, _ = handle(B, integrator, single_wave_rollout=1)
    plan = plans(B, n)
    got = s.shift(plan, None, steps, "hold")
    nominal = np.repeat(plan[:, n - 1:n], steps + 1, axis=1)  # knot 0 = in[n - 1]; the others carry the held control (their state is not read: zero gains)
    sim = s.forward_sim(nominal, np.zeros((B, steps + 1, capi.GAIN)), 1.0)
    assert sim[:, 0].tobytes() == plan[:, n - 1].tobytes()
    np.testing.assert_allclose(got[:, n - steps:, 1:], sim[:, 1:, 1:], rtol=sn.TAIL_RTOL, atol=sn.TAIL_ATOL)
    label = "shift tail against k_rollout<%d> (B = 70, 5 steps)" % integrator
    one = np.ones(B)
    observed.observed(label, dict(cost=one, traj=got[:, n - steps:, 1:]), dict(cost=one, traj=sim[:, 1:, 1:]))
    print("[observed] %s: bits %s" % (label, "agree" if got[:, n - steps:, 1:].tobytes() == sim[:, 1:, 1:].tobytes() else "differ"))


def test_the_refusals_of_the_shift():
    lib = capi.load()
    B, n = 6, 12
    s, cfg, _ = handle(B)
    plan = plans(B, n)
    for steps in (-1, n, n + 5):
        with pytest.raises(TypeError, match="steps"):
            s.shift(plan, None, steps)
    with pytest.raises(TypeError, match="tail"):
        s.shift(plan, None, 1, "coast")
    out = np.zeros_like(plan)
    vp = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
    raw = lambda f, traj, x0, o, steps=1, tail=0: f(s._h, vp(traj), vp(x0), B, n, steps, tail, vp(o))
    for f in (lib.qilqr_shift_batch, lib.qilqr_shift_batch_device):
        assert raw(f, None, None, out) == capi.ERR_INVALID_ARG and b"null" in lib.qilqr_last_error()
        assert raw(f, plan, None, None) == capi.ERR_INVALID_ARG and b"null" in lib.qilqr_last_error()
        assert raw(f, plan, None, out, tail=2) == capi.ERR_INVALID_ARG and b"tail" in lib.qilqr_last_error()
        assert raw(f, plan, None, out, steps=n) == capi.ERR_INVALID_ARG and b"steps" in lib.qilqr_last_error()
        assert raw(f, plan, None, plan) == capi.ERR_INVALID_ARG and b"overlaps" in lib.qilqr_last_error()
        odd = np.zeros(plan.size + 1)[1:].reshape(plan.shape)  # 8 bytes off a 16-byte boundary
        assert odd.ctypes.data % 16 == 8
        assert raw(f, odd, None, out) == capi.ERR_INVALID_ARG and b"aligned" in lib.qilqr_last_error()
        assert raw(f, plan, None, odd) == capi.ERR_INVALID_ARG and b"aligned" in lib.qilqr_last_error()
    x0 = measured_states(plan, 1)
    x0[4, 3:7] *= 1.001
    with pytest.raises(ValueError, match="problem 4"):
        s.shift(plan, x0, 1)
    with pytest.raises(TypeError, match="x0 must be"):
        s.shift(plan, x0[:, :12], 1)
    # the device form on device pointers: the same array, and an output that overlaps the input or x0 by part (16-byte aligned all)
    hip = _Hip()
    try:
        base = hip.alloc(2 * plan.nbytes)
        dev = lambda traj, x0, o, steps=1: lib.qilqr_shift_batch_device(s._h, traj, x0, B, n, steps, 0, o)
        for traj, x0_, o, word in ((base, None, base, b"overlaps the input"), (base, None, base + plan.nbytes - 288, b"overlaps the input"),
                                   (base + 288, None, base, b"overlaps the input"), (base, base + plan.nbytes + 144, base + plan.nbytes, b"overlaps x0"),
                                   (base + 8, None, base + plan.nbytes + 16, b"aligned"), (base, base + plan.nbytes - 8, base + plan.nbytes, b"aligned")):
            assert dev(traj, x0_, o) == capi.ERR_INVALID_ARG and word in lib.qilqr_last_error(), (traj - base, o - base, lib.qilqr_last_error())
        assert dev(base, None, base + plan.nbytes) == 0  # (side by side is fine)
        assert hip.lib.hipStreamSynchronize(C.c_void_p(lib.qilqr_stream(s._h))) == 0
    finally:
        hip.close()
    # a mixed-precision handle, and another B while per-problem models are set
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").shift(plan, None, 1)
    m, _, _ = handle(B, models=True)
    with pytest.raises(TypeError, match="batch models were set for B = 6"):
        m.shift(plan[:5], None, 1)
    m.shift(plan, None, 1)


# ------------------------------------------------------------------------------------------------ the torch forms, and the closed loop

@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/shift_torch_child.py, once: PyTorch's ROCm runtime has to be the first a process initialises, and this one runs the
    library's already.  The arrays it recorded."""
    out = str(tmp_path_factory.mktemp("shift_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.shift_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_shift_device_on_torch_tensors(torch_forms):
    r = torch_forms
    for tail in ("hold", "hover"):
        assert r["device_" + tail].tobytes() == r["host_" + tail].tobytes(), tail  # the host form is the device form
        assert not np.isnan(r["device_" + tail]).any()
    assert r["device_input_after"].tobytes() == r["device_input"].tobytes()
    said = {k[len("refusal_"):]: str(v) for k, v in r.items() if k.startswith("refusal_")}
    for k, word in (("same", "overlaps the input"), ("overlap_behind", "overlaps the input"), ("overlap_before", "overlaps the input"),
                    ("overlap_x0", "overlaps x0"), ("misaligned", "aligned"), ("strided", "contiguous"), ("float32", "float64"),
                    ("host_tensor", "CUDA tensor"), ("x0_shape", "shape"), ("tail", "tail"), ("steps", "steps")):
        assert said[k].startswith("TypeError") and word in said[k], (k, said[k])
    assert said["fine"] == "accepted"


def test_the_closed_loop_against_the_oracle(torch_forms):
    """RecedingHorizon over a mission of 28 knots with a horizon of 24: a start and four ticks with the perfect plant (the measured state
    is knot `steps` of the last plan).  At every tick the init the solve started from is the restatement's shift of the GPU's own last
    plan, the solve has the oracle's exit paths, costs and trajectories from that init over the window's desired trajectory, and takes
    fewer iterations than the oracle's cold start from the same state (the window's desired trajectory with knot 0 replaced)."""
    r = torch_forms
    B, n, M = 6, N, 28
    cfg, _ = dc.tracking_case(B, M, SEED, shared=True)
    des = cfg["desired"]

    def oracle(k0):
        return orc.OracleSolver(orc.model_params(**cfg["model"]), cfg["Q"], cfg["R"], des[k0:k0 + n], cfg["dt"], orc.options(**cfg["options"]))

    def result(tick):
        return {k: r["tick%d_%s" % (tick, k)] for k in KEYS}

    def against_the_oracle(out, init, k0, label):
        o = oracle(k0)
        ref = o.solve_batch(init)
        observed.observed(label, out, ref)
        exit_paths.assert_same_exit_paths(out, ref, o, init, label=label)
        np.testing.assert_allclose(out["cost"], ref["cost"], rtol=1e-9)
        np.testing.assert_allclose(out["traj"], ref["traj"], atol=1e-6)

    init = dc.start_from(np.repeat(des[None, :n], B, axis=0), np.arange(B), SEED)
    assert r["tick0_init"].tobytes() == init.tobytes() and int(r["tick0_k0"]) == 0
    plan = result(0)
    against_the_oracle(plan, init, 0, "closed loop, start")
    for tick in range(1, M - n + 1):
        x0 = r["tick%d_x0" % tick]
        assert np.array_equal(x0, plan["traj"][:, 1, 1:14])
        assert int(r["tick%d_k0" % tick]) == tick and "desired[%d + i]" % tick in str(r["tick%d_describe" % tick])
        shifted = r["tick%d_init" % tick]
        want = sn.shift(plan["traj"], cfg["model"], cfg["dt"], 1, "hold", x0)
        sn.assert_shift(shifted, plan["traj"], want, 1, x0, label="tick %d" % tick)
        new = result(tick)
        assert np.array_equal(new["traj"][:, 0, 14:18], r["tick%d_u0" % tick])
        against_the_oracle(new, shifted, tick, "closed loop, tick %d" % tick)
        cold = np.repeat(des[None, tick:tick + n], B, axis=0)
        cold[:, :, 0] = shifted[:, :, 0]
        cold[:, 0, 1:14] = x0
        cold_ref = oracle(tick).solve_batch(cold)
        print("[observed] closed loop, tick %d: warm iterations %s, cold iterations %s" % (tick, new["iters"].tolist(), cold_ref["iters"].tolist()))
        assert (new["iters"] < cold_ref["iters"]).all(), (tick, new["iters"].tolist(), cold_ref["iters"].tolist())
        np.testing.assert_allclose(new["cost"], cold_ref["cost"], rtol=1e-9)
        plan = new
    # the mission is over: no window of 24 knots is left behind knot 5.  A refused tick leaves the object and the handle's start as they were
    assert str(r["refusal_past_the_mission"]).startswith("IndexError"), r["refusal_past_the_mission"]
    assert str(r["refusal_tick_steps"]).startswith("TypeError") and "steps" in str(r["refusal_tick_steps"])
    assert int(r["after_refusals_k0"]) == M - n and "desired[%d + i]" % (M - n) in str(r["after_refusals_describe"])
    assert bool(r["after_refusals_same_plan"])
    assert (r["after_refusals_status"] <= 1).all() and int(r["after_refusals_k0_again"]) == M - n
