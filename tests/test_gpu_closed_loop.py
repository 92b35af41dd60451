"""The plan's feedback law on the device: qilqr_backwards_pass_device against qilqr_backwards_pass, and the closed-loop flights of
k_closed_loop (qilqr_closed_loop[_device]) against the solver's own rollout (bit for bit), against the restatement from the oracle's
primitives (tests/closed_loop_numpy.py), across its two forms, over windows of knots, with per-sample models, through the device forms'
stream ordering, and through quadrotorilqr_amd.mpc.RecedingHorizon.

Plans are perturbed desired trajectories (closed_loop_numpy.plans): not dynamically feasible, so a flight is off the plan from the second
knot on -- every test that flies asserts it.  n = 24.  The rule of the kernel's two forms came out of the measurement as one of lane fill
(closed_loop_kernels.h, closed_loop_shared_form), not as one threshold in S: S = 1, 5 and 70 take the flattened form (70 crosses a
wavefront there), S = 64 the shared-operand form with one full wavefront, and S = 126 -- added here for that -- the shared-operand form
with a second wavefront whose last two lanes are idle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 24, 21
N_DES, K0 = 40, 7
MODELS3 = [pb.MODEL_A, dict(pb.MODEL_A, mass_kg=1.3, inertia=np.diag([1.2, 0.9, 1.5])), dict(pb.MODEL_A, mass_kg=1.1, g_mpss=9.0, arm_length_m=0.7)]


class Hip:
    """device buffers without torch: the HIP runtime this process already runs on, through ctypes"""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so.7")
        self.ptrs = []

    def alloc(self, nbytes, fill=0xFF):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        assert self.lib.hipMemset(p, C.c_int(fill), C.c_size_t(nbytes)) == 0
        assert self.lib.hipDeviceSynchronize() == 0
        self.ptrs.append(p)
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.lib.hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), C.c_int(1)) == 0
        return p

    def download(self, ptr, shape, dtype=np.float64):
        a = np.empty(shape, dtype=dtype)
        assert self.lib.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(a.nbytes), C.c_int(2)) == 0
        return a

    def synchronize(self, stream):
        assert self.lib.hipStreamSynchronize(C.c_void_p(stream)) == 0

    def close(self):
        for p in self.ptrs:
            self.lib.hipFree(p)
        self.ptrs = []


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


def flew_off_the_plan(traj, plan, i0=0):
    """every sample is off its plan from the second knot of the flight on"""
    d = np.abs(traj[:, :, i0 + 1:, 1:14] - plan[:, None, i0 + 1:, 1:14])
    return bool((d.max(axis=3) > 1e-6).all())


def case(B, **kw):
    """(cfg, plan, solver, gains): B plans, a handle, and the gains of its backward pass about them"""
    cfg, plan = cn.plans(B, N, SEED)
    s = capi.from_config(cfg, **kw)
    gains, _ = s.backwards_pass(plan)
    return cfg, plan, s, gains


# ------------------------------------------------------------------------------------------------ 1. the backward pass over device arrays

def configure(kind, B):
    """(solver, plan) of one of the three configurations"""
    if kind == "schedule":
        cfg, _ = dc.tracking_case(B, N_DES, SEED, shared=True)
        plan = dc.start_from(np.repeat(cfg["desired"][None, K0:K0 + N], B, axis=0), np.arange(B), SEED)
        s = capi.from_config(cfg)
        Qs = pb.waypoint_schedule(0.01 * pb.Q_DEMO, 10 * pb.Q_DEMO, N_DES, (3, 12, 19, 30, 39))
        for k in range(N_DES):  # (no two knots alike: a wrong index shows)
            Qs[k] = Qs[k] * (1.0 + 0.01 * k)
        s.set_state_weight_schedule(Qs)
        s.set_horizon_start(K0)
        return s, plan
    cfg, plan = cn.plans(B, N, SEED)
    s = capi.from_config(cfg)
    if kind == "limits":
        s.set_control_limits(1.0, 3.5)
    return s, plan


@pytest.mark.parametrize("kind", ["plain", "schedule", "limits"])
@pytest.mark.parametrize("B", [6, 70])
def test_backwards_pass_device_has_the_bits_of_backwards_pass(hip, B, kind):
    s, plan = configure(kind, B)
    gains, terms = s.backwards_pass(plan)
    assert np.isfinite(gains).all() and np.abs(gains[:, :-1, 4:]).max() > 0
    d_plan, d_gains, d_terms = hip.upload(plan), hip.alloc(gains.nbytes), hip.alloc(terms.nbytes)
    lib = capi.load()
    assert lib.qilqr_backwards_pass_device(s._h, d_plan, B, N, d_gains, d_terms) == 0, lib.qilqr_last_error()
    # (drained on return: plain copies read the results)
    assert hip.download(d_gains, gains.shape).tobytes() == gains.tobytes()
    assert hip.download(d_terms, terms.shape).tobytes() == terms.tobytes()
    assert hip.download(d_plan, plan.shape).tobytes() == plan.tobytes()
    # terms are optional
    d_again = hip.alloc(gains.nbytes)
    assert lib.qilqr_backwards_pass_device(s._h, d_plan, B, N, d_again, None) == 0
    assert hip.download(d_again, gains.shape).tobytes() == gains.tobytes()
    if kind == "schedule":  # (the schedule and the start are read: another start gives other gains)
        s.set_horizon_start(0)
        assert s.backwards_pass(plan)[0].tobytes() != gains.tobytes()
    for bad in ((None, d_gains), (d_plan, None)):
        assert lib.qilqr_backwards_pass_device(s._h, bad[0], B, N, bad[1], None) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ 2. the solver's own rollout, bit for bit

@pytest.mark.parametrize("ext", ["plain", "limits", "models"])
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("B", [6, 70])
def test_one_sample_from_the_plans_own_start_has_the_bits_of_forward_sim(B, integrator, ext):
    cfg, plan, s, _ = case(B, single_wave_rollout=1)
    s.set_integrator(integrator)
    if ext == "limits":
        s.set_control_limits(1.0, 3.5)
    if ext == "models":
        s.set_models([MODELS3[b % 3] for b in range(B)])
    gains, _ = s.backwards_pass(plan)
    want = s.forward_sim(plan, gains, alpha=0.0)
    got = s.closed_loop(plan, gains, plan[:, 0, 1:14])
    assert got["traj"].shape == (B, 1, N, 18) and got["traj"][:, 0].tobytes() == want.tobytes()
    assert flew_off_the_plan(got["traj"], plan)
    if ext == "limits":
        sat = (want[:, :, 14:18] == 1.0) | (want[:, :, 14:18] == 3.5)
        assert sat.any() and np.array_equal(got["stats"][:, 0, 3], sat.sum(axis=(1, 2)))
    else:
        assert (got["stats"][..., 3] == 0).all()


# ------------------------------------------------------------------------------------------------ 3. the restatement

@pytest.fixture(scope="module")
def restated():
    """B = 3, S = 70: plans, gains, sampled states, and the restatement's free flights (computed once, never written to)"""
    B, S = 3, 70
    cfg, plan, s, gains = case(B, single_wave_rollout=1)
    x0 = cn.sample_states(plan, S, 0, SEED + 1)
    free = {integ: cn.closed_loop(plan, gains, x0, cfg["model"], cfg["dt"], integrator=integ) for integ in (0, 1)}
    for a in (plan, gains, x0) + tuple(v for f in free.values() for v in f):
        a.setflags(write=False)
    return cfg, plan, gains, x0, free


def test_forward_sim_on_these_plans_is_inside_the_bound(restated):
    """the choice of perturbations: the solver's own rollout against the oracle's on the same plans and gains stays inside the bound the
    flights are held to"""
    cfg, plan, gains, _, _ = restated
    s = capi.from_config(cfg, single_wave_rollout=1)
    o = orc.OracleSolver(orc.model_params(**cfg["model"]), cfg["Q"], cfg["R"], cfg["desired"], cfg["dt"], orc.options(**cfg["options"]))
    for alpha in (0.0, 1.0):
        want = np.stack([o.forward_sim(plan[b], gains[b], alpha) for b in range(len(plan))])
        np.testing.assert_allclose(s.forward_sim(plan, gains, alpha), want, rtol=cn.RTOL, atol=cn.ATOL)


@pytest.mark.parametrize("integrator, limited", [(0, False), (0, True), (1, True)])
def test_flights_against_the_restatement(restated, integrator, limited):
    cfg, plan, gains, x0, free = restated
    B, S = x0.shape[0], x0.shape[1]
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    want_traj, want_stats = free[integrator]
    if limited:
        # between the samples' extremes: the median over the samples of a free flight's smallest and of its largest control.  A sample
        # whose free flight stays inside is not clamped (and flies its free flight); the others are clamped at least once.
        u = want_traj[..., 14:18]
        lo, hi = float(np.median(u.min(axis=(2, 3)))), float(np.median(u.max(axis=(2, 3))))
        s.set_control_limits(lo, hi)
        want_traj, want_stats = cn.closed_loop(plan, gains, x0, cfg["model"], cfg["dt"], integrator=integrator, limits=(lo, hi))
    got = s.closed_loop(plan, gains, x0)
    err = np.abs(got["traj"] - want_traj) / (cn.ATOL + cn.RTOL * np.abs(want_traj))
    print("[observed] integrator %d, limits %s: largest error over its bound %.3g (trajectories), %.3g (statistics)" % (
        integrator, limited, err.max(), (np.abs(got["stats"] - want_stats) / (cn.ATOL + cn.RTOL * np.abs(want_stats))).max()))
    np.testing.assert_allclose(got["traj"], want_traj, rtol=cn.RTOL, atol=cn.ATOL)
    np.testing.assert_allclose(got["stats"][..., :3], want_stats[..., :3], rtol=cn.RTOL, atol=cn.ATOL)
    assert np.array_equal(got["stats"][..., 3], want_stats[..., 3])
    assert np.array_equal(got["traj"][:, :, 0, 1:14], x0) and flew_off_the_plan(got["traj"], plan)
    # the statistics are those of the trajectories: recomputed from the restatement's primitives on the GPU's own flight
    for b, j in ((0, 0), (B - 1, S - 1)):
        dx = np.array([orc.state_minus(got["traj"][b, j, i, 1:14], plan[b, i, 1:14]) for i in range(N)])
        mine = (np.linalg.norm(dx[:, 0:3], axis=1).max(), np.linalg.norm(dx[:, 3:6], axis=1).max(), np.linalg.norm(dx[-1]))
        np.testing.assert_allclose(got["stats"][b, j, :3], mine, rtol=cn.RTOL, atol=cn.ATOL)
    count = got["stats"][..., 3]
    if limited:
        print("[observed] samples never clamped: %d of %d; most clamped pairs in one sample: %d" % ((count == 0).sum(), count.size, count.max()))
        assert (count == 0).any() and (count > 0).any()
        assert got["traj"][..., 14:18].min() == lo and got["traj"][..., 14:18].max() == hi
        stats_only = s.closed_loop(plan, gains, x0, traj=False)
        assert sorted(stats_only) == ["stats"] and stats_only["stats"].tobytes() == got["stats"].tobytes()
    else:
        assert (count == 0).all()
        traj_only = s.closed_loop(plan, gains, x0, stats=False)
        assert sorted(traj_only) == ["traj"] and traj_only["traj"].tobytes() == got["traj"].tobytes()


# ------------------------------------------------------------------------------------------------ 4. one arithmetic across the forms

@pytest.mark.parametrize("integrator", [0, 1])
def test_a_samples_bits_do_not_depend_on_the_form_that_carried_it(restated, integrator):
    cfg, plan, gains, x0, _ = restated
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    s.set_control_limits(0.5, 5.0)
    whole = s.closed_loop(plan, gains, x0)  # S = 70: the flattened form, wavefronts that hold samples of two plans
    assert (whole["stats"][..., 3] > 0).any()
    for j in (0, 63, 64, 69):  # S = 1: the flattened form
        alone = s.closed_loop(plan, gains, x0[:, j])
        assert alone["traj"][:, 0].tobytes() == whole["traj"][:, j].tobytes() and alone["stats"][:, 0].tobytes() == whole["stats"][:, j].tobytes(), j
    pick = [69, 0, 64, 7, 63]  # S = 5: the flattened form, a wavefront over three plans
    five = s.closed_loop(plan, gains, x0[:, pick])
    assert five["traj"].tobytes() == whole["traj"][:, pick].tobytes() and five["stats"].tobytes() == whole["stats"][:, pick].tobytes()
    one_wave = s.closed_loop(plan, gains, x0[:, :64])  # S = 64: the shared-operand form, exactly one wavefront per plan
    assert one_wave["traj"].tobytes() == whole["traj"][:, :64].tobytes() and one_wave["stats"].tobytes() == whole["stats"][:, :64].tobytes()
    again = list(range(70)) + list(range(56))  # S = 126: the shared-operand form, two wavefronts per plan, two idle lanes in the second
    two_waves = s.closed_loop(plan, gains, x0[:, again])
    assert two_waves["traj"].tobytes() == whole["traj"][:, again].tobytes() and two_waves["stats"].tobytes() == whole["stats"][:, again].tobytes()


@pytest.mark.parametrize("B, S", [(6, 5), (70, 1), (70, 5), (6, 64), (6, 70), (3, 126)])
def test_every_sample_is_flown_with_its_own_plan_and_state(B, S):
    """larger batches and every S of both forms: sample (b, j) against the same sample flown alone"""
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 2)
    whole = s.closed_loop(plan, gains, x0)
    assert not np.isnan(whole["traj"]).any() and flew_off_the_plan(whole["traj"], plan)
    for b, j in ((0, 0), (B - 1, S - 1), (B // 2, S // 2)):
        alone = s.closed_loop(plan[b:b + 1], gains[b:b + 1], x0[b:b + 1, j:j + 1])
        assert alone["traj"][0, 0].tobytes() == whole["traj"][b, j].tobytes() and alone["stats"][0, 0].tobytes() == whole["stats"][b, j].tobytes()


# ------------------------------------------------------------------------------------------------ 5. windows

@pytest.mark.parametrize("S", [5, 64, 70, 126])
def test_windows_of_knots(hip, S):
    B = 3
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 3)
    whole = s.closed_loop(plan, gains, x0)
    # a run 0 .. 11 continued from its own knot 11 over 11 .. 23 is the run 0 .. 23; what lies outside a window stays NaN
    first = s.closed_loop(plan, gains, x0, 0, 11)
    assert np.isnan(first["traj"][:, :, 12:]).all() and first["traj"][:, :, :12].tobytes() == whole["traj"][:, :, :12].tobytes()
    rest = s.closed_loop(plan, gains, first["traj"][:, :, 11, 1:14], 11, N - 1)
    assert np.isnan(rest["traj"][:, :, :11]).all() and rest["traj"][:, :, 11:].tobytes() == whole["traj"][:, :, 11:].tobytes()
    assert np.array_equal(rest["stats"][..., 2], whole["stats"][..., 2])
    assert np.array_equal(np.maximum(first["stats"][..., :2], rest["stats"][..., :2]), whole["stats"][..., :2])
    # i0 = i1 = 9: the policy at a measured state is knot 9 of the run 9 .. 23 from that state
    x9 = cn.sample_states(plan, S, 9, SEED + 4)
    run = s.closed_loop(plan, gains, x9, 9, N - 1)
    at = s.closed_loop(plan, gains, x9, 9, 9)
    assert at["traj"][:, :, 9].tobytes() == run["traj"][:, :, 9].tobytes()
    assert np.isnan(at["traj"][:, :, :9]).all() and np.isnan(at["traj"][:, :, 10:]).all() and np.isnan(run["traj"][:, :, :9]).all()
    assert np.array_equal(at["traj"][:, :, 9, 1:14], x9) and flew_off_the_plan(run["traj"], plan, 9)
    # the device form leaves every byte outside the window as it was
    d = [hip.upload(a) for a in (plan, gains, x9)]
    d_traj, d_stats = hip.alloc(8 * B * S * N * 18), hip.alloc(8 * B * S * 4)
    lib = capi.load()
    assert lib.qilqr_closed_loop_device(s._h, d[0], d[1], d[2], B, N, S, 9, 12, d_traj, d_stats) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    raw = hip.download(d_traj, (B, S, N, 18 * 8), np.uint8)
    assert (raw[:, :, :9] == 0xFF).all() and (raw[:, :, 13:] == 0xFF).all()
    assert raw[:, :, 9:13].tobytes() == run["traj"][:, :, 9:13].tobytes()


# ------------------------------------------------------------------------------------------------ 6. models, and what a call refuses

@pytest.mark.parametrize("S", [5, 64, 70, 126])
def test_per_sample_models(S):
    B = 3
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 5)
    plain = s.closed_loop(plan, gains, x0)
    own = B * S - 2  # the one sample whose model is the handle's
    models = [MODELS3[1 + r % 2] for r in range(B * S)]
    models[own] = cfg["model"]
    s.set_models(models)
    got = s.closed_loop(plan, gains, x0)
    flat = lambda a: a.reshape((B * S,) + a.shape[2:])
    assert flat(got["traj"])[own].tobytes() == flat(plain["traj"])[own].tobytes()
    assert flat(got["stats"])[own].tobytes() == flat(plain["stats"])[own].tobytes()
    others = np.delete(np.arange(B * S), own)
    assert (np.abs(flat(got["traj"])[others, 2:, 1:14] - flat(plain["traj"])[others, 2:, 1:14]).max(axis=(1, 2)) > 1e-6).all()
    # ... and each of them is the restatement's flight with that model
    want_traj, want_stats = cn.closed_loop(plan[:1], gains[:1], x0[:1, :3], cfg["model"], cfg["dt"], models=models[:3])
    np.testing.assert_allclose(got["traj"][:1, :3], want_traj, rtol=cn.RTOL, atol=cn.ATOL)
    np.testing.assert_allclose(got["stats"][:1, :3], want_stats, rtol=cn.RTOL, atol=cn.ATOL)
    # another count is refused: B models for B x S samples, and B S models for one sample per plan
    with pytest.raises(TypeError, match=r"B \* S samples.*set for %d.*B \* S = %d" % (B * S, B)):
        s.closed_loop(plan, gains, x0[:, 0])
    s.set_models(models[:B])
    with pytest.raises(TypeError, match=r"B \* S samples"):
        s.closed_loop(plan, gains, x0)
    assert s.closed_loop(plan, gains, x0[:, 0])["traj"].shape == (B, 1, N, 18)


def test_what_a_call_refuses_on_a_handle():
    B, S = 3, 5
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 6)
    with pytest.raises(TypeError, match="precision 0"):
        capi.from_config(cfg, precision="f32").closed_loop(plan, gains, x0)
    with pytest.raises(TypeError, match="no output"):
        s.closed_loop(plan, gains, x0, traj=False, stats=False)
    for i0, i1 in ((-1, 3), (3, 2), (0, N)):
        with pytest.raises(TypeError, match="i0 <= i1"):
            s.closed_loop(plan, gains, x0, i0, i1)
    bad = x0.copy()
    bad[2, 3, 3:7] *= 1.001
    with pytest.raises(ValueError, match="quaternion not normalized at problem 2, sample 3"):
        s.closed_loop(plan, gains, bad)
    for shape_error in (lambda: s.closed_loop(plan, gains[:, :, :48], x0), lambda: s.closed_loop(plan, gains, x0[:, :, :12]),
                        lambda: s.closed_loop(plan[:, :, :17], gains, x0)):
        with pytest.raises(TypeError):
            shape_error()
    assert s.closed_loop(plan, gains, x0)["stats"].shape == (B, S, 4)  # (the handle is served after them)


# ------------------------------------------------------------------------------------------------ 7. stream ordering

@pytest.mark.parametrize("S", [1, 64, 70, 126])
def test_the_device_forms_in_a_row_and_one_synchronise(hip, S):
    B = 6
    cfg, plan, s, gains = case(B)
    x0 = cn.sample_states(plan, S, 0, SEED + 7)
    want = s.closed_loop(plan, gains, x0)
    d_plan, d_x0 = hip.upload(plan), hip.upload(x0)
    d_gains, d_traj, d_stats = hip.alloc(gains.nbytes), hip.alloc(want["traj"].nbytes), hip.alloc(want["stats"].nbytes)
    lib = capi.load()
    assert lib.qilqr_backwards_pass_device(s._h, d_plan, B, N, d_gains, None) == 0, lib.qilqr_last_error()
    assert lib.qilqr_closed_loop_device(s._h, d_plan, d_gains, d_x0, B, N, S, 0, N - 1, d_traj, d_stats) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    assert hip.download(d_traj, want["traj"].shape).tobytes() == want["traj"].tobytes()
    assert hip.download(d_stats, want["stats"].shape).tobytes() == want["stats"].tobytes()
    # statistics only
    d_only = hip.alloc(want["stats"].nbytes)
    assert lib.qilqr_closed_loop_device(s._h, d_plan, d_gains, d_x0, B, N, S, 0, N - 1, None, d_only) == 0
    hip.synchronize(lib.qilqr_stream(s._h))
    assert hip.download(d_only, want["stats"].shape).tobytes() == want["stats"].tobytes()


@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/closed_loop_torch_child.py, once: PyTorch's ROCm runtime has to be the first a process initialises, and this one runs the
    library's already.  The arrays it recorded."""
    out = str(tmp_path_factory.mktemp("closed_loop_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.closed_loop_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_the_torch_forms(torch_forms):
    r = torch_forms
    for k in ("gains", "terms", "traj", "stats"):
        assert r["device_" + k].tobytes() == r["host_" + k].tobytes() and not np.isnan(r["device_" + k]).any(), k
    assert r["device_stats_only"].tobytes() == r["host_stats"].tobytes()
    said = {k[len("refusal_"):]: str(v) for k, v in r.items() if k.startswith("refusal_")}
    assert said["fine"] == "accepted", said["fine"]
    for k, kind, text in (("no_output", "TypeError", "no output"), ("overlap", "TypeError", "overlaps an input"), ("x0_shape", "TypeError", "x0 must have shape"),
                          ("gains_shape", "TypeError", "gains must have shape"), ("float32", "TypeError", "float64"),
                          ("host_tensor", "TypeError", "CUDA tensor"), ("window", "TypeError", "i0 <= i1"), ("gains_missing", "TypeError", "gains"),
                          ("control_without_gains", "RuntimeError", "gains=True")):
        assert said[k].startswith(kind) and text in said[k], (k, said[k])


def test_receding_horizon_with_gains_and_control(torch_forms):
    r = torch_forms
    for tick in range(3):
        tag = "tick%d_" % tick
        # the defaults return what they returned: the same keys, and the plans of the loop that asks for gains
        assert r[tag + "plain_keys"].tolist() == ["cost", "iters", "status", "traj", "u0"]
        assert r[tag + "keys"].tolist() == ["cost", "gains", "iters", "status", "traj", "u0"]
        for k in ("traj", "cost", "status", "iters", "u0"):
            assert r[tag + k].tobytes() == r[tag + "plain_" + k].tobytes(), (tick, k)
        assert (r[tag + "status"] <= 1).all()
        # the gains are the backward pass on the new plan, at the horizon start it was solved at
        assert r[tag + "gains"].tobytes() == r[tag + "host_gains"].tobytes() and np.abs(r[tag + "gains"][:, :-1, 4:]).max() > 0
        # control(x, i) is the flight of one sample over the one knot i
        for i in (0, 3):
            got, want = r[tag + "control%d" % i], r[tag + "host_control%d" % i]
            assert got.shape == (6, 4) and got.tobytes() == want.tobytes(), (tick, i)
            assert np.abs(got - r[tag + "traj"][:, i, 14:18]).max() > 1e-3  # (off the plan the law is not the plan's control)
        # at the plan's own state it is the plan's first control (x (-) x need not be an exact zero under fused arithmetic)
        np.testing.assert_allclose(r[tag + "control_on_plan"], r[tag + "u0"], rtol=0, atol=1e-12)
    assert not r["plain_allocated_gains"]
