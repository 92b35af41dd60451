"""Linear covariance analysis on the device (k_cov_build, k_cov_chain, k_cov_summary: cov_kernels.h) through the C ABI on plain device
buffers: every instantiation against the host program (tests/host_cov_harness.cpp, the bar of the issue: 1e-10 of sqrt(r_kk r_ll)) and the
restatement (tests/lincov_numpy.py, at the bars tests/test_covariance_cpu.py derives for its central differences), the sphere tables at
capacity and across the per-problem table's second tile, a plan's independence of its batch, guard bytes, refused calls, the open loop --
and against the device's own Monte Carlo: 4096 flights of the law from sampled states under sampled gusts, whose sample covariance and mean
must lie within six of their own sampling deviations of what the analysis says.  RecedingHorizon.evaluate_covariance in a torch process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle as orc  # noqa: E402
from quadrotorilqr_amd import capi  # noqa: E402
from tests import closed_loop_numpy as cn, lincov_cases as lc, lincov_numpy as ln  # noqa: E402
from tests.test_covariance_cpu import COV_BAR, MEAN_BAR, RULE, relative  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes behind the end of every output, prefilled with 0xFF like the output
RTOL = ln.RTOL
SHAPES = dict(cov=lambda b, n: (b, n, 12, 12), mean=lambda b, n: (b, n, 12), summary=lambda b, n: (b, 8))


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def harness():
    return lc.build_harness(["-O2"], "host_cov_harness")


def handle(cfg, integrator=0, models=None, shared=None, own=None, counts=None, **kw):
    s = capi.from_config(cfg, **kw)
    s.set_integrator(integrator)
    if models is not None:
        s.set_models(models)
    if shared is not None:
        s.set_obstacles(shared)
    if own is not None:
        s.set_batch_obstacles(own, counts)
    return s


def dev_cov(hip, s, plan, gains, state_sigma=lc.SIGMA12, sigma=lc.GUST_SIGMA, mean=None, tau_force_s=0.0, tau_torque_s=0.0, held=False, i0=0, i1=None,
            outputs=("cov", "mean", "summary"), expect=0, d_gains=None):
    """one call on 0xFF-prefilled outputs with a guard behind each: dict of the outputs asked for, plus "raw" (their bytes) -- after asserting
    that every guard kept its bits.  expect: the return code."""
    lib = capi.load()
    b, n = plan.shape[:2]
    i1 = n - 1 if i1 is None else i1
    rule = capi.cov_rule(state_sigma, dict(sigma=sigma, mean=0.0 if mean is None else mean, tau_force_s=tau_force_s, tau_torque_s=tau_torque_s), held)
    d_plan = hip.upload(plan)
    if d_gains is None:
        d_gains = hip.upload(gains) if gains is not None else None
    ptr = {k: hip.alloc(8 * int(np.prod(SHAPES[k](b, n))) + GUARD) for k in outputs}
    rc = lib.qilqr_covariance_device(s._h, C.byref(rule), d_plan, d_gains, b, n, i0, i1, ptr.get("cov"), ptr.get("mean"), ptr.get("summary"))
    assert rc == expect, (rc, lib.qilqr_last_error())
    hip.synchronize(lib.qilqr_stream(s._h))
    out = dict(raw={}, text=lib.qilqr_last_error().decode() if rc else "")
    for k in outputs:
        nbytes = 8 * int(np.prod(SHAPES[k](b, n)))
        raw = hip.download(ptr[k], (nbytes + GUARD,), dtype=np.uint8)
        assert (raw[nbytes:] == 0xFF).all(), "the call wrote behind the end of " + k
        out[k], out["raw"][k] = raw[:nbytes].view(np.float64).reshape(SHAPES[k](b, n)), raw[:nbytes]
    return out


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def against_harness(got, want, i0, i1, label):
    """covariances within 1e-10 of sqrt(r_kk r_ll), means within 1e-10 of sqrt(r_kk); the discrete words of the summary exact and the others,
    smooth functions of entries held to 1e-10, within 1e-9; knots outside the window keep their bits"""
    win = slice(i0, i1 + 1)
    ec, em = relative(dict(cov=got["cov"][:, win], mean=got["mean"][:, win]), dict(cov=want["cov"][:, win], mean=want["mean"][:, win]))
    print("[observed] %s: device against host, covariance %.3g of sqrt(r_kk r_ll), mean %.3g of sqrt(r_kk)" % (label, ec, em))
    assert ec <= RTOL and em <= RTOL, (label, ec, em)
    assert untouched(got["cov"][:, :i0]) and untouched(got["cov"][:, i1 + 1:]) and untouched(got["mean"][:, :i0]) and untouched(got["mean"][:, i1 + 1:]), label
    assert np.array_equal(got["summary"][:, [1, 5, 6]], want["summary"][:, [1, 5, 6]]), (label, got["summary"], want["summary"])
    np.testing.assert_allclose(got["summary"][:, [0, 2, 3, 4, 7]], want["summary"][:, [0, 2, 3, 4, 7]], rtol=10 * RTOL, err_msg=label)
    cov = got["cov"][:, win]
    assert cov.tobytes() == np.ascontiguousarray(np.swapaxes(cov, -1, -2)).tobytes() and (np.einsum("bnii->bni", cov) >= 0.0).all(), label


# ------------------------------------------------------------------------------------------------ 1. every instantiation

@pytest.mark.parametrize("n", [2, 9, 16, 17])
@pytest.mark.parametrize("modeled", [False, True])
@pytest.mark.parametrize("integrator", [0, 1])
def test_every_instantiation_against_the_harness_and_the_restatement(hip, harness, integrator, modeled, n):
    """{Euler, Runge-Kutta} x {the handle's model, per-problem models} at B = 3 with 8 shared spheres and a moving one per plan; n = 2 (one
    step), 9, 16 and 17 (the chain's prefetch runs one knot ahead: its last load is knot i1 - 1's), over a window inside the horizon"""
    cfg, plan, gains, shared, own, counts = lc.standard(integrator, modeled, lc.B, n)
    models = lc.MODELS3 if modeled else None
    i0, i1 = (0, 1) if n == 2 else (1, n - 2)
    label = str((integrator, modeled, n))
    s = handle(cfg, integrator, models, shared, own, counts)
    got = dev_cov(hip, s, plan, gains, i0=i0, i1=i1, **RULE)
    host = lc.host_run(harness, cfg, plan, gains, integrator=integrator, models=models, i0=i0, i1=i1, shared=shared, own=own, counts=counts, **RULE)
    want = ln.covariance(plan, gains, cfg["model"], cfg["dt"], lc.SIGMA12, lc.GUST_SIGMA, integrator=integrator, models=models, i0=i0, i1=i1,
                         shared=shared, own=lc.own_rows(own, counts), **RULE)
    gp, gz = ln.margins(want, i0, i1)
    assert gp > 1e-6 and gz > 1e-6, (label, gp, gz)
    against_harness(got, host, i0, i1, label)
    win = slice(i0, i1 + 1)
    ec, em = relative(dict(cov=got["cov"][:, win], mean=got["mean"][:, win]), dict(cov=want["cov"][:, win], mean=want["mean"][:, win]))
    assert ec <= COV_BAR and em <= MEAN_BAR, (label, ec, em)
    assert np.array_equal(got["summary"][:, [1, 5, 6]], want["summary"][:, [1, 5, 6]]), label
    # each output alone has the bits it has among the others (the summary then reads the handle's scratch)
    for only in ("cov", "mean", "summary"):
        assert dev_cov(hip, s, plan, gains, i0=i0, i1=i1, outputs=(only,), **RULE)["raw"][only].tobytes() == got["raw"][only].tobytes(), (label, only)


# ------------------------------------------------------------------------------------------------ 2. the sphere tables

def test_sphere_tables_at_capacity(hip, harness):
    """64 shared spheres and 64 own with counts 64, 0, 37; rows beyond a count hold a sphere of radius 1 on the path, ruinous if it were
    read.  The last sphere in use of each table is the nearest of its plan: a sphere about the plan's first knot, deeper than any other
    (radius 2 in the shared table, 3 in a plan's own, where no other in use exceeds 0.16)."""
    cfg, plan, gains, _, _, _ = lc.standard(1, False, 3, 9)
    r = np.random.default_rng(5)
    counts = np.array([64, 0, 37], dtype=np.int32)
    shared, own = np.zeros((64, 5)), np.zeros((3, 64, 8))
    shared[:, :3] = plan[np.arange(64) % 3, np.arange(64) % 9, 1:4] + 0.4 * (2.0 * r.random((64, 3)) - 1.0)
    shared[:, 3], shared[:, 4] = 0.1 + 0.02 * (np.arange(64) % 4), 10.0
    for b in range(3):
        own[b, :, :3] = plan[b, np.arange(64) % 9, 1:4] + 0.4 * (2.0 * r.random((64, 3)) - 1.0)
        own[b, :, 3:6] = 0.1 * (2.0 * r.random((64, 3)) - 1.0)
        own[b, :, 6], own[b, :, 7] = 0.12, 30.0
        for j in range(counts[b], 64):
            own[b, j] = (*plan[b, j % 9, 1:4], 0.0, 0.0, 0.0, 1.0, 1e6)
    shared[63, :4] = (*(plan[1, 0, 1:4] + 0.01), 2.0)
    own[0, 63] = (*(plan[0, 0, 1:4] + 0.01), 0.0, 0.0, 0.0, 3.0, 30.0)
    own[2, 36] = (*(plan[2, 0, 1:4] - 0.01), 0.0, 0.0, 0.0, 3.0, 30.0)
    s = handle(cfg, 1, None, shared, own, counts)
    got = dev_cov(hip, s, plan, gains, **RULE)
    host = lc.host_run(harness, cfg, plan, gains, integrator=1, shared=shared, own=own, counts=counts, **RULE)
    against_harness(got, host, 0, 8, "capacity")
    assert got["summary"][:, 6].tolist() == [64 + 63, 63, 64 + 36], got["summary"]  # (its knot is the harness's: against_harness)
    want = ln.covariance(plan, gains, cfg["model"], cfg["dt"], lc.SIGMA12, lc.GUST_SIGMA, integrator=1, shared=shared, own=lc.own_rows(own, counts), **RULE)
    np.testing.assert_allclose(got["summary"][:, 4], want["summary"][:, 4], rtol=MEAN_BAR)


def test_the_second_tile_of_the_per_problem_table(hip, harness):
    """B = 70, own counts (b + 1) % 4, a model per plan: rows 0, 63, 64 and 69 have the bytes of the plan alone with its own table and model"""
    Bt, n, K = 70, 4, 3
    cfg, plan, gains, shared, _, _ = lc.standard(0, True, Bt, n)
    models = [lc.MODELS3[b % 3] for b in range(Bt)]
    counts = ((np.arange(Bt) + 1) % 4).astype(np.int32)
    r = np.random.default_rng(8)
    own = np.zeros((Bt, K, 8))
    own[..., :3] = plan[:, [1, 2, 3], 1:4] + 0.3 * (2.0 * r.random((Bt, K, 3)) - 1.0)
    own[..., 3:6] = 0.2 * (2.0 * r.random((Bt, K, 3)) - 1.0)
    own[..., 6], own[..., 7] = 0.15, 25.0
    for b in range(Bt):
        own[b, counts[b]:] = (*plan[b, 2, 1:4], 0.0, 0.0, 0.0, 1.0, 1e6)
    s = handle(cfg, 0, models, shared, own, counts)
    whole = dev_cov(hip, s, plan, gains, **RULE)
    host = lc.host_run(harness, cfg, plan, gains, models=models, shared=shared, own=own, counts=counts, **RULE)
    against_harness(whole, host, 0, n - 1, "tile")
    assert set(whole["summary"][counts > 0, 6].astype(int)) - set(range(8)), "no plan is nearest to a sphere of its own"
    for b in (0, 63, 64, 69):
        one = handle(cfg, 0, models[b:b + 1], shared, own[b:b + 1], counts[b:b + 1])
        alone = dev_cov(hip, one, plan[b:b + 1], gains[b:b + 1], **RULE)
        for k in ("cov", "mean", "summary"):
            assert alone[k][0].tobytes() == whole[k][b].tobytes(), (b, k)


# ------------------------------------------------------------------------------------------------ 3. independence, refusals, the open loop

def test_a_plans_bits_do_not_depend_on_the_batch(hip):
    cfg, plan, gains, shared, own, counts = lc.standard(1, True, lc.B, 9)
    kw = dict(tau_torque_s=0.02, held=False, **RULE)
    whole = dev_cov(hip, handle(cfg, 1, lc.MODELS3, shared, own, counts), plan, gains, i0=2, **kw)
    for b in range(lc.B):
        one = handle(cfg, 1, lc.MODELS3[b:b + 1], shared, own[b:b + 1], counts[b:b + 1])
        alone = dev_cov(hip, one, plan[b:b + 1], gains[b:b + 1], i0=2, **kw)
        for k in ("cov", "mean", "summary"):
            assert alone["raw"][k].tobytes() == whole["raw"][k].reshape(lc.B, -1)[b].tobytes(), (b, k)


def test_refused_calls_on_a_live_handle_leave_the_outputs_untouched(hip):
    cfg, plan, gains, shared, own, counts = lc.standard(0, False, lc.B, 9)
    s = handle(cfg, 0, None, shared, own, counts)
    for change, why in [(dict(i1=9), "0 <= i0 <= i1 <= n - 1"), (dict(i0=5, i1=4), "0 <= i0 <= i1 <= n - 1"), (dict(state_sigma=-1.0), "every sigma"),
                        (dict(tau_force_s=float("nan")), "correlation times"), (dict(mean=float("inf")), "the mean must be finite")]:
        got = dev_cov(hip, s, plan, gains, expect=capi.ERR_INVALID_ARG, **change)
        assert why in got["text"] and all(untouched(got[k]) for k in ("cov", "mean", "summary")), (change, got["text"])
    # the handle's own reasons: models or spheres for another B, the mixed-precision mode
    two = dev_cov(hip, s, plan[:2], gains[:2], expect=capi.ERR_INVALID_ARG)
    assert "per-problem obstacles were set for another B" in two["text"] and untouched(two["cov"]) and untouched(two["summary"])
    s.clear_batch_obstacles()
    s.set_models(lc.MODELS3[:2])
    got = dev_cov(hip, s, plan, gains, expect=capi.ERR_INVALID_ARG)
    assert "per-problem models were set for another B" in got["text"] and untouched(got["cov"]) and untouched(got["mean"])
    s.clear_models()
    assert np.isfinite(dev_cov(hip, s, plan, gains)["cov"]).all()
    got = dev_cov(hip, handle(cfg, precision="f32"), plan, gains, expect=capi.ERR_INVALID_ARG)
    assert "precision 0" in got["text"] and untouched(got["cov"])
    # an output that overlaps an input
    lib = capi.load()
    d_plan, d_gains = hip.upload(plan), hip.upload(gains)
    rule = capi.cov_rule(lc.SIGMA12, dict(sigma=lc.GUST_SIGMA))
    assert lib.qilqr_covariance_device(s._h, C.byref(rule), d_plan, d_gains, lc.B, 9, 0, 8, None, d_plan + 16, None) == capi.ERR_INVALID_ARG
    assert "an output overlaps an input" in lib.qilqr_last_error().decode()
    hip.synchronize(lib.qilqr_stream(s._h))
    assert hip.download(d_plan, plan.shape).tobytes() == plan.tobytes()


@pytest.mark.parametrize("integrator", [0, 1])
def test_without_gains_is_a_zero_gain_array(hip, harness, integrator):
    cfg, plan, gains, shared, own, counts = lc.standard(integrator, False, lc.B, 9)
    s = handle(cfg, integrator, None, shared, own, counts)
    null = dev_cov(hip, s, plan, None, held=True, **RULE)
    zero = dev_cov(hip, s, plan, np.zeros_like(gains), held=True, **RULE)
    for k in ("cov", "mean", "summary"):
        assert null["raw"][k].tobytes() == zero["raw"][k].tobytes(), k
    assert not null["summary"][:, 7].any() and (dev_cov(hip, s, plan, gains, held=True, **RULE)["cov"] != null["cov"]).any()
    against_harness(null, lc.host_run(harness, cfg, plan, None, integrator=integrator, held=True, shared=shared, own=own, counts=counts, **RULE), 0, 8, "open loop")


def test_known_answers_on_the_device(hip):
    cfg, plan, gains, shared, _, _ = lc.standard(1, False, lc.B, 9)
    s = handle(cfg, 1)
    still = dev_cov(hip, s, plan, gains, state_sigma=np.zeros(12), sigma=np.zeros(6))
    assert not still["cov"].any() and not still["mean"].any() and not still["summary"][:, [0, 1, 2, 3, 7]].any()
    assert (still["summary"][:, 4] == np.inf).all() and (still["summary"][:, 5:7] == -1).all()
    one = dev_cov(hip, s, plan, gains, i0=4, i1=4, **RULE)
    assert np.array_equal(one["cov"][:, 4], np.broadcast_to(np.diag(lc.SIGMA12 * lc.SIGMA12), (lc.B, 12, 12))) and not one["mean"][:, 4].any()
    assert untouched(one["cov"][:, :4]) and untouched(one["cov"][:, 5:]) and np.array_equal(one["summary"][:, 1], np.full(lc.B, 4.0))
    white, short = (dev_cov(hip, s, plan, gains, tau_force_s=t, tau_torque_s=t, mean=lc.GUST_MEAN) for t in (0.0, 1e-6 * cfg["dt"]))
    held, long = dev_cov(hip, s, plan, gains, held=True, mean=lc.GUST_MEAN), dev_cov(hip, s, plan, gains, tau_force_s=1e30, tau_torque_s=1e30, mean=lc.GUST_MEAN)
    for k in ("cov", "mean", "summary"):
        assert white["raw"][k].tobytes() == short["raw"][k].tobytes() and held["raw"][k].tobytes() == long["raw"][k].tobytes(), k
    assert (held["cov"][:, -1] != white["cov"][:, -1]).any()


# ------------------------------------------------------------------------------------------------ 4. against the device's own Monte Carlo

@pytest.mark.parametrize("integrator", [0, 1])
def test_against_the_devices_own_monte_carlo(hip, integrator):
    """B = 2, n = 12, S = 4096: plans from a small solve (hence consistent), gains from qilqr_backwards_pass_device, no limits; start states
    from qilqr_sample_states_device, gusts from qilqr_sample_gusts_device with n_w = n, flown by qilqr_closed_loop_scored_device; dx on the
    host by oracle.state_minus.  Every entry of the sample covariance within 6 sqrt((S_kk S_ll + S_kl^2) / (S - 1)) of d_cov -- the entry's
    own sampling deviation under a Gaussian -- and, with a mean wrench, every sample mean within 6 sqrt(S_kk / S) of d_mean.  The bars are
    derived, not tuned; the CPU check of the model observed 2.96 and 1.7."""
    Bm, n, S = 2, 12, 4096
    lib = capi.load()
    cfg, init = cn.plans(Bm, n, 3)
    s = handle(cfg, integrator)
    d_init, d_plan, d_gains = hip.upload(init), hip.alloc(8 * Bm * n * 18), hip.alloc(8 * Bm * n * 52)
    assert lib.qilqr_solve_batch_device(s._h, C.c_void_p(d_init), None, Bm, n, C.c_void_p(d_plan), None, None, None, None, None) == 0, lib.qilqr_last_error()
    assert lib.qilqr_backwards_pass_device(s._h, d_plan, Bm, n, d_gains, None) == 0, lib.qilqr_last_error()
    plan, gains = hip.download(d_plan, (Bm, n, 18)), hip.download(d_gains, (Bm, n, 52))
    assert np.isfinite(plan).all() and np.isfinite(gains).all()
    d_nom, d_x0, d_w = hip.upload(np.ascontiguousarray(plan[:, 0, 1:14])), hip.alloc(8 * Bm * S * 13), hip.alloc(8 * Bm * S * n * 6)
    d_traj = hip.alloc(8 * Bm * S * n * 18)
    sig12 = np.ascontiguousarray(lc.SIGMA12)
    worst = {}
    for tag, mean in (("cov", None), ("mean", lc.GUST_MEAN)):
        m = capi.gust_model(lc.GUST_SIGMA, mean, lc.TAU_FORCE, 0.0)
        assert lib.qilqr_sample_states_device(s._h, d_nom, sig12.ctypes.data, 77, Bm, S, 0, 0, 0, d_x0) == 0, lib.qilqr_last_error()
        assert lib.qilqr_sample_gusts_device(s._h, C.byref(m), 78, Bm, S, n, 0, 0, d_w) == 0, lib.qilqr_last_error()
        assert lib.qilqr_closed_loop_scored_device(s._h, d_plan, d_gains, d_x0, d_w, n, None, Bm, n, S, 0, n - 1, d_traj, None, None) == 0, lib.qilqr_last_error()
        hip.synchronize(lib.qilqr_stream(s._h))
        traj = hip.download(d_traj, (Bm, S, n, 18))
        got = dev_cov(hip, s, plan, None, mean=mean, tau_force_s=lc.TAU_FORCE, d_gains=d_gains)
        dx = np.empty((Bm, S, n, 12))
        for b, j, i in np.ndindex(Bm, S, n):
            dx[b, j, i] = orc.state_minus(traj[b, j, i, 1:14], plan[b, i, 1:14])
        Sg = got["cov"]
        d = np.einsum("bnii->bni", Sg)
        if tag == "cov":
            c = dx - dx.mean(axis=1, keepdims=True)
            sample = np.einsum("bjnk,bjnl->bnkl", c, c) / (S - 1)
            dev = np.sqrt((d[..., :, None] * d[..., None, :] + Sg * Sg) / (S - 1))
            worst[tag] = float((np.abs(sample - Sg) / dev).max())
        else:
            worst[tag] = float((np.abs(dx.mean(axis=1) - got["mean"])[:, 1:] / np.sqrt(d / S)[:, 1:]).max())
            assert np.abs(got["mean"][:, -1]).max() > 1e-5
    print("[observed] integrator %d: sample covariance within %.3g, sample mean within %.3g of their own sampling deviations" % (integrator, worst["cov"], worst["mean"]))
    assert worst["cov"] <= 6.0 and worst["mean"] <= 6.0, worst


# ------------------------------------------------------------------------------------------------ 5. RecedingHorizon.evaluate_covariance

def test_evaluate_covariance_has_the_bits_of_the_direct_call(hip, tmp_path):
    """tests/lincov_torch_child.py, in a process of its own (PyTorch's ROCm runtime has to be the first a process initialises), records what
    RecedingHorizon.evaluate_covariance and the direct torch call return about the same plan and gains; here the C ABI is called on them too"""
    out = str(tmp_path / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.lincov_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        rec = {k: z[k] for k in z.files}
    assert "needs the gains" in str(rec["refusal_without_gains"]) and "must have shape" in str(rec["refusal_shape"])
    assert rec["rh_summary"].tobytes() == rec["direct_summary"].tobytes() and rec["rh_cov"].reshape(rec["direct_cov"].shape).tobytes() == rec["direct_cov"].tobytes()
    assert rec["rh_summary_only"].tobytes() == rec["rh_summary"].tobytes() and bool(rec["cov_is_none"])
    cfg, _, shared = lc.torch_case()
    s = handle(cfg, 1, None, shared)
    got = dev_cov(hip, s, rec["plan"], rec["gains"], **lc.TORCH_GUST)
    assert got["summary"].tobytes() == rec["rh_summary"].tobytes() and got["cov"].tobytes() == rec["rh_cov"].tobytes()
    assert np.isfinite(got["summary"]).all() and (got["summary"][:, 6] >= 0).all()
