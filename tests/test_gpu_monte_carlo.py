"""The Monte-Carlo kernels on the device (k_sample_gusts, k_sample_states, k_reduce_scores: monte_carlo_kernels.h) through the C ABI
on plain device buffers, against the restatement in NumPy (tests/monte_carlo_numpy.py) with its bounds, and against themselves: a row's
bits do not depend on the batch it is drawn in, nothing is written behind the end of an output, a plan's summary does not depend on the
other plans, four enqueues in a row are right behind one synchronise; and RecedingHorizon.evaluate_sampled, in a torch process of its
own, against evaluate() fed what it sampled.  B = 3, n = 24, S in {1, 5, 64, 70, 126, 130}."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi  # noqa: E402
from tests import closed_loop_numpy as cn, monte_carlo_numpy as mn  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, SEED = 3, 24, (0x5eed << 32) | 1234
SIZES = [1, 5, 64, 70, 126, 130]
MEAN6 = np.array([0.4, -0.2, 0.1, 0.01, -0.02, 0.03])
SIGMA6 = np.array([1.5, 1.2, 0.8, 0.05, 0.04, 0.06])
SIGMA12 = np.array([0.05, 0.04, 0.06, 0.03, 0.02, 0.04, 0.1, 0.12, 0.08, 0.05, 0.06, 0.04])
GUARD = 64  # bytes behind the end of every output, prefilled with 0xFF like the output


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def handle():
    """(cfg, solver, x_nom): a handle -- its dt, its stream -- and the measured states of B plans"""
    cfg, plan = cn.plans(B, N, 5)
    x = np.ascontiguousarray(cn.sample_states(plan, 1, 0, 6)[:, 0])
    x.setflags(write=False)
    return cfg, capi.from_config(cfg), x


def guarded(hip, shape):
    return hip.alloc(8 * int(np.prod(shape)) + GUARD)


def fetch(hip, ptr, shape):
    """the output and whether the guard behind it kept its bits"""
    words = int(np.prod(shape))
    raw = hip.download(ptr, (8 * words + GUARD,), dtype=np.uint8)
    return raw[:8 * words].view(np.float64).reshape(shape), bool((raw[8 * words:] == 0xFF).all())


def dev_gusts(hip, s, seed, b, S, n_w, sigma=SIGMA6, mean=MEAN6, tau_f=0.0, tau_t=0.0, b0=0, s0=0):
    lib = capi.load()
    m = capi.gust_model(sigma, mean, tau_f, tau_t)
    d = guarded(hip, (b, S, n_w, 6))
    assert lib.qilqr_sample_gusts_device(s._h, C.byref(m), seed, b, S, n_w, b0, s0, d) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    out, kept = fetch(hip, d, (b, S, n_w, 6))
    assert kept, "k_sample_gusts wrote behind the end of its output"
    return out


def dev_states(hip, s, seed, x_nom, S, sigma=SIGMA12, b0=0, s0=0, flags=0):
    lib = capi.load()
    b = len(x_nom)
    d_nom, d = hip.upload(x_nom), guarded(hip, (b, S, 13))
    sig = np.ascontiguousarray(sigma, dtype=np.float64)
    assert lib.qilqr_sample_states_device(s._h, d_nom, sig.ctypes.data, seed, b, S, b0, s0, flags, d) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    out, kept = fetch(hip, d, (b, S, 13))
    assert kept, "k_sample_states wrote behind the end of its output"
    return out


def dev_reduce(hip, s, score):
    lib = capi.load()
    b, S = score.shape[:2]
    d_score, d = hip.upload(score), guarded(hip, (b, 8))
    assert lib.qilqr_reduce_scores_device(s._h, d_score, b, S, d) == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    out, kept = fetch(hip, d, (b, 8))
    assert kept, "k_reduce_scores wrote behind the end of its output"
    return out


# ------------------------------------------------------------------------------------------------ 1. against the restatement

@pytest.mark.parametrize("n_w", [1, N])
@pytest.mark.parametrize("taus", [(0.0, 0.0), (0.4, 0.15)])
def test_device_gusts_against_the_restatement(hip, handle, taus, n_w):
    cfg, s, _ = handle
    got = dev_gusts(hip, s, SEED, B, 70, n_w, tau_f=taus[0], tau_t=taus[1], b0=2, s0=65530)  # (samples past 65 535)
    want = mn.gusts(SEED, B, 70, n_w, cfg["dt"], SIGMA6, MEAN6, taus[0], taus[1], b0=2, s0=65530)
    over = (np.abs(got - want) / (1e-12 * np.maximum(np.maximum(SIGMA6, np.abs(MEAN6)), 1.0))).max()
    print("[observed] device gusts %s, n_w = %d: error over its bound %.3g" % (taus, n_w, over))
    assert np.isfinite(got).all() and over <= 1.0
    if n_w > 1 and taus[0] > 0:  # the correlation is there: successive force rows are closer than independent ones would be
        f = got[..., 0] - MEAN6[0]
        assert (f[..., 1:] * f[..., :-1]).mean() > 0.5 * (f * f).mean()


def test_device_states_against_the_restatement(hip, handle):
    _, s, x_nom = handle
    got = dev_states(hip, s, SEED, x_nom, 70, b0=1, s0=4)
    want = mn.states(SEED, x_nom, 70, SIGMA12, b0=1, s0=4)
    pose, vel = np.abs(got[..., :7] - want[..., :7]).max(), (np.abs(got[..., 7:] - want[..., 7:]) / np.maximum(SIGMA12[6:], 1.0)).max()
    print("[observed] device states: pose error %.3g, velocity error %.3g (bounds 1e-12)" % (pose, vel))
    assert pose <= 1e-12 and vel <= 1e-12
    assert np.abs(np.linalg.norm(got[..., 3:7], axis=-1) - 1.0).max() <= 1e-12
    still = dev_states(hip, s, SEED, x_nom, 5, sigma=np.zeros(12))
    assert np.abs(still - x_nom[:, None]).max() <= 1e-14
    flagged, plain = dev_states(hip, s, SEED, x_nom, 70, flags=1), dev_states(hip, s, SEED, x_nom, 70)
    assert flagged[:, 0].tobytes() == x_nom.tobytes() and flagged[:, 1:].tobytes() == plain[:, 1:].tobytes() and not np.array_equal(plain[:, 0], x_nom)


# ------------------------------------------------------------------------------------------------ 2. the geometry plays no part, 3. containment

def test_a_rows_bits_do_not_depend_on_the_batch(hip, handle):
    """the same (b, s) at S = 1, 5, 64, 70 and 126 (one block and several, full and part blocks), and sub-blocks at (b0, s0); every
    output is followed by guard words, which keep their bits (dev_gusts, dev_states)"""
    _, s, x_nom = handle
    kw = dict(tau_f=0.4, tau_t=0.15)
    whole_g = dev_gusts(hip, s, SEED, B, 130, N, **kw)
    whole_x = dev_states(hip, s, SEED, x_nom, 130)
    for S in SIZES[:-1]:
        assert dev_gusts(hip, s, SEED, B, S, N, **kw).tobytes() == np.ascontiguousarray(whole_g[:, :S]).tobytes(), S
        assert dev_states(hip, s, SEED, x_nom, S).tobytes() == np.ascontiguousarray(whole_x[:, :S]).tobytes(), S
    assert dev_gusts(hip, s, SEED, B, 126, 1, **kw).tobytes() == np.ascontiguousarray(whole_g[:, :126, :1]).tobytes()
    assert dev_gusts(hip, s, SEED, 2, 67, N, b0=1, s0=60, **kw).tobytes() == np.ascontiguousarray(whole_g[1:, 60:127]).tobytes()
    assert dev_states(hip, s, SEED, x_nom[1:], 67, b0=1, s0=60).tobytes() == np.ascontiguousarray(whole_x[1:, 60:127]).tobytes()
    assert dev_states(hip, s, SEED, x_nom[1:], 67, b0=1, s0=60, flags=1).tobytes() == np.ascontiguousarray(whole_x[1:, 60:127]).tobytes()
    # plans and samples differ, and so do seeds
    assert not np.array_equal(whole_g[0], whole_g[1]) and not np.array_equal(whole_g[:, 0], whole_g[:, 1])
    assert not np.array_equal(dev_gusts(hip, s, SEED + (1 << 32), B, 5, N, **kw), whole_g[:, :5])
    # an odd number of rows: the last chunk of k_sample_gusts is a short one
    odd = dev_gusts(hip, s, SEED, B, 70, 11, **kw)
    assert odd.tobytes() == np.ascontiguousarray(whole_g[:, :70, :11]).tobytes()


def test_any_precision_mode_samples_the_same_bits(hip, handle):
    cfg, s, x_nom = handle
    f32 = capi.from_config(cfg, precision="f32")
    assert dev_gusts(hip, f32, SEED, B, 5, N, tau_f=0.3).tobytes() == dev_gusts(hip, s, SEED, B, 5, N, tau_f=0.3).tobytes()
    assert dev_states(hip, f32, SEED, x_nom, 5).tobytes() == dev_states(hip, s, SEED, x_nom, 5).tobytes()


# ------------------------------------------------------------------------------------------------ 4. the reduction

@pytest.mark.parametrize("S", SIZES)
def test_device_reduction_against_numpy(hip, handle, S):
    _, s, _ = handle
    score = mn.special_scores(B, S, 40 + S)
    assert mn.extremes_are_unique(score)
    got, want = dev_reduce(hip, s, score), mn.summary(score)
    mn.assert_summary(got, want, "S = %d" % S)
    ok = ~np.isnan(want[:, 0])
    print("[observed] device reduction, S = %d: mean error %.3g relative, deviation error %.3g relative" % (
        S, (np.abs(got[ok, 0] - want[ok, 0]) / want[ok, 0]).max(), (np.abs(got[ok, 1] - want[ok, 1]) / np.maximum(want[ok, 1], 1e-300)).max()))
    assert np.isposinf(got[2, 5]) and got[2, 6] == -1 and got[1, 7] > 0
    for b in range(B):  # the plan alone (B = 1) has the bits it has among three
        assert dev_reduce(hip, s, score[b:b + 1]).tobytes() == got[b:b + 1].tobytes(), b


def test_device_reduction_of_ties_and_of_nothing(hip, handle):
    _, s, _ = handle
    score = mn.special_scores(2, 130, 9)
    score[0, [3, 67, 129], 0] = 1e4
    score[0, [70, 6], 1] = -5.0
    score[1, :, 0] = np.nan
    score[1, :, 1] = np.inf
    got = dev_reduce(hip, s, score)
    assert got[0, 2] == 1e4 and got[0, 3] == 3 and got[0, 5] == -5.0 and got[0, 6] == 6
    assert np.isnan(got[1, :3]).all() and got[1, 3] == -1 and np.isposinf(got[1, 5]) and got[1, 6] == -1 and got[1, 7] == 1.0


# ------------------------------------------------------------------------------------------------ 5. ordering

@pytest.mark.parametrize("S", [5, 70])
def test_four_enqueues_in_a_row_and_one_synchronise(hip, S):
    """sample states, sample gusts, the scored flight and the reduction, enqueued without a wait between them, twice on the same
    buffers with two seeds: each round against the same calls made one by one"""
    cfg, plan = cn.plans(B, N, 5)
    s = capi.from_config(cfg)
    gains, _ = s.backwards_pass(plan)
    x_nom = np.ascontiguousarray(cn.sample_states(plan, 1, 0, 6)[:, 0])
    lib = capi.load()
    m = capi.gust_model(SIGMA6, MEAN6, 0.4, 0.15)
    d_plan, d_gains, d_nom = hip.upload(plan), hip.upload(gains), hip.upload(x_nom)
    d_x0, d_w, d_score, d_sum = hip.alloc(8 * B * S * 13), hip.alloc(8 * B * S * N * 6), hip.alloc(8 * B * S * 4), hip.alloc(8 * B * 8)
    sig = np.ascontiguousarray(SIGMA12)
    for seed in (SEED, SEED + 7):
        assert lib.qilqr_sample_states_device(s._h, d_nom, sig.ctypes.data, seed, B, S, 0, 0, 1, d_x0) == 0, lib.qilqr_last_error()
        assert lib.qilqr_sample_gusts_device(s._h, C.byref(m), seed, B, S, N, 0, 0, d_w) == 0, lib.qilqr_last_error()
        assert lib.qilqr_closed_loop_scored_device(s._h, d_plan, d_gains, d_x0, d_w, N, None, B, N, S, 0, N - 1, None, None, d_score) == 0, lib.qilqr_last_error()
        assert lib.qilqr_reduce_scores_device(s._h, d_score, B, S, d_sum) == 0, lib.qilqr_last_error()
        hip.synchronize(lib.qilqr_stream(s._h))
        x0, w = dev_states(hip, s, seed, x_nom, S, flags=1), dev_gusts(hip, s, seed, B, S, N, tau_f=0.4, tau_t=0.15)
        assert hip.download(d_x0, x0.shape).tobytes() == x0.tobytes() and hip.download(d_w, w.shape).tobytes() == w.tobytes()
        score = s.closed_loop(plan, gains, x0, traj=False, stats=False, wrench=w, score=True)["score"]
        assert hip.download(d_score, score.shape).tobytes() == score.tobytes() and np.isfinite(score[..., 0]).all()
        assert hip.download(d_sum, (B, 8)).tobytes() == dev_reduce(hip, s, score).tobytes()


# ------------------------------------------------------------------------------------------------ 6. what the calls refuse on a handle

def test_what_the_calls_refuse_on_a_handle(hip, handle):
    """with a handle every refusal of the arguments still comes first and leaves the output untouched; the handle itself is refused
    for nothing (tests/test_monte_carlo_cpu.py goes through every reason without one)"""
    _, s, x_nom = handle
    lib = capi.load()
    m, sig = capi.gust_model(1.0), np.ascontiguousarray(SIGMA12)
    d_w, d_nom, d_x0, d_score, d_sum = hip.alloc(8 * B * 5 * N * 6), hip.upload(x_nom), hip.alloc(8 * B * 5 * 13), hip.alloc(8 * B * 5 * 4), hip.alloc(8 * B * 8)
    bad = capi.gust_model([1, 1, np.nan, 1, 1, 1])
    refused = [(lambda: lib.qilqr_sample_gusts_device(s._h, C.byref(bad), 1, B, 5, N, 0, 0, d_w), "sigma must be finite"),
               (lambda: lib.qilqr_sample_gusts_device(s._h, C.byref(m), 1, B, 5, 0, 0, 0, d_w), "n_w must be positive"),
               (lambda: lib.qilqr_sample_gusts_device(s._h, C.byref(m), 1, B, 5, N, -1, 0, d_w), "must not be negative"),
               (lambda: lib.qilqr_sample_gusts_device(s._h, C.byref(m), 1, B, 5, N, 0, 0, d_w + 8), "16-byte aligned"),
               (lambda: lib.qilqr_sample_states_device(s._h, d_nom, sig.ctypes.data, 1, B, 5, 0, 0, 2, d_x0), "unknown flag bits"),
               (lambda: lib.qilqr_sample_states_device(s._h, d_x0 + 16, sig.ctypes.data, 1, B, 5, 0, 0, 0, d_x0), "d_x0 overlaps d_x_nom"),
               (lambda: lib.qilqr_sample_states_device(s._h, d_nom, None, 1, B, 5, 0, 0, 0, d_x0), "null argument"),
               (lambda: lib.qilqr_reduce_scores_device(s._h, d_score, B, 5, d_score + 32), "d_summary overlaps d_score"),
               (lambda: lib.qilqr_reduce_scores_device(s._h, d_score, B, 0, d_sum), "must be positive")]
    for call, why in refused:
        assert call() == capi.ERR_INVALID_ARG and why in lib.qilqr_last_error().decode(), why
    hip.synchronize(lib.qilqr_stream(s._h))
    for ptr, words in ((d_w, B * 5 * N * 6), (d_x0, B * 5 * 13), (d_sum, B * 8)):
        assert (hip.download(ptr, (8 * words,), dtype=np.uint8) == 0xFF).all()


# ------------------------------------------------------------------------------------------------ 7. RecedingHorizon.evaluate_sampled

@pytest.fixture(scope="module")
def torch_forms(tmp_path_factory):
    """tests/monte_carlo_torch_child.py, once (PyTorch's ROCm runtime has to be the first a process initialises).  The arrays it recorded."""
    out = str(tmp_path_factory.mktemp("monte_carlo_torch") / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.monte_carlo_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["euler_", "rk4_limits_"])
def test_evaluate_sampled_against_evaluate_fed_what_it_sampled(torch_forms, tag):
    # (the child's constants, restated: importing it would initialise torch in this process)
    r = torch_forms
    S, seed0 = 70, 33
    sigma12 = SIGMA12
    gust = dict(sigma=np.array([1.0, 0.8, 0.6, 0.03, 0.02, 0.04]), mean=np.array([0.3, -0.2, 0.1, 0.0, 0.01, 0.0]))
    x = r[tag + "x"]
    for call, (seed, n_w) in enumerate(((seed0 + 10, N), (seed0 + 11, N), (seed0 + 12, 1))):
        c = "%scall%d_" % (tag, call)
        x0, w, score = r[c + "x0"], r[c + "wrench"], r[c + "score"]
        assert x0.shape == (B, S, 13) and w.shape == (B, S, n_w, 6) and score.shape == (B, S, 4) and r[c + "summary"].shape == (B, 8)
        # what was flown: evaluate() fed the downloaded samples gives the same bits
        assert r[c + "stats"].tobytes() == r[c + "host_stats"].tobytes() and score.tobytes() == r[c + "host_score"].tobytes()
        # what was sampled: the restatement's states and gusts, sample 0 the measured state itself
        want_x0 = mn.states(seed, x, S, sigma12, first_is_nominal=True)
        assert x0[:, 0].tobytes() == x.tobytes() and np.abs(x0 - want_x0).max() <= 1e-12
        want_w = mn.gusts(seed, B, S, n_w, float(r["dt"]), gust["sigma"], gust["mean"], 0.4, 0.1)
        assert (np.abs(w - want_w) / (1e-12 * np.maximum(np.maximum(gust["sigma"], np.abs(gust["mean"])), 1.0))).max() <= 1.0
        # what was reduced: NumPy's summary of that score
        assert mn.extremes_are_unique(score) and np.isfinite(score[..., 0]).all() and np.isfinite(score[..., 1]).all()
        mn.assert_summary(r[c + "summary"], mn.summary(score), c)
    assert r[tag + "call0_score"].tobytes() != r[tag + "call1_score"].tobytes()  # (another seed, other flights)
    if tag == "rk4_limits_":
        assert (r[tag + "call0_stats"][..., 3] > 0).any()  # the limits were felt
    # without a gust, sample 0 under the nominal flag is closed_loop_device from the measured state
    assert bool(r[tag + "calm_wrench_is_none"]) and r[tag + "calm_x0"][:, 0].tobytes() == x.tobytes()
    assert r[tag + "calm_stats"][:, :1].tobytes() == r[tag + "nominal_stats"].tobytes() and r[tag + "calm_score"][:, :1].tobytes() == r[tag + "nominal_score"].tobytes()
    mn.assert_summary(r[tag + "calm_summary"], mn.summary(r[tag + "calm_score"]), tag + "calm")
    assert r[tag + "unflagged_x0"][:, 1:].tobytes() == r[tag + "calm_x0"][:, 1:].tobytes() and not np.array_equal(r[tag + "unflagged_x0"][:, 0], x)
    assert r[tag + "unflagged_score"][:, 1:].tobytes() == r[tag + "calm_score"][:, 1:].tobytes()


def test_the_torch_forms_check_their_tensors(torch_forms):
    said = {k[len("refusal_"):]: str(v) for k, v in torch_forms.items() if k.startswith("refusal_")}
    assert said["fine"] == "accepted", said["fine"]
    for k, kind, text in (("without_gains", "RuntimeError", "gains=True"), ("gusts_shape", "TypeError", "out must have shape"),
                          ("gusts_float32", "TypeError", "float64"), ("gusts_host", "TypeError", "CUDA tensor"), ("gusts_sigma", "TypeError", "1, 2 or 6 words"),
                          ("gusts_negative", "TypeError", "sigma must be finite"), ("states_shape", "TypeError", "x_nom must have shape"),
                          ("states_sigma", "TypeError", "1 or 12 words"), ("reduce_shape", "TypeError", "out must have shape"),
                          ("sampled_n_w", "TypeError", "n_w must be 1 or"), ("sampled_x", "TypeError", "expected shape")):
        assert said[k].startswith(kind) and text in said[k], (k, said[k])
