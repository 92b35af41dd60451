"""The Monte-Carlo kernels without a device: philox.h, the per-lane routines of monte_carlo_kernels.h and the rules of
monte_carlo_launch.h (compiled with g++ into the stand-alone program tests/host_monte_carlo_harness.cpp) against the generator's published
vectors, against the restatement in NumPy (tests/monte_carlo_numpy.py), against the statistics the draws must have, and against
themselves (a sub-block is a slice, n_w = 1 is row 0, the nominal flag touches sample 0 only); what the three calls refuse, through
the rules and through the C ABI.  B = 3, n = 24."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as orc
from quadrotorilqr_amd import capi, problems as pb
from tests import closed_loop_numpy as cn, monte_carlo_numpy as mn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B, N, SEED = 3, 24, (0x5eed << 32) | 1234  # (a seed with a high word)
DT = pb.DT_DEMO
NEW_SYMBOLS = ("qilqr_sample_gusts_device", "qilqr_sample_states_device", "qilqr_reduce_scores_device")
KNOWN = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
MEAN6 = np.array([0.4, -0.2, 0.1, 0.01, -0.02, 0.03])
SIGMA6 = np.array([1.5, 1.2, 0.8, 0.05, 0.04, 0.06])
SIGMA12 = np.array([0.05, 0.04, 0.06, 0.03, 0.02, 0.04, 0.1, 0.12, 0.08, 0.05, 0.06, 0.04])


def build_harness(flags, name):
    d = tempfile.mkdtemp(prefix="host_monte_carlo_harness_")
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(HERE, "host_monte_carlo_harness.cpp"), "-lm"])
    return exe


@pytest.fixture(scope="module")
def harness():
    return build_harness(["-O2"], "host_monte_carlo_harness")


def through_files(exe, command, words):
    d = tempfile.mkdtemp(prefix="monte_carlo_case_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    np.asarray(words, dtype=np.float64).tofile(fin)
    subprocess.check_call([exe, command, fin, fout])
    return np.fromfile(fout)


def seed_words(seed):
    return [seed & 0xffffffff, seed >> 32]


def host_draws(exe, seed, index):
    """index (N, 5) of (plan, sample, row, stream, pair) -> words (N, 4) uint64, normals (N, 2)"""
    index = np.asarray(index, dtype=np.float64).reshape(-1, 5)
    out = through_files(exe, "draws", np.concatenate([seed_words(seed) + [len(index)], index.ravel()])).reshape(-1, 6)
    return out[:, :4].astype(np.uint64), out[:, 4:]


def host_gusts(exe, seed, b, s, n_w, sigma=SIGMA6, mean=MEAN6, tau_f=0.0, tau_t=0.0, b0=0, s0=0, dt=DT):
    head = [b, s, n_w, b0, s0] + seed_words(seed) + [dt, tau_f, tau_t]
    return through_files(exe, "gusts", np.concatenate([head, mean, sigma])).reshape(b, s, n_w, 6)


def host_states(exe, seed, x_nom, s, sigma=SIGMA12, b0=0, s0=0, flags=0):
    b = len(x_nom)
    head = [b, s, b0, s0] + seed_words(seed) + [flags, 0]
    return through_files(exe, "states", np.concatenate([head, sigma, np.asarray(x_nom).ravel()])).reshape(b, s, 13)


def host_reduce(exe, score):
    b, s = score.shape[:2]
    return through_files(exe, "reduce", np.concatenate([[b, s], score.ravel()])).reshape(b, 8)


@pytest.fixture(scope="module")
def x_nom():
    """the measured states of B plans: knot 0 of closed_loop_numpy's plans, moved off the plan"""
    _, plan = cn.plans(B, N, 5)
    x = np.ascontiguousarray(cn.sample_states(plan, 1, 0, 6)[:, 0])
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ 1. the generator

@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_known_answers_of_philox(harness, counter, key, want):
    c, k = [int(w, 16) for w in counter.split()], [int(w, 16) for w in key.split()]
    assert " ".join("%08x" % int(w) for w in mn.philox(np.array(c), np.array(k))) == want
    assert subprocess.check_output([harness, "philox"] + counter.split() + key.split()).decode().strip() == want


def draw_index():
    """draws over every index, with plans and samples above 65 535 (b0 + b, s0 + s), both streams, rows and pairs"""
    r = np.random.default_rng(3)
    n = 4000
    return np.stack([r.integers(0, 200000, n), r.integers(0, 300000, n), r.integers(0, 500, n), r.integers(0, 2, n), r.integers(0, 6, n)], axis=1)


def test_raw_words_are_the_restatements(harness):
    idx = draw_index()
    assert (idx[:, 0] > 65535).any() and (idx[:, 1] > 65535).any() and SEED >> 32
    got, _ = host_draws(harness, SEED, idx)
    assert np.array_equal(got, mn.words(SEED, idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], idx[:, 4]))
    # one by hand, through the command line: counter {row, sample, plan, stream << 16 | pair}, key {seed lo, seed hi}
    by_hand = mn.philox(np.array([5, 70000, 80000, (1 << 16) | 3]), np.array([SEED & 0xffffffff, SEED >> 32]))
    text = subprocess.check_output([harness, "words", str(SEED), "80000", "70000", "5", "1", "3"]).decode().split()
    assert [int(w, 16) for w in text] == [int(w) for w in by_hand]
    # every index and both halves of the seed are felt
    base = mn.words(SEED, 7, 8, 9, 0, 1)
    for other in (mn.words(SEED + 1, 7, 8, 9, 0, 1), mn.words(SEED + (1 << 32), 7, 8, 9, 0, 1), mn.words(SEED, 6, 8, 9, 0, 1), mn.words(SEED, 7, 9, 9, 0, 1),
                  mn.words(SEED, 7, 8, 10, 0, 1), mn.words(SEED, 7, 8, 9, 1, 1), mn.words(SEED, 7, 8, 9, 0, 2)):
        assert not np.array_equal(base, other)


def test_normals_against_the_restatement(harness):
    idx = draw_index()
    _, got = host_draws(harness, SEED, idx)
    z0, z1 = mn.draws(SEED, idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], idx[:, 4])
    err = max(np.abs(got[:, 0] - z0).max(), np.abs(got[:, 1] - z1).max())
    print("[observed] normals, harness against NumPy: max error %.3g (bound %.0e)" % (err, mn.NORMAL_ATOL))
    assert err <= mn.NORMAL_ATOL


def test_normals_at_the_ends_of_the_words(harness):
    run = lambda w: [float.fromhex(v) for v in subprocess.check_output([harness, "normals"] + [w] * 4).decode().split()]
    z0, z1 = run("0")
    assert abs(z0 - np.sqrt(106.0 * np.log(2.0))) < 1e-14 and abs(z0 - 8.5716743) < 1e-7 and z1 == 0.0
    assert run("ffffffff") == [0.0, 0.0]  # (a zero of either sign)
    z = mn.normals(np.zeros(4, dtype=np.uint64))
    assert abs(z[0] - z0) < 1e-14 and z[1] == 0.0
    z = mn.normals(np.full(4, 0xffffffff, dtype=np.uint64))
    assert z[0] == 0.0 and z[1] == 0.0


def moment_normals(sample0):
    """key (1234, 0), counters i < 200, s < 64, b < 4, word 3 = 0: z0 and z1 of each, (4, 64, 200, 2)"""
    b, s, i = np.meshgrid(np.arange(4), np.arange(64) + sample0, np.arange(200), indexing="ij")
    return np.stack(mn.draws(1234, b, s, i, 0, 0), axis=-1)


def test_the_first_two_moments():
    z = moment_normals(0)
    n = z.size
    assert n == 102400
    print("[observed] mean %.5f (bound %.4f), std %.5f (bound %.4f)" % (z.mean(), 4 / np.sqrt(n), z.std(), 4 / np.sqrt(2 * n)))
    assert abs(z.mean()) < 4.0 / np.sqrt(n) and abs(z.std() - 1.0) < 4.0 / np.sqrt(2.0 * n)


def test_the_lag_one_autocorrelation_of_a_correlated_gust():
    """rho = 0.8 on component 0 (z0 of pair 0) of samples 64 .. 127: the recursion's lag-1 autocorrelation within 4 standard errors of rho"""
    rho = 0.8
    xi = moment_normals(64)[..., 0]  # (4, 64, 200)
    g = np.empty_like(xi)
    g[..., 0] = xi[..., 0]
    for i in range(1, 200):
        g[..., i] = rho * g[..., i - 1] + np.sqrt((1 - rho) * (1 + rho)) * xi[..., i]
    r1 = (g[..., 1:] * g[..., :-1]).mean() / (g * g).mean()
    bound = 4.0 * np.sqrt((1.0 - rho * rho) / 51200.0)
    print("[observed] lag-1 autocorrelation %.5f (rho %.1f, bound %.4f)" % (r1, rho, bound))
    assert abs(r1 - rho) < bound


# ------------------------------------------------------------------------------------------------ 2. gusts

def gust_bound(sigma, mean):
    return 1e-12 * np.maximum(np.maximum(sigma, np.abs(mean)), 1.0)


@pytest.mark.parametrize("taus", [(0.0, 0.0), (0.5, 0.0), (0.3, 0.15)])
def test_gusts_against_the_restatement(harness, taus):
    S = 7
    got = host_gusts(harness, SEED, B, S, N, tau_f=taus[0], tau_t=taus[1], b0=2, s0=3)
    want = mn.gusts(SEED, B, S, N, DT, SIGMA6, MEAN6, taus[0], taus[1], b0=2, s0=3)
    over = (np.abs(got - want) / gust_bound(SIGMA6, MEAN6)).max()
    print("[observed] gusts %s: error over its bound %.3g" % (taus, over))
    assert over <= 1.0
    # the statistics of the process: deviation sigma about the mean at every knot (3 * 7 flights only: within 5 standard errors)
    wide = host_gusts(harness, SEED, 8, 64, N, tau_f=taus[0], tau_t=taus[1])
    assert (np.abs(wide.mean(axis=(0, 1, 2)) - MEAN6) < 5 * SIGMA6 / np.sqrt(512.0)).all()  # (correlated rows: counted as one per flight)
    assert (np.abs(wide.std(axis=(0, 1)) / SIGMA6 - 1.0) < 5 / np.sqrt(2 * 512.0)).all()


def test_white_gusts_are_the_mean_plus_sigma_xi(harness):
    S = 5
    got = host_gusts(harness, SEED, B, S, N)
    b, s, i, j = (v.ravel() for v in np.meshgrid(np.arange(B), np.arange(S), np.arange(N), np.arange(3), indexing="ij"))
    _, z = host_draws(harness, SEED, np.stack([b, s, i, np.zeros_like(b), j], axis=1))
    xi = z.reshape(B, S, N, 6)
    assert (MEAN6 + SIGMA6 * xi).tobytes() == got.tobytes()


def test_gusts_one_row_a_sub_block_and_sigma_zero(harness):
    S = 6
    kw = dict(tau_f=0.4, tau_t=0.2)
    whole = host_gusts(harness, SEED, B, S, N, **kw)
    assert host_gusts(harness, SEED, B, S, 1, **kw).tobytes() == np.ascontiguousarray(whole[:, :, :1]).tobytes()
    part = host_gusts(harness, SEED, 2, 3, N, b0=1, s0=2, **kw)
    assert part.tobytes() == np.ascontiguousarray(whole[1:3, 2:5]).tobytes()
    assert not np.array_equal(whole[0, 0], whole[0, 1]) and not np.array_equal(whole[0, 0], whole[1, 0])
    assert not np.array_equal(whole, host_gusts(harness, SEED + 1, B, S, N, **kw))
    still = host_gusts(harness, SEED, B, S, N, sigma=np.zeros(6), **kw)
    assert np.array_equal(still, np.broadcast_to(MEAN6, still.shape))


# ------------------------------------------------------------------------------------------------ 3. start states

def test_states_against_the_restatement(harness, x_nom):
    S = 9
    got = host_states(harness, SEED, x_nom, S, b0=1, s0=4)
    want = mn.states(SEED, x_nom, S, SIGMA12, b0=1, s0=4)
    pose, vel = np.abs(got[..., :7] - want[..., :7]).max(), (np.abs(got[..., 7:] - want[..., 7:]) / np.maximum(SIGMA12[6:], 1.0)).max()
    print("[observed] states: pose error %.3g, velocity error %.3g (bounds 1e-12)" % (pose, vel))
    assert pose <= 1e-12 and vel <= 1e-12
    assert np.abs(np.linalg.norm(got[..., 3:7], axis=-1) - 1.0).max() <= 1e-12
    # the samples are about the nominal state with the deviations asked for: the tangent from x_nom to each, against sigma
    wide = host_states(harness, SEED, x_nom, 400)
    tangent = np.array([[orc.state_minus(wide[b, s], x_nom[b]) for s in range(400)] for b in range(B)])
    assert (np.abs(tangent.std(axis=(0, 1)) / SIGMA12 - 1.0) < 5 / np.sqrt(2 * 1200.0)).all()


def test_states_sigma_zero_a_sub_block_and_the_nominal_flag(harness, x_nom):
    S = 6
    still = host_states(harness, SEED, x_nom, S, sigma=np.zeros(12))
    assert np.abs(still - x_nom[:, None]).max() <= 1e-14
    whole = host_states(harness, SEED, x_nom, S)
    assert host_states(harness, SEED, x_nom[1:], 3, b0=1, s0=2).tobytes() == np.ascontiguousarray(whole[1:, 2:5]).tobytes()
    flagged = host_states(harness, SEED, x_nom, S, flags=1)
    assert flagged[:, 0].tobytes() == x_nom.tobytes() and flagged[:, 1:].tobytes() == whole[:, 1:].tobytes()
    assert not np.array_equal(whole[:, 0], x_nom)
    # the flag names sample s0 + s == 0: a block that starts elsewhere has none
    assert host_states(harness, SEED, x_nom, 3, s0=2, flags=1).tobytes() == np.ascontiguousarray(whole[:, 2:5]).tobytes()


# ------------------------------------------------------------------------------------------------ 4. the reduction

@pytest.mark.parametrize("S", [1, 5, 64, 70, 130])
def test_the_reduction_against_numpy(harness, S):
    score = mn.special_scores(B, S, 40 + S)
    assert mn.extremes_are_unique(score)
    got, want = host_reduce(harness, score), mn.summary(score)
    mn.assert_summary(got, want, "S = %d" % S)
    ok = ~np.isnan(want[:, 0])
    print("[observed] S = %d: mean error %.3g relative, deviation error %.3g relative" % (
        S, (np.abs(got[ok, 0] - want[ok, 0]) / want[ok, 0]).max(), (np.abs(got[ok, 1] - want[ok, 1]) / np.maximum(want[ok, 1], 1e-300)).max()))
    assert np.isposinf(got[2, 5]) and got[2, 6] == -1 and got[2, 4] == 0  # no spheres
    assert got[1, 7] > 0 and got[0, 7] == 0                               # the NaN cost is counted, and only there
    # a plan's bits depend on its own rows only
    assert host_reduce(harness, score[1:2]).tobytes() == got[1:2].tobytes()


def test_the_reduction_of_ties_and_of_nothing(harness):
    score = mn.special_scores(2, 130, 9)
    score[0, [3, 67, 129], 0] = 1e4   # the largest cost three times, in three lanes' shares and two rounds
    score[0, [70, 6], 1] = -5.0       # the smallest clearance twice
    score[1, :, 0] = np.nan           # no finite cost
    score[1, :, 1] = np.inf           # nothing seen
    got = host_reduce(harness, score)
    assert got[0, 2] == 1e4 and got[0, 3] == 3 and got[0, 5] == -5.0 and got[0, 6] == 6
    assert np.isnan(got[1, :3]).all() and got[1, 3] == -1 and np.isposinf(got[1, 5]) and got[1, 6] == -1 and got[1, 7] == 1.0
    mn.assert_summary(got, mn.summary(score), "ties")


# ------------------------------------------------------------------------------------------------ 5. what the calls refuse
NAN, INF = "nan", "inf"
OK_GUSTS = dict(handle=1, model=1, wrench=4096, B=2, S=3, n_w=4, b0=0, s0=0, tau_f=0.5, tau_t=0, mean=[0] * 6, sigma=[1] * 6)
GUSTS_REFUSED = [(dict(model=0), "null argument"), (dict(wrench=0), "null argument"), (dict(B=0), "must be positive"), (dict(S=-1), "must be positive"),
                 (dict(n_w=0), "n_w must be positive"), (dict(b0=-1), "must not be negative"), (dict(s0=-2), "must not be negative"),
                 (dict(wrench=4096 + 8), "16-byte aligned"), (dict(sigma=[1, 1, -0.5, 1, 1, 1]), "sigma must be finite and not negative"),
                 (dict(sigma=[1, NAN, 1, 1, 1, 1]), "sigma must be finite"), (dict(sigma=[1, 1, 1, 1, 1, INF]), "sigma must be finite"),
                 (dict(mean=[0, 0, 0, NAN, 0, 0]), "mean must be finite"), (dict(mean=[INF, 0, 0, 0, 0, 0]), "mean must be finite"),
                 (dict(tau_f=-1), "correlation times"), (dict(tau_t=NAN), "correlation times"), (dict(tau_f=INF), "correlation times"),
                 (dict(handle=0), "null handle")]
GUSTS_ADMITTED = [dict(), dict(n_w=1), dict(b0=70000, s0=1 << 20), dict(sigma=[0] * 6), dict(tau_f=0, tau_t=0)]
OK_STATES = dict(handle=1, sigma_given=1, x_nom=4096, x0=65536, B=2, S=3, b0=0, s0=0, flags=0, sigma=[0.1] * 12)
STATES_REFUSED = [(dict(x_nom=0), "null argument"), (dict(sigma_given=0), "null argument"), (dict(x0=0), "null argument"), (dict(B=0), "must be positive"),
                  (dict(S=0), "must be positive"), (dict(b0=-1), "must not be negative"), (dict(s0=-1), "must not be negative"),
                  (dict(x_nom=4096 + 8), "16-byte aligned"), (dict(x0=65536 + 8), "16-byte aligned"), (dict(sigma=[0.1] * 11 + [-1]), "sigma must be finite"),
                  (dict(sigma=[NAN] + [0.1] * 11), "sigma must be finite"), (dict(flags=2), "unknown flag bits"), (dict(flags=0x80000001), "unknown flag bits"),
                  (dict(x0=4096 + 16), "d_x0 overlaps d_x_nom"), (dict(x_nom=65536 + 8 * 13 * 6 - 16), "d_x0 overlaps d_x_nom"), (dict(handle=0), "null handle")]
STATES_ADMITTED = [dict(), dict(flags=1), dict(sigma=[0] * 12), dict(x_nom=65536 + 8 * 13 * 6)]  # (x_nom may start where x0 ends: 2 * 3 * 13 words)
OK_REDUCE = dict(handle=1, score=4096, summary=65536, B=2, S=3)
REDUCE_REFUSED = [(dict(score=0), "null argument"), (dict(summary=0), "null argument"), (dict(B=0), "must be positive"), (dict(S=0), "must be positive"),
                  (dict(score=4096 + 8), "16-byte aligned"), (dict(summary=65536 + 8), "16-byte aligned"), (dict(summary=4096 + 16), "d_summary overlaps d_score"),
                  (dict(score=65536 + 16), "d_summary overlaps d_score"), (dict(handle=0), "null handle")]
REDUCE_ADMITTED = [dict(), dict(summary=4096 + 8 * 4 * 6), dict(S=1)]


def rule(exe, which, ok, **change):
    call = dict(ok, **change)
    flat = []
    for v in call.values():
        flat += [str(x) for x in v] if isinstance(v, list) else [str(v)]
    return subprocess.check_output([exe, "refuse", which] + flat).decode().strip()


@pytest.mark.parametrize("which,ok,refused,admitted", [("gusts", OK_GUSTS, GUSTS_REFUSED, GUSTS_ADMITTED), ("states", OK_STATES, STATES_REFUSED, STATES_ADMITTED),
                                                       ("reduce", OK_REDUCE, REDUCE_REFUSED, REDUCE_ADMITTED)])
def test_the_rules_of_what_the_calls_refuse(harness, which, ok, refused, admitted):
    for change, why in refused:
        assert re.search(why, rule(harness, which, ok, **change)), (change, rule(harness, which, ok, **change))
    for change in admitted:
        assert rule(harness, which, ok, **change) == "ok", (change, rule(harness, which, ok, **change))
    assert "null handle" not in rule(harness, which, ok, handle=0, B=0)  # the arguments come before the handle


def test_the_abi_without_a_device():
    """every refusal that needs no handle, through ctypes: the arguments are looked at before the handle, so a NULL handle is the last"""
    import ctypes as C
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header) and name in capi.EXPORTS and hasattr(lib, name), name
    assert "#define QILQR_MC_SUMMARY 8" in header and capi.MC_SUMMARY == 8 and C.sizeof(capi.GustModel) == 14 * 8
    assert lib.qilqr_abi_version() == 7
    buf = capi._d16(np.zeros(4096))
    at = lambda words: buf.ctypes.data + 8 * words
    last = lambda: lib.qilqr_last_error().decode()

    def gusts(model=True, B=2, S=3, n_w=4, b0=0, s0=0, wrench=at(0), **m):
        gm = capi.gust_model(m.get("sigma", 1.0), m.get("mean"), m.get("tau_f", 0.0), m.get("tau_t", 0.0))
        return lib.qilqr_sample_gusts_device(None, C.byref(gm) if model else None, SEED, B, S, n_w, b0, s0, wrench), last()

    for change, why in [(dict(model=False), "null argument"), (dict(wrench=None), "null argument"), (dict(B=0), "must be positive"), (dict(n_w=-3), "n_w must be positive"),
                        (dict(s0=-1), "must not be negative"), (dict(wrench=at(1)), "16-byte aligned"), (dict(sigma=[1, 1, 1, 1, -1, 1]), "sigma must be finite"),
                        (dict(mean=[0, np.inf, 0, 0, 0, 0]), "mean must be finite"), (dict(tau_t=np.nan), "correlation times"), (dict(), "null handle")]:
        rc, text = gusts(**change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)

    def states(x_nom=at(0), sigma=np.full(12, 0.1), B=2, S=3, b0=0, s0=0, flags=0, x0=at(64)):
        sp = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64).ctypes.data
        return lib.qilqr_sample_states_device(None, x_nom, sp, SEED, B, S, b0, s0, flags, x0), last()

    for change, why in [(dict(x_nom=None), "null argument"), (dict(sigma=None), "null argument"), (dict(x0=None), "null argument"), (dict(S=0), "must be positive"),
                        (dict(b0=-1), "must not be negative"), (dict(x0=at(65)), "16-byte aligned"), (dict(sigma=np.full(12, -0.1)), "sigma must be finite"),
                        (dict(flags=4), "unknown flag bits"), (dict(x0=at(2)), "d_x0 overlaps d_x_nom"), (dict(), "null handle")]:
        rc, text = states(**change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)

    def reduce(score=at(0), B=2, S=3, summary=at(64)):
        return lib.qilqr_reduce_scores_device(None, score, B, S, summary), last()

    for change, why in [(dict(score=None), "null argument"), (dict(summary=None), "null argument"), (dict(B=-1), "must be positive"), (dict(score=at(1)), "16-byte aligned"),
                        (dict(summary=at(4)), "d_summary overlaps d_score"), (dict(), "null handle")]:
        rc, text = reduce(**change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)


# ------------------------------------------------------------------------------------------------ 6. the sanitizers

def test_the_harness_under_the_address_and_undefined_behaviour_sanitizers(x_nom):
    """the stand-alone program, compiled and run once with -fsanitize=address,undefined: every command, odd sizes"""
    exe = build_harness(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "host_monte_carlo_harness_san")
    assert subprocess.check_output([exe, "philox"] + KNOWN[2][0].split() + KNOWN[2][1].split()).decode().strip() == KNOWN[2][2]
    words, z = host_draws(exe, SEED, draw_index()[:50])
    assert np.isfinite(z).all() and (words < 1 << 32).all()
    assert np.isfinite(host_gusts(exe, SEED, B, 5, 11, tau_f=0.3, b0=65536, s0=70000)).all()
    assert np.isfinite(host_states(exe, SEED, x_nom, 7, flags=1)).all()
    for S in (1, 70, 130):
        score = mn.special_scores(B, S, S)
        assert np.array_equal(host_reduce(exe, score)[:, 2:], mn.summary(score)[:, 2:], equal_nan=True)
    assert rule(exe, "states", OK_STATES) == "ok" and "overlaps" in rule(exe, "reduce", OK_REDUCE, summary=4096 + 16)
