"""Linear covariance analysis of a plan's closed loop without a device: the host-compilable routines of quadrotorilqr_amd/csrc/cov_kernels.h
and the rule of cov_launch.h, compiled with g++ into the stand-alone program tests/host_cov_harness.cpp, against the restatement
(tests/lincov_numpy.py: oracle.discrete_step(diffs=True), oracle.gains_to_kK and central differences of the restated flight's step), against
answers known without one, and against themselves; the refusals through the harness and through the C ABI; the kernels of cov.hip by name.
B = 3, n = 12, dynamically consistent plans with the oracle's gains, 8 shared spheres and a moving one per plan.

THE BARS.  The issue sets |a - r| <= 1e-10 sqrt(r_kk r_ll) per covariance entry (closed_loop_numpy.RTOL) and the same against sqrt(r_kk) for
the mean, to be widened only if the observed CPU error forces it, to at most 100 times that error.  It does: the restatement's G is a
central difference at h = 1e-6, whose own rounding error is eps |x| / (2 h) ~ 1e-10 absolute on entries of the order dt / mass ~ 1e-2, and
every gust term of the recursion inherits that 1e-8.  Observed, harness against restatement over both integrators and models on / off:
2.6e-9 of sqrt(r_kk r_ll) on the covariances, 1.7e-8 of sqrt(r_kk) on the means (F itself agrees to 2e-15).  COV_BAR = 1e-7 (38 times the
observed error) and MEAN_BAR = 1e-6 (60 times).  Where both sides use the analytic G -- the kernels against the harness,
tests/test_gpu_covariance.py -- the bar stays 1e-10."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from quadrotorilqr_amd import capi
from tests import lincov_cases as lc, lincov_numpy as ln

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = lc.B, lc.N
COV_BAR, MEAN_BAR = 1e-7, 1e-6
EPS = 2.0 ** -52
KERNELS = ["_ZN5qilqr11k_cov_buildILi%dEJ%sEEEvNS_11ModelConstsIdEENS_12CovBuildArgsEDpT0_" % (i, e) for i in (0, 1) for e in ("", "NS_11BatchModelsE")] + \
    ["_ZN5qilqr11k_cov_chainENS_12CovChainArgsE", "_ZN5qilqr13k_cov_summaryENS_14CovSummaryArgsE"]
RULE = dict(mean=lc.GUST_MEAN, tau_force_s=lc.TAU_FORCE)


@pytest.fixture(scope="module")
def harness():
    return lc.build_harness(["-O2"], "host_cov_harness")


def relative(got, want):
    """(largest covariance error over sqrt(r_kk r_ll), largest mean error over sqrt(r_kk)) over the knots of the window"""
    live = ~np.isnan(want["cov"][:, :, 0, 0])
    d = np.sqrt(np.einsum("bnii->bni", want["cov"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        ec = np.abs(got["cov"] - want["cov"]) / (d[..., :, None] * d[..., None, :])
        em = np.abs(got["mean"] - want["mean"]) / d
    assert np.isfinite(ec[live]).all() and np.isfinite(em[live]).all()
    return float(ec[live].max()), float(em[live].max())


def compare_summaries(got, want, i0, i1, label):
    gp, gz = ln.margins(want, i0, i1)
    assert gp > 1e-6 and gz > 1e-6, (label, gp, gz)  # the runner-up of every discrete word is further away than any error here
    assert np.array_equal(got[:, [1, 5, 6]], want["summary"][:, [1, 5, 6]]), label
    np.testing.assert_allclose(got[:, [0, 2, 3, 7]], want["summary"][:, [0, 2, 3, 7]], rtol=COV_BAR, err_msg=label)
    np.testing.assert_allclose(got[:, 4], want["summary"][:, 4], rtol=MEAN_BAR, err_msg=label)


# ------------------------------------------------------------------------------------------------ 1. G against central differences

@pytest.mark.parametrize("integrator", [0, 1])
def test_the_wrench_jacobian_against_central_differences_of_the_flights_own_step(harness, integrator):
    """G of the harness (the routines k_cov_build calls) against central differences, h = 1e-6, of the device's disturbed step compiled for
    the host.  The bar is the difference quotient's own rounding: each next state carries a few roundings of words up to |x|, and their
    difference is divided by 2 h -- 8 eps max(1, |x|) / h, about 5e-9; the truncation term h^2 / 6 G''' is below 1e-12."""
    cfg, plan, gains, _, _, _ = lc.standard(integrator, True)
    got = lc.host_run(harness, cfg, plan, gains, integrator=integrator, models=lc.MODELS3)["G"]
    worst = 0.0
    for b in range(B):
        for i in range(N - 1):
            x, u = plan[b, i, 1:14], plan[b, i, 14:18]
            w = np.vstack([s * ln.H * np.eye(6)[k] for k in range(6) for s in (1.0, -1.0)])
            nxt = lc.host_step(harness, lc.MODELS3[b], integrator, cfg["dt"], np.tile(x, (12, 1)), np.tile(u, (12, 1)), w)
            G = np.stack([orc.state_minus(nxt[2 * k], nxt[2 * k + 1]) / (2.0 * ln.H) for k in range(6)], axis=1)
            bar = 8.0 * EPS * max(1.0, np.abs(nxt).max()) / ln.H
            worst = max(worst, np.abs(got[b, i] - G).max() / bar)
    print("[observed] integrator %d: G against central differences, %.3g of its bar" % (integrator, worst))
    assert worst <= 1.0
    assert np.abs(got[:, :N - 1]).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 2. the harness against the restatement

@pytest.mark.parametrize("modeled", [False, True])
@pytest.mark.parametrize("integrator", [0, 1])
def test_the_analysis_against_the_restatement(harness, integrator, modeled):
    cfg, plan, gains, shared, own, counts = lc.standard(integrator, modeled)
    models = lc.MODELS3 if modeled else None
    for i0, i1 in ((0, N - 1), (2, 9)):
        label = str((integrator, modeled, i0, i1))
        want = ln.covariance(plan, gains, cfg["model"], cfg["dt"], lc.SIGMA12, lc.GUST_SIGMA, integrator=integrator, models=models, i0=i0, i1=i1,
                             shared=shared, own=lc.own_rows(own, counts), **RULE)
        got = lc.host_run(harness, cfg, plan, gains, integrator=integrator, models=models, i0=i0, i1=i1, shared=shared, own=own, counts=counts, **RULE)
        ec, em = relative(got, want)
        print("[observed] %s: covariance error %.3g of sqrt(r_kk r_ll), mean error %.3g of sqrt(r_kk), F error %.3g"
              % (label, ec, em, np.nanmax(np.abs(got["F"] - want["F"]))))
        assert ec <= COV_BAR and em <= MEAN_BAR, label
        assert np.isnan(got["cov"][:, :i0]).all() and np.isnan(got["cov"][:, i1 + 1:]).all() and np.isnan(got["mean"][:, i1 + 1:]).all()
        compare_summaries(got["summary"], want, i0, i1, label)
    assert (got["summary"][:, 6] >= 0).all() and (got["summary"][:, 7] > 0).all()


def test_the_open_loop_and_the_held_wrench_against_the_restatement(harness):
    cfg, plan, _, shared, own, counts = lc.standard(1, False)
    for held in (False, True):
        want = ln.covariance(plan, None, cfg["model"], cfg["dt"], lc.SIGMA12, lc.GUST_SIGMA, integrator=1, held=held, shared=shared,
                             own=lc.own_rows(own, counts), **RULE)
        got = lc.host_run(harness, cfg, plan, None, integrator=1, held=held, shared=shared, own=own, counts=counts, **RULE)
        ec, em = relative(got, want)
        assert ec <= COV_BAR and em <= MEAN_BAR, (held, ec, em)
        compare_summaries(got["summary"], want, 0, N - 1, str(held))
        assert not got["summary"][:, 7].any()  # the open loop asks for no control
        assert np.abs(got["cross"][:, 1:] - want["cross"][:, 1:]).max() <= MEAN_BAR * np.abs(want["cross"][:, 1:]).max() and got["cross"][:, 1:].any()


# ------------------------------------------------------------------------------------------------ 3. known answers, no restatement

def test_with_every_sigma_zero_every_word_is_zero(harness):
    """no uncertainty in, none out: covariances, means and the deviations of the summary are +0; the knot of the largest deviation is the
    first; z is the plain clearance over 0 as IEEE division gives it (-inf, with its knot, where a path runs through a sphere; else +inf, which
    z < best never takes: knot and sphere stay -1), +inf without spheres"""
    cfg, plan, gains, shared, own, counts = lc.standard(0, False)
    for integrator in (0, 1):
        got = lc.host_run(harness, cfg, plan, gains, state_sigma=np.zeros(12), sigma=np.zeros(6), integrator=integrator, shared=shared, own=own, counts=counts)
        assert not got["cov"].any() and not got["mean"].any() and not got["cross"].any()
        assert not got["summary"][:, [0, 1, 2, 3, 7]].any()
        assert np.isinf(got["summary"][:, 4]).all() and np.array_equal(got["summary"][:, 5] >= 0, got["summary"][:, 4] < 0)
        bare = lc.host_run(harness, cfg, plan, gains, state_sigma=np.zeros(12), sigma=np.zeros(6), integrator=integrator)["summary"]
        assert (bare[:, 4] == np.inf).all() and (bare[:, 5:7] == -1).all() and not bare[:, [0, 1, 2, 3, 7]].any()


def test_a_window_of_one_knot_is_the_start_covariance(harness):
    cfg, plan, gains, _, _, _ = lc.standard(0, False)
    got = lc.host_run(harness, cfg, plan, gains, i0=5, i1=5, **RULE)
    assert np.array_equal(got["cov"][:, 5], np.broadcast_to(np.diag(lc.SIGMA12 * lc.SIGMA12), (B, 12, 12))) and not got["mean"][:, 5].any()
    assert np.isnan(np.delete(got["cov"], 5, axis=1)).all()
    assert np.array_equal(got["summary"][:, 1], np.full(B, 5.0)) and np.array_equal(got["summary"][:, 0], got["summary"][:, 2])


def test_white_noise_leaves_no_cross_covariance(harness):
    cfg, plan, gains, _, _, _ = lc.standard(1, False)
    for g in (None, gains):
        got = lc.host_run(harness, cfg, plan, g, integrator=1, mean=lc.GUST_MEAN)
        assert not got["cross"].any() and np.isfinite(got["cov"]).all() and (got["cov"][:, 1:] != got["cov"][:, :-1]).any()


def test_stored_covariances_are_symmetric_bit_for_bit_with_a_positive_diagonal(harness):
    for integrator in (0, 1):
        cfg, plan, gains, _, _, _ = lc.standard(integrator, True)
        cov = lc.host_run(harness, cfg, plan, gains, integrator=integrator, models=lc.MODELS3, **RULE)["cov"]
        assert cov.tobytes() == np.ascontiguousarray(np.swapaxes(cov, -1, -2)).tobytes()
        assert (np.einsum("bnii->bni", cov) >= 0.0).all()
        assert (np.linalg.eigvalsh(cov) > -1e-12 * np.einsum("bnii->bn", cov)[..., None]).all()


def test_a_held_wrench_is_a_correlation_of_one_and_tau_zero_is_white_noise(harness):
    """QILQR_COV_WRENCH_HELD is rho = 1: exp(-dt / 1e30) rounds to 1, so an enormous correlation time gives its bits.  tau = 0 is rho = 0:
    exp(-dt / (1e-6 dt)) underflows to 0, so a vanishing correlation time gives its bits."""
    cfg, plan, gains, shared, _, _ = lc.standard(0, False)
    kw = dict(mean=lc.GUST_MEAN, shared=shared)
    held = lc.host_run(harness, cfg, plan, gains, held=True, **kw)
    long = lc.host_run(harness, cfg, plan, gains, tau_force_s=1e30, tau_torque_s=1e30, **kw)
    white = lc.host_run(harness, cfg, plan, gains, **kw)
    short = lc.host_run(harness, cfg, plan, gains, tau_force_s=1e-6 * cfg["dt"], tau_torque_s=1e-6 * cfg["dt"], **kw)
    for key in ("cov", "mean", "summary", "cross"):
        assert held[key].tobytes() == long[key].tobytes() and white[key].tobytes() == short[key].tobytes(), key
    assert (held["cov"][:, -1] != white["cov"][:, -1]).any()


def test_a_plans_bits_do_not_depend_on_the_batch(harness):
    cfg, plan, gains, shared, own, counts = lc.standard(1, True)
    whole = lc.host_run(harness, cfg, plan, gains, integrator=1, models=lc.MODELS3, shared=shared, own=own, counts=counts, **RULE)
    for b in (0, B - 1):
        alone = lc.host_run(harness, cfg, plan[b:b + 1], gains[b:b + 1], integrator=1, models=lc.MODELS3[b:b + 1], shared=shared, own=own[b:b + 1],
                            counts=counts[b:b + 1], **RULE)
        for key in ("cov", "mean", "summary"):
            assert alone[key][0].tobytes() == whole[key][b].tobytes(), (b, key)


def test_the_harness_under_the_address_and_undefined_behaviour_sanitizers():
    """the stand-alone program, compiled and run once with -fsanitize=address,undefined: both integrators, models, both sphere tables, the rule"""
    exe = lc.build_harness(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "host_cov_harness_san")
    for integrator in (0, 1):
        cfg, plan, gains, shared, own, counts = lc.standard(integrator, True)
        got = lc.host_run(exe, cfg, plan, gains, integrator=integrator, models=lc.MODELS3, i0=1, i1=N - 2, shared=shared, own=own, counts=counts, **RULE)
        assert np.isfinite(got["cov"][:, 1:N - 1]).all() and np.isfinite(got["summary"]).all()
        lc.host_step(exe, cfg["model"], integrator, cfg["dt"], plan[0, 0, 1:14], plan[0, 0, 14:18], np.full(6, 1e-3))
    assert rule(exe) == "ok"


# ------------------------------------------------------------------------------------------------ 4. what the call refuses
OK_CALL = dict(rule=1, sigma0=1e-3, gsigma0=1e-2, tau=0.1, mean0=0.0, flags=1, reserved=0, plan=1 << 16, gains=1 << 18, cov=1 << 20, mean=1 << 22, summary=1 << 23,
               B=2, n=4, i0=0, i1=3, handle=1, f32=0, modeled=0, models_B=0, pobs_B=0)
ORDER = tuple(OK_CALL)
# in the order of the rule (cov_launch.h)
REFUSALS = [
    (dict(rule=0), "null argument"), (dict(plan=0), "null argument"),
    (dict(cov=0, mean=0, summary=0), "no output"),
    (dict(B=0), "must be positive"), (dict(n=-1), "must be positive"),
    (dict(i0=-1), "0 <= i0 <= i1 <= n - 1"), (dict(i0=3, i1=2), "0 <= i0 <= i1 <= n - 1"), (dict(i1=4), "0 <= i0 <= i1 <= n - 1"),
    (dict(sigma0=-1e-3), "every sigma"), (dict(sigma0="nan"), "every sigma"), (dict(gsigma0="inf"), "every sigma"), (dict(gsigma0=-1.0), "every sigma"),
    (dict(tau=-0.1), "correlation times"), (dict(tau="nan"), "correlation times"),
    (dict(mean0="inf"), "the mean must be finite"), (dict(mean0="nan"), "the mean must be finite"),
    (dict(flags=2), "unknown flag bits"), (dict(flags=3), "unknown flag bits"), (dict(reserved=1), "reserved word"),
    (dict(plan=(1 << 16) + 8), "16-byte aligned"), (dict(gains=(1 << 18) + 8), "16-byte aligned"), (dict(summary=(1 << 23) + 8), "16-byte aligned"),
    (dict(cov=(1 << 16) + 16), "an output overlaps an input"), (dict(mean=(1 << 18) + 2 * 4 * 52 * 8 - 16), "an output overlaps an input"),
    (dict(summary=1 << 16), "an output overlaps an input"),
    (dict(mean=(1 << 20) + 16), "the outputs overlap each other"), (dict(summary=(1 << 22) + 2 * 4 * 12 * 8 - 16), "the outputs overlap each other"),
    (dict(handle=0), "null handle"), (dict(f32=1), "precision 0"),
    (dict(modeled=1, models_B=3), "per-problem models were set for another B"), (dict(pobs_B=5), "per-problem obstacles were set for another B"),
]
ADMITTED = [dict(), dict(gains=0), dict(cov=0), dict(mean=0, summary=0), dict(flags=0), dict(i0=3), dict(sigma0=0.0, gsigma0=0.0, tau=0.0),
            dict(modeled=1, models_B=2, pobs_B=2), dict(mean=(1 << 20) + 2 * 4 * 144 * 8), dict(cov=(1 << 18) + 2 * 4 * 52 * 8)]


def rule(exe, **change):
    call = dict(OK_CALL, **change)
    return subprocess.check_output([exe, "refuse"] + [str(call[k]) for k in ORDER]).decode().strip()


def test_the_rule_of_what_the_call_refuses_and_its_order(harness):
    for change, why in REFUSALS:
        assert re.search(why, rule(harness, **change)), (change, rule(harness, **change))
    for change in ADMITTED:
        assert rule(harness, **change) == "ok", (change, rule(harness, **change))
    # the order: a row's reason stands with every later row's fault added at once (but for the pointers and shapes a later row moves:
    # a moved pointer would take this row's own overlap or misalignment away)
    for k, (change, why) in enumerate(REFUSALS):
        later = {}
        for other, _ in REFUSALS[k + 1:]:
            later.update({key: v for key, v in other.items() if key not in change and key not in later and key not in ("plan", "gains", "cov", "mean", "summary", "B", "n", "i0", "i1")})
        got = rule(harness, **dict(later, **change))
        assert re.search(why, got), (change, later, got)


def test_the_abi_without_a_device():
    """the structure and every refusal that needs no handle, through ctypes: the arguments are looked at before the handle"""
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "quadrotor_ilqr.h")).read()
    assert re.search(r"\bint qilqr_covariance_device\(", header) and "qilqr_covariance_device" in capi.EXPORTS and hasattr(lib, "qilqr_covariance_device")
    assert C.sizeof(capi.CovRule) == 216 and capi.CovRule.gust.offset == 96 and capi.CovRule.flags.offset == 208 and capi.CovRule.reserved.offset == 212
    assert "} qilqr_cov_rule;" in header and lib.qilqr_abi_version() == 7 and "#define QILQR_ABI_VERSION 7" in header
    for name, value in (("QILQR_COV", 144), ("QILQR_COV_SUMMARY", 8)):
        assert re.search(r"#define %s %d\b" % (name, value), header)
    assert capi.COV == 144 and capi.COV_SUMMARY == 8 and capi.COV_WRENCH_HELD == 1 and "#define QILQR_COV_WRENCH_HELD 1u" in header
    r = capi.cov_rule(2e-3, dict(sigma=[0.1, 0.01], mean=0.5, tau_force_s=0.3), wrench_held=True)
    assert list(r.state_sigma) == [2e-3] * 12 and list(r.gust.sigma) == [0.1] * 3 + [0.01] * 3 and r.gust.tau_force_s == 0.3 and r.flags == 1 and r.reserved == 0
    assert list(capi.cov_rule(np.arange(12.0)).gust.sigma) == [0.0] * 6 and capi.cov_rule(1.0).flags == 0
    with pytest.raises(TypeError):
        capi.cov_rule([1.0, 2.0])
    b, n = 2, 4
    arrays = dict(plan=capi._d16(np.zeros((b, n, 18))), gains=capi._d16(np.zeros((b, n, 52))), cov=capi._d16(np.zeros((b, n, 144))),
                  mean=capi._d16(np.zeros((b, n, 12))), summary=capi._d16(np.zeros((b, 8))))
    odd = capi._d16(np.zeros(b * n * 144 + 2))[1:]
    assert odd.ctypes.data % 16 == 8

    def call(with_rule=True, sigma=1e-3, gsigma=1e-2, tau=0.1, gmean=0.0, flags=0, reserved=0, B=b, i0=0, i1=n - 1, **ptr):
        a = {k: (v.ctypes.data if v is not None else None) for k, v in dict(arrays, **ptr).items()}
        r = capi.cov_rule([sigma] + [1e-3] * 11, dict(sigma=[gsigma] + [1e-2] * 5, mean=[gmean] + [0.0] * 5, tau_torque_s=tau))
        r.flags, r.reserved = flags, reserved
        rc = lib.qilqr_covariance_device(None, C.byref(r) if with_rule else None, a["plan"], a["gains"], B, n, i0, i1, a["cov"], a["mean"], a["summary"])
        return rc, lib.qilqr_last_error().decode()

    for change, why in [(dict(with_rule=False), "null argument"), (dict(plan=None), "null argument"), (dict(cov=None, mean=None, summary=None), "no output"),
                        (dict(B=0), "must be positive"), (dict(i1=n), "0 <= i0 <= i1 <= n - 1"), (dict(i0=2, i1=1), "0 <= i0 <= i1 <= n - 1"),
                        (dict(sigma=-1.0), "every sigma"), (dict(gsigma=float("nan")), "every sigma"), (dict(tau=float("inf")), "correlation times"),
                        (dict(gmean=float("nan")), "the mean must be finite"), (dict(flags=4), "unknown flag bits"), (dict(reserved=7), "reserved word"),
                        (dict(cov=odd), "16-byte aligned"), (dict(cov=arrays["plan"]), "an output overlaps an input"),
                        (dict(summary=arrays["gains"]), "an output overlaps an input"), (dict(mean=arrays["cov"]), "the outputs overlap each other"),
                        (dict(), "null handle"), (dict(gains=None, cov=None), "null handle")]:
        rc, text = call(**change)
        assert rc == capi.ERR_INVALID_ARG and why in text, (change, rc, text)


# ------------------------------------------------------------------------------------------------ 5. the kernels of the unit, by name

@pytest.mark.parametrize("defines", [[], ["-DQILQR_DIAG"]])
def test_the_kernels_of_the_unit_are_the_listed_ones(defines):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "quadrotorilqr_amd", "csrc")
    asm = subprocess.check_output([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc] + defines +
                                  ["-S", "--cuda-device-only", "-o", "-", os.path.join(csrc, "cov.hip")], stderr=subprocess.DEVNULL).decode()
    got = sorted({line.split()[1] for line in asm.splitlines() if line.lstrip().startswith(".amdhsa_kernel ")})
    assert got == sorted(KERNELS), got
    # no instantiation keeps anything in scratch memory, and the chain runs on the fp64 matrix core
    assert re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm) == ["0"] * len(KERNELS)
    assert asm.count("v_mfma_f64_16x16x4_f64") >= 15
    with open(os.path.join(csrc, "Makefile")) as f:
        assert "SRCS    += cov.hip\n" in f.readlines()
