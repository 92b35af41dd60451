"""What tests/test_covariance_cpu.py and tests/test_gpu_covariance.py share: the stand-alone host program of the linear covariance
analysis (tests/host_cov_harness.cpp) built and called, the rule's inputs, and dynamically consistent plans with gains and spheres.
Nothing here asserts."""
import functools
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as orc
from tests import closed_loop_numpy as cn, mppi_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
B, N, SEED = 3, 12, 3
# the rule of the comparisons: start-state deviations over [rho, theta, dv, dw], a gust model with correlated forces and white torques
SIGMA12 = np.array([2e-3] * 3 + [3e-3] * 3 + [5e-3] * 3 + [4e-3] * 3)
GUST_SIGMA = np.array([2e-2, 1e-2, 3e-2, 1e-3, 2e-3, 1.5e-3])
GUST_MEAN = np.array([0.05, -0.03, 0.04, 2e-3, -1e-3, 1e-3])
TAU_FORCE = 0.05
MODELS3 = mc.MODELS3


def build_harness(flags, name):
    d = tempfile.mkdtemp(prefix="host_cov_harness_")
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(HERE, "host_cov_harness.cpp"), "-lm"])
    return exe


def _run(exe, mode, words):
    d = tempfile.mkdtemp(prefix="cov_case_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    np.asarray(words, dtype=np.float64).tofile(fin)
    subprocess.check_call([exe, mode, fin, fout])
    return np.fromfile(fout)


def host_run(exe, cfg, plan, gains, state_sigma=SIGMA12, sigma=GUST_SIGMA, mean=None, tau_force_s=0.0, tau_torque_s=0.0, held=False, integrator=0,
             models=None, i0=0, i1=None, shared=None, own=None, counts=None):
    """the analysis on the host: dict of cov (B, n, 12, 12), mean (B, n, 12), summary (B, 8), cross (B, n, 12, 6), F, G; NaN outside the window.
    own (B, K, 8) with counts (B), as qilqr_set_batch_obstacles takes them."""
    b, n = plan.shape[:2]
    i1 = n - 1 if i1 is None else i1
    shared = np.zeros((0, 5)) if shared is None else np.asarray(shared, dtype=np.float64).reshape(-1, 5)
    own_K = 0 if own is None else own.shape[1]
    head = [b, n, i0, i1, integrator, models is not None, gains is not None, held, cfg["dt"], len(shared), own_K]
    parts = [np.array(head, dtype=np.float64), mc.model_words(cfg["model"]), np.asarray(cfg["Q"], dtype=np.float64).ravel(),
             np.asarray(cfg["R"], dtype=np.float64).ravel(), np.asarray(state_sigma, dtype=np.float64), np.zeros(6) if mean is None else np.asarray(mean, dtype=np.float64),
             np.asarray(sigma, dtype=np.float64), np.array([tau_force_s, tau_torque_s])]
    if models is not None:
        assert len(models) == b
        parts += [mc.model_words(m) for m in models]
    parts.append(np.asarray(plan, dtype=np.float64).ravel())
    if gains is not None:
        parts.append(np.asarray(gains, dtype=np.float64).ravel())
    parts.append(shared.ravel())
    if own is not None:
        parts += [np.asarray(own, dtype=np.float64).ravel(), np.asarray(counts if counts is not None else [own_K] * b, dtype=np.float64)]
    out = _run(exe, "run", np.concatenate(parts))
    k = b * n
    assert out.size == k * (144 + 12 + 72 + 144 + 72) + b * 8
    o = np.split(out, np.cumsum([k * 144, k * 12, b * 8, k * 72, k * 144]))
    return dict(cov=o[0].reshape(b, n, 12, 12), mean=o[1].reshape(b, n, 12), summary=o[2].reshape(b, 8), cross=o[3].reshape(b, n, 12, 6),
                F=o[4].reshape(b, n, 12, 12), G=o[5].reshape(b, n, 12, 6))


def host_step(exe, model, integrator, dt, x, u, w):
    """rows of the flight's own disturbed step on the host: x (r, 13), u (r, 4), w (r, 6) -> (r, 13)"""
    x, u, w = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (x, u, w))
    rows = np.hstack([x, u, w])
    out = _run(exe, "step", np.concatenate([[integrator, dt, len(rows)], mc.model_words(model), rows.ravel()]))
    return out.reshape(len(rows), 13)


def rolled_out(cfg, plan, integrator, models=None):
    """the plans made dynamically consistent: every knot follows from the one before by the step under its own control"""
    out = np.array(plan, dtype=np.float64)
    for b in range(len(out)):
        mp = orc.model_params(**(models[b] if models is not None else cfg["model"]))
        for i in range(out.shape[1] - 1):
            out[b, i + 1, 1:14] = orc.discrete_step(mp, integrator, out[b, i, 1:14], out[b, i, 14:18], cfg["dt"])
    return np.ascontiguousarray(out)


def spheres_beside(plan, seed):
    """(shared (8, 5), own (b, 2, 8), counts (b)): 8 shared spheres beside plan knots and one moving sphere in use per plan (row 1 of
    every plan's table is beyond its count: a sphere of radius 1 on the path, ruinous if it were read), for any n >= 2"""
    r = np.random.default_rng(seed)
    b, n = plan.shape[:2]
    shared = np.zeros((8, 5))
    for j in range(8):
        shared[j, :3] = plan[j % b, (1 + 2 * j) % n, 1:4] + 0.3 * (2.0 * r.random(3) - 1.0)
        shared[j, 3:] = (0.10 + 0.03 * (j % 3), 20.0 + 5.0 * j)
    own = np.zeros((b, 2, 8))
    for k in range(b):
        own[k, 0, :3] = plan[k, n - 1 - (k % 2), 1:4] + 0.25 * (2.0 * r.random(3) - 1.0)
        own[k, 0, 3:6] = (0.05, -0.04, 0.03)
        own[k, 0, 6:8] = (0.15, 40.0)
        own[k, 1] = (*plan[k, n // 2, 1:4], 0.0, 0.0, 0.0, 1.0, 1e6)
    return shared, own, np.ones(b, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def standard(integrator=0, modeled=False, b=B, n=N, seed=SEED):
    """(cfg, plan (b, n, 18), gains (b, n, 52), shared (8, 5), own (b, 2, 8), counts): cn.plans rolled out, the oracle's gains about them,
    spheres_beside their paths (8 shared spheres, one moving sphere per plan); read-only"""
    cfg, plan = cn.plans(b, n, seed)
    plan = rolled_out(cfg, plan, integrator, [MODELS3[k % 3] for k in range(b)] if modeled else None)
    gains = np.ascontiguousarray(cn.oracle_gains(cfg, plan))
    shared, own, counts = spheres_beside(plan, seed + 7)
    for a in (plan, gains, shared, own, counts):
        a.setflags(write=False)
    return cfg, plan, gains, shared, own, counts


def own_rows(own, counts):
    return [own[k, :counts[k]] for k in range(len(own))]


# ---- tests/lincov_torch_child.py's case: a handle with shared spheres, the plans a solve starts from
TORCH_GUST = dict(sigma=GUST_SIGMA, mean=GUST_MEAN, tau_force_s=TAU_FORCE, tau_torque_s=0.0)


def torch_case():
    """(cfg, init (B, N, 18), shared (8, 5))"""
    cfg, init = cn.plans(B, N, SEED + 2)
    shared, _, _ = spheres_beside(init, SEED + 9)
    return cfg, init, shared
