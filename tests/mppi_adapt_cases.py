"""What tests/test_mppi_adapt_cpu.py and tests/test_gpu_mppi_adapt.py share: the stand-alone host program of the planner's adapted spread
(tests/host_mppi_adapt_harness.cpp) built and called over tests/mppi_cases.py's cases, a spread that varies by plan, knot and rotor, and
the adapt rule of the comparisons.  Nothing here asserts."""
import os
import subprocess
import tempfile

import numpy as np

from tests import mppi_adapt_numpy as ma, mppi_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
B, N = mc.B, mc.N
# floor and cap of the comparisons: the restated spreads of the standard cases stay inside (asserted where they are used)
FLOOR = np.array([0.05, 0.04, 0.06, 0.05])
CAP = np.array([1.5, 1.4, 1.6, 1.5])
RATE = 0.4


def build_harness(flags, name):
    d = tempfile.mkdtemp(prefix="host_mppi_adapt_harness_")
    exe = os.path.join(d, name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, os.path.join(HERE, "host_mppi_adapt_harness.cpp"), "-lm"])
    return exe


def spread_field(b=B, n=N):
    """(b, n, 4): mc.SIGMA scaled by a factor in [0.6, 1.5] that differs for every plan, knot and rotor"""
    k, i, a = np.meshgrid(np.arange(b), np.arange(n), np.arange(4), indexing="ij")
    return np.ascontiguousarray(mc.SIGMA * (0.6 + 0.9 * ((7 * k + 3 * i + 5 * a) % 11) / 10.0))


def constant_spread(sigma, b=B, n=N):
    return np.ascontiguousarray(np.broadcast_to(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (4,)), (b, n, 4)))


def _words(cfg, plan, S, seed, spread, floor, cap, rate, **kw):
    head = mc._pack(cfg, plan, S, seed, 0.0, **kw)
    tail = np.concatenate([np.asarray(spread, dtype=np.float64).ravel(), np.broadcast_to(np.asarray(floor, dtype=np.float64), (4,)),
                           np.broadcast_to(np.asarray(cap, dtype=np.float64), (4,)), [float(rate)]])
    return np.concatenate([head, tail])


def host_fly(exe, cfg, plan, S, seed, spread, **kw):
    """one flight on the host: (score (B, S, 4), eps as flown (B, S, n, 4))"""
    b, n = plan.shape[0], plan.shape[1]
    out = mc._run(exe, "fly", _words(cfg, plan, S, seed, spread, 0.0, 1.0, 1.0, **kw))
    assert out.size == b * S * 4 + b * S * n * 4
    return out[:b * S * 4].reshape(b, S, 4), out[b * S * 4:].reshape(b, S, n, 4)


def host_adapt(exe, cfg, plan, score, seed, spread, lambda_, floor=FLOOR, cap=CAP, rate=RATE, **kw):
    """one adaptation on the host over `score` (B, S, 4): (out_plan (B, n, 18), info (B, 8), out_spread (B, n, 4), var (B, n, 4))"""
    b, n, S = plan.shape[0], plan.shape[1], score.shape[1]
    out = mc._run(exe, "adapt", _words(cfg, plan, S, seed, spread, floor, cap, rate, lambda_=lambda_, score=score, **kw))
    assert out.size == b * n * 18 + b * 8 + 2 * b * n * 4
    o = np.split(out, np.cumsum([b * n * 18, b * 8, b * n * 4]))
    return o[0].reshape(b, n, 18), o[1].reshape(b, 8), o[2].reshape(b, n, 4), o[3].reshape(b, n, 4)


def everything(S, seed=77):
    """mc.everything's case flown with spread_field(): (host keywords, restatement keywords, cfg, plan, x0, spread, the restatement's eps)"""
    host, rest, cfg, plan, x0, _ = mc.everything(S, seed)
    spread = spread_field()
    eps = ma.perturbations(seed, spread, S, cfg["dt"], tau_s=0.3)
    return host, rest, cfg, plan, x0, spread, eps


def compare_spreads(got, want, bound):
    """the comparison of new spreads against a restatement `want` (ma.adapt's dict): entries whose unclamped restated spread lies within
    1e-9 of floor or cap are compared for 'either side' only -> (largest error over its bound among the others, the fraction of
    entries under the margin, all of the marginal ones on either side)"""
    floor, cap = want["floor"], want["cap"]
    near = (np.abs(want["raw"] - floor) < 1e-9) | (np.abs(want["raw"] - cap) < 1e-9)
    per = bound / (got + want["spread"]) + 2.0 * ma.EPS * want["spread"]
    err = np.abs(got - want["spread"])
    either = ((got == floor) | (got == cap) | (err <= per))[near].all() if near.any() else True
    return float((err / per)[~near].max()), float(near.mean()), bool(either)


# ---- tests/mppi_cases.py's planning scenario with the spread adapted between the rounds
PLAN_ADAPT = dict(rate=0.5, floor=0.05, cap=2.0)


def host_plan(exe):
    """the scenario on the harness: mc.PLAN_ROUNDS rounds of flight and adaptation at mc.host_plan's seeds, the spread started at the
    rule's sigma -> (plans after each round, infos, spreads)"""
    cfg, plan, shared = mc.planning()
    spread = constant_spread(mc.PLAN_RULE["sigma"], mc.PLAN_B, mc.PLAN_N)
    plans, infos, spreads = [], [], []
    for r in range(mc.PLAN_ROUNDS):
        kw = dict(shared=shared, **{k: v for k, v in mc.PLAN_RULE.items() if k not in ("sigma", "lambda_")})
        score, _ = host_fly(exe, cfg, plan, mc.PLAN_S, mc.PLAN_SEED + r, spread, **kw)
        plan, info, spread, _ = host_adapt(exe, cfg, plan, score, mc.PLAN_SEED + r, spread, mc.PLAN_RULE["lambda_"], **dict(PLAN_ADAPT, **kw))
        plans.append(plan)
        infos.append(info)
        spreads.append(spread)
    return np.stack(plans), np.stack(infos), np.stack(spreads)
