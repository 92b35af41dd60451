"""What the fleet tests share (tests/test_fleet_cpu.py, tests/test_gpu_fleet.py, tests/fleet_torch_child.py): the host program
tests/host_fleet_harness.cpp built and run, and seeded plans.  The plans carry positions only where it matters (words 1..3 of a knot); the
other words are a hover state, so that the same arrays can be solved."""
import os
import subprocess
import tempfile

import numpy as np

from quadrotorilqr_amd import problems as pb

HERE = os.path.dirname(os.path.abspath(__file__))
DT = 0.05
RULE = dict(radius=0.8, weight=50.0)
_built = {}


def build_harness(flags=("-O2",), name="host_fleet_harness"):
    key = (tuple(flags), name)
    if key not in _built:
        d = tempfile.mkdtemp(prefix="host_fleet_harness_")
        exe = os.path.join(d, name)
        # (-ffp-contract=off: one rounding per operation written, as the device code has it, whatever the machine's instruction set)
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + list(flags) + ["-o", exe, os.path.join(HERE, "host_fleet_harness.cpp"), "-lm"])
        _built[key] = exe
    return _built[key]


def flags_of(cover=False, yield_to_lower=False):
    return (1 if cover else 0) | (2 if yield_to_lower else 0)


def host_run(exe, plan, V, K, dt=DT, radius=RULE["radius"], weight=RULE["weight"], range=np.inf, conflict=None, cover=False, yield_to_lower=False, chunk=None):
    """the call on the host, the partners cut into chunks of `chunk` (None: V): dict of summary (B, 8), nbr (B, K, 4), spheres (B, K, 8),
    counts (B) int32, fit (B, 8)"""
    B, n = plan.shape[:2]
    head = [B, n, V, K, V if chunk is None else chunk, dt, radius, weight, range, radius if conflict is None else conflict, flags_of(cover, yield_to_lower)]
    d = tempfile.mkdtemp(prefix="fleet_case_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    np.concatenate([np.asarray(head, dtype=np.float64), np.ascontiguousarray(plan, dtype=np.float64).ravel()]).tofile(fin)
    subprocess.check_call([exe, "run", fin, fout])
    o = np.fromfile(fout)
    cuts = np.cumsum([B * 8, B * K * 4, B * K * 8, B])
    return dict(summary=o[:cuts[0]].reshape(B, 8), nbr=o[cuts[0]:cuts[1]].reshape(B, K, 4), spheres=o[cuts[1]:cuts[2]].reshape(B, K, 8),
                counts=o[cuts[2]:cuts[3]].astype(np.int32), fit=o[cuts[3]:].reshape(B, 8))


def host_bob(exe, spheres, counts=None):
    """the device setter's row rule on the host: dict of tab (the tiled table), counts (B) int32, dropped, relaid (bob_relayout of the same rows)"""
    B, K = spheres.shape[:2]
    words = (B + 63) // 64 * K * 8 * 64
    d = tempfile.mkdtemp(prefix="fleet_bob_")
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    cnt = np.zeros(B) if counts is None else np.asarray(counts, dtype=np.float64)
    np.concatenate([[B, K, 0.0 if counts is None else 1.0], np.ascontiguousarray(spheres, dtype=np.float64).ravel(), cnt]).tofile(fin)
    subprocess.check_call([exe, "bob", fin, fout])
    o = np.fromfile(fout)
    return dict(tab=o[:words], counts=o[words:words + B].astype(np.int32), dropped=int(o[words + B]), relaid=o[words + B + 1:])


def hover(B, n):
    plan = np.zeros((B, n, 18))
    plan[:, :, 0] = np.arange(n) * DT
    plan[:, :, 4] = 1.0  # (the quaternion's w)
    return plan


def random_plans(B, n, seed, spread=10.0):
    """vehicles on random straight lines with a bend: positions within `spread` metres, a few m/s"""
    rng = np.random.default_rng(seed)
    plan = hover(B, n)
    t = (np.arange(n) * DT)[None, :, None]
    p0, v, a = rng.uniform(-spread, spread, (B, 1, 3)), rng.uniform(-3.0, 3.0, (B, 1, 3)), rng.uniform(-1.0, 1.0, (B, 1, 3))
    plan[:, :, 1:4] = p0 + v * t + 0.5 * a * t * t
    plan[:, :, 8:11] = v + a * t
    return plan


def integer_plans(B, n, seed, side=4):
    """positions on a small integer grid, changing from knot to knot: every d2 is exact and ties abound"""
    rng = np.random.default_rng(seed)
    plan = hover(B, n)
    plan[:, :, 1:4] = rng.integers(-side, side + 1, (B, n, 3)).astype(np.float64)
    return plan


def valid_spheres(B, K, seed):
    rng = np.random.default_rng(seed)
    sp = rng.uniform(-5.0, 5.0, (B, K, 8))
    sp[:, :, 6] = rng.uniform(0.2, 1.5, (B, K))
    sp[:, :, 7] = rng.uniform(0.0, 80.0, (B, K))
    return sp


# ---- tests/fleet_torch_child.py's case, shared with the test that reads what it records
TORCH_B, TORCH_N, TORCH_MISSION = 4, 16, 20
TORCH_DECONFLICT = dict(radius=0.9, weight=40.0, K=2, conflict=0.5, cover=True, yield_to_lower=True)


def torch_case():
    """four vehicles from random starts within a metre of one another, all asked to hover at the origin: every one is in the others' way"""
    cfg = pb.config2(B=TORCH_B, N=TORCH_MISSION, seed=9)
    return cfg, np.ascontiguousarray(cfg["init"][:, :TORCH_N])
