"""Fleet deconfliction on the device (k_fleet_fit, k_fleet_pairs, k_fleet_select, k_bob_set: fleet_kernels.h) through the C ABI on plain
device buffers: qilqr_fleet_neighbours_device against the host program (tests/host_fleet_harness.cpp, the same fleet_math.h) BIT FOR BIT on
every output, over the ego tile's edge, a second tile and more than two partner chunks; guard bytes, each output alone, refused calls, a
fleet's independence of the batch; qilqr_set_batch_obstacles_device against the host setter through the cost and the backward pass; the
chain neighbours -> spheres -> setter -> solve on two crossing vehicles; RecedingHorizon.tick(deconflict=...) in a torch process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from quadrotorilqr_amd import capi, problems as pb  # noqa: E402
from tests import fleet_cases as fc, fleet_numpy as fn  # noqa: E402
from tests.test_gpu_closed_loop import Hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes behind the end of every output, prefilled with 0xFF like the output
OUTPUTS = ("summary", "nbr", "spheres", "counts")
SHAPES = dict(summary=lambda b, k: (b, 8), nbr=lambda b, k: (b, k, 4), spheres=lambda b, k: (b, k, 8), counts=lambda b, k: (b,))
DTYPES = dict(summary=np.float64, nbr=np.float64, spheres=np.float64, counts=np.int32)
VP = C.c_void_p


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.close()


@pytest.fixture(scope="module")
def harness():
    return fc.build_harness()


@pytest.fixture(scope="module")
def solver():
    return capi.from_config(pb.config2(B=1, N=4))


def dev_fleet(hip, s, plan, V, K, outputs=OUTPUTS, expect=0, radius=fc.RULE["radius"], weight=fc.RULE["weight"], range=np.inf, conflict=None, cover=False,
              yield_to_lower=False):
    """one call on 0xFF-prefilled outputs with a guard behind each: dict of the outputs asked for, plus "raw" (their bytes) -- after asserting
    that every guard kept its bits.  expect: the return code."""
    lib = capi.load()
    b, n = plan.shape[:2]
    rule = capi.fleet_rule(radius, weight, range, conflict, cover, yield_to_lower)
    d_plan = hip.upload(plan)
    size = {k: int(np.prod(SHAPES[k](b, K))) * np.dtype(DTYPES[k]).itemsize for k in outputs}
    ptr = {k: hip.alloc(size[k] + GUARD) for k in outputs}
    rc = lib.qilqr_fleet_neighbours_device(s._h, C.byref(rule), d_plan, b, n, V, K, ptr.get("summary"), ptr.get("nbr"), ptr.get("spheres"), ptr.get("counts"))
    assert rc == expect, (rc, lib.qilqr_last_error())
    hip.synchronize(lib.qilqr_stream(s._h))
    out = dict(raw={}, text=lib.qilqr_last_error().decode() if rc else "")
    for k in outputs:
        raw = hip.download(ptr[k], (size[k] + GUARD,), dtype=np.uint8)
        assert (raw[size[k]:] == 0xFF).all(), "the call wrote behind the end of " + k
        out[k], out["raw"][k] = raw[:size[k]].view(DTYPES[k]).reshape(SHAPES[k](b, K)), raw[:size[k]]
    assert hip.download(d_plan, plan.shape).tobytes() == plan.tobytes()
    return out


def same_bits(got, want, label, keys=OUTPUTS):
    for k in keys:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).astype(DTYPES[k]).tobytes(), (label, k, got[k], want[k])


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


# ------------------------------------------------------------------------------------------------ 1. the device against the host program, bit for bit

@pytest.mark.parametrize("V, n, K, fleets", [(1, 2, 1, 1), (2, 1, 8, 1), (63, 17, 8, 1), (64, 2, 16, 1), (65, 17, 1, 1), (130, 17, 16, 1), (130, 2, 8, 1), (65, 17, 16, 3),
                                            (65, 1, 8, 3)])
def test_every_output_has_the_bits_of_the_host_program(hip, harness, solver, V, n, K, fleets):
    dt = pb.DT_DEMO
    plan = fc.random_plans(fleets * V, n, 100 + V + n + K, spread=6.0)
    for flags in (dict(), dict(cover=True), dict(yield_to_lower=True, conflict=3.0), dict(cover=True, yield_to_lower=True, range=5.0, conflict=3.0)):
        got = dev_fleet(hip, solver, plan, V, K, **flags)
        same_bits(got, fc.host_run(harness, plan, V, K, dt=dt, **flags), (V, n, K, fleets, flags))
        assert V == 1 or got["summary"][:, 0].min() < np.inf


@pytest.mark.parametrize("V, fleets", [(130, 1), (65, 3)])
def test_ties_on_integer_coordinates_have_the_bits_of_the_host_program(hip, harness, solver, V, fleets):
    plan = fc.integer_plans(fleets * V, 5, 7 + V, side=2)
    for flags in (dict(), dict(yield_to_lower=True)):
        got = dev_fleet(hip, solver, plan, V, 16, **flags)
        same_bits(got, fc.host_run(harness, plan, V, 16, dt=pb.DT_DEMO, **flags), (V, flags))
        d = got["nbr"][:, :, 1]
        assert (d[:, 1:] == d[:, :-1]).any()  # (ties were there to be broken)


def test_a_vehicle_that_is_nowhere_on_the_device(hip, harness, solver):
    plan = fc.random_plans(70, 6, 41, spread=3.0)
    plan[3, :, 1:4] = np.nan
    plan[68, 2, 3] = np.inf
    got = dev_fleet(hip, solver, plan, 70, 16, cover=True)
    same_bits(got, fc.host_run(harness, plan, 70, 16, dt=pb.DT_DEMO, cover=True), "nan")
    assert np.isfinite(got["spheres"]).all() and got["counts"][3] == 0 and not (got["nbr"][:, :, 0] == 3).any()


# ------------------------------------------------------------------------------------------------ 2. memory discipline

def test_each_output_alone_has_the_bits_it_has_among_the_others(hip, solver):
    plan = fc.random_plans(65, 5, 51, spread=4.0)
    kw = dict(cover=True, range=6.0, conflict=2.0)
    whole = dev_fleet(hip, solver, plan, 65, 8, **kw)
    for k in OUTPUTS:
        alone = dev_fleet(hip, solver, plan, 65, 8, outputs=(k,), **kw)
        assert alone["raw"][k].tobytes() == whole["raw"][k].tobytes(), k


def test_refused_calls_on_a_live_handle_leave_the_outputs_untouched(hip, solver):
    plan = fc.random_plans(6, 4, 52)
    for V, K, change, why in [(4, 2, dict(), "V must divide B"), (6, 17, dict(), "K must be 1"), (6, 2, dict(radius=-1.0), "radius"), (6, 2, dict(range=0.0), "range"),
                              (6, 2, dict(conflict=float("nan")), "conflict"), (6, 2, dict(weight=float("inf")), "weight")]:
        got = dev_fleet(hip, solver, plan, V, K, expect=capi.ERR_INVALID_ARG, **change)
        assert why in got["text"] and all(untouched(got[k]) for k in OUTPUTS), (change, got["text"])
    got = dev_fleet(hip, capi.from_config(pb.config2(B=1, N=4), precision="f32"), plan, 6, 2, expect=capi.ERR_INVALID_ARG)
    assert "precision 0" in got["text"] and all(untouched(got[k]) for k in OUTPUTS)
    lib = capi.load()
    d_plan = hip.upload(plan)
    rule = capi.fleet_rule(1.0, 1.0)
    assert lib.qilqr_fleet_neighbours_device(solver._h, C.byref(rule), d_plan, 6, 4, 6, 2, d_plan + 16, None, None, None) == capi.ERR_INVALID_ARG
    assert "an output overlaps the plan" in lib.qilqr_last_error().decode()
    hip.synchronize(lib.qilqr_stream(solver._h))
    assert hip.download(d_plan, plan.shape).tobytes() == plan.tobytes()


def test_a_fleets_rows_have_the_bytes_of_that_fleet_alone(hip, solver):
    V, K = 65, 8
    plan = fc.random_plans(3 * V, 6, 53, spread=5.0)
    whole = dev_fleet(hip, solver, plan, V, K, cover=True, conflict=3.0)
    for g in range(3):
        rows = slice(g * V, (g + 1) * V)
        alone = dev_fleet(hip, solver, plan[rows], V, K, cover=True, conflict=3.0)
        shifted = dict(alone, nbr=alone["nbr"].copy(), summary=alone["summary"].copy())
        shifted["nbr"][:, :, 0] += np.where(alone["nbr"][:, :, 0] >= 0, g * V, 0)
        shifted["summary"][:, 2] += np.where(alone["summary"][:, 2] >= 0, g * V, 0)
        same_bits({k: whole[k][rows] for k in OUTPUTS}, shifted, g)


# ------------------------------------------------------------------------------------------------ 3. the device setter against the host setter

def table_on(trajs, K, seed):
    """(B, K, 8) valid moving spheres that reach their problem's knots"""
    r = np.random.default_rng(seed)
    B, n = trajs.shape[:2]
    sp = np.zeros((B, K, 8))
    for b in range(B):
        for j in range(K):
            i = int(r.integers(0, n))
            v = r.normal(size=3) * 0.5
            c = trajs[b, i, 1:4] + r.normal(size=3) * 0.2
            sp[b, j] = [*(c - i * pb.DT_DEMO * v), *v, r.uniform(0.5, 1.0), r.uniform(5.0, 40.0)]
    return sp


def device_set(hip, s, spheres, counts=None, dropped=True):
    lib = capi.load()
    B, K = spheres.shape[:2]
    d_sp = hip.upload(spheres)
    d_cnt = hip.upload(np.asarray(counts, dtype=np.int32)) if counts is not None else None
    d_drop = hip.alloc(4 + GUARD) if dropped else None
    rc = lib.qilqr_set_batch_obstacles_device(s._h, d_sp, d_cnt, B, K, d_drop)
    assert rc == 0, lib.qilqr_last_error()
    hip.synchronize(lib.qilqr_stream(s._h))
    if not dropped:
        return None
    raw = hip.download(d_drop, (4 + GUARD,), dtype=np.uint8)
    assert (raw[4:] == 0xFF).all()
    return int(raw[:4].view(np.int32)[0])


def passes(s, trajs):
    gains, terms = s.backwards_pass(trajs)
    return s.cost_trajectory(trajs).tobytes() + gains.tobytes() + terms.tobytes()


@pytest.mark.parametrize("B", [8, 70])
def test_the_cost_and_the_backward_pass_have_the_bits_of_a_host_set_table(hip, B):
    cfg = pb.config2(B=B, N=10, seed=5)
    trajs, K = cfg["init"], 4
    sp, counts = table_on(trajs, K, B), (np.arange(B) + 1) % 4
    dev, host, bare = capi.from_config(cfg), capi.from_config(cfg), capi.from_config(cfg)
    assert device_set(hip, dev, sp, counts) == 0
    host.set_batch_obstacles(sp, counts)
    want = passes(host, trajs)
    assert passes(dev, trajs) == want and want != passes(bare, trajs)
    assert "set on the device" in dev.describe(B) and "set on the device" not in host.describe(B)
    assert dev.describe(B).split("batch obstacles")[0] == host.describe(B).split("batch obstacles")[0]  # (the same route)
    with pytest.raises(TypeError, match="batch obstacles were set for B = %d" % B):
        dev.cost_trajectory(trajs[:B - 1])
    # invalid rows interleaved: dropped, the kept rows move up; the host-set table of the kept rows gives the same bits
    K2 = 6
    wide = np.zeros((B, K2, 8))
    wide[:, [0, 2, 3, 5]] = sp
    wide[:, 1], wide[:, 4] = sp[:, 0], sp[:, 1]
    wide[:, 1, 6], wide[:, 4, 0] = -1.0, np.nan
    wide[1::2, 4] = sp[1::2, 2]  # (every other problem's row 4 is valid)
    cnt2 = np.minimum((np.arange(B) + 2) % 8, K2)
    used = np.arange(K2)[None] < cnt2[:, None]
    bad = np.zeros((B, K2), dtype=bool)
    bad[:, 1], bad[0::2, 4] = True, True
    kept_rows = np.zeros((B, K2, 8))
    for b in range(B):
        rows = wide[b][used[b] & ~bad[b]]
        kept_rows[b, :len(rows)] = rows
    kept = (used & ~bad).sum(axis=1)
    assert device_set(hip, dev, wide, cnt2) == int((used & bad).sum()) > 0
    host.set_batch_obstacles(kept_rows, kept)
    assert passes(dev, trajs) == passes(host, trajs)


def test_capacity_reuse_then_the_host_setter_then_the_clear(hip):
    B = 8
    cfg = pb.config2(B=B, N=10, seed=6)
    trajs = cfg["init"]
    dev, host, bare = capi.from_config(cfg), capi.from_config(cfg), capi.from_config(cfg)
    none = passes(bare, trajs)
    tables = {K: table_on(trajs, K, 60 + K) for K in (4, 2)}
    seen = []
    for K in (4, 2, 4):
        device_set(hip, dev, tables[K], dropped=False)
        host.set_batch_obstacles(tables[K])
        seen.append(passes(dev, trajs))
        assert seen[-1] == passes(host, trajs) != none, K
        assert "K = %d" % K in dev.describe(B)
    assert seen[0] == seen[2] != seen[1]
    dev.set_batch_obstacles(tables[2], np.full(B, 1, dtype=np.int32))
    host.set_batch_obstacles(tables[2], np.full(B, 1, dtype=np.int32))
    assert passes(dev, trajs) == passes(host, trajs) and "at most 1 used per problem" in dev.describe(B)
    device_set(hip, dev, tables[4], dropped=False)  # (and back to the device setter)
    assert passes(dev, trajs) == seen[0]
    dev.clear_batch_obstacles()
    assert passes(dev, trajs) == none and dev.describe(B) == bare.describe(B)


# ------------------------------------------------------------------------------------------------ 4. end to end

def crossing(n):
    """two vehicles on crossing lines, at the crossing at the same time, offset laterally and in height"""
    cfg = pb.config2(B=2, N=n)
    s = (np.arange(n) / (n - 1.0))[:, None]
    des = np.repeat(cfg["desired"][None], 2, axis=0).copy()
    des[0, :, 1:4] = np.array([-3.0, 0.0, 0.0]) + s * np.array([6.0, 0.0, 0.0])
    des[1, :, 1:4] = np.array([0.3, -3.0, 0.2]) + s * np.array([0.0, 6.0, 0.0])
    speed = 6.0 / ((n - 1) * cfg["dt"])
    des[0, :, 8], des[1, :, 9] = speed, speed  # (identity attitude: body velocity = world velocity)
    return cfg, des


def solve_device(hip, s, init, des):
    lib = capi.load()
    B, n = init.shape[:2]
    d_init, d_des = hip.upload(init), hip.upload(des) if des is not None else None
    d_traj, d_cost = hip.alloc(init.nbytes), hip.alloc(8 * B)
    d_int = [hip.alloc(4 * B) for _ in range(4)]
    rc = lib.qilqr_solve_batch_device(s._h, VP(d_init), VP(d_des), C.c_int32(B), C.c_int32(n), VP(d_traj), VP(d_cost), *[VP(p) for p in d_int])
    assert rc == 0, lib.qilqr_last_error()
    return hip.download(d_traj, init.shape), hip.download(d_cost, (B,)), hip.download(d_int[0], (B,), dtype=np.int32)


def test_two_crossing_vehicles_neighbours_to_spheres_to_setter_to_solve(hip):
    n, K = 30, 1
    cfg, des = crossing(n)
    lib = capi.load()
    rule = dict(radius=1.5, weight=400.0, yield_to_lower=True, cover=True)
    first, second = capi.from_config(cfg), capi.from_config(cfg)
    parent, _, _ = solve_device(hip, first, des, des)
    got = dev_fleet(hip, first, parent, 2, K, **rule)
    assert list(got["counts"]) == [0, 1] and got["nbr"][1, 0, 0] == 0 and got["summary"][0, 0] == got["summary"][1, 0] < 1.0
    # the chain on the device: the outputs of the neighbours call straight into the setter, then the solve
    r = capi.fleet_rule(**rule)
    d_parent, d_sp, d_cnt = hip.upload(parent), hip.alloc(8 * 2 * K * 8), hip.alloc(4 * 2)
    assert lib.qilqr_fleet_neighbours_device(first._h, C.byref(r), d_parent, 2, n, 2, K, None, None, d_sp, d_cnt) == 0
    assert lib.qilqr_set_batch_obstacles_device(first._h, d_sp, d_cnt, 2, K, None) == 0
    replanned, cost, status = solve_device(hip, first, parent, des)
    print("[observed] status of the re-plan:", status)
    # a second handle given the downloaded spheres through the host setter: the same bits
    second.set_batch_obstacles(got["spheres"], got["counts"])
    again, cost2, _ = solve_device(hip, second, parent, des)
    assert again.tobytes() == replanned.tobytes() and cost.tobytes() == cost2.tobytes()
    before, after = np.sqrt(fn.pair_values(parent, 2)[0][1, 0]), np.sqrt(fn.pair_values(replanned, 2)[0][1, 0])
    print("[observed] smallest separation of the two plans: %.4f m before, %.4f m after the re-plan" % (before, after))
    assert after > before
    assert np.abs(replanned[1, :, 1] - parent[1, :, 1]).max() > 1e-3  # (the lateral part of the sphere's gradient moved vehicle 1 sideways)


# ------------------------------------------------------------------------------------------------ 5. the torch child

def test_tick_with_deconflict_has_the_bits_of_the_three_calls_made_directly(hip, tmp_path):
    """tests/fleet_torch_child.py, in a process of its own (PyTorch's ROCm runtime has to be the first a process initialises), records what
    RecedingHorizon.tick(deconflict=...) and the direct torch calls return; here the three calls are made through the C ABI on its plans"""
    out = str(tmp_path / "recorded.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "tests.fleet_torch_child", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(out) as z:
        rec = {k: z[k] for k in z.files}
    B, K = fc.TORCH_B, fc.TORCH_DECONFLICT["K"]
    rule = {k: v for k, v in fc.TORCH_DECONFLICT.items() if k != "K"}
    # "separation" is the direct summary, and so the other outputs
    for a, b in (("tick1_separation", "direct_summary"), ("tick1_neighbours", "direct_nbr"), ("tick1_spheres", "direct_spheres"), ("tick1_counts", "direct_counts")):
        assert rec[a].tobytes() == rec[b].tobytes(), a
    assert rec["tick1_counts"].sum() > 0 and int(rec["tick1_dropped"][0]) == 0 and not rec["tick1_counts"][0]  # (row 0 yields to nobody)
    assert "batch obstacles" not in str(rec["describe_before"]) and "set on the device" in str(rec["describe_after"]) and "set on the device" in str(rec["describe_tick2"])
    assert not bool(rec["tick2_has_separation"])
    assert "deconflict must be a dict" in str(rec["refusal_keys"]) and "fleet must divide B" in str(rec["refusal_fleet"])
    assert "must be torch.int32" in str(rec["refusal_counts_dtype"]) and "must have shape" in str(rec["refusal_spheres_shape"])
    # the three calls through the C ABI on the plan the tick started from, on a handle of its own at the tick's horizon start
    cfg, _ = fc.torch_case()
    s = capi.from_config(cfg)
    s.set_horizon_start(1)
    got = dev_fleet(hip, s, rec["tick1_init"], B, K, **rule)
    same_bits(got, dict(summary=rec["tick1_separation"], nbr=rec["tick1_neighbours"], spheres=rec["tick1_spheres"], counts=rec["tick1_counts"]), "tick 1")
    assert device_set(hip, s, got["spheres"], got["counts"]) == 0
    traj, _, _ = solve_device(hip, s, rec["tick1_init"], None)
    assert traj.tobytes() == rec["tick1_traj"].tobytes()
    # the tick without deconflict afterwards still used the table: the bits of this handle, not those of one without it
    s.set_horizon_start(2)
    traj2, _, _ = solve_device(hip, s, rec["tick2_init"], None)
    assert traj2.tobytes() == rec["tick2_traj"].tobytes()
    bare = capi.from_config(cfg)
    bare.set_horizon_start(2)
    assert solve_device(hip, bare, rec["tick2_init"], None)[0].tobytes() != traj2.tobytes()
