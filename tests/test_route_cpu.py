"""The kernel choices of a call (quadrotorilqr_amd/csrc/route.h), built for the host with g++ and checked against
tests/golden/routes.json: the choices the code made before they were gathered into plan_route, recorded over handles with each
extension alone and combined, the mixed mode, general weights, the Runge-Kutta extension, the device configuration's A/B fields, the
call's own facts and batch sizes from 1 to 65536, with the run-time choices at a few live counts.  The rule that says which k_linearize
instantiations exist (lin_instantiated) is checked against tests/golden/linearize_keys.json: the 58 keys of the hand-written dispatch it
replaced, extracted from that dispatch's case lines."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROUTE_H = os.path.join(HERE, "..", "quadrotorilqr_amd", "csrc", "route.h")


@pytest.fixture(scope="module")
def hr():
    so = os.path.join(HERE, "libhost_route_harness.so")
    src = os.path.join(HERE, "host_route_harness.cpp")
    deps = [src, ROUTE_H, os.path.join(HERE, "..", "include", "quadrotor_ilqr.h")]
    if not os.path.exists(so) or any(os.path.getmtime(so) < os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hr_route.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.hr_lin_keys.argtypes = [C.POINTER(C.c_long), C.c_int]
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "routes.json")) as f:
        return json.load(f)


def test_route_h_needs_no_hip():
    with open(ROUTE_H) as f:
        includes = [line for line in f if line.startswith("#include")]
    assert includes and not any("hip" in line for line in includes), includes


def test_every_recorded_choice(hr, golden):
    n_in, n_out = len(golden["inputs"]), len(golden["outputs"])
    rows = np.array(golden["rows"], dtype=np.int64)
    assert rows.shape[1] == n_in + n_out and len(rows) >= 200
    out = np.zeros(n_out, dtype=np.int64)
    bad = []
    for row in rows:
        inp = np.ascontiguousarray(row[:n_in])
        assert hr.hr_route(inp.ctypes.data_as(C.POINTER(C.c_long)), out.ctypes.data_as(C.POINTER(C.c_long))) == n_out
        diff = [(name, int(want), int(got)) for name, want, got in zip(golden["outputs"], row[n_in:], out) if want != got]
        if diff:
            bad.append((dict(zip(golden["inputs"], map(int, inp))), diff))
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; first: {bad[:3]}"


def test_the_grid_covers_what_it_claims(golden):
    cols = {name: i for i, name in enumerate(golden["inputs"])}
    rows = np.array(golden["rows"], dtype=np.int64)
    seen = lambda name: set(rows[:, cols[name]].tolist())  # noqa: E731
    assert {1, 64, 1024, 1025, 2048, 4096, 4097, 8192, 65536} <= seen("B")
    assert {0, 1, 2, 5, 7, 8} <= seen("force_general")
    assert {0, 1, 2, 3} <= seen("single_wave_rollout") and {0, 1} <= seen("round_launch")
    assert {-1, 0, 1} <= seen("compaction") and {0, 2, 4} <= seen("streams")
    ext = set(map(tuple, rows[:, [cols["limited"], cols["modeled"], cols["obstacles"]]].tolist()))
    assert ext == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert {0, 1} <= seen("f32") and {0, 1} <= seen("integrator")
    for fact in ("desired_batch", "cost_hist", "early_out"):
        assert 1 in seen(fact)
    assert 0 in seen("iterates")


def test_two_streams_at_1024_run_without_compaction(hr, golden):
    """The combined launch is not taken on sub-batch streams, and the compaction stays off for a batch whose kernels it stands for."""
    row = dict.fromkeys(golden["inputs"], 0)
    row.update(symmetric=1, q_symmetric=1, ur_zero=1, q_diag=1, streams=2, sync_every=2, B=1024, hw_queues=4, iterates=1)
    inp = np.array([row[k] for k in golden["inputs"]], dtype=np.int64)
    out = np.zeros(len(golden["outputs"]), dtype=np.int64)
    hr.hr_route(inp.ctypes.data_as(C.POINTER(C.c_long)), out.ctypes.data_as(C.POINTER(C.c_long)))
    got = dict(zip(golden["outputs"], out.tolist()))
    assert got["combined"] == 1 and got["parts"] == 2 and got["compact"] == 0 and got["tail_kinds"] == 0


def test_linearize_instantiations_are_the_recorded_ones(hr):
    """lin_instantiated admits exactly the recorded keys over the whole key space (4 kinds x 2 integrators x 2 placements x 2 precisions
    x 8 extension forms): an instantiation added or lost by a change of the rule shows here, by name."""
    with open(os.path.join(HERE, "golden", "linearize_keys.json")) as f:
        want = json.load(f)
    assert want["columns"] == ["lin_kind", "integrator", "tiled", "f32", "ext"] and len(want["rows"]) == 58
    out = np.zeros((256, 5), dtype=np.int64)
    n = hr.hr_lin_keys(out.ctypes.data_as(C.POINTER(C.c_long)), len(out))
    assert 0 <= n <= len(out), n
    got, exp = set(map(tuple, out[:n].tolist())), set(map(tuple, want["rows"]))
    assert len(exp) == 58
    assert got == exp, {"admitted but not recorded": sorted(got - exp), "recorded but not admitted": sorted(exp - got)}
