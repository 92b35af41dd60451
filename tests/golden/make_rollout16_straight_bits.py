#!/usr/bin/env python3
"""Records tests/golden/rollout16_straight_bits.npz: what the rollout of the commit BEFORE the step's knot loop got its steady state writes,
bit for bit (tests/test_gpu_rollout_straight_bits.py compares the working tree's library with it).  Needs a GPU.

The library is named by QILQR_LIB and by nothing else -- a build of the commit the fixture is to stand for, never the working tree's by
default -- and that commit is an argument, stored in the fixture:
    QILQR_LIB=/path/to/parent/libquadrotor_ilqr.so python3 tests/golden/make_rollout16_straight_bits.py <commit> [output.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    lib = os.environ.get("QILQR_LIB")
    if not lib or len(sys.argv) < 2:
        sys.exit(__doc__)
    commit = sys.argv[1]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "rollout16_straight_bits.npz")
    from quadrotorilqr_amd import capi  # (binds QILQR_LIB when it is imported)
    from tests import rollout16_straight_cases as sc
    assert os.path.samefile(capi.LIB_PATH, lib), (capi.LIB_PATH, lib)
    fix = {"commit": np.array(commit), "library": np.array(os.path.basename(lib))}
    for cid, prec, n, kinds, alpha in sc.cases():
        out, dg = sc.rollout(capi, prec, n, kinds, alpha)
        assert np.isfinite(out).all(), cid
        if prec == "f64":  # (fp32 storage rounds the nominal quaternions: Log renormalises at every knot there)
            traj, _ = sc.inputs(n, kinds)
            for r, kind in enumerate(kinds):
                sc.check_row(kind, n, traj[r], out[r])
        # (fp32 storage: every value the kernel stores is a float, so float32 keeps its bits)
        fix["out:" + cid] = out.astype(np.float32) if prec == "f32" else out
        assert np.array_equal(fix["out:" + cid].astype(np.float64), out), cid
        fix["in:" + cid] = dg
    np.savez_compressed(path, **fix)
    print(f"recorded {len(sc.cases())} rollouts of commit {commit} with {lib} -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
