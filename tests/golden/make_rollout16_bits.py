#!/usr/bin/env python3
"""Records tests/golden/rollout16_bits.npz: what the rollout of the commit BEFORE a change of its step writes, bit for bit
(tests/test_gpu_rollout_same_bits.py compares the working tree's library with it).  Needs a GPU.

The library is named by QILQR_LIB and by nothing else -- a build of the commit the fixture is to stand for, never the working tree's by
default -- and that commit is an argument, stored in the fixture:
    QILQR_LIB=/path/to/parent/libquadrotor_ilqr.so python3 tests/golden/make_rollout16_bits.py <commit> [output.npz]"""
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
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "rollout16_bits.npz")
    from quadrotorilqr_amd import capi  # (binds QILQR_LIB when it is imported)
    from tests import rollout16_bits_cases as rc
    assert os.path.samefile(capi.LIB_PATH, lib), (capi.LIB_PATH, lib)
    fix = {"commit": np.array(commit), "library": np.array(os.path.basename(lib))}
    for cid, prec, n, kinds, alpha in rc.cases():
        out, dg = rc.rollout(capi, prec, n, kinds, alpha)
        assert np.isfinite(out).all(), cid
        # (fp32 storage: every value the kernel stores is a float, so float32 keeps its bits)
        fix["out:" + cid] = out.astype(np.float32) if prec == "f32" else out
        assert np.array_equal(fix["out:" + cid].astype(np.float64), out), cid
        fix["in:" + cid] = dg
    for rounds in (0, 1):
        out, text = rc.solve(capi, rounds)
        assert "k_round" in text, text
        for k in rc.SOLVE_KEYS:
            fix[f"solve{rounds}:{k}"] = out[k]
    np.savez_compressed(path, **fix)
    print(f"recorded {len(rc.cases())} rollouts and 2 solves of commit {commit} with {lib} -> {path} ({os.path.getsize(path)} bytes)")
    print("solve: status", fix["solve0:status"], "iters", fix["solve0:iters"], "n_fwd", fix["solve0:n_fwd"])


if __name__ == "__main__":
    main()
