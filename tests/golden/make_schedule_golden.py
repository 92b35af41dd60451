"""Writes tests/golden/schedule_solves.npz: the NumPy restatement's solves (tests/schedule_numpy_ilqr.py, the symmetrised recursion) of
the inputs of tests/schedule_cases.py -- problems 0-2 of config2(B=6, N, seed=7) for N in {12, 24, 40} under the terminal, waypoint and
dense state-weight schedules -- so that the GPU tests need not spend a minute and a half recomputing them.  tests/test_schedule_cpu.py
recomputes every one and compares.  Run from the repository root: python -m tests.golden.make_schedule_golden"""
import numpy as np

from tests import schedule_cases as sc


def main():
    out = {}
    for N in sc.SIZES:
        for kind in sc.KINDS:
            for b in sc.PROBLEMS:
                r, key = sc.compute(N, kind, b, 1), f"{kind}_{N}_{b}"
                out[key + "_traj"] = r["traj"]
                out[key + "_cost"] = np.float64(r["cost"])
                out[key + "_hist"] = r["cost_hist"]
                out[key + "_counts"] = np.array([r[k] for k in sc.COUNTS], dtype=np.int64)
    np.savez_compressed(sc.GOLDEN, **out)


if __name__ == "__main__":
    main()
