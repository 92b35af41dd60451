#!/usr/bin/env python3
"""Diagnostic: what a receding-horizon tick costs.
  1. device time of the shift (k_shift, one launch) by HIP events on the solver's stream: steps = 1 and 5, n = 100, B = 1024 and 8192
     (configs[1]'s problems and eight times as many), with the bytes it moves over that time;
  2. a warm tick (horizon start, shift, solve from the shifted plan) against a cold solve from the same measured state (the desired
     trajectory with knot 0 replaced), on the same build, at B = 1024: host ms around a drained solve, and mean iterations.
usage (repository root): PYTHONPATH=. python3 profiles/microbench/mpc_tick.py [reps=20] [ticks=8]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402


def shift_times(B, n, steps, reps, inner=50):
    cfg = pb.config2(B=B, N=n)
    s = capi.from_config(cfg, device=0)
    dev = torch.device("cuda", 0)
    plan = torch.from_numpy(s.solve_batch(cfg["init"])["traj"]).to(dev)
    out = torch.empty_like(plan)
    x0 = plan[:, steps, 1:14].contiguous()
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    torch.cuda.synchronize()
    rows = []
    for anchored in (False, True):
        for _ in range(5):  # code object loaded, clocks out of idle
            s.shift_device(plan, out, x0=x0 if anchored else None, steps=steps, wait_current_stream=False)
        stream.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(inner):
                s.shift_device(plan, out, x0=x0 if anchored else None, steps=steps, wait_current_stream=False)
            e1.record(stream)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / inner)
        us = np.array(us)
        moved = 2 * 8 * 18 * B * n  # bytes read + written (the tail reads one knot and writes `steps` of them: inside the same count)
        rows.append((anchored, float(np.median(us)), float(us.min()), float(us.max()), moved / np.median(us) / 1e3))
    return rows


def warm_against_cold(B, n, ticks, reps):
    mission = n + ticks
    cfg = pb.config2(B=B, N=mission)  # (the hover mission: every window of it is the same desired trajectory)
    dev = torch.device("cuda", 0)
    s = capi.from_config(cfg, device=0)
    rh = mpc.RecedingHorizon(s, B, n)
    res = rh.start(cfg["init"][:, :n])
    cold_s = capi.from_config(cfg, device=0)
    cold_out = [torch.empty((B, n, 18), dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.float64, device=dev)] + \
               [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)]
    desired = torch.from_numpy(cfg["desired"]).to(dev)
    warm_ms, cold_ms, warm_it, cold_it = [], [], [], []
    for tick in range(1, ticks + 1):
        x0 = res["traj"][:, 1, 1:14].contiguous()  # the perfect plant
        cold = desired[tick:tick + n].unsqueeze(0).repeat(B, 1, 1).contiguous()
        cold[:, 0, 1:14] = x0
        cold_s.set_horizon_start(tick)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = rh.tick(x0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        cold_s.solve_batch_device(cold, *cold_out)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        warm_ms.append((t1 - t0) * 1e3)
        cold_ms.append((t2 - t1) * 1e3)
        warm_it.append(float(res["iters"].double().mean()))
        cold_it.append(float(cold_out[3].double().mean()))
        rel = float(((res["cost"] - cold_out[1]).abs() / cold_out[1].abs()).max())
        print(f"  tick {tick}: warm {warm_ms[-1]:7.3f} ms, {warm_it[-1]:5.2f} iterations | cold {cold_ms[-1]:7.3f} ms, {cold_it[-1]:5.2f} iterations | "
              f"max rel cost difference {rel:.1e}")
    return np.array(warm_ms), np.array(cold_ms), np.array(warm_it), np.array(cold_it)


def main():
    reps, ticks = 20, 8
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "ticks":
            ticks = int(v)
    if not torch.cuda.is_available():
        sys.exit("mpc_tick.py measures on the GPU: no device, no number")
    n = 100
    for B in (1024, 8192):
        for steps in (1, 5):
            for anchored, med, lo, hi, gbs in shift_times(B, n, steps, reps):
                print(f"k_shift B={B} n={n} steps={steps} x0={'yes' if anchored else 'no '}: {med:7.2f} us per launch (min {lo:.2f}, max {hi:.2f}), "
                      f"{gbs:7.1f} GB/s read + written")
    print(f"warm tick against cold solve, B=1024 n={n}, {ticks} ticks of one knot, perfect plant:")
    w, c, wi, ci = warm_against_cold(1024, n, ticks, reps)
    print(f"warm tick (start + shift + solve): median {np.median(w):.3f} ms (min {w.min():.3f}, max {w.max():.3f}), mean iterations {wi.mean():.2f}")
    print(f"cold solve from the same state:    median {np.median(c):.3f} ms (min {c.min():.3f}, max {c.max():.3f}), mean iterations {ci.mean():.2f}")


if __name__ == "__main__":
    main()
