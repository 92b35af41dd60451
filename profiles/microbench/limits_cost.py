#!/usr/bin/env python3
"""What the per-rotor thrust limits (qilqr_set_control_limits) cost: whole device-resident solves of configs[1]'s problems (N = 100)
at B = 1024 and 8192, three cases per size --
  default   the handle without limits (the tuned route: k_round / k_backward4 / k_rollout16 ...)
  box_inf   the box route with limits -inf .. +inf (k_backward<true> box form + k_rollout; no bound is ever active)
  box_demo  the box route with the demo's limits 0 .. 9.81 N per rotor (bounds active: the solves themselves change)
solves/s from the median of `reps` timed solves behind two untimed ones, and the mean iterations / backward passes per problem
(the limited solves are other solves: compare their time per backward pass too).
usage: PYTHONPATH=. python3 profiles/microbench/limits_cost.py [reps=5]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402

kw = dict(a.split("=") for a in sys.argv[1:])
reps = int(kw.get("reps", 5))
dev = torch.device("cuda", 0)
for B in (1024, 8192):
    cfg = pb.config2(B=B, N=100)
    init = torch.from_numpy(cfg["init"]).to(dev)
    bufs = (torch.empty_like(init), torch.empty(B, dtype=torch.float64, device=dev), [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)])
    for case, limits in (("default", None), ("box_inf", (-np.inf, np.inf)), ("box_demo", (0.0, 9.81))):
        s = capi.from_config(cfg, device=0)
        if limits:
            s.set_control_limits(*limits)
        for _ in range(2):
            s.solve_batch_device(init, bufs[0], bufs[1], *bufs[2])
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s.solve_batch_device(init, bufs[0], bufs[1], *bufs[2])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = float(np.median(ts))
        iters, n_bwd = bufs[2][1].double().mean().item(), bufs[2][2].double().mean().item()
        status = np.bincount(bufs[2][0].cpu().numpy(), minlength=5)
        print(f"B={B:5d} {case:9s}: {t * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f}) {B / t:9.0f} solves/s  iters {iters:6.2f}  backward passes {n_bwd:6.2f}"
              f"  status counts {status.tolist()}", flush=True)
        s.close()
