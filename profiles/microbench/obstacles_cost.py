#!/usr/bin/env python3
"""What the spherical obstacles (qilqr_set_obstacles) cost: whole device-resident solves of configs[1]'s problems (N = 100) at
B = 1024 and 8192, three cases per size --
  default    the handle without obstacles (the tuned route: k_round where it applies)
  far        16 spheres that no trajectory reaches: the same solves to the bit, so the difference is the route (no k_round) and the
             obstacle loop of k_linearize's cost half
  on_paths   16 spheres on the paths (around the hover target at the origin and the starts): the solves themselves change
solves/s from the median of `reps` timed solves behind two untimed ones, and the mean iterations / backward passes per problem
(compare the time per backward pass too where the solves differ).
usage: PYTHONPATH=. python3 profiles/microbench/obstacles_cost.py [reps=5]"""
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
r = np.random.default_rng(16)
FAR = np.column_stack([r.uniform(-1, 1, (16, 3)) * 50.0 + np.array([500.0, 0.0, 0.0]), np.full(16, 2.0), np.full(16, 100.0)])
for B in (1024, 8192):
    cfg = pb.config2(B=B, N=100)
    # on the paths: four spheres around the hover target, twelve around knots of the starts
    starts = cfg["init"][r.integers(0, B, 12), r.integers(0, 100, 12), 1:4]
    centers = np.vstack([r.normal(size=(4, 3)) * 0.3, starts])
    ON = np.column_stack([centers, r.uniform(0.3, 0.8, 16), r.uniform(5.0, 50.0, 16)])
    init = torch.from_numpy(cfg["init"]).to(dev)
    bufs = (torch.empty_like(init), torch.empty(B, dtype=torch.float64, device=dev), [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)])
    for case, spheres in (("default", None), ("far", FAR), ("on_paths", ON)):
        s = capi.from_config(cfg, device=0)
        if spheres is not None:
            s.set_obstacles(spheres)
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
