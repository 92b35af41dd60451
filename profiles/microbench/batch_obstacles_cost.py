#!/usr/bin/env python3
"""What the per-problem, moving spheres (qilqr_set_batch_obstacles) cost: whole device-resident solves of configs[1]'s problems (N = 100) at
B = 1024 and 8192, four cases per size --
  default       the handle without obstacles (the tuned route: k_round where it applies)
  shared_far    16 shared spheres (qilqr_set_obstacles) that no trajectory reaches: the route without k_round, the LDS loop
  problem_far   16 per-problem spheres that no trajectory reaches: the same solves to the bit, so the difference against shared_far is
                the per-problem table's loads from L2 / HBM in k_linearize's cost half
  problem_paths 16 per-problem moving spheres, some timed to cross the problem's own start: the solves themselves change
solves/s from the median of `reps` timed solves behind two untimed ones, and the mean iterations / backward passes per problem.
usage: PYTHONPATH=. python3 profiles/microbench/batch_obstacles_cost.py [reps=5]"""
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
K = 16
FAR = np.column_stack([r.uniform(-1, 1, (K, 3)) * 50.0 + np.array([500.0, 0.0, 0.0]), np.full(K, 2.0), np.full(K, 100.0)])
for B in (1024, 8192):
    cfg = pb.config2(B=B, N=100)
    dt = cfg["dt"]
    far = np.zeros((B, K, 8))
    far[:, :, :3] = FAR[None, :, :3] + r.uniform(-1, 1, (B, K, 3))
    far[:, :, 3:6] = r.normal(size=(B, K, 3)) * 0.5
    far[:, :, 6:] = FAR[None, :, 3:]
    # on the paths: per problem, four spheres that cross its start at a random knot, twelve that move about the hover target
    on = np.zeros((B, K, 8))
    i0 = r.integers(0, 100, (B, 4))
    v = r.normal(size=(B, K, 3)) * 0.5
    at = cfg["init"][np.arange(B)[:, None], i0, 1:4] + r.normal(size=(B, 4, 3)) * 0.1
    on[:, :4, :3] = at - (i0 * dt)[..., None] * v[:, :4]
    on[:, 4:, :3] = r.normal(size=(B, K - 4, 3)) * 0.3
    on[:, :, 3:6] = v
    on[:, :, 6] = r.uniform(0.3, 0.8, (B, K))
    on[:, :, 7] = r.uniform(5.0, 50.0, (B, K))
    init = torch.from_numpy(cfg["init"]).to(dev)
    bufs = (torch.empty_like(init), torch.empty(B, dtype=torch.float64, device=dev), [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)])
    for case in ("default", "shared_far", "problem_far", "problem_paths"):
        s = capi.from_config(cfg, device=0)
        if case == "shared_far":
            s.set_obstacles(FAR)
        elif case == "problem_far":
            s.set_batch_obstacles(far)
        elif case == "problem_paths":
            s.set_batch_obstacles(on)
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
        print(f"B={B:5d} {case:13s}: {t * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f}) {B / t:9.0f} solves/s  iters {iters:6.2f}  backward passes "
              f"{n_bwd:6.2f}  status counts {status.tolist()}", flush=True)
        s.close()
