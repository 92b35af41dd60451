#!/usr/bin/env python3
"""What per-problem models (qilqr_set_batch_models) cost: whole device-resident solves of configs[1]'s problems (N = 100) at B = 1024
and 8192, four cases per size --
  default     the handle without models (the tuned route: k_round / k_backward4 / k_rollout16 ...)
  general     the general route with the handle's one model (force_general = 2, single_wave_rollout = 1: k_backward<true>, k_rollout,
              k_linearize on plain records)
  models_same the models route with B copies of the handle's model (the same solves, bit for bit, as `general`: the table's own cost)
  models      the models route with B distinct models (mass, inertia, arm, torque ratio within 5 % of model A: the solves change a
              little -- compare the time per backward pass too)
solves/s from the median of `reps` timed solves behind two untimed ones, and the mean iterations / backward passes per problem.
usage: PYTHONPATH=. python3 profiles/microbench/models_cost.py [reps=5]"""
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
    r = np.random.default_rng(B)
    f = lambda: r.uniform(0.95, 1.05, B)
    m = cfg["model"]
    inertia = np.eye(3)[None] * f()[:, None, None]
    distinct = dict(mass_kg=m["mass_kg"] * f(), inertia=inertia, arm_length_m=m["arm_length_m"] * f(),
                    torque_to_thrust_ratio_m=m["torque_to_thrust_ratio_m"] * f(), g_mpss=m["g_mpss"])
    init = torch.from_numpy(cfg["init"]).to(dev)
    bufs = (torch.empty_like(init), torch.empty(B, dtype=torch.float64, device=dev), [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)])
    for case, general, models in (("default", False, None), ("general", True, None), ("models_same", False, m), ("models", False, distinct)):
        s = capi.from_config(cfg, device=0, **(dict(force_general=2, single_wave_rollout=1) if general else {}))
        if models is not None:
            s.set_models(models if models is distinct else dict(models, mass_kg=np.full(B, m["mass_kg"])))
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
        print(f"B={B:5d} {case:11s}: {t * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f}) {B / t:9.0f} solves/s  iters {iters:6.2f}  backward passes {n_bwd:6.2f}"
              f"  per backward pass {t * 1e6 / max(n_bwd, 1e-9):8.1f} us  status counts {status.tolist()}", flush=True)
        s.close()
