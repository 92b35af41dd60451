#!/usr/bin/env python3
"""What a state-weight schedule (qilqr_set_state_weight_schedule) costs: whole device-resident solves of configs[1]'s problems
(N = 100) at B = 1024 and 8192, four cases per size --
  default    the handle without a schedule (the tuned route: k_round / k_backward4)
  one_wave   force_general = 2 without a schedule: the backward kernel a scheduled handle takes (k_backward<true>, a wavefront per
             trajectory, three launches per round), on the symmetric, diagonal-kind records of the handle's Q
  constant   the schedule Qs[i] = Q_DEMO: the same problems as the two above (the iterations differ in rounding at most), so against
             one_wave the difference is the dense record of kind 0 (216 doubles a knot) and the schedule's fill of Q
  terminal   0.01 Q_DEMO with 10 Q_DEMO at the last knot: what the feature is for; the solves themselves change
solves/s from the median of `reps` timed solves behind two untimed ones, and the mean iterations / backward passes per problem
(compare the time per backward pass where the solves differ).
usage: PYTHONPATH=. python3 profiles/microbench/schedule_cost.py [reps=5]"""
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
N = 100
dev = torch.device("cuda", 0)
CASES = (("default", {}, None), ("one_wave", dict(force_general=2), None),
         ("constant", {}, pb.terminal_schedule(pb.Q_DEMO, pb.Q_DEMO, N)),
         ("terminal", {}, pb.terminal_schedule(0.01 * pb.Q_DEMO, 10.0 * pb.Q_DEMO, N)))
for B in (1024, 8192):
    cfg = pb.config2(B=B, N=N)
    init = torch.from_numpy(cfg["init"]).to(dev)
    bufs = (torch.empty_like(init), torch.empty(B, dtype=torch.float64, device=dev), [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4)])
    for case, handle_kw, Qs in CASES:
        s = capi.from_config(cfg, device=0, **handle_kw)
        if Qs is not None:
            s.set_state_weight_schedule(Qs)
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
              f"  us per problem and backward pass {t * 1e6 / B / max(n_bwd, 1e-9):7.3f}  status counts {status.tolist()}", flush=True)
        s.close()
