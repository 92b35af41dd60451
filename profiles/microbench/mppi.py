#!/usr/bin/env python3
"""Diagnostic: what the sampling planner costs on the device, at section 8l's workload: 64 plans x 1024 samples x
100 knots, 8 shared spheres on the handle.  Device time per call by HIP events on the solver's stream (warmed; the median of `reps`
windows of `inner` calls, with the windows' minimum and maximum), every yardstick in the same run on the same build:
  1. k_mppi_flight against the two-kernel route that stores what it draws in registers: k_sample_gusts (a row per knot) plus
     k_closed_loop_scored under those wrenches, at the same (B, S, n);
  2. k_mppi_update plus the nominal flight (one call: qilqr_mppi_update_device) against the flight they follow.
usage (repository root): PYTHONPATH=. python3 profiles/microbench/mppi.py [reps=10] [inner=4] [out=profiles/mppi_microbench.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402

N, B, S = 100, 64, 1024
GUST = dict(sigma=[1.0, 1.0, 1.0, 0.03, 0.03, 0.03], tau_force_s=0.5, tau_torque_s=0.2)
RULE = dict(sigma=0.5, lambda_=1000.0, tau_s=0.5, collision_cost=20.0, first_is_nominal=True)


def time_calls(stream, call, reps, inner):
    for _ in range(3):  # code object loaded, clocks out of idle
        call()
    stream.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            call()
        e1.record(stream)
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / inner)
    return np.array(us)


def line(tag, us):
    return f"{tag}: {np.median(us):9.1f} us per call (min {us.min():.1f} - max {us.max():.1f})"


def main():
    reps, inner, out_path = 10, 4, os.path.join(ROOT, "profiles", "mppi_microbench.txt")
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
        elif k == "out":
            out_path = v
    if not torch.cuda.is_available():
        sys.exit("mppi.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pb.config2(B=B, N=N)
    s = capi.from_config(cfg, device=0)
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    rh = mpc.RecedingHorizon(s, B, N)
    plan = rh.start(cfg["init"][:B], gains=True)["traj"]
    r = np.random.default_rng(7)
    path = plan.cpu().numpy()[:, :, 1:4].reshape(-1, 3)
    spheres = np.zeros((8, 5))
    spheres[:, :3] = path[r.integers(0, len(path), 8)] + 0.3 * (2.0 * r.random((8, 3)) - 1.0)
    spheres[:, 3], spheres[:, 4] = 0.15, 25.0
    s.set_obstacles(spheres)
    wrench, x0 = new(B, S, N, capi.WRENCH), plan[:, None, 0, 1:14].repeat(1, S, 1).contiguous()
    score, out_plan, info = new(B, S, capi.CL_SCORE), new(B, N, capi.KNOT), new(B, capi.MPPI_INFO)
    torch.cuda.synchronize()

    lines = [f"the sampling planner, {B} plans x {S} samples x {N} knots (median of {reps} windows of {inner} calls; {torch.cuda.get_device_name(0)}):"]
    us_gust = time_calls(stream, lambda: s.sample_gusts_device(wrench, 7, GUST["sigma"], tau_force_s=0.5, tau_torque_s=0.2, wait_current_stream=False), reps, inner)
    lines.append(line("  k_sample_gusts, correlated, a row per knot            ", us_gust))
    us_cl = time_calls(stream, lambda: s.closed_loop_device(plan, rh.gains, x0, wrench=wrench, out_score=score, wait_current_stream=False), reps, inner)
    lines.append(line("  k_closed_loop_scored under those wrenches             ", us_cl))
    us_fly = time_calls(stream, lambda: s.mppi_flight_device(plan, score, 7, wait_current_stream=False, **RULE), reps, inner)
    lines.append(line("  k_mppi_flight                                         ", us_fly))
    us_up = time_calls(stream, lambda: s.mppi_update_device(plan, score, out_plan, info, 7, wait_current_stream=False, **RULE), reps, inner)
    lines.append(line("  k_mppi_update + the nominal flight (one call)         ", us_up))
    one = new(B, 1, capi.CL_SCORE)
    us_one = time_calls(stream, lambda: s.mppi_flight_device(out_plan, one, 7, wait_current_stream=False, **dict(RULE, sigma=0.0)), reps, inner)
    lines.append(line("  k_mppi_flight at S = 1 (the nominal flight's grid)    ", us_one))
    two = float(np.median(us_gust) + np.median(us_cl))
    spread = float((us_fly.max() - us_fly.min()) + (us_gust.max() - us_gust.min()) + (us_cl.max() - us_cl.min()))
    lines.append(f"  the fused flight {np.median(us_fly):.1f} us against the two-kernel route {two:.1f} us (the windows' spread: {spread:.1f} us): "
                 + ("not longer" if np.median(us_fly) <= two + spread else "LONGER -- see make resources and the counters"))
    lines.append(f"  the update and the nominal flight {np.median(us_up):.1f} us against the {np.median(us_fly):.1f} us flight they follow: "
                 + ("below it" if np.median(us_up) < np.median(us_fly) else "NOT below it"))
    torch.cuda.synchronize()
    i = info.cpu().numpy()
    lines.append(f"  (info: J_min {i[:, 0].min():.4g} .. {i[:, 0].max():.4g}, effective samples {i[:, 2].min():.3g} .. {i[:, 2].max():.3g}, finite {int(i[:, 3].min())} .. "
                 f"{int(i[:, 3].max())} of {S}, nominal cost {i[:, 4].min():.4g} .. {i[:, 4].max():.4g})")
    text = "\n".join(lines)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
