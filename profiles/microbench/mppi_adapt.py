#!/usr/bin/env python3
"""Diagnostic: what the planner's adapted spread costs on the device, at section 8o's workload: 64 plans x 1024
samples x 100 knots, 8 shared spheres on the handle, explicit Euler.  Device time per call by HIP events on the solver's stream (warmed;
the median of `reps` windows of `inner` calls, with the windows' minimum and maximum), each new kernel against the kernel it was made
of, in the same run on the same build:
  1. k_mppi_flight against k_mppi_flight_spread (a spread that varies by plan, knot and rotor);
  2. k_mppi_update plus the nominal flight (qilqr_mppi_update_device) against k_mppi_adapt plus the nominal flight
     (qilqr_mppi_adapt_device).
usage (repository root): PYTHONPATH=. python3 profiles/microbench/mppi_adapt.py [reps=10] [inner=4] [out=profiles/mppi_adapt_microbench.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402

N, B, S = 100, 64, 1024
RULE = dict(sigma=0.5, lambda_=1000.0, tau_s=0.5, collision_cost=20.0, first_is_nominal=True)
ADAPT = dict(floor=0.05, cap=2.0, rate=0.5)


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


def verdict(name, new, old):
    ratio = float(np.median(new) / np.median(old))
    return f"  {name}: {np.median(new):.1f} us against {np.median(old):.1f} us, a factor {ratio:.3f}: " + (
        "within a tenth" if ratio <= 1.1 else "MORE than a tenth slower -- see make resources (occupancy, LDS)")


def main():
    reps, inner, out_path = 10, 4, os.path.join(ROOT, "profiles", "mppi_adapt_microbench.txt")
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
        elif k == "out":
            out_path = v
    if not torch.cuda.is_available():
        sys.exit("mppi_adapt.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pb.config2(B=B, N=N)
    s = capi.from_config(cfg, device=0)
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    rh = mpc.RecedingHorizon(s, B, N)
    plan = rh.start(cfg["init"][:B])["traj"]
    r = np.random.default_rng(7)
    path = plan.cpu().numpy()[:, :, 1:4].reshape(-1, 3)
    spheres = np.zeros((8, 5))
    spheres[:, :3] = path[r.integers(0, len(path), 8)] + 0.3 * (2.0 * r.random((8, 3)) - 1.0)
    spheres[:, 3], spheres[:, 4] = 0.15, 25.0
    s.set_obstacles(spheres)
    score, out_plan, info = new(B, S, capi.CL_SCORE), new(B, N, capi.KNOT), new(B, capi.MPPI_INFO)
    spread = torch.from_numpy(RULE["sigma"] * (0.6 + 0.9 * r.random((B, N, 4)))).to(dev)
    out_spread = new(B, N, 4)
    torch.cuda.synchronize()

    lines = [f"the planner's adapted spread, {B} plans x {S} samples x {N} knots (median of {reps} windows of {inner} calls; {torch.cuda.get_device_name(0)}):"]
    us_fly = time_calls(stream, lambda: s.mppi_flight_device(plan, score, 7, wait_current_stream=False, **RULE), reps, inner)
    lines.append(line("  k_mppi_flight                                         ", us_fly))
    us_up = time_calls(stream, lambda: s.mppi_update_device(plan, score, out_plan, info, 7, wait_current_stream=False, **RULE), reps, inner)
    lines.append(line("  k_mppi_update + the nominal flight (one call)         ", us_up))
    us_fly_s = time_calls(stream, lambda: s.mppi_flight_spread_device(plan, spread, score, 7, wait_current_stream=False, **RULE), reps, inner)
    lines.append(line("  k_mppi_flight_spread                                  ", us_fly_s))
    us_ad = time_calls(stream, lambda: s.mppi_adapt_device(plan, spread, score, out_plan, out_spread, info, 7, RULE["sigma"], RULE["lambda_"], ADAPT["floor"],
                                                           ADAPT["cap"], ADAPT["rate"], tau_s=RULE["tau_s"], collision_cost=RULE["collision_cost"],
                                                           first_is_nominal=True, wait_current_stream=False), reps, inner)
    lines.append(line("  k_mppi_adapt + the nominal flight (one call)          ", us_ad))
    lines.append(verdict("the flight with a spread", us_fly_s, us_fly))
    lines.append(verdict("the adaptation and the nominal flight", us_ad, us_up))
    torch.cuda.synchronize()
    i, sp = info.cpu().numpy(), out_spread.cpu().numpy()
    lines.append(f"  (info: J_min {i[:, 0].min():.4g} .. {i[:, 0].max():.4g}, effective samples {i[:, 2].min():.3g} .. {i[:, 2].max():.3g}, finite {int(i[:, 3].min())} .. "
                 f"{int(i[:, 3].max())} of {S}; new spread {sp.min():.3g} .. {sp.max():.3g} N)")
    text = "\n".join(lines)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
