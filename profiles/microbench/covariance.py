#!/usr/bin/env python3
"""Diagnostic: what the linear covariance analysis costs on the device, at section 8l's workload: 64 plans x 100
knots, 8 shared spheres on the handle, explicit Euler and Runge-Kutta.  Device time per call by HIP events on the solver's stream (warmed;
the median of `reps` windows of `inner` calls, with the windows' minimum and maximum), and in the same run on the same build the sampled
route it screens for: k_sample_gusts + k_closed_loop_scored + k_reduce_scores at S = 1024.
usage (repository root): PYTHONPATH=. python3 profiles/microbench/covariance.py [reps=10] [inner=4] [out=profiles/covariance_microbench.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402

N, B, S = 100, 64, 1024
GUST = dict(sigma=[1.0, 1.0, 1.0, 0.03, 0.03, 0.03], tau_force_s=0.5, tau_torque_s=0.2)
SIGMA12 = [0.05] * 3 + [0.03] * 3 + [0.1] * 3 + [0.05] * 3


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
    reps, inner, out_path = 10, 4, os.path.join(ROOT, "profiles", "covariance_microbench.txt")
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
        elif k == "out":
            out_path = v
    if not torch.cuda.is_available():
        sys.exit("covariance.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    lines = [f"linear covariance analysis, {B} plans x {N} knots, 8 shared spheres (median of {reps} windows of {inner} calls; {torch.cuda.get_device_name(0)}):"]
    for integrator, name in ((0, "Euler"), (1, "Runge-Kutta")):
        cfg = pb.config2(B=B, N=N)
        s = capi.from_config(cfg, device=0)
        s.set_integrator(integrator)
        stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
        rh = mpc.RecedingHorizon(s, B, N)
        plan = rh.start(cfg["init"][:B], gains=True)["traj"]
        r = np.random.default_rng(7)
        path = plan.cpu().numpy()[:, :, 1:4].reshape(-1, 3)
        spheres = np.zeros((8, 5))
        spheres[:, :3] = path[r.integers(0, len(path), 8)] + 0.3 * (2.0 * r.random((8, 3)) - 1.0)
        spheres[:, 3], spheres[:, 4] = 0.15, 25.0
        s.set_obstacles(spheres)
        cov, mean, summary = new(B, N, capi.COV), new(B, N, 12), new(B, capi.COV_SUMMARY)
        kw = dict(gust=GUST, wait_current_stream=False)
        us_all = time_calls(stream, lambda: s.covariance_device(plan, rh.gains, SIGMA12, cov=cov, mean=mean, summary=summary, **kw), reps, inner)
        us_sum = time_calls(stream, lambda: s.covariance_device(plan, rh.gains, SIGMA12, summary=summary, **kw), reps, inner)
        us_cov = time_calls(stream, lambda: s.covariance_device(plan, rh.gains, SIGMA12, cov=cov, **kw), reps, inner)
        us_one = time_calls(stream, lambda: s.covariance_device(plan, rh.gains, SIGMA12, cov=cov, i0=0, i1=1, **kw), reps, inner)
        lines.append(f" {name}:")
        lines.append(line("  qilqr_covariance_device, cov + mean + summary (3 launches)", us_all))
        lines.append(line("  ... the summary alone (3 launches, Sigma to scratch)      ", us_sum))
        lines.append(line("  ... the covariances alone (build + chain, 2 launches)     ", us_cov))
        lines.append(line("  ... the covariances of a window of one step (2 launches)  ", us_one))
        per_knot = (np.median(us_cov) - np.median(us_one)) / (N - 2)
        lines.append(f"  the chain: ({np.median(us_cov):.1f} - {np.median(us_one):.1f}) us / {N - 2} further knots = {per_knot:.3f} us per knot;"
                     f" the whole call {np.median(us_all) / (N - 1):.3f} us per knot")
        wrench, x0 = new(B, S, N, capi.WRENCH), plan[:, None, 0, 1:14].repeat(1, S, 1).contiguous()
        score, msum = new(B, S, capi.CL_SCORE), new(B, capi.MC_SUMMARY)
        us_g = time_calls(stream, lambda: s.sample_gusts_device(wrench, 7, GUST["sigma"], tau_force_s=0.5, tau_torque_s=0.2, wait_current_stream=False), reps, inner)
        us_f = time_calls(stream, lambda: s.closed_loop_device(plan, rh.gains, x0, wrench=wrench, out_score=score, wait_current_stream=False), reps, inner)
        us_r = time_calls(stream, lambda: s.reduce_scores_device(score, msum, wait_current_stream=False), reps, inner)
        lines.append(line(f"  k_sample_gusts at S = {S}                                 ", us_g))
        lines.append(line(f"  k_closed_loop_scored at S = {S}                           ", us_f))
        lines.append(line(f"  k_reduce_scores at S = {S}                                ", us_r))
        route = float(np.median(us_g) + np.median(us_f) + np.median(us_r))
        lines.append(f"  the analysis {np.median(us_all):.1f} us against the sampled route {route:.1f} us: "
                     + (f"{route / np.median(us_all):.1f} times shorter" if np.median(us_all) < route else "NOT below it"))
        torch.cuda.synchronize()
        w = summary.cpu().numpy()
        lines.append(f"  (summary: max sqrt(tr P) {w[:, 0].min():.4g} .. {w[:, 0].max():.4g} m, smallest z {w[:, 4].min():.4g} .. {w[:, 4].max():.4g},"
                     f" largest control deviation {w[:, 7].min():.4g} .. {w[:, 7].max():.4g} N)")
        s.close()
    text = "\n".join(lines)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
