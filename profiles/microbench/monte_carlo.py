#!/usr/bin/env python3
"""Diagnostic: what the ends of the Monte-Carlo loop cost on the device, at section 8k's workload: 64 plans x
1024 samples x 100 knots, a gust per knot, 8 shared spheres on the handle, no trajectories.
  1. k_sample_gusts (white and correlated, and one row per flight), k_sample_states and k_reduce_scores: device time per launch by HIP
     events on the solver's stream (warmed; `reps` windows of `inner` launches), and the bytes per second the gust kernel writes against
     the 6.3 TB/s a streaming kernel reaches on this part (8.0 TB/s on paper);
  2. the scored flight they feed, and the whole of RecedingHorizon.evaluate_sampled: by events, and wall clock to the summary on the host;
  3. the parent's way in the same run: problems.gust_wrenches on the host plus RecedingHorizon.evaluate(x0, wrench) fed host arrays, wall
     clock to the scores on the host (the reduction to a summary, in NumPy, is not counted).
usage (repository root): PYTHONPATH=. python3 profiles/microbench/monte_carlo.py [reps=10] [inner=4] [baseline=1] [only=gusts]
(only=gusts: the correlated gust kernel alone, 20 launches and nothing else -- what a counter run profiles)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402

N, B, S = 100, 64, 1024
GUST = dict(sigma=[1.0, 1.0, 1.0, 0.03, 0.03, 0.03], tau_force_s=0.5, tau_torque_s=0.2)
SIGMA12 = [0.1] * 3 + [0.05] * 3 + [0.1] * 6
HBM_MEASURED, HBM_PAPER = 6.3e12, 8.0e12


def time_launches(stream, call, reps, inner):
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


def line(tag, us, extra=""):
    return f"{tag}: {np.median(us):9.1f} us per launch (min {us.min():.1f}, max {us.max():.1f}){extra}"


def main():
    reps, inner, baseline, only = 10, 4, 1, ""
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
        elif k == "baseline":
            baseline = int(v)
        elif k == "only":
            only = v
    if not torch.cuda.is_available():
        sys.exit("monte_carlo.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pb.config2(B=B, N=N)
    s = capi.from_config(cfg, device=0)
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    wrench = new(B, S, N, capi.WRENCH)
    torch.cuda.synchronize()
    gusts = lambda out, **kw: (lambda: s.sample_gusts_device(out, 7, GUST["sigma"], wait_current_stream=False, **kw))
    if only == "gusts":
        for _ in range(20):
            gusts(wrench, tau_force_s=0.5, tau_torque_s=0.2)()
        stream.synchronize()
        return

    rh = mpc.RecedingHorizon(s, B, N)
    res = rh.start(cfg["init"][:B], gains=True)
    plan = res["traj"]
    r = np.random.default_rng(7)
    path = plan.cpu().numpy()[:, :, 1:4].reshape(-1, 3)
    spheres = np.zeros((8, 5))
    spheres[:, :3] = path[r.integers(0, len(path), 8)] + 0.3 * (2.0 * r.random((8, 3)) - 1.0)
    spheres[:, 3], spheres[:, 4] = 0.15, 25.0
    s.set_obstacles(spheres)
    x_nom = plan[:, 0, 1:14].contiguous()
    x0, wrench1 = new(B, S, capi.STATE), new(B, S, 1, capi.WRENCH)
    stats, score, summary = new(B, S, capi.CL_STATS), new(B, S, capi.CL_SCORE), new(B, capi.MC_SUMMARY)
    torch.cuda.synchronize()

    print(f"the Monte-Carlo kernels, {B} plans x {S} samples x {N} knots (median of {reps} windows of {inner} launches):")
    nbytes = wrench.numel() * 8
    rate = lambda us: f", {nbytes / 1e6:.0f} MB written at {nbytes / np.median(us) / 1e6:.2f} TB/s = {nbytes / np.median(us) * 1e6 / HBM_MEASURED:.2f} of the measured HBM rate, {nbytes / np.median(us) * 1e6 / HBM_PAPER:.2f} of the paper one"
    us_white = time_launches(stream, gusts(wrench), reps, inner)
    print(line("  k_sample_gusts, white, a row per knot      ", us_white, rate(us_white)))
    us_corr = time_launches(stream, gusts(wrench, tau_force_s=0.5, tau_torque_s=0.2), reps, inner)
    print(line("  k_sample_gusts, correlated, a row per knot ", us_corr, rate(us_corr)))
    us_one = time_launches(stream, gusts(wrench1), reps, inner)
    print(line("  k_sample_gusts, one row per flight         ", us_one))
    us_states = time_launches(stream, lambda: s.sample_states_device(x_nom, x0, 7, SIGMA12, first_is_nominal=True, wait_current_stream=False), reps, inner)
    print(line("  k_sample_states                            ", us_states))
    fly = lambda: s.closed_loop_device(plan, rh.gains, x0, out_stats=stats, wrench=wrench, out_score=score, wait_current_stream=False)
    us_fly = time_launches(stream, fly, reps, inner)
    print(line("  k_closed_loop_scored on what they sampled  ", us_fly))
    us_red = time_launches(stream, lambda: s.reduce_scores_device(score, summary, wait_current_stream=False), reps, inner)
    print(line("  k_reduce_scores                            ", us_red))
    sampling = float(np.median(us_corr) + np.median(us_states))
    print(f"  sampling (correlated gusts + states) {sampling:.1f} us against the {np.median(us_fly):.1f} us flight it feeds: "
          + ("below it" if sampling <= np.median(us_fly) else "ABOVE it -- the store pattern of k_sample_gusts needs another look"))
    sm = summary.cpu().numpy()
    print(f"  (summary: mean cost {sm[:, 0].mean():.4g}, worst {sm[:, 2].max():.4g}, plans with a collision {(sm[:, 4] > 0).sum()} of {B}, diverged fraction {sm[:, 7].max():.3g})")

    x_host = x_nom.cpu().numpy()
    us_all = time_launches(stream, lambda: rh.evaluate_sampled(x_nom, S, 7, SIGMA12, gust=GUST), reps, inner)
    print(line("  evaluate_sampled, all four (events on the solver's stream)", us_all))
    wall = []
    for k in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = rh.evaluate_sampled(x_host, S, 11 + k, SIGMA12, gust=GUST)["summary"].cpu().numpy()
        wall.append(time.perf_counter() - t0)
    print(f"  evaluate_sampled from the measured states on the host to the summary on the host: {np.median(wall) * 1e3:.2f} ms wall (finite: {bool(np.isfinite(out).all())})")

    if baseline:
        x0_host = x0.cpu().numpy()
        t_gen, t_eval = [], []
        for k in range(3):
            t0 = time.perf_counter()
            w = pb.gust_wrenches(B, S, N, 11 + k, 1.0, 0.03)
            t1 = time.perf_counter()
            got = rh.evaluate(x0_host, w)
            sc = got["score"].cpu().numpy()
            t2 = time.perf_counter()
            t_gen.append(t1 - t0)
            t_eval.append(t2 - t1)
        print(f"  the parent's way: problems.gust_wrenches {np.median(t_gen) * 1e3:.1f} ms + evaluate(x0, wrench) from host arrays to the scores on the host "
              f"{np.median(t_eval) * 1e3:.1f} ms = {(np.median(t_gen) + np.median(t_eval)) * 1e3:.1f} ms wall ({w.nbytes / 1e6:.0f} MB of wrenches; finite: {bool(np.isfinite(sc[..., 0]).all())})")
        print(f"  the parent's way / evaluate_sampled, wall: {(np.median(t_gen) + np.median(t_eval)) / np.median(wall):.0f}x")


if __name__ == "__main__":
    main()
