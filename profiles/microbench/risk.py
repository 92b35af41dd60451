#!/usr/bin/env python3
"""Diagnostic: what the risk measures and the choice among candidates add to the Monte-Carlo loop on the device,
at section 8l's workload: 64 plans = 16 vehicles x 4 candidates, x 1024 samples x 100 knots, a gust per knot, 8 shared spheres, 3 levels.
  1. k_risk_scores, k_select_plans with k_gather_plans, k_reduce_scores and the scored flight they follow: device time per call by HIP
     events on the solver's stream (warmed; median of `reps` windows of `inner` calls), and k_risk_scores at other sample counts;
  2. RecedingHorizon.evaluate_sampled without and with risk levels and candidates, and with select() behind it: by events, and wall
     clock to the choice on the host;
  3. the caller's routes without these kernels, in the same run: torch.sort of the cost column plus indexing and a tail mean on the
     device (events on torch's stream), and the download of B x S x 4 words with NumPy's sort on the host (wall clock).
The condition (section 8l's own): risk + selection + gather stay below the flight they follow.
usage (repository root): PYTHONPATH=. python3 profiles/microbench/risk.py [reps=10] [inner=4]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402
from profiles.microbench.monte_carlo import GUST, SIGMA12, line, time_launches  # noqa: E402

N, V, C, S = 100, 16, 4, 1024
B = V * C
LEVELS = (0.9, 0.95, 0.99)


def main():
    reps, inner = 10, 4
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
    if not torch.cuda.is_available():
        sys.exit("risk.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    cfg = pb.config2(B=B, N=N)
    s = capi.from_config(cfg, device=0)
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    rh = mpc.RecedingHorizon(s, B, N)
    plan = rh.start(cfg["init"][:B], gains=True)["traj"]
    r = np.random.default_rng(7)
    path = plan.cpu().numpy()[:, :, 1:4].reshape(-1, 3)
    spheres = np.zeros((8, 5))
    spheres[:, :3] = path[r.integers(0, len(path), 8)] + 0.3 * (2.0 * r.random((8, 3)) - 1.0)
    spheres[:, 3], spheres[:, 4] = 0.15, 25.0
    s.set_obstacles(spheres)
    x_nom = plan[:, 0, 1:14].contiguous()
    x0, wrench = new(B, S, capi.STATE), new(B, S, N, capi.WRENCH)
    stats, score, summary, risk = new(B, S, capi.CL_STATS), new(B, S, capi.CL_SCORE), new(B, capi.MC_SUMMARY), new(B, len(LEVELS), capi.RISK)
    choice, info, out_plan, out_gains = new(V, dtype=torch.int32), new(V, capi.SELECT_INFO), new(V, N, capi.KNOT), new(V, N, capi.GAIN)
    s.sample_states_device(x_nom, x0, 7, SIGMA12, first_is_nominal=True)
    s.sample_gusts_device(wrench, 7, GUST["sigma"], tau_force_s=0.5, tau_torque_s=0.2, wait_current_stream=False)
    torch.cuda.synchronize()

    print(f"risk and selection, {B} plans = {V} vehicles x {C} candidates, x {S} samples x {N} knots, {len(LEVELS)} levels (median of {reps} windows of {inner} calls):")
    us_fly = time_launches(stream, lambda: s.closed_loop_device(plan, rh.gains, x0, out_stats=stats, wrench=wrench, out_score=score, wait_current_stream=False), reps, inner)
    print(line("  k_closed_loop_scored (the flight)                 ", us_fly))
    us_red = time_launches(stream, lambda: s.reduce_scores_device(score, summary, wait_current_stream=False), reps, inner)
    print(line("  k_reduce_scores                                   ", us_red))
    us_risk = time_launches(stream, lambda: s.risk_scores_device(score, risk, LEVELS, wait_current_stream=False), reps, inner)
    print(line("  k_risk_scores (LDS, a block barrier per stage)    ", us_risk))
    us_clear = time_launches(stream, lambda: s.risk_scores_device(score, risk, LEVELS, column="clearance", wait_current_stream=False), reps, inner)
    print(line("  k_risk_scores, clearance column                   ", us_clear))
    s.risk_scores_device(score, risk, LEVELS, wait_current_stream=False)
    select = lambda **kw: (lambda: s.select_plans_device(summary, C, choice, info, objective="cvar", level=1, risk=risk, max_collision_fraction=0.5,
                                                         wait_current_stream=False, **kw))
    us_sel = time_launches(stream, select(), reps, inner)
    print(line("  k_select_plans                                    ", us_sel))
    us_gat = time_launches(stream, select(plan=plan, gains=rh.gains, out_plan=out_plan, out_gains=out_gains), reps, inner)
    print(line("  k_select_plans + k_gather_plans                   ", us_gat))
    added = float(np.median(us_risk) + np.median(us_gat))
    print(f"  added to the loop (risk + selection + gather) {added:.1f} us against the {np.median(us_fly):.1f} us flight it follows: "
          + ("below it" if added <= np.median(us_fly) else "ABOVE it"))
    for S_other in (64, 128, 256, 4096):
        sc, rk = new(B, S_other, capi.CL_SCORE).normal_(), new(B, len(LEVELS), capi.RISK)
        torch.cuda.synchronize()
        us = time_launches(stream, lambda: s.risk_scores_device(sc, rk, LEVELS, wait_current_stream=False), reps, inner)
        print(line(f"  k_risk_scores at S = {S_other:4d}                        ", us))
    ch = choice.cpu().numpy()
    print(f"  (choices {np.bincount(ch, minlength=C).tolist()} over the candidates, fallback for {int(info[:, 3].sum().item())} vehicles)")

    us_plain = time_launches(stream, lambda: rh.evaluate_sampled(x_nom, S, 7, SIGMA12, gust=GUST), reps, inner)
    print(line("  evaluate_sampled as it was (events on the solver's stream)    ", us_plain))
    us_cand = time_launches(stream, lambda: rh.evaluate_sampled(x_nom, S, 7, SIGMA12, gust=GUST, candidates=C), reps, inner)
    print(line("  evaluate_sampled with candidates alone (samplers per candidate)", us_cand))
    us_full = time_launches(stream, lambda: (rh.evaluate_sampled(x_nom, S, 7, SIGMA12, gust=GUST, risk_levels=LEVELS, candidates=C), rh.select(C, level=1)), reps, inner)
    print(line("  evaluate_sampled with risk and candidates, and select()       ", us_full))
    x_host = x_nom.cpu().numpy()
    wall = []
    for k in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rh.evaluate_sampled(x_host, S, 11 + k, SIGMA12, gust=GUST, risk_levels=LEVELS, candidates=C)
        got = rh.select(C, level=1)["choice"].cpu().numpy()
        wall.append(time.perf_counter() - t0)
    print(f"  from the measured states on the host to the choice on the host: {np.median(wall) * 1e3:.2f} ms wall (choices {np.bincount(got, minlength=C).tolist()})")

    # ---- the caller's routes without the kernels
    cur = torch.cuda.current_stream(dev)
    ranks = [int(min(S - 1, max(0, np.ceil(lv * S) - 1))) for lv in LEVELS]

    def torch_route():
        keys, _ = torch.sort(torch.nan_to_num(score[..., 0], nan=float("inf")), dim=1)
        return torch.stack([torch.stack([keys[:, k], keys[:, k:].mean(dim=1)], dim=1) for k in ranks], dim=1)

    us_torch = time_launches(cur, torch_route, reps, inner)
    print(line("  the torch route: torch.sort + indexing + tail means (torch's stream)", us_torch))
    same = torch.allclose(torch_route()[..., 0], risk[..., 0], equal_nan=True)
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = score.cpu().numpy()
        keys = np.sort(np.where(np.isnan(sc[..., 0]), np.inf, sc[..., 0]), axis=1)
        out = np.stack([np.stack([keys[:, k], keys[:, k:].mean(axis=1)], axis=1) for k in ranks], axis=1)
        host.append(time.perf_counter() - t0)
    print(f"  the host route: download of {B} x {S} x 4 words + NumPy sort and tail means: {np.median(host) * 1e3:.2f} ms wall (order statistics equal the kernel's: {bool(same)}, {out.shape})")
    print(f"  k_risk_scores / the torch route: {np.median(us_risk) / np.median(us_torch):.2f}")


if __name__ == "__main__":
    main()
