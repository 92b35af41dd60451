#!/usr/bin/env python3
"""Diagnostic: what fleet deconfliction costs on the device, at n = 100 knots and K = 8 neighbours: one fleet of
1024, 16 fleets of 64, one fleet of 8192.  Device time per call by HIP events on the solver's stream (warmed; the median of `reps` windows
of `inner` calls, with the windows' minimum and maximum) of qilqr_fleet_neighbours_device and of qilqr_set_batch_obstacles_device, and in
the same run the two routes they replace: the host route (download the plans, NumPy pairs, qilqr_set_batch_obstacles; wall clock, it
ends in a synchronise) and the torch expression a user would otherwise write on the same device (broadcast difference, amin over the
knots, topk; HIP events on torch's stream; partner tiles of 1024 at V = 8192, where the whole broadcast does not fit).
usage (repository root): PYTHONPATH=. python3 profiles/microbench/fleet.py [reps=10] [inner=4] [out=profiles/fleet_microbench.txt]
With trace=1 it only enqueues 20 pairs of the two calls at B = V = 1024 and at 16 fleets of 64, for a kernel trace in a run of its own:
rocprofv3 --kernel-trace --stats -d DIR -- python3 profiles/microbench/fleet.py trace=1"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402

N, K = 100, 8
RULE = dict(radius=1.0, weight=50.0)
CASES = ((1024, 1024), (1024, 64), (8192, 8192))  # (B, V)


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


def time_host(call, reps, warm=True):
    if warm:
        call()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        us.append((time.perf_counter() - t0) * 1e6)
    return np.array(us)


def say(lines, text):
    lines.append(text)
    print(text, flush=True)


def line(tag, us):
    return f"{tag}: {np.median(us):11.1f} us per call (min {us.min():.1f} - max {us.max():.1f})"


def plans(B, rng):
    """vehicles on straight lines through a cube whose side grows with the fleet: a few neighbours within a few metres of each"""
    t = (np.arange(N) * pb.DT_DEMO)[None, :, None]
    side = 4.0 * B ** (1.0 / 3.0)
    plan = np.zeros((B, N, 18))
    plan[:, :, 0], plan[:, :, 4] = t[..., 0], 1.0
    plan[:, :, 1:4] = rng.uniform(-side, side, (B, 1, 3)) + rng.uniform(-2.0, 2.0, (B, 1, 3)) * t
    return plan


def numpy_pairs(plan, V):
    """the host route's arithmetic: per fleet the smallest squared distance over the knots of every pair, then the K nearest per vehicle"""
    B = plan.shape[0]
    idx = np.empty((B, K), dtype=np.int64)
    for g in range(B // V):
        p = plan[g * V:(g + 1) * V, :, 1:4]
        d2 = np.full((V, V), np.inf)
        for i in range(N):  # (knot by knot: V x V x n x 3 at once is 2.4 GB at V = 1024)
            e = p[:, None, i] - p[None, :, i]
            np.minimum(d2, (e * e).sum(-1), out=d2)
        np.fill_diagonal(d2, np.inf)
        idx[g * V:(g + 1) * V] = np.argsort(d2, axis=1, kind="stable")[:, :K] + g * V
    return idx


def torch_pairs(pos, V, tile=1024):
    """pos (G, V, n, 3) on the device -> (d2, index) of the K nearest per vehicle: broadcast difference, amin over the knots, topk"""
    best = None
    for p0 in range(0, V, tile):
        e = pos[:, :, None] - pos[:, None, p0:p0 + tile]         # (G, V, tile, n, 3)
        d2 = (e * e).sum(-1).amin(-1)                            # (G, V, tile)
        rows = torch.arange(p0, min(p0 + tile, V), device=pos.device)
        d2[:, rows, rows - p0] = float("inf")
        best = d2 if best is None else torch.cat([best, d2], dim=2)
    return torch.topk(best, K, dim=2, largest=False)


def main():
    reps, inner, out_path, trace = 10, 4, os.path.join(ROOT, "profiles", "fleet_microbench.txt"), False
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
        elif k == "out":
            out_path = v
        elif k == "trace":
            trace = v != "0"
    if not torch.cuda.is_available():
        sys.exit("fleet.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    lines = []
    say(lines, f"fleet deconfliction, n = {N} knots, K = {K} (median of {reps} windows of {inner} calls; {torch.cuda.get_device_name(0)}):")
    s = capi.from_config(pb.config2(B=1, N=N), device=0)
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    if trace:
        for B, V in CASES[:2]:
            plan = torch.from_numpy(plans(B, np.random.default_rng(B + V))).to(dev)
            new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
            spheres, counts = new(B, K, 8), new(B, dtype=torch.int32)
            torch.cuda.synchronize()
            for _ in range(20):
                s.fleet_neighbours_device(plan, V, K, range=6.0, spheres=spheres, counts=counts, wait_current_stream=False, **RULE)
                s.set_batch_obstacles_device(spheres, counts, wait_current_stream=False)
            stream.synchronize()
        s.close()
        return
    for B, V in CASES:
        rng = np.random.default_rng(B + V)
        h_plan = plans(B, rng)
        plan = torch.from_numpy(h_plan).to(dev)
        new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
        summary, nbr, spheres, counts, dropped = new(B, capi.FLEET_SUMMARY), new(B, K, capi.FLEET_NBR), new(B, K, 8), new(B, dtype=torch.int32), new(1, dtype=torch.int32)
        torch.cuda.synchronize()
        kw = dict(summary=summary, nbr=nbr, spheres=spheres, counts=counts, wait_current_stream=False, **RULE)
        us_n = time_calls(stream, lambda: s.fleet_neighbours_device(plan, V, K, range=6.0, **kw), reps, inner)
        us_s = time_calls(stream, lambda: s.set_batch_obstacles_device(spheres, counts, dropped, wait_current_stream=False), reps, inner)
        torch.cuda.synchronize()
        say(lines, f" B = {B} as {B // V} fleet(s) of {V}:")
        say(lines, line("  qilqr_fleet_neighbours_device (3 launches)          ", us_n))
        say(lines, line("  qilqr_set_batch_obstacles_device (1 launch + memset)", us_s))
        pair_knots = float(B) * (V - 1) * N
        say(lines, f"  {pair_knots:.3g} pair-knots: {np.median(us_n) * 1e3 / pair_knots:.4f} ns per pair-knot; spheres per vehicle {counts.float().mean().item():.2f},"
                     f" dropped {int(dropped.item())}")

        # the host route: download, NumPy pairs, the host setter (spheres of the right shape; their values are not the point)
        h_spheres = np.zeros((B, K, 8))
        h_spheres[:, :, 6], h_spheres[:, :, 7] = RULE["radius"], RULE["weight"]

        def host_route():
            got = plan.cpu().numpy()
            idx = numpy_pairs(got, V)
            h_spheres[:, :, :3] = got[idx, 0, 1:4]
            s.set_batch_obstacles(h_spheres)

        us_h = time_host(host_route, reps, True) if V <= 1024 else time_host(host_route, 1, False)  # (minutes at V = 8192: one call)
        say(lines, line("  host route: download + NumPy pairs + host setter    ", us_h))
        s.clear_batch_obstacles()
        # the torch expression, on torch's stream
        pos = plan.view(B // V, V, N, 18)[..., 1:4].contiguous()
        cur = torch.cuda.current_stream(dev)
        us_t = time_calls(cur, lambda: torch_pairs(pos, V), reps if V <= 1024 else max(2, reps // 5), 1)
        say(lines, line("  torch: broadcast difference, amin, topk             ", us_t))
        say(lines, f"  the two calls {np.median(us_n) + np.median(us_s):.1f} us: {np.median(us_h) / (np.median(us_n) + np.median(us_s)):.0f} times below the host route,"
                     f" {np.median(us_t) / (np.median(us_n) + np.median(us_s)):.1f} times below the torch expression")
        d2, idx = torch_pairs(pos, V)
        torch.cuda.synchronize()
        same = (idx + torch.arange(B // V, device=dev)[:, None, None] * V).view(B, K).double() == nbr[:, :, 0]
        say(lines, f"  (the torch expression names the same {K} partners for {same.all(dim=1).float().mean().item() * 100:.1f} % of the vehicles)")
    s.close()
    text = "\n".join(lines)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
