#!/usr/bin/env python3
"""Diagnostic: what a closed-loop Monte-Carlo flight costs.
  1. k_closed_loop at 64 plans x 1024 samples x 100 knots, statistics only and with trajectories: device time per launch by HIP events
     on the solver's stream (warmed; `reps` windows of `inner` launches), samples x knots per second;
  2. the only way to do that work without it: qilqr_forward_sim on the 65 536 replicated trajectories, its rollout kernel's device time
     from qilqr_profile, with single_wave_rollout = 1 (k_rollout, the same per-lane routine) and with the default route;
  3. the two forms of k_closed_loop against each other at 1024 plans x S samples, S = 1 .. 1024, statistics only -- where the
     shared-operand form is ahead of the flattened one (closed_loop_kernels.h, closed_loop_shared_form).  Needs the diagnostics build, which can
     force a form: QILQR_LIB=quadrotorilqr_amd/lib/libquadrotor_ilqr_diag.so; skipped on the product build.
  4. the scored flight: k_closed_loop_scored at the workload of 1. under a zero-mean gust per knot with 8 shared
     spheres on the handle, statistics and score, no trajectories -- and its switches one at a time -- against the only way to the same
     cost without it: k_closed_loop with trajectories, the 944 MB brought to the host, and qilqr_cost_trajectory on the 65 536 flights
     (wall times); then, on the diagnostics build, the two forms of the scored
     kernel against each other.
usage (repository root): PYTHONPATH=. python3 profiles/microbench/closed_loop.py [reps=10] [inner=4] [baseline=1] [forms=1] [scored=1]
(baseline=2: the parent's way of leg 4 only, without leg 2; forms=0 and scored=0 skip legs 3 and 4)"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from quadrotorilqr_amd import capi, problems as pb  # noqa: E402

N = 100


def plans_and_gains(s, cfg, B, dev):
    """B plans of config2 (the hover mission from random starts, solved) and the gains about them, on the device"""
    plan = torch.from_numpy(s.solve_batch(cfg["init"][:B])["traj"]).to(dev)
    gains = torch.empty((B, N, capi.GAIN), dtype=torch.float64, device=dev)
    s.backwards_pass_device(plan, gains)
    return plan, gains


def samples_about(plan, S, seed):
    """(B, S, 13) on the device: knot 0 of every plan, moved by up to 0.2 m, 0.1 in the quaternion's vector part and 0.2 in the velocities"""
    g = torch.Generator(device=plan.device)
    g.manual_seed(seed)
    x = plan[:, None, 0, 1:14].repeat(1, S, 1)
    d = 2.0 * torch.rand(x.shape, generator=g, dtype=torch.float64, device=plan.device) - 1.0
    x[..., 0:3] += 0.2 * d[..., 0:3]
    x[..., 4:7] += 0.1 * d[..., 4:7]
    x[..., 3:7] /= x[..., 3:7].norm(dim=-1, keepdim=True)
    x[..., 7:13] += 0.2 * d[..., 7:13]
    return x.contiguous()


def time_launches(s, stream, call, reps, inner):
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


def line(tag, us, work):
    med = float(np.median(us))
    return f"{tag}: {med:9.1f} us per launch (min {us.min():.1f}, max {us.max():.1f}), {work / med:8.1f} M sample-knots/s"


def scored_leg(s, cfg, stream, plan, gains, x0, stats, traj, reps, inner, baseline, forms, dev):
    """leg 4: the scored kernel at 64 plans x 1024 samples x 100 knots, and the parent's way to the same cost"""
    B, S = x0.shape[0], x0.shape[1]
    work = B * S * N
    r = np.random.default_rng(7)
    path = plan[:B].cpu().numpy()[:, :, 1:4].reshape(-1, 3)
    spheres = np.zeros((8, 5))
    spheres[:, :3] = path[r.integers(0, len(path), 8)] + 0.3 * (2.0 * r.random((8, 3)) - 1.0)
    spheres[:, 3] = 0.15
    spheres[:, 4] = 25.0
    s.set_obstacles(spheres)
    gust = torch.from_numpy(pb.gust_wrenches(B, S, N, 3, 1.0, 0.03)).to(dev)
    gust1 = gust[:, :, :1].contiguous()
    score = torch.empty((B, S, capi.CL_SCORE), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    print(f"k_closed_loop_scored, {B} plans x {S} samples x {N} knots, 8 shared spheres, no trajectories:")
    call = lambda **kw: (lambda: s.closed_loop_device(plan[:B], gains[:B], x0, out_stats=stats, wait_current_stream=False, **kw))
    legs = (("  statistics only (k_closed_loop, again)   ", dict()),
            ("  gust per knot, statistics                ", dict(wrench=gust)),
            ("  score, statistics, no gust               ", dict(out_score=score)),
            ("  gust per knot, statistics and score      ", dict(wrench=gust, out_score=score)),
            ("  one gust per flight, statistics and score", dict(wrench=gust1, out_score=score)))
    med = {}
    for tag, kw in legs:
        us = time_launches(s, stream, call(**kw), reps, inner)
        med[tag] = float(np.median(us))
        print(line(tag, us, work))
    sc = score.cpu().numpy()
    print(f"  (flights that enter a sphere: {(sc[..., 3] > 0).mean():.3f}; smallest clearance {sc[..., 1].min():.3f} m; mean cost {sc[..., 0].mean():.4g})")
    if baseline:
        us_traj = time_launches(s, stream, lambda: s.closed_loop_device(plan[:B], gains[:B], x0, out_traj=traj, out_stats=stats, wait_current_stream=False), reps, inner)
        print(line("  the parent's way, 1: k_closed_loop with trajectories", us_traj, work))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flown = traj.cpu().numpy().reshape(B * S, N, 18)
        t_copy = time.perf_counter() - t0
        print(f"  the parent's way, 2: the {flown.nbytes / 1e6:.0f} MB of trajectories to the host: {t_copy * 1e3:.1f} ms")
        f = capi.from_config(cfg, device=0)
        f.set_obstacles(spheres)
        f.cost_trajectory(flown)  # (workspace, code object, clocks)
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            cost = f.cost_trajectory(flown)
            wall.append(time.perf_counter() - t0)
        print(f"  the parent's way, 3: qilqr_cost_trajectory on the {B * S} flights: {np.median(wall) * 1e3:.1f} ms wall (finite: {bool(np.isfinite(cost).all())})")
        total = np.median(us_traj) + t_copy * 1e6 + np.median(wall) * 1e6
        tag = legs[3][0]
        print(f"  the parent's way in all: {total / 1e3:.1f} ms; the scored kernel: {med[tag]:.1f} us")
        f.close()
    lib = capi.load()
    if forms and hasattr(lib, "qilqr_debug_set_closed_loop_form"):
        lib.qilqr_debug_set_closed_loop_form.argtypes = [C.c_int32]
        Bt = 1024
        print(f"the two forms of the scored kernel at {Bt} plans x S samples x {N} knots, gust per knot, statistics and score (us per launch, median of {reps} windows of {inner}):")
        for St in (32, 60, 64, 96, 128, 1024):
            x = samples_about(plan[:Bt], St, 2 + St)
            st = torch.empty((Bt, St, capi.CL_STATS), dtype=torch.float64, device=dev)
            sco = torch.empty((Bt, St, capi.CL_SCORE), dtype=torch.float64, device=dev)
            w = torch.from_numpy(pb.gust_wrenches(Bt, St, N, 5, 1.0, 0.03)).to(dev)
            torch.cuda.synchronize()
            m = {}
            for form in (0, 1, 0, 1):
                lib.qilqr_debug_set_closed_loop_form(form)
                us = time_launches(s, stream, lambda: s.closed_loop_device(plan[:Bt], gains[:Bt], x, out_stats=st, wrench=w, out_score=sco, wait_current_stream=False), reps, inner)
                m.setdefault(form, []).append(float(np.median(us)))
            flat, shared = min(m[0]), min(m[1])
            by_rule = "shared-operand" if 64 * St >= 63 * 64 * ((St + 63) // 64) else "flattened"
            print(f"  S = {St:4d}: flattened {flat:9.1f} (other pass {max(m[0]):9.1f}) | shared-operand {shared:9.1f} (other pass {max(m[1]):9.1f}) | shared / flattened {shared / flat:.3f} | the rule takes the {by_rule} form")
        lib.qilqr_debug_set_closed_loop_form(-1)
    s.clear_obstacles()


def main():
    reps, inner, baseline, forms, scored = 10, 4, 1, 1, 1
    for a in sys.argv[1:]:
        k, _, v = a.partition("=")
        if k == "reps":
            reps = int(v)
        elif k == "inner":
            inner = int(v)
        elif k == "baseline":
            baseline = int(v)
        elif k == "forms":
            forms = int(v)
        elif k == "scored":
            scored = int(v)
    if not torch.cuda.is_available():
        sys.exit("closed_loop.py measures on the GPU: no device, no number")
    dev = torch.device("cuda", 0)
    B, S = 64, 1024
    cfg = pb.config2(B=4096, N=N)
    s = capi.from_config(cfg, device=0)
    stream = torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev)
    plan, gains = plans_and_gains(s, cfg, 4096, dev)
    x0 = samples_about(plan[:B], S, 1)
    stats = torch.empty((B, S, capi.CL_STATS), dtype=torch.float64, device=dev)
    traj = torch.empty((B, S, N, capi.KNOT), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    work = B * S * N
    print(f"k_closed_loop, {B} plans x {S} samples x {N} knots ({'shared-operand' if 64 * S >= 63 * 64 * ((S + 63) // 64) else 'flattened'} form by the rule):")
    us_stats = time_launches(s, stream, lambda: s.closed_loop_device(plan[:B], gains[:B], x0, out_stats=stats, wait_current_stream=False), reps, inner)
    print(line("  statistics only    ", us_stats, work))
    us_traj = time_launches(s, stream, lambda: s.closed_loop_device(plan[:B], gains[:B], x0, out_traj=traj, out_stats=stats, wait_current_stream=False), reps, inner)
    print(line("  with trajectories  ", us_traj, work) + f", {8 * 18 * work / np.median(us_traj) / 1e3:.1f} GB/s written")
    worst = stats[..., 0].max().item()
    print(f"  (largest position error of a sample: {worst:.3f} m; samples that end within 1 cm of the plan: {(stats[..., 2] < 0.01).double().mean().item():.3f})")

    if baseline == 1:
        # the parent's way: every sample a trajectory of its own -- plan and gains replicated S times, knot 0 replaced by the sample
        rep_plan = np.repeat(plan[:B].cpu().numpy(), S, axis=0)
        rep_plan[:, 0, 1:14] = x0.cpu().numpy().reshape(B * S, 13)
        rep_gains = np.repeat(gains[:B].cpu().numpy(), S, axis=0)
        for tag, kw in (("single_wave_rollout = 1 (k_rollout)", dict(single_wave_rollout=1)), ("the default route", dict())):
            f = capi.from_config(cfg, device=0, profile=1, **kw)
            f.forward_sim(rep_plan, rep_gains, 0.0)  # (workspace, code object, clocks)
            ms = []
            for _ in range(3):
                f.profile_reset()
                out = f.forward_sim(rep_plan, rep_gains, 0.0)
                p = f.profile_get()
                ms.append(p["rollout_ms"] / max(p["rollout_launches"], 1))
            print(line(f"qilqr_forward_sim on {B * S} replicated trajectories, {tag}, rollout kernel", np.array(ms) * 1e3, work))
            # (the replica starts at the sample as knot 0 of its own plan, so its dx at knot 0 is zero: not the same flight, the same work)
            print(f"    finite: {bool(np.isfinite(out).all())}; replicated operands it reads: {8 * 70 * work / 1e9:.2f} GB")
            f.close()

    if scored:
        scored_leg(s, cfg, stream, plan, gains, x0, stats, traj, reps, inner, baseline, forms, dev)
    if not forms:
        return
    lib = capi.load()
    if not hasattr(lib, "qilqr_debug_set_closed_loop_form"):
        print("the two forms against each other: skipped (the product build has one rule; run with QILQR_LIB=.../libquadrotor_ilqr_diag.so)")
        return
    lib.qilqr_debug_set_closed_loop_form.argtypes = [C.c_int32]
    Bt = 1024
    print(f"the two forms at {Bt} plans x S samples x {N} knots, statistics only (us per launch, median of {reps} windows of {inner}):")
    ahead = []
    for S in (1, 4, 16, 32, 48, 56, 60, 64, 96, 120, 128, 192, 900, 1024):
        x = samples_about(plan[:Bt], S, 2 + S)
        st = torch.empty((Bt, S, capi.CL_STATS), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        med = {}
        for form in (0, 1, 0, 1):  # alternating: the two are compared in one call
            lib.qilqr_debug_set_closed_loop_form(form)
            us = time_launches(s, stream, lambda: s.closed_loop_device(plan[:Bt], gains[:Bt], x, out_stats=st, wait_current_stream=False), reps, inner)
            med.setdefault(form, []).append(float(np.median(us)))
        flat, shared = min(med[0]), min(med[1])
        if shared <= flat:
            ahead.append(S)
        print(f"  S = {S:4d}: flattened {flat:9.1f} (other pass {max(med[0]):9.1f}) | shared-operand {shared:9.1f} (other pass {max(med[1]):9.1f}) | shared / flattened {shared / flat:.3f}")
    lib.qilqr_debug_set_closed_loop_form(-1)
    print(f"the shared-operand form is at or ahead of the flattened one at S = {ahead} (of the S measured)")


if __name__ == "__main__":
    main()
