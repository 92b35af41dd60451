"""quadrotorilqr_amd.mpc.RecedingHorizon.start / tick with `explore`, QuadrotorILQRBatch.mppi_flight_device / mppi_update_device on torch
tensors, and the planning scenario of tests/mppi_cases.py on the device, run in a process of their own for tests/test_gpu_mppi.py, for the
reason tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records,
asserts nothing: the test reads the arrays this writes.
usage: python -m tests.mppi_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc, mppi_cases as mc  # noqa: E402
from tests.monte_carlo_torch_child import refusal  # noqa: E402

SEED, B, N, S, MISSION, ROUNDS = 41, 3, 12, 70, 16, 2
EXPLORE = dict(S=S, seed=900, sigma=[0.5, 0.4, 0.6, 0.5], lambda_=50.0, tau_s=0.3, collision_cost=20.0, iterations=ROUNDS)


def handle():
    cfg, _ = dc.tracking_case(B, MISSION, SEED, shared=True)
    des = cfg["desired"]
    init = dc.start_from(np.repeat(des[None, :N], B, axis=0), np.arange(B), SEED)
    s = capi.from_config(cfg)
    s.set_obstacles(np.array([[*(des[5, 1:4] + 0.1), 0.2, 30.0]]))
    s.set_control_limits(0.2, 6.0)
    return s, init


def record(rec, tag, res):
    rec[tag + "_keys"] = np.array(list(res))
    for k, v in res.items():
        rec["%s_%s" % (tag, k)] = v.cpu().numpy()


def direct(s, plan):
    """the rounds of EXPLORE by the direct calls, then the solve: (info, traj, cost)"""
    dev = plan.device
    new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    score, info, other = new(B, S, 4), new(B, 8), new(B, N, 18)
    kw = dict(tau_s=EXPLORE["tau_s"], collision_cost=EXPLORE["collision_cost"], first_is_nominal=True)
    for r in range(ROUNDS):
        s.mppi_flight_device(plan, score, EXPLORE["seed"] + r, EXPLORE["sigma"], EXPLORE["lambda_"], **kw)
        s.mppi_update_device(plan, score, other, info, EXPLORE["seed"] + r, EXPLORE["sigma"], EXPLORE["lambda_"], **kw)
        plan, other = other, plan
    cost, ints = new(B), [new(B, dtype=torch.int32) for _ in range(4)]
    s.solve_batch_device(plan, plan, cost, *ints)
    torch.cuda.synchronize()
    return info.cpu().numpy(), plan.cpu().numpy(), cost.cpu().numpy()


def explore(rec):
    s, init = handle()
    x = None
    rh = mpc.RecedingHorizon(s, B, N)
    res = rh.start(init, explore=EXPLORE)
    torch.cuda.synchronize()
    record(rec, "start", res)
    last = res["traj"].clone()
    x = np.ascontiguousarray(cn.sample_states(last.cpu().numpy(), 1, 1, SEED + 3, pos_m=0.05, ang_rad=0.05, vel_sigma=0.05)[:, 0])
    res = rh.tick(x, explore=EXPLORE)
    torch.cuda.synchronize()
    record(rec, "tick", res)
    rec["refusal_missing"] = np.array(refusal(lambda: rh.tick(x, explore=dict(S=5, seed=1))))
    rec["refusal_unknown"] = np.array(refusal(lambda: rh.tick(x, explore=dict(EXPLORE, rounds=3))))
    # the same by the direct calls, on a handle of its own
    s2, _ = handle()
    s2.set_horizon_start(0)
    dev = rh.device
    rec["start_direct_info"], rec["start_direct_traj"], rec["start_direct_cost"] = direct(s2, torch.from_numpy(init).to(dev))
    shifted = torch.zeros((B, N, 18), dtype=torch.float64, device=dev)
    s2.shift_device(last, shifted, x0=torch.from_numpy(x).to(dev), steps=1, tail="hold")
    s2.set_horizon_start(1)
    torch.cuda.synchronize()
    rec["tick_direct_info"], rec["tick_direct_traj"], rec["tick_direct_cost"] = direct(s2, shifted)
    # explore=None, and the calls without the argument
    for tag, kw in (("plain", {}), ("none", dict(explore=None))):
        s3, _ = handle()
        rh3 = mpc.RecedingHorizon(s3, B, N)
        res = rh3.start(init, **kw)
        torch.cuda.synchronize()
        record(rec, "start_" + tag, res)
        res = rh3.tick(x, **kw)
        torch.cuda.synchronize()
        record(rec, "tick_" + tag, res)


def planning(rec):
    cfg, plan, shared = mc.planning()
    s = capi.from_config(cfg)
    s.set_obstacles(shared)
    dev = torch.device("cuda", 0)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    cur, other, score, info = torch.from_numpy(plan).to(dev), new(mc.PLAN_B, mc.PLAN_N, 18), new(mc.PLAN_B, mc.PLAN_S, 4), new(mc.PLAN_B, 8)
    infos = []
    for r in range(mc.PLAN_ROUNDS):
        s.mppi_flight_device(cur, score, mc.PLAN_SEED + r, **mc.PLAN_RULE)
        s.mppi_update_device(cur, score, other, info, mc.PLAN_SEED + r, **mc.PLAN_RULE)
        torch.cuda.synchronize()  # (every stream of the device, the solver's own included)
        infos.append(info.cpu().numpy().copy())
        cur, other = other, cur
    rec["planning_info"] = np.stack(infos)


if __name__ == "__main__":
    rec = {}
    explore(rec)
    planning(rec)
    np.savez(sys.argv[1], **rec)
