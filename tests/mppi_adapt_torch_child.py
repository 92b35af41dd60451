"""quadrotorilqr_amd.mpc.RecedingHorizon.start / tick with explore["adapt"], and QuadrotorILQRBatch.mppi_flight_spread_device /
mppi_adapt_device on torch tensors, run in a process of their own for tests/test_gpu_mppi_adapt.py, for the reason
tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records, asserts
nothing: the test reads the arrays this writes.
usage: python -m tests.mppi_adapt_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import mpc  # noqa: E402
from tests import closed_loop_numpy as cn  # noqa: E402
from tests.monte_carlo_torch_child import refusal  # noqa: E402
from tests.mppi_torch_child import B, EXPLORE, N, ROUNDS, S, SEED, direct as direct_without, handle, record  # noqa: E402

ADAPT = dict(rate=0.5, floor=[0.05, 0.04, 0.06, 0.05], cap=2.0)
ADAPTING = dict(EXPLORE, adapt=ADAPT)


def direct(s, plan, spread):
    """the rounds of ADAPTING by the direct calls, then the solve: (info, traj, cost, spread)"""
    dev = plan.device
    new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    score, info, other, other_spread = new(B, S, 4), new(B, 8), new(B, N, 18), new(B, N, 4)
    kw = dict(tau_s=EXPLORE["tau_s"], collision_cost=EXPLORE["collision_cost"], first_is_nominal=True)
    for r in range(ROUNDS):
        s.mppi_flight_spread_device(plan, spread, score, EXPLORE["seed"] + r, EXPLORE["sigma"], EXPLORE["lambda_"], **kw)
        s.mppi_adapt_device(plan, spread, score, other, other_spread, info, EXPLORE["seed"] + r, EXPLORE["sigma"], EXPLORE["lambda_"],
                            ADAPT["floor"], ADAPT["cap"], ADAPT["rate"], **kw)
        plan, other, spread, other_spread = other, plan, other_spread, spread
    cost, ints = new(B), [new(B, dtype=torch.int32) for _ in range(4)]
    s.solve_batch_device(plan, plan, cost, *ints)
    torch.cuda.synchronize()
    return info.cpu().numpy(), plan.cpu().numpy(), cost.cpu().numpy(), spread.cpu().numpy()


def main(rec):
    s, init = handle()
    rh = mpc.RecedingHorizon(s, B, N)
    res = rh.start(init, explore=ADAPTING)
    torch.cuda.synchronize()
    record(rec, "start", res)
    rec["start_spread"] = rh.spread.cpu().numpy()
    last = res["traj"].clone()
    x = np.ascontiguousarray(cn.sample_states(last.cpu().numpy(), 1, 1, SEED + 3, pos_m=0.05, ang_rad=0.05, vel_sigma=0.05)[:, 0])
    # a tick refused behind the shift of the spread (the flight is admitted, the adaptation's rate is not) leaves the spread what it was
    rec["refusal_rate"] = np.array(refusal(lambda: rh.tick(x, explore=dict(EXPLORE, adapt=dict(ADAPT, rate=2.0)))))
    rec["spread_after_refusal"] = rh.spread.cpu().numpy()
    rec["k0_after_refusal"] = np.array(rh.k0)
    rec["refusal_adapt_keys"] = np.array(refusal(lambda: rh.tick(x, explore=dict(EXPLORE, adapt=dict(rate=0.5)))))
    res = rh.tick(x, explore=ADAPTING)
    torch.cuda.synchronize()
    record(rec, "tick", res)
    rec["tick_spread"] = rh.spread.cpu().numpy()
    # the same by the direct calls, on a handle of its own
    s2, _ = handle()
    s2.set_horizon_start(0)
    dev = rh.device
    sig = torch.tensor(EXPLORE["sigma"], dtype=torch.float64, device=dev)
    out = direct(s2, torch.from_numpy(init).to(dev), sig.expand(B, N, 4).contiguous())
    rec["start_direct_info"], rec["start_direct_traj"], rec["start_direct_cost"], rec["start_direct_spread"] = out
    shifted = torch.zeros((B, N, 18), dtype=torch.float64, device=dev)
    s2.shift_device(last, shifted, x0=torch.from_numpy(x).to(dev), steps=1, tail="hold")
    s2.set_horizon_start(1)
    torch.cuda.synchronize()
    shifted_spread = torch.from_numpy(np.concatenate([out[3][:, 1:], np.broadcast_to(np.array(EXPLORE["sigma"]), (B, 1, 4))], axis=1)).to(dev)
    rec["tick_shifted_spread"] = shifted_spread.cpu().numpy()
    out = direct(s2, shifted, shifted_spread)
    rec["tick_direct_info"], rec["tick_direct_traj"], rec["tick_direct_cost"], rec["tick_direct_spread"] = out
    # explore without adapt, explore=None, and the calls without the argument: tests/mppi_torch_child.py's sequence
    for tag, kw in (("explore", dict(explore=EXPLORE)), ("plain", {}), ("none", dict(explore=None))):
        s3, _ = handle()
        rh3 = mpc.RecedingHorizon(s3, B, N)
        res = rh3.start(init, **kw)
        torch.cuda.synchronize()
        record(rec, "start_" + tag, res)
        res = rh3.tick(x, **kw)
        torch.cuda.synchronize()
        record(rec, "tick_" + tag, res)
        rec["spread_is_none_" + tag] = np.array(rh3.spread is None)
    # ... and explore without adapt by the direct calls of the planner as it was
    s4, _ = handle()
    s4.set_horizon_start(0)
    rec["start_without_info"], rec["start_without_traj"], rec["start_without_cost"] = direct_without(s4, torch.from_numpy(init).to(dev))


if __name__ == "__main__":
    rec = {}
    main(rec)
    np.savez(sys.argv[1], **rec)
