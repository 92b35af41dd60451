"""The torch forms of the plan's feedback law -- QuadrotorILQRBatch.backwards_pass_device and closed_loop_device, and
quadrotorilqr_amd.mpc.RecedingHorizon with gains=True and control() -- run in a process of their own for tests/test_gpu_closed_loop.py, for
the reason tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records,
asserts nothing: the test reads the arrays this writes.  usage: python -m tests.closed_loop_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc  # noqa: E402

SEED, B, N, S, MISSION = 21, 6, 24, 5, 28


def refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the kind and the text are what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return "accepted"


def device_forms(rec):
    """backwards_pass_device -> closed_loop_device -> one synchronise, against the host forms on the same handle"""
    dev = torch.device("cuda", 0)
    cfg, plan = cn.plans(B, N, SEED)
    s = capi.from_config(cfg)
    x0 = cn.sample_states(plan, S, 0, SEED + 1)
    t_plan, t_x0 = torch.from_numpy(plan).to(dev), torch.from_numpy(x0).to(dev)
    t_gains = torch.full((B, N, capi.GAIN), float("nan"), dtype=torch.float64, device=dev)
    t_terms = torch.full((B, 2), float("nan"), dtype=torch.float64, device=dev)
    t_traj = torch.full((B, S, N, capi.KNOT), float("nan"), dtype=torch.float64, device=dev)
    t_stats = torch.full((B, S, capi.CL_STATS), float("nan"), dtype=torch.float64, device=dev)
    s.backwards_pass_device(t_plan, t_gains, t_terms)
    s.closed_loop_device(t_plan, t_gains, t_x0, out_traj=t_traj, out_stats=t_stats)  # (enqueued, not drained)
    torch.cuda.current_stream().wait_event(torch.cuda.ExternalStream(capi.load().qilqr_stream(s._h), device=dev).record_event())
    torch.cuda.synchronize()
    rec["device_gains"], rec["device_terms"] = t_gains.cpu().numpy(), t_terms.cpu().numpy()
    rec["device_traj"], rec["device_stats"] = t_traj.cpu().numpy(), t_stats.cpu().numpy()
    gains, terms = s.backwards_pass(plan)
    host = s.closed_loop(plan, gains, x0)
    rec["host_gains"], rec["host_terms"], rec["host_traj"], rec["host_stats"] = gains, terms, host["traj"], host["stats"]
    # statistics only: the trajectory array is not needed
    t_only = torch.full((B, S, capi.CL_STATS), float("nan"), dtype=torch.float64, device=dev)
    s.closed_loop_device(t_plan, t_gains, t_x0, out_stats=t_only)
    s.cost_trajectory(plan[:1, :4])  # (a draining call of the handle orders the read below)
    rec["device_stats_only"] = t_only.cpu().numpy()
    calls = dict(
        no_output=lambda: s.closed_loop_device(t_plan, t_gains, t_x0),
        overlap=lambda: s.closed_loop_device(t_plan, t_gains, t_x0, out_stats=t_x0.view(-1)[:B * S * 4].view(B, S, 4)),
        x0_shape=lambda: s.closed_loop_device(t_plan, t_gains, t_x0[:, :, :12].contiguous(), out_stats=t_stats),
        gains_shape=lambda: s.closed_loop_device(t_plan, t_gains[:, :, :48].contiguous(), t_x0, out_stats=t_stats),
        float32=lambda: s.closed_loop_device(t_plan, t_gains, t_x0, out_stats=t_stats.float()),
        host_tensor=lambda: s.closed_loop_device(t_plan, t_gains, t_x0, out_stats=t_stats.cpu()),
        window=lambda: s.closed_loop_device(t_plan, t_gains, t_x0, out_stats=t_stats, i0=5, i1=4),
        gains_missing=lambda: s.backwards_pass_device(t_plan, None),
        fine=lambda: s.closed_loop_device(t_plan, t_gains, t_x0, out_stats=t_stats, i0=4, i1=5),
    )
    for k, call in calls.items():
        rec["refusal_" + k] = np.array(refusal(call))
    torch.cuda.synchronize()


def receding_horizon(rec):
    """RecedingHorizon: a start and two ticks with gains=True and control() between them, beside the same loop with the defaults"""
    cfg, _ = dc.tracking_case(B, MISSION, SEED, shared=True)
    des = cfg["desired"]
    init = dc.start_from(np.repeat(des[None, :N], B, axis=0), np.arange(B), SEED)
    s, s_plain = capi.from_config(cfg), capi.from_config(cfg)
    rh, plain = mpc.RecedingHorizon(s, B, N), mpc.RecedingHorizon(s_plain, B, N)
    rec["refusal_control_without_gains"] = np.array(refusal(lambda: plain.control(init[:, 0, 1:14])))
    res, res_plain = rh.start(init, gains=True), plain.start(init)
    for tick in range(3):
        if tick:
            x0 = res["traj"][:, 1, 1:14].clone()
            res, res_plain = rh.tick(x0, gains=True), plain.tick(x0)
        torch.cuda.synchronize()
        tag = "tick%d_" % tick
        rec[tag + "keys"], rec[tag + "plain_keys"] = np.array(sorted(res)), np.array(sorted(res_plain))
        for k in ("traj", "cost", "status", "iters", "u0"):
            rec[tag + k], rec[tag + "plain_" + k] = res[k].cpu().numpy(), res_plain[k].cpu().numpy()
        plan, gains = res["traj"].cpu().numpy(), res["gains"].cpu().numpy()
        rec[tag + "gains"] = gains
        rec[tag + "host_gains"] = s.backwards_pass(plan)[0]  # (at the handle's horizon start: the one the plan was solved at)
        for i in (0, 3):
            x = cn.sample_states(plan, 1, i, SEED + 10 * tick + i)[:, 0]
            rec[tag + "control%d" % i] = rh.control(x, i).cpu().numpy()
            rec[tag + "host_control%d" % i] = s.closed_loop(plan, gains, x, i0=i, i1=i, stats=False)["traj"][:, 0, i, 14:18]
        rec[tag + "control_on_plan"] = rh.control(res["traj"][:, 0, 1:14], 0).cpu().numpy()
    rec["plain_allocated_gains"] = np.array(plain.gains is not None or plain._ctl is not None)


if __name__ == "__main__":
    rec = {}
    device_forms(rec)
    receding_horizon(rec)
    np.savez(sys.argv[1], **rec)
