"""quadrotorilqr_amd.mpc.RecedingHorizon.evaluate and the torch form of the scored flight (QuadrotorILQRBatch.closed_loop_device with wrench
and out_score), run in a process of their own for tests/test_gpu_scored_flight.py, for the reason tests/shift_torch_child.py gives:
PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records, asserts nothing: the test reads the arrays
this writes.  usage: python -m tests.scored_flight_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc  # noqa: E402

SEED, B, N, S, MISSION = 21, 6, 24, 70, 28


def refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the kind and the text are what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return "accepted"


def evaluate(rec):
    """a start and one tick with gains=True, evaluate() after each: against closed_loop through capi on the same handle and plan"""
    cfg, _ = dc.tracking_case(B, MISSION, SEED, shared=True)
    des = cfg["desired"]
    init = dc.start_from(np.repeat(des[None, :N], B, axis=0), np.arange(B), SEED)
    s = capi.from_config(cfg)
    s.set_obstacles(np.array([[des[6, 1] + 0.2, des[6, 2], des[6, 3], 0.25, 30.0], [des[15, 1], des[15, 2] - 0.2, des[15, 3], 0.2, 0.0]]))
    rh = mpc.RecedingHorizon(s, B, N)
    rec["refusal_evaluate_without_gains"] = np.array(refusal(lambda: rh.evaluate(np.zeros((B, S, 13)))))
    res = rh.start(init, gains=True)
    for tick in range(2):
        if tick:
            res = rh.tick(res["traj"][:, 1, 1:14].clone(), gains=True)
        torch.cuda.synchronize()
        tag = "tick%d_" % tick
        plan, gains = res["traj"].cpu().numpy(), res["gains"].cpu().numpy()
        x0 = cn.sample_states(plan, S, 0, SEED + 3 + tick)
        gust = pb.gust_wrenches(B, S, N if tick else 1, SEED + 5 + tick, 1.0, 0.03)
        got = rh.evaluate(torch.from_numpy(x0).to(rh.device) if tick else x0, gust)
        rec[tag + "keys"] = np.array(sorted(got))
        rec[tag + "stats"], rec[tag + "score"] = got["stats"].cpu().numpy(), got["score"].cpu().numpy()
        host = s.closed_loop(plan, gains, x0, traj=False, wrench=gust, score=True)  # (at the handle's horizon start: the plan's)
        rec[tag + "host_stats"], rec[tag + "host_score"] = host["stats"], host["score"]
        calm = rh.evaluate(x0)
        rec[tag + "calm_score"] = calm["score"].cpu().numpy()
        rec[tag + "host_calm_score"] = s.closed_loop(plan, gains, x0, traj=False, score=True)["score"]
    rec["refusal_x0_shape"] = np.array(refusal(lambda: rh.evaluate(np.zeros((B, 13)))))
    rec["refusal_wrench_shape"] = np.array(refusal(lambda: rh.evaluate(np.zeros((B, S, 13)), np.zeros((B, S + 1, 1, 6)))))
    # the torch form's checks of the new tensors
    dev = rh.device
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    t_x0 = torch.from_numpy(x0).to(dev)
    calls = dict(
        score_shape=lambda: s.closed_loop_device(res["traj"], rh.gains, t_x0, out_score=t(B, S, 3)),
        wrench_float32=lambda: s.closed_loop_device(res["traj"], rh.gains, t_x0, out_score=t(B, S, 4), wrench=t(B, S, 1, 6).float()),
        wrench_rows=lambda: s.closed_loop_device(res["traj"], rh.gains, t_x0, out_score=t(B, S, 4), wrench=t(B, S, 2, 6)),
        desired_host=lambda: s.closed_loop_device(res["traj"], rh.gains, t_x0, out_score=t(B, S, 4), desired=t(B, N, 18).cpu()),
        fine=lambda: s.closed_loop_device(res["traj"], rh.gains, t_x0, out_score=t(B, S, 4), wrench=t(B, S, N, 6), desired=res["traj"].clone()),
    )
    for k, call in calls.items():
        rec["refusal_" + k] = np.array(refusal(call))
    torch.cuda.synchronize()


if __name__ == "__main__":
    rec = {}
    evaluate(rec)
    np.savez(sys.argv[1], **rec)
