"""The torch forms of receding-horizon stepping -- QuadrotorILQRBatch.shift_device and quadrotorilqr_amd.mpc.RecedingHorizon -- run in a
process of their own for tests/test_gpu_shift.py: PyTorch brings its own ROCm runtime, which has to be the first one a process
initialises (as in bench.py), and the pytest process has initialised the library's by then.  Computes and records, asserts nothing: the
test reads the arrays this writes.  usage: python -m tests.shift_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc, problems as pb  # noqa: E402
from tests import desired_cases as dc  # noqa: E402

SEED, B, N, MISSION = 21, 6, 24, 28


def refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the kind and the text are what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return "accepted"


def device_form(rec):
    """shift_device against shift on the same handle, and what the wrapper refuses"""
    Bs, n = 70, 24
    dev = torch.device("cuda", 0)
    s = capi.from_config(pb.config2(B=1, N=8))
    plan = dc.tracking_desired(np.arange(Bs), n, SEED + 1)
    x0 = np.ascontiguousarray(plan[:, 3, 1:14]) + 0.0
    t_in, t_x0 = torch.from_numpy(plan).to(dev), torch.from_numpy(x0).to(dev)
    for tail in ("hold", "hover"):
        t_out = torch.full_like(t_in, float("nan"))
        s.shift_device(t_in, t_out, x0=t_x0, steps=3, tail=tail)
        s.cost_trajectory(plan[:1, :4])  # (enqueued, not drained: a draining call of the handle orders the read below)
        rec["device_" + tail] = t_out.cpu().numpy()
        rec["host_" + tail] = s.shift(plan, x0, 3, tail)
    rec["device_input_after"] = t_in.cpu().numpy()
    rec["device_input"] = plan
    flat = torch.zeros(2 * plan.size, dtype=torch.float64, device=dev)
    a, b = flat[:plan.size].view(Bs, n, 18), flat[plan.size:].view(Bs, n, 18)
    calls = dict(
        same=lambda: s.shift_device(a, a),
        overlap_behind=lambda: s.shift_device(a, flat[plan.size - 36:2 * plan.size - 36].view(Bs, n, 18)),
        overlap_before=lambda: s.shift_device(flat[36:plan.size + 36].view(Bs, n, 18), a),
        overlap_x0=lambda: s.shift_device(a, b, x0=flat[plan.size + 18:plan.size + 18 + Bs * 13].view(Bs, 13)),
        misaligned=lambda: s.shift_device(flat[1:plan.size + 1].view(Bs, n, 18), torch.zeros((Bs, n, 18), dtype=torch.float64, device=dev)),
        strided=lambda: s.shift_device(a, torch.zeros((Bs, n, 36), dtype=torch.float64, device=dev)[:, :, ::2]),
        float32=lambda: s.shift_device(a, torch.zeros((Bs, n, 18), dtype=torch.float32, device=dev)),
        host_tensor=lambda: s.shift_device(a, torch.zeros((Bs, n, 18), dtype=torch.float64)),
        x0_shape=lambda: s.shift_device(a, b, x0=torch.zeros((Bs, 12), dtype=torch.float64, device=dev)),
        tail=lambda: s.shift_device(a, b, tail="coast"),
        steps=lambda: s.shift_device(a, b, steps=n),
        fine=lambda: s.shift_device(a, b, x0=torch.from_numpy(x0).to(dev), steps=2, tail="hover"),
    )
    for k, call in calls.items():
        rec["refusal_" + k] = np.array(refusal(call))
    torch.cuda.synchronize()


def closed_loop(rec):
    """RecedingHorizon over a mission of 28 knots, horizon 24: a start and four ticks with the perfect plant"""
    cfg, _ = dc.tracking_case(B, MISSION, SEED, shared=True)
    des = cfg["desired"]
    s = capi.from_config(cfg)
    rh = mpc.RecedingHorizon(s, B, N)

    def keep(tag, res):
        torch.cuda.synchronize()
        rec[tag + "_init"] = rh.init.cpu().numpy()
        for k in ("traj", "cost", "status", "iters"):
            rec[tag + "_" + k] = res[k].cpu().numpy()
        rec[tag + "_n_bwd"], rec[tag + "_n_fwd"] = rh.n_bwd.cpu().numpy(), rh.n_fwd.cpu().numpy()
        rec[tag + "_u0"] = res["u0"].cpu().numpy()
        rec[tag + "_k0"] = np.array(rh.k0)
        rec[tag + "_describe"] = np.array(s.describe(B))

    init = dc.start_from(np.repeat(des[None, :N], B, axis=0), np.arange(B), SEED)
    rec["loop_init"] = init
    res = rh.start(init, keep_init=True)
    keep("tick0", res)
    for tick in range(1, MISSION - N + 1):
        x0 = res["traj"][:, 1, 1:14]  # the perfect plant: knot 1 of the last plan (a view: tick copies it before the shift)
        rec["tick%d_x0" % tick] = x0.cpu().numpy()
        res = rh.tick(x0, steps=1, tail="hold", keep_init=True)
        keep("tick%d" % tick, res)
    # refused ticks leave the object and the handle as they were: past the mission, and steps out of range
    last = res["traj"].clone()
    rec["refusal_past_the_mission"] = np.array(refusal(lambda: rh.tick(res["traj"][:, 1, 1:14])))
    rec["refusal_tick_steps"] = np.array(refusal(lambda: rh.tick(None, steps=N)))
    rec["after_refusals_k0"] = np.array(rh.k0)
    rec["after_refusals_describe"] = np.array(s.describe(B))
    rec["after_refusals_same_plan"] = np.array(bool((rh._buf[rh._cur] == last).all()))
    again = rh.tick(res["traj"][:, 1, 1:14], advance=False)  # (the same window once more: still served)
    torch.cuda.synchronize()
    rec["after_refusals_status"] = again["status"].cpu().numpy()
    rec["after_refusals_k0_again"] = np.array(rh.k0)


if __name__ == "__main__":
    rec = {}
    device_form(rec)
    closed_loop(rec)
    np.savez(sys.argv[1], **rec)
