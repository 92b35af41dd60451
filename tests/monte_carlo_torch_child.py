"""quadrotorilqr_amd.mpc.RecedingHorizon.evaluate_sampled and the torch forms of the Monte-Carlo calls (QuadrotorILQRBatch.sample_gusts_device,
sample_states_device, reduce_scores_device), run in a process of their own for tests/test_gpu_monte_carlo.py, for the reason
tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records, asserts
nothing: the test reads the arrays this writes.  usage: python -m tests.monte_carlo_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc  # noqa: E402

SEED, B, N, S, MISSION = 33, 3, 24, 70, 28
SIGMA12 = np.array([0.05, 0.04, 0.06, 0.03, 0.02, 0.04, 0.1, 0.12, 0.08, 0.05, 0.06, 0.04])
GUST = dict(sigma=[1.0, 0.8, 0.6, 0.03, 0.02, 0.04], mean=[0.3, -0.2, 0.1, 0.0, 0.01, 0.0], tau_force_s=0.4, tau_torque_s=0.1)


def refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the kind and the text are what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return "accepted"


def spheres(des):
    """8 shared spheres about the desired path, some in the way"""
    r = np.random.default_rng(SEED)
    out = np.zeros((8, 5))
    for j in range(8):
        out[j, :3] = des[2 + 3 * (j % 7), 1:4] + 0.3 * (2.0 * r.random(3) - 1.0)
        out[j, 3], out[j, 4] = 0.12 + 0.04 * (j % 3), 20.0 + 5.0 * j
    return out


def flights(rec, tag, integrator, limits):
    cfg, _ = dc.tracking_case(B, MISSION, SEED, shared=True)
    des = cfg["desired"]
    init = dc.start_from(np.repeat(des[None, :N], B, axis=0), np.arange(B), SEED)
    s = capi.from_config(cfg)
    s.set_integrator(integrator)
    if limits:
        s.set_control_limits(*limits)
    s.set_obstacles(spheres(des))
    rh = mpc.RecedingHorizon(s, B, N)
    if not integrator:
        rec["refusal_without_gains"] = np.array(refusal(lambda: rh.evaluate_sampled(np.zeros((B, 13)), S, 1, 0.1)))
    res = rh.start(init, gains=True)
    torch.cuda.synchronize()
    plan = res["traj"].cpu().numpy()
    x = np.ascontiguousarray(cn.sample_states(plan, 1, 0, SEED + 3)[:, 0])  # the measured states: off the plan
    rec[tag + "x"], rec["dt"] = x, np.array(float(cfg["dt"]))
    # two calls in a row on the same buffers, with two seeds and two gust lengths' worth of buffers kept apart by n_w; nothing is waited
    # for in between but by torch's stream, which copies the first call's results before the second overwrites them
    kept = []
    for call, (seed, n_w) in enumerate(((SEED + 10, N), (SEED + 11, N), (SEED + 12, 1))):
        got = rh.evaluate_sampled(x if call else torch.from_numpy(x).to(rh.device), S, seed, SIGMA12, gust=GUST, n_w=n_w)
        kept.append({k: v.clone() for k, v in got.items()})
        kept[-1]["x0"], kept[-1]["wrench"] = rh.sampled[0].clone(), rh.sampled[1].clone()
    torch.cuda.synchronize()
    for call, keep in enumerate(kept):
        ctag = "%scall%d_" % (tag, call)
        for k, v in keep.items():
            rec[ctag + k] = v.cpu().numpy()
        # the parent's way, fed what was sampled: the same flights from host arrays
        host = rh.evaluate(rec[ctag + "x0"], rec[ctag + "wrench"])
        rec[ctag + "host_stats"], rec[ctag + "host_score"] = host["stats"].cpu().numpy(), host["score"].cpu().numpy()
    # no gust, the nominal flag: sample 0 is the flight of closed_loop_device from the measured state
    calm = rh.evaluate_sampled(x, S, SEED + 13, SIGMA12)
    rec[tag + "calm_stats"], rec[tag + "calm_score"], rec[tag + "calm_summary"] = (calm[k].cpu().numpy() for k in ("stats", "score", "summary"))
    rec[tag + "calm_x0"] = rh.sampled[0].cpu().numpy()
    rec[tag + "calm_wrench_is_none"] = np.array(rh.sampled[1] is None)
    dev = rh.device
    t_stats, t_score = (torch.zeros((B, 1, 4), dtype=torch.float64, device=dev) for _ in range(2))
    s.closed_loop_device(res["traj"], rh.gains, torch.from_numpy(x[:, None]).to(dev).contiguous(), out_stats=t_stats, out_score=t_score)
    torch.cuda.current_stream(dev).wait_event(rh._stream.record_event())
    rec[tag + "nominal_stats"], rec[tag + "nominal_score"] = t_stats.cpu().numpy(), t_score.cpu().numpy()
    unflagged = rh.evaluate_sampled(x, S, SEED + 13, SIGMA12, first_is_nominal=False)
    rec[tag + "unflagged_x0"] = rh.sampled[0].cpu().numpy()
    rec[tag + "unflagged_score"] = unflagged["score"].cpu().numpy()
    if integrator:
        return
    # the torch forms' checks
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    calls = dict(
        gusts_shape=lambda: s.sample_gusts_device(t(B, S, N, 5), 1, 1.0),
        gusts_float32=lambda: s.sample_gusts_device(t(B, S, N, 6).float(), 1, 1.0),
        gusts_host=lambda: s.sample_gusts_device(t(B, S, N, 6).cpu(), 1, 1.0),
        gusts_sigma=lambda: s.sample_gusts_device(t(B, S, N, 6), 1, [1.0, 2.0, 3.0]),
        gusts_negative=lambda: s.sample_gusts_device(t(B, S, N, 6), 1, -1.0),
        states_shape=lambda: s.sample_states_device(t(B + 1, 13), t(B, S, 13), 1, 0.1),
        states_sigma=lambda: s.sample_states_device(t(B, 13), t(B, S, 13), 1, [0.1] * 11),
        reduce_shape=lambda: s.reduce_scores_device(t(B, S, 4), t(B, 7)),
        sampled_n_w=lambda: rh.evaluate_sampled(x, S, 1, 0.1, gust=GUST, n_w=2),
        sampled_x=lambda: rh.evaluate_sampled(np.zeros((B, S, 13)), S, 1, 0.1),
        fine=lambda: (s.sample_gusts_device(t(B, S, 1, 6), 1, [1.0, 0.1], tau_force_s=0.2), s.sample_states_device(t(B, 13), t(B, S, 13), 1, 0.0),
                      s.reduce_scores_device(t(B, S, 4), t(B, 8))),
    )
    for k, call in calls.items():
        rec["refusal_" + k] = np.array(refusal(call))
    torch.cuda.synchronize()


if __name__ == "__main__":
    rec = {}
    flights(rec, "euler_", 0, None)
    flights(rec, "rk4_limits_", 1, (1.0, 4.0))
    np.savez(sys.argv[1], **rec)
