"""quadrotorilqr_amd.mpc.RecedingHorizon.evaluate_sampled with candidates and risk levels, and RecedingHorizon.select, run in a process of
their own for tests/test_gpu_risk.py, for the reason tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a
process initialises.  Computes and records, asserts nothing: the test reads the arrays this writes.
usage: python -m tests.risk_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc  # noqa: E402
from tests import closed_loop_numpy as cn, desired_cases as dc  # noqa: E402
from tests.monte_carlo_torch_child import GUST, SIGMA12, refusal, spheres  # noqa: E402

SEED, V, C, N, S, MISSION = 33, 3, 4, 24, 70, 28
B = V * C
DISPLACED, KNOT_HIT, OFFSET = 2, 12, np.array([0.0, 3.0, 0.0])  # the candidate whose plan is moved into the sphere, where, and by what


def same_plans(obstacles):
    """a RecedingHorizon of V vehicles x C candidates whose candidates all hold the vehicle's plan and gains, word for word, and the
    measured states (B, 13), the same for every candidate of a vehicle"""
    cfg, _ = dc.tracking_case(B, MISSION, SEED, shared=True)
    des = cfg["desired"]
    init = dc.start_from(np.repeat(des[None, :N], B, axis=0), np.arange(B), SEED)
    s = capi.from_config(cfg)
    s.set_obstacles(obstacles(des))
    rh = mpc.RecedingHorizon(s, B, N)
    rh.start(init, gains=True)
    buf = rh._buf[rh._cur]
    buf.copy_(buf[:V].repeat(C, 1, 1))
    rh.gains.copy_(rh.gains[:V].repeat(C, 1, 1))
    torch.cuda.synchronize()
    plan = buf.cpu().numpy()
    x = np.ascontiguousarray(cn.sample_states(plan, 1, 0, SEED + 3)[:, 0])
    x[:] = np.tile(x[:V], (C, 1))
    return s, rh, plan, x


def record(rec, tag, res, sel=None):
    for k, v in res.items():
        rec[tag + k] = v.cpu().numpy()
    for k, v in (sel or {}).items():
        rec[tag + "sel_" + k] = v.cpu().numpy()


def common_random_numbers(rec):
    s, rh, plan, x = same_plans(spheres)
    rec["crn_plan"], rec["crn_gains"] = plan, rh.gains.cpu().numpy()
    for S_now in (S, 5):  # (V S even, and odd: the sampled states then go through the copy with padded candidates)
        tag = "crn%d_" % S_now
        res = rh.evaluate_sampled(x, S_now, SEED + 20, SIGMA12, gust=GUST, candidates=C, risk_levels=(0.5, 0.9))
        record(rec, tag, res, rh.select(C, objective="cvar", level=1))
        rec[tag + "x0"] = rh.sampled[0].cpu().numpy()
    # what select() says without what it needs
    rh.evaluate_sampled(x, 5, SEED + 20, SIGMA12, candidates=C)
    rec["refusal_select_without_risk"] = np.array(refusal(lambda: rh.select(C, objective="cvar")))
    rec["refusal_select_mean_is_fine"] = np.array(refusal(lambda: rh.select(C, objective="mean")))
    rh.evaluate_sampled(x, 5, SEED + 20, SIGMA12, candidates=C, risk_levels=(0.5,), risk_column="clearance")
    rec["refusal_select_clearance_risk"] = np.array(refusal(lambda: rh.select(C, objective="var")))
    rec["refusal_candidates"] = np.array(refusal(lambda: rh.evaluate_sampled(x, 5, 1, 0.1, candidates=5)))
    rec["refusal_select_c"] = np.array(refusal(lambda: rh.select(5)))
    dev = rh.device
    t = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    calls = dict(
        risk_shape=lambda: s.risk_scores_device(t(B, S, 4), t(B, 3, 4), (0.5, 0.9)),
        risk_levels=lambda: s.risk_scores_device(t(B, S, 4), t(B, 9, 4), [0.1] * 9),
        risk_column=lambda: s.risk_scores_device(t(B, S, 4), t(B, 1, 4), 0.5, column="hits"),
        risk_level_one=lambda: s.risk_scores_device(t(B, S, 4), t(B, 1, 4), 1.0),
        select_choice_dtype=lambda: s.select_plans_device(t(B, 8), C, t(V), t(V, 4), objective="mean"),
        select_partial=lambda: s.select_plans_device(t(B, 8), C, t(V, dtype=torch.int32), t(V, 4), objective="mean", plan=t(B, N, 18)),
        select_multiple=lambda: s.select_plans_device(t(B, 8), 5, t(V, dtype=torch.int32), t(V, 4), objective="mean"),
        fine=lambda: (s.risk_scores_device(t(B, S, 4), t(B, 2, 4), (0.5, 0.9), column="clearance"),
                      s.select_plans_device(t(B, 8), C, t(V, dtype=torch.int32), t(V, 4), objective="worst")),
    )
    for k, call in calls.items():
        rec["refusal_" + k] = np.array(refusal(call))
    torch.cuda.synchronize()


def a_real_choice(rec):
    """one sphere 3 m off the path; candidate DISPLACED of every vehicle flies its plan moved by those 3 m, from states moved with it"""
    def one_sphere(des):
        return np.array([[*(des[2 + KNOT_HIT, 1:4] + OFFSET), 0.3, 20.0]])

    s, rh, plan, x = same_plans(one_sphere)
    rows = slice(DISPLACED * V, (DISPLACED + 1) * V)
    buf = rh._buf[rh._cur]
    centre = torch.from_numpy(one_sphere(dc.tracking_case(B, MISSION, SEED, shared=True)[0]["desired"])[0, :3]).to(rh.device)
    move = centre - buf[rows, KNOT_HIT, 1:4]  # (V, 3): knot KNOT_HIT of the moved plan is the sphere's centre
    buf[rows, :, 1:4] += move[:, None, :]
    x[rows, 0:3] += move.cpu().numpy()
    torch.cuda.synchronize()
    rec["choice_plan"], rec["choice_gains"] = buf.cpu().numpy(), rh.gains.cpu().numpy()
    res = rh.evaluate_sampled(x, S, SEED + 21, SIGMA12, gust=GUST, candidates=C, risk_levels=(0.9,))
    record(rec, "choice_", res, rh.select(C, objective="cvar", level=0, max_collision_fraction=0.0))
    record(rec, "choice_mean_", {}, rh.select(C, objective="mean", max_collision_fraction=0.0))


def defaults(rec):
    cfg, _ = dc.tracking_case(V, MISSION, SEED, shared=True)
    des = cfg["desired"]
    s = capi.from_config(cfg)
    s.set_obstacles(spheres(des))
    rh = mpc.RecedingHorizon(s, V, N)
    res = rh.start(dc.start_from(np.repeat(des[None, :N], V, axis=0), np.arange(V), SEED), gains=True)
    torch.cuda.synchronize()
    x = np.ascontiguousarray(cn.sample_states(res["traj"].cpu().numpy(), 1, 0, SEED + 3)[:, 0])
    a = {k: v.clone() for k, v in rh.evaluate_sampled(x, S, SEED + 22, SIGMA12, gust=GUST).items()}
    b = rh.evaluate_sampled(x, S, SEED + 22, SIGMA12, gust=GUST, risk_levels=None, risk_column="cost", candidates=1)
    rec["defaults_keys_a"], rec["defaults_keys_b"] = np.array(sorted(a)), np.array(sorted(b))
    record(rec, "defaults_a_", a)
    record(rec, "defaults_b_", b)
    torch.cuda.synchronize()


if __name__ == "__main__":
    rec = {}
    common_random_numbers(rec)
    a_real_choice(rec)
    defaults(rec)
    np.savez(sys.argv[1], **rec)
