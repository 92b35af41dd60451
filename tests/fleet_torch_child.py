"""quadrotorilqr_amd.mpc.RecedingHorizon with deconflict=... and the torch forms of the two fleet calls
(QuadrotorILQRBatch.fleet_neighbours_device, set_batch_obstacles_device), run in a process of their own for tests/test_gpu_fleet.py, for the
reason tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records,
asserts nothing: the test reads the arrays this writes.  usage: python -m tests.fleet_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc  # noqa: E402
from tests import fleet_cases as fc  # noqa: E402

B, N, DECONFLICT = fc.TORCH_B, fc.TORCH_N, fc.TORCH_DECONFLICT
K = DECONFLICT["K"]


def refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the kind and the text are what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return "accepted"


if __name__ == "__main__":
    rec = {}
    cfg, init = fc.torch_case()
    s = capi.from_config(cfg)
    rh = mpc.RecedingHorizon(s, B, N)
    res = rh.start(init)
    rec["describe_before"] = np.array(s.describe(B))
    x0 = res["traj"][:, 1, 1:14].clone()
    res = rh.tick(x0, deconflict=DECONFLICT, keep_init=True)
    torch.cuda.synchronize()
    rec["tick1_init"], rec["tick1_traj"], rec["tick1_cost"] = rh.init.cpu().numpy(), res["traj"].cpu().numpy(), res["cost"].cpu().numpy()
    rec["tick1_separation"], rec["tick1_neighbours"] = res["separation"].cpu().numpy(), res["neighbours"].cpu().numpy()
    rec["tick1_spheres"], rec["tick1_counts"], rec["tick1_dropped"] = rh._fleet[3].cpu().numpy(), rh._fleet[4].cpu().numpy(), rh._fleet[5].cpu().numpy()
    rec["describe_after"] = np.array(s.describe(B))
    # the direct torch calls on the same shifted plan
    t = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=rh.device)
    d_sum, d_nbr, d_sph, d_cnt = t(B, capi.FLEET_SUMMARY), t(B, K, capi.FLEET_NBR), t(B, K, 8), t(B, dtype=torch.int32)
    kw = {k: v for k, v in DECONFLICT.items() if k != "K"}
    s.fleet_neighbours_device(rh.init, B, K, summary=d_sum, nbr=d_nbr, spheres=d_sph, counts=d_cnt, **kw)
    torch.cuda.current_stream(rh.device).wait_event(rh._stream.record_event())
    rec["direct_summary"], rec["direct_nbr"], rec["direct_spheres"], rec["direct_counts"] = (a.cpu().numpy() for a in (d_sum, d_nbr, d_sph, d_cnt))
    # a tick without deconflict afterwards: the table of the last one is still set
    x0 = res["traj"][:, 1, 1:14].clone()
    res = rh.tick(x0, keep_init=True)
    torch.cuda.synchronize()
    rec["tick2_init"], rec["tick2_traj"] = rh.init.cpu().numpy(), res["traj"].cpu().numpy()
    rec["tick2_has_separation"] = np.array("separation" in res)
    rec["describe_tick2"] = np.array(s.describe(B))
    # what the wrappers refuse
    rec["refusal_keys"] = np.array(refusal(lambda: rh.tick(x0, advance=False, deconflict=dict(radius=1.0, weight=1.0))))
    rec["refusal_fleet"] = np.array(refusal(lambda: rh.tick(x0, advance=False, deconflict=dict(DECONFLICT, fleet=3))))
    rec["refusal_counts_dtype"] = np.array(refusal(lambda: s.set_batch_obstacles_device(d_sph, t(B))))
    rec["refusal_spheres_shape"] = np.array(refusal(lambda: s.fleet_neighbours_device(rh.init, B, K, 1.0, 1.0, spheres=t(B, K, 7))))
    torch.cuda.synchronize()
    np.savez(sys.argv[1], **rec)
