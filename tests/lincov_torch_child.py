"""quadrotorilqr_amd.mpc.RecedingHorizon.evaluate_covariance and the torch form of the covariance call
(QuadrotorILQRBatch.covariance_device), run in a process of their own for tests/test_gpu_covariance.py, for the reason
tests/shift_torch_child.py gives: PyTorch's ROCm runtime has to be the first one a process initialises.  Computes and records, asserts
nothing: the test reads the arrays this writes.  usage: python -m tests.lincov_torch_child OUT.npz"""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda")

from quadrotorilqr_amd import capi, mpc  # noqa: E402
from tests import lincov_cases as lc  # noqa: E402


def refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the kind and the text are what is recorded)
        return "%s: %s" % (type(e).__name__, e)
    return "accepted"


if __name__ == "__main__":
    rec = {}
    cfg, init, shared = lc.torch_case()
    s = capi.from_config(cfg)
    s.set_integrator(1)
    s.set_obstacles(shared)
    rh = mpc.RecedingHorizon(s, lc.B, lc.N)
    rec["refusal_without_gains"] = np.array(refusal(lambda: rh.evaluate_covariance(lc.SIGMA12)))
    res = rh.start(init, gains=True)
    got = rh.evaluate_covariance(lc.SIGMA12, gust=lc.TORCH_GUST, cov=True)
    rec["rh_summary"], rec["rh_cov"] = got["summary"].cpu().numpy(), got["cov"].cpu().numpy()
    only = rh.evaluate_covariance(lc.SIGMA12, gust=lc.TORCH_GUST)
    rec["rh_summary_only"], rec["cov_is_none"] = only["summary"].cpu().numpy(), np.array(only["cov"] is None)
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=rh.device)
    d_cov, d_sum = t(lc.B, lc.N, capi.COV), t(lc.B, capi.COV_SUMMARY)
    s.covariance_device(res["traj"], rh.gains, lc.SIGMA12, gust=lc.TORCH_GUST, cov=d_cov, summary=d_sum)
    torch.cuda.current_stream(rh.device).wait_event(rh._stream.record_event())
    rec["direct_cov"], rec["direct_summary"] = d_cov.cpu().numpy(), d_sum.cpu().numpy()
    rec["refusal_shape"] = np.array(refusal(lambda: s.covariance_device(res["traj"], rh.gains, lc.SIGMA12, cov=t(lc.B, lc.N, 143))))
    torch.cuda.synchronize()
    rec["plan"], rec["gains"] = res["traj"].cpu().numpy(), rh.gains.cpu().numpy()
    np.savez(sys.argv[1], **rec)
