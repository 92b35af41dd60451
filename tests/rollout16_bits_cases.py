"""The cases of tests/test_gpu_rollout_same_bits.py and of its recorder (tests/golden/make_rollout16_bits.py): inputs of forward_sim at the
smallest shapes at which each branch of k_rollout16's step exists, made of integer hashes, IEEE divisions and square roots only
(problems.counter_uniform) -- the same bytes on every machine; the fixture holds their digest beside the recorded result.

Shapes:  n = 1 (no advance, the odd wavefront has no knot), 2 ("step -1" only), 3 and 4 (the first T hand-off, the discarded step after the
last knot on either parity), 7 (operands requested ahead -- seen >= i + 3 -- with both register sets), 18 (one R16_CHUNK announcement);
B = 1 (one live row, three rows alias it) and B = 5 (a second, ragged block).
Rows:    hover      the rollout sits on its nominal trajectory exactly: the small-angle selects of Log, Exp and the Jacobian coefficient
         perturbed  a nominal trajectory that is not a flight, a start beside its first knot: the series
         spin16     a start with |dt omega|^2 = 2.25: Exp's sixteen-term series (EXP_MAX = 0.25 < x <= EXP2_MAX = 12), Log's closed forms
         spinfar    |dt omega|^2 = 16 > EXP2_MAX: the out-of-line closed forms of Exp
Gains of order 1e-1, step sizes 1 and 0.25, fp64 and fp32 storage (precision = 1)."""
import hashlib

import numpy as np

from quadrotorilqr_amd import problems as pb

NS = (1, 2, 3, 4, 7, 18)
ALPHAS = (1.0, 0.25)
PRECISIONS = ("f64", "f32")
MIXED = ("hover", "perturbed", "spin16", "spinfar", "perturbed")  # the rows of a B = 5 case
SINGLE = ("perturbed", "spinfar")                                   # B = 1
SOLVE_B, SOLVE_N, SOLVE_SEED = 8, 12, 21
SOLVE_KEYS = ("status", "iters", "n_bwd", "n_fwd", "cost")


def _u(seed, count, lo, hi):
    """`count` values in [lo, hi) keyed by seed"""
    return lo + (hi - lo) * pb.counter_uniform(seed, np.arange(count), 7)


def row(kind, n, seed):
    """(nominal trajectory (n, 18) with the start state in knot 0, gains (n, 52) = [k(4) | K column-major]) of one trajectory"""
    dt, uh = pb.DT_DEMO, pb.hover_thrust(pb.MODEL_A)
    traj = pb.hover_desired(n, dt, uh)
    gains = np.zeros((n, 52))
    gains[:, 4:] = _u(seed, n * 48, -0.1, 0.1).reshape(n, 48)
    if kind == "hover":
        traj[:, 1:4] = np.array([0.5, -0.25, 2.0])  # (the feed-forward term stays zero: the rollout repeats the nominal controls)
        return traj, gains
    gains[:, :4] = _u(seed + 1, n * 4, -0.1, 0.1).reshape(n, 4)
    traj[:, 1:4] = _u(seed + 2, n * 3, -0.5, 0.5).reshape(n, 3)
    q = np.concatenate([np.ones((n, 1)), _u(seed + 3, n * 3, -0.15, 0.15).reshape(n, 3)], 1)
    traj[:, 4:8] = q / np.sqrt((q * q).sum(1))[:, None]
    traj[:, 8:14] = _u(seed + 4, n * 6, -0.3, 0.3).reshape(n, 6)
    traj[:, 14:18] = uh + _u(seed + 5, n * 4, -0.2, 0.2).reshape(n, 4)
    # the start: beside the nominal trajectory's first knot
    traj[0, 1:4] += _u(seed + 6, 3, -0.3, 0.3)
    q0 = traj[0, 4:8] + np.concatenate([[0.0], _u(seed + 7, 3, -0.12, 0.12)])
    traj[0, 4:8] = q0 / np.sqrt((q0 * q0).sum())
    traj[0, 8:14] += _u(seed + 8, 6, -0.5, 0.5)
    if kind != "perturbed":
        w = {"spin16": 15.0, "spinfar": 40.0}[kind]  # |dt omega| = 1.5, 4.0
        traj[0, 11:14] = w * np.array([2.0, -1.0, 2.0]) / 3.0
    return traj, gains


def cases():
    """[(id, precision, n, kinds of the rows, alpha)]"""
    out = []
    for prec in PRECISIONS:
        for n in NS:
            for alpha in ALPHAS:
                out.append((f"{prec}-n{n}-B5-mixed-a{alpha}", prec, n, MIXED, alpha))
                for kind in SINGLE:
                    out.append((f"{prec}-n{n}-B1-{kind}-a{alpha}", prec, n, (kind,), alpha))
    return out


def inputs(n, kinds):
    rows = [row(kind, n, 1000 * n + 100 * r + 11) for r, kind in enumerate(kinds)]
    return np.ascontiguousarray(np.stack([t for t, _ in rows])), np.ascontiguousarray(np.stack([g for _, g in rows]))


def digest(traj, gains):
    return np.frombuffer(hashlib.sha256(traj.tobytes() + gains.tobytes()).digest(), dtype=np.uint8)


def rollout(capi, prec, n, kinds, alpha):
    """forward_sim of one case with the library `capi` is bound to -> (candidate trajectories, digest of the inputs)"""
    traj, gains = inputs(n, kinds)
    cfg = pb.config2(B=len(kinds), N=n)
    s = capi.from_config(cfg, precision=prec)
    out = s.forward_sim(traj, gains, alpha)
    s.close()
    return out, digest(traj, gains)


def solve(capi, rounds_per_launch):
    """the batch solve of the second test -> (results, the handle's description of its kernels)"""
    cfg = pb.config2(B=SOLVE_B, N=SOLVE_N, seed=SOLVE_SEED)
    s = capi.from_config(cfg, rounds_per_launch=rounds_per_launch)
    out, text = s.solve_batch(cfg["init"]), s.describe(SOLVE_B)
    s.close()
    return out, text
