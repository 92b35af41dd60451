"""The cases of tests/test_gpu_rollout_straight_bits.py and of its recorder (tests/golden/make_rollout16_straight_bits.py): inputs of
forward_sim at the smallest shapes at which the rollout step's steady-state loop (rollout16_kernel.h, r16_wave_X: pairs of steps without
per-step decisions, the general step for a wavefront's last knots) can go wrong, with rows whose rare branches first appear in the middle
of that loop.  Built like tests/rollout16_bits_cases.py, of integer hashes, IEEE divisions, square roots and products only; the sines and
cosines of the rotations below are written out as constants, so the inputs are the same bytes on every machine.  The fixture holds their
digest.

Shapes:  n = 5, 6 (the steady-state loop is entered once: by the even wavefront at 5, by both at 6), 16, 17, 19, 20 (the first announcement of a
         chunk of sixteen knots on either wavefront; a wavefront's last knot one and two behind it), 33, 34 (the second chunk);
         B = 1 (one live row, three rows alias it: the wavefront leaves the straight line only when that row does) and B = 5 (four
         different rows in the first block, one in a second); alpha = 1 and 0.25; fp64 and fp32 storage.
Rows:    hover, perturbed, spin16, spinfar: the rows of rollout16_bits_cases (`perturbed`, whose nominal trajectory is not a flight, is in
                    Log's closed form at most knots)
         plain      on the straight line throughout -- the series, nothing rare: a hover as the nominal trajectory, nominal poses,
                    velocities and controls a little beside it, gains of order 1e-2, a start 0.3 m, 0.05 rad and 0.05 rad/s off
         kick16     plain, and the nominal controls of knot K0 hold a torque pulse: |dt omega|^2 goes over EXP_MAX = 0.25 behind K0 --
                    Exp's predicate first appears mid-trajectory, in this row only
         kickfar    the same over EXP2_MAX = 12: the out-of-line closed forms
         logleave   plain, and the nominal attitude turns by 0.8 rad from knot K0 on: s2 > LOG_MAX = 0.0625, Log's closed form
         logflip    the same by 3.5 rad: w <= 0
         normoff    plain, and the nominal quaternions from knot K0 on have |q|^2 - 1 = 4e-9: Log's renormalisation
         startoff   plain, and the start quaternion has |q|^2 - 1 = 6e-9: Log's renormalisation at knot 0 and the compose's in the odd
                    wavefront's first pose (T_1 = T_0 E_0)
         back       hover (on its nominal trajectory exactly, at rest: Exp's small-angle selects at every knot), but the nominal pose of
                    knots K0 and K0 + 1 stands beside the rollout (0.3 m, 0.2 rad; zero gains there, so the rollout does not move): the row
                    is off its nominal trajectory for two knots -- Log's series -- and exactly on it again behind them: the small-angle selects
K0 = 4; at n = 5 and 6, where a condition that appears at knot 4 is never looked at, K0 = 2.
The compose's renormalisation INSIDE the step loop cannot be reached through forward_sim: a pose's quaternion is the renormalised T_1
times increments whose norm is 1 to rounding, far inside manif's 1e-10.
check_row() states what each kind claims about its row in terms of a recorded result; the test applies it to the fixture."""
import hashlib

import numpy as np

from quadrotorilqr_amd import problems as pb
from tests import rollout16_bits_cases as rc

NS = (5, 6, 16, 17, 19, 20, 33, 34)
ALPHAS = (1.0, 0.25)
PRECISIONS = ("f64", "f32")
# the rows of the B = 5 cases (four rows of the first block | the second block's row) and of the B = 1 cases, by step size
MIXES = {1.0: (("plain", "kick16", "plain", "plain", "spin16"), ("plain", "plain", "logleave", "plain", "back")),
         0.25: (("plain", "plain", "plain", "kickfar", "spinfar"), ("hover", "normoff", "perturbed", "plain", "startoff"))}
SINGLES = {1.0: ("plain", "kick16", "logflip"), 0.25: ("plain", "kickfar", "normoff")}
EXP_MAX, EXP2_MAX, LOG_MAX, EPS = 0.25, 12.0, 0.0625, 1e-10

# (sin, cos) of half the angles used: 0.2, 0.8 and 3.5 rad
HALF = {0.2: (0.09983341664682815, 0.9950041652780258), 0.8: (0.3894183423086505, 0.9210609940028851),
        3.5: (0.9839859468739369, -0.17824605564949209)}


def k0(n):
    return 4 if n >= 7 else 2


def _qmul(a, b):
    """Hamilton product of quaternions (w, x, y, z)"""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _turn(angle):
    """rotation by `angle` about (1, 1, 0) / sqrt 2 as (w, x, y, z)"""
    s, c = HALF[angle]
    return np.array([c, s / np.sqrt(2.0), s / np.sqrt(2.0), 0.0])


def plain(n, seed):
    dt, uh = pb.DT_DEMO, pb.hover_thrust(pb.MODEL_A)
    u = lambda s, count, lo, hi: lo + (hi - lo) * pb.counter_uniform(seed + s, np.arange(count), 7)
    traj = pb.hover_desired(n, dt, uh)
    gains = u(0, n * 52, -0.02, 0.02).reshape(n, 52)
    traj[:, 1:4] = np.array([0.5, -0.25, 2.0]) + u(1, n * 3, -0.2, 0.2).reshape(n, 3)
    q = np.concatenate([np.ones((n, 1)), u(2, n * 3, -0.005, 0.005).reshape(n, 3)], 1)
    traj[:, 4:8] = q / np.sqrt((q * q).sum(1))[:, None]
    traj[:, 8:14] = u(3, n * 6, -0.05, 0.05).reshape(n, 6)
    traj[:, 14:18] = uh + u(4, n * 4, -0.005, 0.005).reshape(n, 4)
    # the start: beside the nominal trajectory's first knot
    traj[0, 1:4] += u(5, 3, -0.3, 0.3)
    q0 = traj[0, 4:8] + np.concatenate([[0.0], u(6, 3, -0.02, 0.02)])
    traj[0, 4:8] = q0 / np.sqrt((q0 * q0).sum())
    traj[0, 8:11] += u(7, 3, -0.5, 0.5)
    traj[0, 11:14] = np.array([0.03, -0.025, 0.02]) + u(8, 3, -0.01, 0.01)
    return traj, gains


def row(kind, n, seed):
    """(nominal trajectory (n, 18) with the start state in knot 0, gains (n, 52)) of one trajectory"""
    k = k0(n)
    if kind == "back":
        traj, gains = rc.row("hover", n, seed)
        traj[k:k + 2, 1:4] += 0.3
        traj[k:k + 2, 4:8] = _qmul(traj[k, 4:8], np.array([HALF[0.2][1], HALF[0.2][0], 0.0, 0.0]))
        gains[k:k + 2] = 0.0
        return traj, gains
    if kind in ("hover", "perturbed", "spin16", "spinfar"):
        return rc.row(kind, n, seed)
    traj, gains = plain(n, seed)
    if kind in ("kick16", "kickfar"):
        traj[k, 14:18] += {"kick16": 40.0, "kickfar": 250.0}[kind] * np.array([1.0, 0.0, -1.0, 0.0])
    elif kind in ("logleave", "logflip"):
        for i in range(k, n):
            traj[i, 4:8] = _qmul(traj[i, 4:8], _turn({"logleave": 0.8, "logflip": 3.5}[kind]))
    elif kind == "normoff":
        traj[k:, 4:8] *= 1.0 + 2e-9
    elif kind == "startoff":
        traj[0, 4:8] *= 1.0 + 3e-9
    else:
        assert kind == "plain", kind
    return traj, gains


def cases():
    """[(id, precision, n, kinds of the rows, alpha)]"""
    out = []
    for prec in PRECISIONS:
        for n in NS:
            for alpha in ALPHAS:
                for m, kinds in enumerate(MIXES[alpha]):
                    out.append((f"{prec}-n{n}-B5-mix{m}-a{alpha}", prec, n, kinds, alpha))
                for kind in SINGLES[alpha]:
                    out.append((f"{prec}-n{n}-B1-{kind}-a{alpha}", prec, n, (kind,), alpha))
    return out


def inputs(n, kinds):
    rows = [row(kind, n, 2000 * n + 100 * r + 17) for r, kind in enumerate(kinds)]
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


def conditions(traj, out, dt=pb.DT_DEMO):
    """per knot of one row: |dt omega|^2 of the rollout, and of the rollout's attitude against the nominal one the squared vector part s2,
    the scalar part w and |norm^2 - 1| of the difference quaternion -- what Exp's and Log's branches look at"""
    x = dt * dt * (out[:, 11:14] ** 2).sum(1)
    qd = np.array([_qmul(np.concatenate([qn[:1], -qn[1:]]), q) for qn, q in zip(traj[:, 4:8], out[:, 4:8])])
    s2 = (qd[:, 1:] ** 2).sum(1)
    return x, s2, qd[:, 0], np.abs((qd ** 2).sum(1) - 1.0)


def check_row(kind, n, traj, out):
    """what the kind says about its row, asserted of a result `out` (n, 18); margins of a factor of two against storage rounding"""
    k = k0(n)
    x, s2, w, off = conditions(traj, out)
    calm = (x[:k + 1] < EXP_MAX / 2).all() and (x[:k + 1] > 2 * EPS).all()
    on_series = lambda a, b: (s2[a:b] < LOG_MAX / 2).all() and (s2[a:b] > 2 * EPS).all() and (w[a:b] > 0).all()
    if kind in ("hover", "perturbed", "spin16", "spinfar"):
        return
    if kind == "plain":
        assert (x < EXP_MAX / 2).all() and (x > 2 * EPS).all() and on_series(1, n) and (off[1:] < EPS / 2).all(), (kind, n)
    elif kind == "kick16":
        assert calm and on_series(1, k + 1) and ((x[k + 1:] > 2 * EXP_MAX) & (x[k + 1:] < EXP2_MAX / 2)).all(), (kind, n, x)
    elif kind == "kickfar":
        assert calm and on_series(1, k + 1) and (x[k + 1:] > 2 * EXP2_MAX).any(), (kind, n, x)
    elif kind == "logleave":
        assert on_series(1, k) and (s2[k] > 2 * LOG_MAX) and w[k] > 0 and (x[:k + 2] < EXP_MAX / 2).all(), (kind, n, s2, w)
    elif kind == "logflip":
        assert on_series(1, k) and w[k] < -0.05, (kind, n, s2, w)
    elif kind == "normoff":
        assert (off[1:k] < EPS / 2).all() and (off[k:] > 2 * EPS).all() and on_series(1, n) and (x < EXP_MAX / 2).all(), (kind, n, off)
    elif kind == "startoff":
        assert off[0] > 2 * EPS and (off[1:] < EPS / 2).all() and on_series(1, n), (kind, n, off)
    elif kind == "back":
        assert (x < EPS / 2).all() and (s2[:k] < EPS / 2).all() and on_series(k, k + 2) and (s2[k + 2:] < EPS / 2).all(), (kind, n, x, s2)
    else:
        raise AssertionError(kind)
