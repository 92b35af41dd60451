"""The scored closed-loop flight (qilqr_closed_loop_scored) restated from the oracle's primitives, as include/quadrotor_ilqr.h words it:
the comparand of tests/test_scored_flight_cpu.py (the device routine compiled for the host) and of tests/test_gpu_scored_flight.py (the
kernel).  The flight is tests/closed_loop_numpy.py's with the step disturbed by a wrench: oracle.continuous_dynamics plus the wrench
terms, then oracle.euler_step (for Runge-Kutta, four stages through oracle.state_add).  The score is oracle.cost per knot plus the sphere
terms of tests/obstacle_numpy_ilqr.py and tests/moving_obstacle_numpy_ilqr.py, and the clearances.  NumPy and the CPU oracle only."""
import numpy as np

from oracle import oracle as orc
from tests import closed_loop_numpy as cn, desired_cases as dc, moving_obstacle_numpy_ilqr as mov, obstacle_numpy_ilqr as obs

RTOL, ATOL = cn.RTOL, cn.ATOL  # the bound the project holds this chain of steps to


def disturbed_xdot(mp, x, u, w):
    """the continuous dynamics at x (13) under u and the wrench w = {F world, tau body}: acc_lin += R^T F / m, acc_ang += I^-1 tau"""
    xdot = orc.continuous_dynamics(mp, x, u)
    R = dc._rotmat(np.asarray(x[3:7], dtype=np.float64))
    inertia = np.array(mp.inertia, dtype=np.float64).reshape(3, 3)
    xdot[6:9] += R.T @ w[0:3] / mp.mass_kg
    xdot[9:12] += np.linalg.solve(inertia, w[3:6])
    return xdot


def disturbed_step(mp, integrator, x, u, dt, w):
    """one step under the wrench w held over the step: explicit Euler, or the Runge-Kutta step of oracle.discrete_step (every stage
    from x, R each stage's own)"""
    if integrator == 0:
        return orc.euler_step(x, disturbed_xdot(mp, x, u, w), dt)
    k, xdot = np.zeros(12), np.zeros(12)
    for h, c in ((0.0, 1.0 / 6.0), (dt / 2.0, 2.0 / 6.0), (dt / 2.0, 2.0 / 6.0), (dt, 1.0 / 6.0)):
        k = disturbed_xdot(mp, orc.state_add(x, h * k), u, w)
        xdot += c * k
    return orc.euler_step(x, xdot, dt)


def pose(x):
    T = np.eye(4)
    T[:3, :3] = dc._rotmat(np.asarray(x[3:7], dtype=np.float64))
    T[:3, 3] = x[0:3]
    return T


def knot_score(x, u, Q, R, des, spheres5):
    """(knot cost, smallest clearance) of one flown knot: the tracking cost, then the spheres (K, 5) in order"""
    kc = orc.cost(Q, R, x, u, des[1:14], des[14:18]) + obs.penalty(spheres5, pose(x))
    if len(spheres5) == 0:
        return kc, np.inf, np.zeros(0)
    clear = np.linalg.norm(x[None, 0:3] - spheres5[:, 0:3], axis=1) - spheres5[:, 3]
    return kc, clear.min(), clear


def scored_flight(plan, gains, x0, model, dt, Q, R, desired, i0=0, i1=None, integrator=0, models=None, limits=None, wrench=None, Qs=None,
                  shared=None, own=None):
    """plan (B, n, 18), gains (B, n, 52), x0 (B, S, 13) -> traj (B, S, n, 18; NaN outside i0 .. i1), stats (B, S, 4), score (B, S, 4),
    clear (B, S, n): every knot's smallest clearance (NaN outside the window; +inf without spheres).
    desired: (n, 18) the window of the handle's desired trajectory, or (B, n, 18) one per plan.  Qs: None (Q at every knot) or (n, 144)
    the window of a schedule.  wrench: None, (B, S, 1, 6) or (B, S, n, 6).  shared: (K, 5) spheres; own: a list of B arrays (K_b, 8)."""
    plan, gains, x0 = (np.asarray(a, dtype=np.float64) for a in (plan, gains, x0))
    B, n, S = plan.shape[0], plan.shape[1], x0.shape[1]
    i1 = n - 1 if i1 is None else i1
    _, K = orc.gains_to_kK(gains)
    traj, stats, score = np.full((B, S, n, 18), np.nan), np.zeros((B, S, 4)), np.zeros((B, S, 4))
    clear_all = np.full((B, S, n), np.nan)
    shared = np.zeros((0, 5)) if shared is None else np.asarray(shared, dtype=np.float64).reshape(-1, 5)
    desired = np.asarray(desired, dtype=np.float64)
    if limits is not None:
        lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (4,)) for v in limits)
    for b in range(B):
        des = desired[b] if desired.ndim == 3 else desired
        mine = np.zeros((0, 8)) if own is None else np.asarray(own[b], dtype=np.float64).reshape(-1, 8)
        for j in range(S):
            mp = orc.model_params(**(models[b * S + j] if models is not None else model))
            x = x0[b, j].copy()
            pos = ang = cost = 0.0
            clamped = hits = 0
            best, best_knot = np.inf, -1
            for i in range(i0, i1 + 1):
                dx = orc.state_minus(x, plan[b, i, 1:14])
                u = plan[b, i, 14:18] + K[b, i] @ dx
                if limits is not None:
                    clamped += int(((u < lo) | (u > hi)).sum())
                    u = np.minimum(np.maximum(u, lo), hi)
                pos, ang = max(pos, np.linalg.norm(dx[0:3])), max(ang, np.linalg.norm(dx[3:6]))
                traj[b, j, i, 0] = plan[b, i, 0]
                traj[b, j, i, 1:14] = x
                traj[b, j, i, 14:18] = u
                spheres = np.vstack([shared, mov.at_time(mine, i * dt)])
                kc, kmin, _ = knot_score(x, u, Q if Qs is None else np.asarray(Qs[i]).reshape(12, 12), R, des[i], spheres)
                cost += kc
                clear_all[b, j, i] = kmin
                if kmin < best:
                    best, best_knot = kmin, i
                hits += int(kmin < 0.0)
                if i < i1:
                    if wrench is None:
                        x = orc.discrete_step(mp, integrator, x, u, dt)
                    else:
                        x = disturbed_step(mp, integrator, x, u, dt, wrench[b, j, i if wrench.shape[2] > 1 else 0])
            stats[b, j] = (pos, ang, np.linalg.norm(dx), clamped)
            score[b, j] = (cost, best, best_knot, hits)
    return traj, stats, score, clear_all


def margins(clear):
    """how far the discrete parts of a score are from flipping, from every knot's smallest clearance (B, S, n; NaN outside the window):
    (the least gap between a sample's smallest and second smallest knot clearance, the least |clearance| of any knot)"""
    c = np.where(np.isnan(clear), np.inf, clear)
    s = np.sort(c, axis=2)
    gap = (s[..., 1] - s[..., 0]) if c.shape[2] > 1 else np.full(c.shape[:2], np.inf)
    gap = np.where(np.isfinite(s[..., 1]), gap, np.inf)
    return float(gap.min()), float(np.abs(clear[~np.isnan(clear)]).min()) if (~np.isnan(clear)).any() else np.inf
