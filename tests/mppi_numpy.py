"""The sampling planner (qilqr_mppi_flight_device, qilqr_mppi_update_device) restated from their definition in include/quadrotor_ilqr.h,
sharing no text with the library: the perturbations over tests/monte_carlo_numpy.py's draws (stream 2), the open-loop flight over the
oracle's step and tests/scored_flight_numpy.py's knot score, the update with math.fsum for its sums (so that the restatement's own sums
carry one rounding).  The comparand of tests/test_mppi_cpu.py and tests/test_gpu_mppi.py.

The bounds, derived and not tuned:
  a perturbation word   atol 1e-12 max(sigma_a, 1): the gust word's bar of tests/monte_carlo_numpy.py (the recursion is a contraction)
  a score               rtol = atol = 1e-10, tests/scored_flight_numpy.py's; knot and collision count exactly, after
                        the restatement's own margins
  a new control         update_bound() below
"""
import math

import numpy as np

from oracle import oracle as orc
from tests import monte_carlo_numpy as mn, moving_obstacle_numpy_ilqr as mov, scored_flight_numpy as sn

STREAM_CONTROLS = 2
EPS = 2.0 ** -53


def coeffs(sigma, tau_s, dt):
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (4,))
    rho = math.exp(-dt / tau_s) if tau_s > 0 else 0.0
    return sigma, rho, sigma * math.sqrt((1.0 - rho) * (1.0 + rho))


def eps_atol(sigma):
    return mn.NORMAL_ATOL * max(float(np.max(sigma)), 1.0)


def perturbations(seed, B, S, n, dt, sigma, tau_s=0.0, b0=0, first_is_nominal=False):
    """eps (B, S, n, 4): g_0 = sigma xi_0, g_i = rho g_{i-1} + kappa xi_i; xi normal a % 2 of pair a // 2 of row i"""
    sigma, rho, kappa = coeffs(sigma, tau_s, dt)
    b, s, i, j = np.meshgrid(np.arange(B) + b0, np.arange(S), np.arange(n), np.arange(2), indexing="ij")
    z0, z1 = mn.draws(seed, b, s, i, STREAM_CONTROLS, j)
    xi = np.stack([z0, z1], axis=-1).reshape(B, S, n, 4)
    out = np.empty_like(xi)
    g = sigma * xi[:, :, 0]
    out[:, :, 0] = g
    for k in range(1, n):
        g = rho * g + kappa * xi[:, :, k]
        out[:, :, k] = g
    if first_is_nominal:
        out[:, 0] = 0.0
    return out


def flight(plan, x0, eps, model, dt, Q, R, desired, integrator=0, models=None, limits=None, Qs=None, shared=None, own=None):
    """plan (B, n, 18), x0 (B, 13) or None (the plan's knot 0), eps (B, S, n, 4) -> score (B, S, 4), clear (B, S, n): every knot's smallest
    clearance, gap: the least distance of an unclamped control to a limit (inf without limits), traj (B, S, n, 18).
    desired: (n, 18) the window of the handle's desired trajectory, or (B, n, 18) one per plan.  Qs: None or (n, 144) the window of a
    schedule.  models: a list of B dicts (plan b flies with model b).  shared: (K, 5) spheres; own: a list of B arrays (K_b, 8)."""
    plan, eps = np.asarray(plan, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    B, n, S = plan.shape[0], plan.shape[1], eps.shape[1]
    score, clear_all, traj = np.zeros((B, S, 4)), np.full((B, S, n), np.nan), np.zeros((B, S, n, 18))
    shared = np.zeros((0, 5)) if shared is None else np.asarray(shared, dtype=np.float64).reshape(-1, 5)
    desired = np.asarray(desired, dtype=np.float64)
    gap = np.inf
    if limits is not None:
        lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (4,)) for v in limits)
    for b in range(B):
        des = desired[b] if desired.ndim == 3 else desired
        mine = np.zeros((0, 8)) if own is None else np.asarray(own[b], dtype=np.float64).reshape(-1, 8)
        mp = orc.model_params(**(models[b] if models is not None else model))
        for j in range(S):
            x = np.array(plan[b, 0, 1:14] if x0 is None else x0[b], dtype=np.float64)
            cost, hits, best, best_knot = 0.0, 0, np.inf, -1
            for i in range(n):
                u = plan[b, i, 14:18] + eps[b, j, i]
                if limits is not None:
                    gap = min(gap, float(np.abs(u - lo).min()), float(np.abs(u - hi).min()))
                    u = np.minimum(np.maximum(u, lo), hi)
                traj[b, j, i, 0], traj[b, j, i, 1:14], traj[b, j, i, 14:18] = plan[b, i, 0], x, u
                spheres = np.vstack([shared, mov.at_time(mine, i * dt)])
                kc, kmin, _ = sn.knot_score(x, u, Q if Qs is None else np.asarray(Qs[i]).reshape(12, 12), R, des[i], spheres)
                cost += kc
                clear_all[b, j, i] = kmin
                if kmin < best:
                    best, best_knot = kmin, i
                hits += int(kmin < 0.0)
                if i < n - 1:
                    x = orc.discrete_step(mp, integrator, x, u, dt)
            score[b, j] = (cost, best, best_knot, hits)
    return score, clear_all, gap, traj


def keys(score, collision_cost):
    score = np.asarray(score, dtype=np.float64)
    return np.where(score[..., 3] > 0, score[..., 0] + collision_cost * score[..., 3], score[..., 0])


def update(plan, score, eps, lambda_, collision_cost=0.0, limits=None):
    """-> (u (B, n, 4) the new controls, info (B, 4): J_min, its sample, the effective sample size, the finite keys, scale (B, n, 4):
    sum_j w_j |eps_j| / eta, what update_bound() scales by)"""
    plan, eps = np.asarray(plan, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    B, n = plan.shape[:2]
    J = keys(score, collision_cost)
    u, info, scale = plan[:, :, 14:18].copy(), np.zeros((B, 4)), np.zeros((B, n, 4))
    for b in range(B):
        fin = np.isfinite(J[b])
        if not fin.any():
            info[b] = (np.nan, -1, 0, 0)
            continue
        jmin = J[b][fin].min()
        w = np.array([math.exp(-(k - jmin) / lambda_) if f else 0.0 for k, f in zip(J[b], fin)])
        eta = math.fsum(w)
        info[b] = (jmin, np.flatnonzero(fin & (J[b] == jmin))[0], eta * eta / math.fsum(w * w), fin.sum())
        for i in range(n):
            for a in range(4):
                u[b, i, a] = plan[b, i, 14 + a] + math.fsum(w * eps[b, :, i, a]) / eta
                scale[b, i, a] = math.fsum(w * np.abs(eps[b, :, i, a])) / eta
    if limits is not None:
        lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (4,)) for v in limits)
        u = np.minimum(np.maximum(u, lo), hi)
    return u, info, scale


def update_lanes(S):
    T = 64
    while T < S and T < 1024:
        T *= 2
    return T


def update_bound(scale, S, sigma):
    """The first-order bound on |du_library - du_restatement|, per word.  du = N / D with N = sum w_j eps_j and D = sum w_j over the same
    keys, so the exponent's argument -(J - J_min) / lambda has the same bits on both sides.  Relative errors, in units of 2^-53:
        a weight          4: the device's exp within 3 ulp (OpenCL's table for double), the host's within 1 -- once in N, once in D
        a product w eps   1 (the library rounds it before it adds)
        the additions     one rounding each on the longest path of the fixed order: cdiv(S, T) in the lane's fold, 6 in the butterfly,
                          T / 64 - 1 over the wavefronts (T the lanes of the block) -- once in N, once in D
        the quotient and the sum plan_u + du: 2
    and every eps carries the draws' own bar (eps_atol: absolute, and sum w atol / eta = atol).  The relative part scales
    sum_j w_j |eps_j| / eta (the terms' magnitudes, not their sum's: cancellation does not help), and the whole is doubled."""
    T = update_lanes(S)
    path = -(-S // T) + 6 + (T // 64 - 1)
    rel = (4 + 4 + 1 + 2 * path + 2) * EPS
    return 2.0 * (rel * np.asarray(scale) + eps_atol(sigma))
