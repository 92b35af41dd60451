"""The planner's adapted spread (qilqr_mppi_flight_spread_device, qilqr_mppi_adapt_device) restated from their definition in
include/quadrotor_ilqr.h, sharing no text with the library: the perturbations are tests/mppi_numpy.py's of unit deviation times the
spread, the flight is that file's, the adaptation's sums are math.fsum's (one rounding each).  The comparand of
tests/test_mppi_adapt_cpu.py and tests/test_gpu_mppi_adapt.py.

The bounds, derived and not tuned:
  a perturbation word   atol 1e-12 max(spread, 1): the gust word's bar, scaled by the deviation
  a score               rtol = atol = 1e-10
  a new control         tests/mppi_numpy.py's update_bound
  a variance, a spread  var_bound() and adapt_bound() below
"""
import math

import numpy as np

from tests import monte_carlo_numpy as mn, mppi_numpy as mp

EPS = mp.EPS


def eps_atol(spread):
    return mn.NORMAL_ATOL * max(float(np.max(spread)), 1.0)


def perturbations(seed, spread, S, dt, tau_s=0.0, b0=0, first_is_nominal=False):
    """eps (B, S, n, 4) = spread[b, i, a] z: z the recursion with sigma = 1"""
    spread = np.asarray(spread, dtype=np.float64)
    B, n = spread.shape[:2]
    z = mp.perturbations(seed, B, S, n, dt, 1.0, tau_s=tau_s, b0=b0, first_is_nominal=first_is_nominal)
    return spread[:, None] * z


def adapt(plan, score, eps, spread, lambda_, floor, cap, rate, collision_cost=0.0, limits=None):
    """-> dict: u (B, n, 4) and info (B, 4) and scale as mp.update's; var (B, n, 4) the weighted variances, scale2 = sum w eps^2 / eta,
    v the blended variances, raw = sqrt(v) before the clamp, spread the new one.  Without a finite key var = 0 and the spread is the old."""
    plan, eps, spread = (np.asarray(a, dtype=np.float64) for a in (plan, eps, spread))
    floor, cap = (np.broadcast_to(np.asarray(v, dtype=np.float64), (4,)) for v in (floor, cap))
    B, n = plan.shape[:2]
    u, info, scale = mp.update(plan, score, eps, lambda_, collision_cost, limits)
    J = mp.keys(score, collision_cost)
    var, scale2, v, raw, new = np.zeros((B, n, 4)), np.zeros((B, n, 4)), spread * spread, spread.copy(), spread.copy()
    for b in range(B):
        fin = np.isfinite(J[b])
        if not fin.any():
            continue
        jmin = J[b][fin].min()
        w = np.array([math.exp(-(k - jmin) / lambda_) if f else 0.0 for k, f in zip(J[b], fin)])
        eta = math.fsum(w)
        for i in range(n):
            for a in range(4):
                e = eps[b, :, i, a]
                du = math.fsum(w * e) / eta
                e2 = math.fsum(w * e * e) / eta
                scale2[b, i, a] = e2
                var[b, i, a] = max(e2 - du * du, 0.0)
                v[b, i, a] = (1.0 - rate) * spread[b, i, a] ** 2 + rate * var[b, i, a]
                raw[b, i, a] = math.sqrt(v[b, i, a])
                new[b, i, a] = min(max(raw[b, i, a], floor[a]), cap[a])
    return dict(u=u, info=info, scale=scale, var=var, scale2=scale2, v=v, raw=raw, spread=new, floor=floor, cap=cap)


def var_bound(scale, scale2, S, spread):
    """The first-order bound on |var_library - var_restatement|, per word; var = M2 / D - (M1 / D)^2 over the same keys.  Relative errors
    in units of 2^-53, with path = cdiv(S, T) + 6 + T / 64 - 1 the additions on the longest path of the fixed order (update_bound's):
        M2 / D     a weight 4 in M2 and 4 in D, the two products w eps and (w eps) eps 2, the additions 2 path, the quotient 1
                   -- times sum w eps^2 / eta (scale2)
        (M1 / D)^2 du carries update_bound's relative part without the sum plan_u + du, r1 = 4 + 4 + 1 + 2 path + 1, times
                   sum w |eps| / eta (scale) >= |du|; the square doubles it and rounds once: (2 r1 + 1) scale^2
        the difference rounds once: at most scale2
    and every eps carries the draws' own bar a = eps_atol(spread) (d(eps^2) = 2 |eps| a, d(du^2) = 2 |du| a): 4 scale a.  Doubled."""
    T = mp.update_lanes(S)
    path = -(-S // T) + 6 + (T // 64 - 1)
    r2 = 4 + 4 + 2 + 2 * path + 1
    r1 = 4 + 4 + 1 + 2 * path + 1
    scale, scale2 = np.asarray(scale), np.asarray(scale2)
    return 2.0 * (EPS * ((r2 + 1) * scale2 + (2 * r1 + 1) * scale * scale) + 4.0 * scale * eps_atol(spread))


def adapt_bound(scale, scale2, S, spread, v, rate):
    """... on |v_library - v_restatement|, v = (1 - rate) s_old^2 + rate var the blended variance: rate times var_bound, and one rounding
    each for s_old^2, the two products and the sum -- 4 2^-53 v, doubled as the rest.  (1 - rate is the same IEEE difference on both
    sides.)  A spread is sqrt(v): |s_a - s_b| = |v_a - v_b| / (s_a + s_b), plus the root's own rounding."""
    return rate * var_bound(scale, scale2, S, spread) + 2.0 * 4.0 * EPS * np.asarray(v)
