"""NumPy restatement of the extensions together: the per-knot state-weight schedule (tests/schedule_numpy_ilqr.py), the shared spheres
(tests/obstacle_numpy_ilqr.py) and the problem's own, moving spheres (tests/moving_obstacle_numpy_ilqr.py) in one knot cost, the comparand
of tests/test_composed_cpu.py, tests/test_gpu_linearize_keys.py and tests/test_gpu_composed.py.  Test infrastructure: nothing in the
product imports it.

Knot i takes Qs[i] wherever the handle's Q stood (the handle's Q without a schedule), then the handle's shared spheres, then the problem's
own at t_i = i dt, each in index order: what the cost half of k_linearize computes when a handle has all three.  The per-problem model goes
in through Model, as everywhere.  The mixin sits in front of the restatements the other mixins sit in front of, and each of those is this
one with the other table empty (tests/test_composed_cpu.py: bit for bit)."""
import numpy as np

from tests.moving_obstacle_numpy_ilqr import WORDS, at_time
from tests.obstacle_numpy_ilqr import ObstacleILQR, ObstacleLimitedILQR, knot_cost


class _Composed:
    """the cost with Qs[i] and every sphere of knot i (a mixin in front of an obstacle restatement)"""
    Qs = None
    own = np.zeros((0, WORDS))

    def set_state_weight_schedule(self, Qs):
        self.Qs = None if Qs is None else np.asarray(Qs, dtype=float).reshape(-1, 12, 12).copy()

    def set_problem_obstacles(self, own):
        self.own = np.asarray(own, dtype=float).reshape(-1, WORDS)

    def q_at(self, i):
        return self.Q if self.Qs is None else self.Qs[i]

    def knot_spheres(self, i):
        """every sphere of knot i in the order they are added: the shared ones, then the problem's own at t_i = i dt"""
        return np.vstack([self.spheres.reshape(-1, 5), at_time(self.own, i * self.dt)])

    def cost_trajectory(self, pts):
        c = 0.0
        for i, (T, v, u) in enumerate(pts):
            c += knot_cost(self.knot_spheres(i), self.q_at(i), self.R, T, v, u, *self.des[i])
        return c

    def cost_knot_diffs(self, T, v, u, i):
        return knot_cost(self.knot_spheres(i), self.q_at(i), self.R, T, v, u, *self.des[i], diffs=True)


class ComposedILQR(_Composed, ObstacleILQR):
    """the unconstrained recursion with every extension of the cost: recursion 0 is ObstacleILQR's (the reference's forms), recursion 1
    the symmetric-weight kernels', as ScheduleILQR states it"""

    def backwards_pass(self, pts):
        if self.recursion != 1:
            return super().backwards_pass(pts)
        n = len(pts)
        vx, vxx = np.zeros(12), np.zeros((12, 12))
        ks, Ks = [None] * n, [None] * n
        QuTk = kTQuuk = 0.0
        for i in range(n - 1, -1, -1):
            T, v, u = pts[i]
            _, Jx, Ju = self.step(T, v, u, self.dt, True)
            _, C = self.cost_knot_diffs(T, v, u, i)
            Qx = C["x"] + Jx.T @ vx
            Qu = C["u"] + Ju.T @ vx
            Qxx = C["xx"] + Jx.T @ vxx @ Jx
            Quu = C["uu"] + Ju.T @ vxx @ Ju
            Qxu = C["xu"] + Jx.T @ vxx @ Ju
            K = -np.linalg.solve(Quu, Qxu.T)
            k = -np.linalg.solve(Quu, Qu)
            ks[i], Ks[i] = k, K
            QuTk += Qu @ k
            kTQuuk += -(Qu @ k)
            vx = Qx + K.T @ Qu
            vxx = Qxx + Qxu @ K
            vxx = 0.5 * (vxx + vxx.T)
        return ks, Ks, (QuTk, kTQuuk)


class ComposedLimitedILQR(_Composed, ObstacleLimitedILQR):
    """ObstacleLimitedILQR (thrust limits, restarts) with every extension of the cost"""
