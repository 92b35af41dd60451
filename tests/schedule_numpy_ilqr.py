"""NumPy restatement of the per-knot state-weight schedule (qilqr_set_state_weight_schedule), the comparand of
tests/test_schedule_cpu.py and tests/test_gpu_schedule.py.  Test infrastructure: nothing in the product imports it.

Knot i (0-based, the last included) of every problem takes Qs[i] wherever the handle's Q stood: the knot cost, C_x and C_xx
(cost.hh:36-61 with Q -> Qs[i]); R, the desired trajectory, the model and dt stay.  The mixin below sits in front of the restatements it
extends (tests/obstacle_numpy_ilqr.py's, which are tests/independent_numpy_ilqr.py's ILQR and tests/limited_numpy_ilqr.py's LimitedILQR
with the spheres; without spheres they are those restatements), as obstacle_numpy_ilqr.py's own mixin does; the backward passes take the
cost through cost_knot_diffs, in the reference's form (recursion 0) and the substituted, symmetrised one (recursion 1)."""
import numpy as np

from tests.obstacle_numpy_ilqr import ObstacleILQR, ObstacleLimitedILQR, knot_cost


class _Schedule:
    """the cost with Qs[i] at knot i (a mixin in front of a restatement); without a schedule the restatement's own Q"""
    Qs = None

    def set_state_weight_schedule(self, Qs):
        self.Qs = None if Qs is None else np.asarray(Qs, dtype=float).reshape(-1, 12, 12).copy()

    def q_at(self, i):
        return self.Q if self.Qs is None else self.Qs[i]

    def cost_trajectory(self, pts):
        c = 0.0
        for i, (T, v, u) in enumerate(pts):
            c += knot_cost(self.spheres, self.q_at(i), self.R, T, v, u, *self.des[i])
        return c

    def cost_knot_diffs(self, T, v, u, i):
        return knot_cost(self.spheres, self.q_at(i), self.R, T, v, u, *self.des[i], diffs=True)


class ScheduleILQR(_Schedule, ObstacleILQR):
    """the unconstrained recursion with the schedule: recursion 0 is ObstacleILQR's (the reference's forms, Q_uu solved from its lower
    triangle as Eigen's LDL^T reads it), recursion 1 the symmetric-weight kernels' (gains substituted, V_xx symmetrised)"""

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


class ScheduleLimitedILQR(_Schedule, ObstacleLimitedILQR):
    """LimitedILQR (thrust limits, restarts) with the schedule: its backward pass takes the cost through cost_knot_diffs"""
