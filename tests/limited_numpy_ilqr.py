"""A NumPy restatement of the per-rotor thrust limits (qilqr_set_control_limits, an extension the reference does not have): control-
limited DDP (Tassa, Mansard & Todorov, ICRA 2014) on top of tests/independent_numpy_ilqr.py, the comparand of the device's box route.

Test infrastructure: nothing in the product imports it.  The oracle (oracle/ilqr_oracle.c) states the reference and is not extended;
this file adds to ILQR, unchanged and imported:
  * box_qp: the projected-Newton QP of quadrotorilqr_amd/csrc/box_qp.h, in its order of decisions and with its constants (the
    device and this restatement must take the same decisions), written again from the algorithm, not translated line by line;
  * backwards_pass: Q_uu (+ mu, the restarts) and Q_u into the box QP at every knot; K with zero rows for the clamped rotors;
    the full value updates V_x = Q_x + Q_xu k + K^T (Q_uu k + Q_u), V_xx = Q_xx + Q_xu K; the terms Q_u^T k and k^T Q_uu k;
  * forward_sim: the control law's u clamped to [lo, hi];
  * solve: ILQR.solve's loop with the Levenberg-Marquardt restarts of the oracle (orc_set_regularisation) and the exit status 4
    (STATUS_QP_FAILED) of a QP that broke down.
"""
import numpy as np

from tests.independent_numpy_ilqr import ILQR, cost_knot, knot_from_state, se3_log

ITERS, TRIALS, ARMIJO, BACKTRACK = 16, 30, 0.1, 0.6
STATUS_QP_FAILED = 4


def clamp(c, lo, hi):
    """c < lo ? lo : (c > hi ? hi : c), elementwise (a NaN stays a NaN)"""
    c = np.asarray(c, dtype=float)
    return np.where(c < lo, lo, np.where(c > hi, hi, c))


def masked_ldl(H, clamped):
    """unpivoted LDL^T of H (lower triangle) with the rows / columns in `clamped` replaced by identity: (L, d, ok)"""
    M = np.array(H, dtype=float)
    for a in range(4):
        if clamped[a]:
            M[a, :] = 0.0
            M[:, a] = 0.0
            M[a, a] = 1.0
    L, d = np.eye(4), np.zeros(4)
    for j in range(4):
        d[j] = M[j, j] - sum(L[j, m] ** 2 * d[m] for m in range(j))
        for i in range(j + 1, 4):
            L[i, j] = (M[i, j] - sum(L[i, m] * L[j, m] * d[m] for m in range(j))) / d[j]
    return L, d, not bool(np.any(d <= 0.0))  # (a NaN pivot is not <= 0: the NaN propagates, as on the device)


def ldl_solve(L, d, r):
    y = np.zeros(4)
    for i in range(4):
        y[i] = r[i] - L[i, :i] @ y[:i]
    z = np.zeros(4)
    for i in range(3, -1, -1):
        z[i] = y[i] / d[i] - L[i + 1:, i] @ z[i + 1:]
    return z


def clamped_set(x, l, h, grad):
    return ((x == l) & (grad > 0)) | ((x == h) & (grad < 0))


def objective(H, g, x):
    return float(x @ (0.5 * (H @ x) + g))


def box_qp(H, g, l, h):
    """argmin 1/2 x^T H x + g^T x on l <= x <= h: (x, clamped[4] bool, (L, d) of the masked factor, ok)"""
    H, g, l, h = (np.asarray(a, dtype=float) for a in (H, g, l, h))
    x = clamp(np.zeros(4), l, h)
    f = objective(H, g, x)
    prev, full = None, False
    for it in range(ITERS):
        grad = g + H @ x
        c = clamped_set(x, l, h, grad)
        if c.all():
            break
        L, d, ok = masked_ldl(H, c)
        if not ok:
            return x, c, (L, d), False
        if it > 0 and prev is not None and (c == prev).all() and full:
            break
        r = np.where(c, 0.0, g + H[:, c] @ x[c])
        z = ldl_solve(L, d, r)
        dx = np.where(c, 0.0, -z - x)
        gd = float(grad @ dx)
        step, accepted = 1.0, False
        for _ in range(TRIALS):
            xt = clamp(x + step * dx, l, h)
            ft = objective(H, g, xt)
            if ft - f <= ARMIJO * step * gd:
                accepted = True
                break
            step *= BACKTRACK
        if not accepted:
            break
        x, f, prev, full = xt, ft, c, step == 1.0
    grad = g + H @ x
    c = clamped_set(x, l, h, grad)
    L, d, ok = masked_ldl(H, c)
    return x, c, (L, d), ok


def box_gain(factor, clamped, Qux):
    """K (4 x 12): -H_FF^-1 Q_ux[F, :] on the free rows, zero rows for the clamped ones"""
    L, d = factor
    K = np.zeros_like(np.asarray(Qux, dtype=float))
    for j in range(K.shape[1]):
        z = ldl_solve(L, d, np.where(clamped, 0.0, Qux[:, j]))
        K[:, j] = np.where(clamped, 0.0, -z)
    return K


class LimitedILQR(ILQR):
    """ILQR with per-rotor thrust limits lo <= u <= hi (and, optionally, the oracle's Levenberg-Marquardt restarts)"""

    def __init__(self, model, Q, R, desired, dt, options, lo, hi, integrator=0):
        super().__init__(model, Q, R, desired, dt, options, integrator=integrator)
        self.lo = np.broadcast_to(np.asarray(lo, dtype=float), (4,)).copy()
        self.hi = np.broadcast_to(np.asarray(hi, dtype=float), (4,)).copy()
        self.mu_init, self.mu_factor, self.mu_max = 0.0, 1.0, 0.0
        self.mu = 0.0          # the regularisation of the next backwards_pass (solve sets it)
        self.qp_failed = False  # the last backwards_pass met a QP that broke down
        self.clamped = None     # [n][4] the clamped sets of the last backwards_pass

    def set_regularisation(self, mu_init, mu_factor, mu_max):
        self.mu_init, self.mu_factor, self.mu_max = mu_init, mu_factor, mu_max

    def backwards_pass(self, pts):
        n = len(pts)
        vx, vxx = np.zeros(12), np.zeros((12, 12))
        ks, Ks = [np.zeros(4)] * n, [np.zeros((4, 12))] * n
        self.clamped = np.zeros((n, 4), dtype=bool)
        self.qp_failed = False
        QuTk = kTQuuk = 0.0
        for i in range(n - 1, -1, -1):
            T, v, u = pts[i]
            _, Jx, Ju = self.step(T, v, u, self.dt, True)
            _, C = self.cost_knot_diffs(T, v, u, i)
            Qx = C["x"] + Jx.T @ vx
            Qu = C["u"] + Ju.T @ vx
            Qxx = C["xx"] + Jx.T @ vxx @ Jx
            Quu = C["uu"] + Ju.T @ vxx @ Ju + self.mu * np.eye(4)
            Quu = 0.5 * (Quu + Quu.T)
            Qxu = C["xu"] + Jx.T @ vxx @ Ju
            k, c, factor, ok = box_qp(Quu, Qu, self.lo - u, self.hi - u)
            if not ok:
                self.qp_failed = True
                break
            K = box_gain(factor, c, Qxu.T)
            ks[i], Ks[i] = k, K
            self.clamped[i] = c
            QuTk += Qu @ k
            kTQuuk += k @ Quu @ k
            vx = Qx + Qxu @ k + K.T @ (Quu @ k + Qu)
            vxx = Qxx + Qxu @ K
            vxx = 0.5 * (vxx + vxx.T)
        return ks, Ks, (QuTk, kTQuuk)

    def cost_knot_diffs(self, T, v, u, i):
        return cost_knot(self.Q, self.R, T, v, u, *self.des[i], diffs=True)

    def forward_sim(self, pts, ks, Ks, alpha):
        out = []
        T, v = pts[0][0].copy(), pts[0][1].copy()
        for i, (Tn, vn, un) in enumerate(pts):
            dx = np.concatenate([se3_log(np.linalg.inv(Tn) @ T), v - vn])
            u = clamp(un + alpha * ks[i] + Ks[i] @ dx, self.lo, self.hi)
            out.append((T, v, u))
            T, v = self.step(T, v, u, self.dt)
        return out

    def solve(self, traj):
        traj = np.asarray(traj, dtype=float)
        times = traj[:, 0].copy()
        pts = self.unpack(traj)
        new_cost = self.cost_trajectory(pts)
        hist, n_bwd, n_fwd, status, i = [], 0, 0, 2, 0
        self.mu = 0.0
        while i < self.o["max_iters"]:
            ks, Ks, (a, b) = self.backwards_pass(pts)
            n_bwd += 1
            if self.qp_failed:
                status = STATUS_QP_FAILED
                break
            cost = new_cost
            if i > 0 and self.is_converged(cost, cost + a + b / 2.0):
                status = 0
                break
            if i == 0:
                pts = self.forward_sim(pts, ks, Ks, 1.0)
                new_cost = self.cost_trajectory(pts)
                n_fwd += 1
            else:
                step, found = 1.0, False
                for _ in range(self.o["ls_max_iters"]):
                    cand = self.forward_sim(pts, ks, Ks, step)
                    c = self.cost_trajectory(cand)
                    n_fwd += 1
                    if c - cost < self.o["desired_reduction_frac"] * (step * a + step * step * b / 2.0):
                        pts, new_cost, found = cand, c, True
                        break
                    step *= self.o["step_update"]
                if not found:
                    new_cost = cost
                    if self.mu_init > 0.0:  # the restarts: same iterate, larger mu, backward pass again (not an iteration)
                        nxt = self.mu * self.mu_factor if self.mu > 0.0 else self.mu_init
                        if nxt <= self.mu_max:
                            self.mu = nxt
                            continue
                    status = 3
                    break
            if self.mu > 0.0:
                self.mu = self.mu / self.mu_factor
                if self.mu < self.mu_init:
                    self.mu = 0.0
            hist.append(new_cost)
            i += 1
            if i - 1 > 0 and self.is_converged(cost, new_cost):
                status = 1
                break
        out = np.array([knot_from_state(times[j], T, v, u) for j, (T, v, u) in enumerate(pts)])
        return dict(traj=out, cost=new_cost, status=status, iters=len(hist), n_bwd=n_bwd, n_fwd=n_fwd,
                    cost_hist=np.array(hist))
