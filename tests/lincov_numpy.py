"""Linear covariance analysis of a plan's closed loop (qilqr_covariance_device) restated as include/quadrotor_ilqr.h words it, from the
oracle's primitives and not from the new headers: A and B are oracle.discrete_step(diffs=True), K is oracle.gains_to_kK, and G is taken by
central differences of tests/scored_flight_numpy.disturbed_step, the restated flight's own step.  The comparand of
tests/test_covariance_cpu.py (the host program) and of tests/test_gpu_covariance.py (the kernels).  NumPy and the CPU oracle only."""
import numpy as np

from oracle import oracle as orc
from tests import closed_loop_numpy as cn, desired_cases as dc, moving_obstacle_numpy_ilqr as mov, scored_flight_numpy as sn

RTOL = cn.RTOL  # 1e-10: the bar the project holds this chain of steps to
H = 1e-6        # the step of the central differences


def wrench_jacobian(step, x, u, h=H):
    """(12, 6): central differences of step(x, u, w) about w = 0, the difference of the two next states taken by oracle.state_minus"""
    G = np.zeros((12, 6))
    for w in range(6):
        e = np.zeros(6)
        e[w] = h
        G[:, w] = orc.state_minus(step(x, u, e), step(x, u, -e)) / (2.0 * h)
    return G


def knot_matrices(mp, integrator, knot, K, dt):
    """(F (12, 12), G (12, 6)) of the step from plan knot `knot` (18): F = A + B K (K (4, 12), or None: the open loop)"""
    x, u = knot[1:14], knot[14:18]
    _, A, Bm = orc.discrete_step(mp, integrator, x, u, dt, diffs=True)
    F = A if K is None else A + Bm @ K
    G = wrench_jacobian(lambda xx, uu, w: sn.disturbed_step(mp, integrator, xx, uu, dt, w), x, u)
    return F, G


def coeffs(sigma, tau_force_s, tau_torque_s, dt, held=False):
    """(S_g (6, 6), rho (6)): the gust model's stationary covariance and one-step correlation (gust_coeffs' formula; held: rho = 1)"""
    tau = np.array([tau_force_s] * 3 + [tau_torque_s] * 3)
    rho = np.ones(6) if held else np.where(tau > 0.0, np.exp(-dt / np.where(tau > 0.0, tau, 1.0)), 0.0)
    return np.diag(np.asarray(sigma, dtype=np.float64) ** 2), rho


def mirrored(S):
    """entry (k, l) with k <= l, mirrored"""
    return np.triu(S) + np.triu(S, 1).T


def recursion(F, G, state_sigma, Sg, rho, mean, i0, i1):
    """F (n, 12, 12), G (n, 12, 6) -> cov (n, 12, 12), m (n, 12), cross (n, 12, 6); NaN outside knots i0 .. i1"""
    n = len(F)
    cov, m, cross = np.full((n, 12, 12), np.nan), np.full((n, 12), np.nan), np.full((n, 12, 6), np.nan)
    S, C, mu = np.diag(np.asarray(state_sigma, dtype=np.float64) ** 2), np.zeros((12, 6)), np.zeros(12)
    for i in range(i0, i1 + 1):
        cov[i], m[i], cross[i] = S, mu, C
        if i == i1:
            break
        Fi, Gi = F[i], G[i]
        S = mirrored(Fi @ S @ Fi.T + Fi @ C @ Gi.T + Gi @ C.T @ Fi.T + Gi @ Sg @ Gi.T)
        C = (Fi @ C + Gi @ Sg) * rho[None, :]
        mu = Fi @ mu + Gi @ np.asarray(mean, dtype=np.float64)
    return cov, m, cross


def spheres_at(shared, own, t):
    """(K, 5): the shared spheres, then the plan's own at time t"""
    shared = np.zeros((0, 5)) if shared is None else np.asarray(shared, dtype=np.float64).reshape(-1, 5)
    own = np.zeros((0, 8)) if own is None else np.asarray(own, dtype=np.float64).reshape(-1, 8)
    return np.vstack([shared, mov.at_time(own, t)])


def summary(cov, m, plan, K, dt, i0, i1, shared=None, own=None):
    """one plan: (the 8 words, per-knot sqrt(tr P) (n), z (n, spheres)); NaN outside the window"""
    n = len(plan)
    pos, rot, ustd = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n)
    z = np.full((n, len(spheres_at(shared, own, 0.0))), np.nan)
    for i in range(i0, i1 + 1):
        P = cov[i][:3, :3]
        pos[i], rot[i] = np.sqrt(np.trace(P)), np.sqrt(np.trace(cov[i][3:6, 3:6]))
        R = dc._rotmat(np.asarray(plan[i, 4:8], dtype=np.float64))
        p = plan[i, 1:4] + R @ m[i][:3]
        for j, sp in enumerate(spheres_at(shared, own, i * dt)):
            d = p - sp[:3]
            nb = R.T @ d / np.linalg.norm(d)
            with np.errstate(divide="ignore", invalid="ignore"):
                z[i, j] = (np.linalg.norm(d) - sp[3]) / np.sqrt(nb @ P @ nb)
        if K is not None:
            ustd[i] = np.sqrt(max(float(K[i][a] @ cov[i] @ K[i][a]) for a in range(4)))
    words = np.zeros(8)
    words[0], words[1], words[2], words[3] = np.nanmax(pos), np.nanargmax(pos), pos[i1], np.nanmax(rot)
    words[4], words[5], words[6] = np.inf, -1, -1
    if z.shape[1] and np.isfinite(z[i0:i1 + 1]).any():
        flat = np.where(np.isnan(z), np.inf, z)
        i, j = np.unravel_index(np.argmin(flat), flat.shape)
        if flat[i, j] < np.inf:
            words[4], words[5], words[6] = flat[i, j], i, j
    words[7] = ustd.max()
    return words, pos, z


def covariance(plan, gains, model, dt, state_sigma, sigma, mean=None, tau_force_s=0.0, tau_torque_s=0.0, held=False, integrator=0, models=None,
               i0=0, i1=None, shared=None, own=None):
    """plan (B, n, 18), gains (B, n, 52) or None -> dict: cov (B, n, 12, 12), mean (B, n, 12), cross (B, n, 12, 6), summary (B, 8), pos (B, n),
    z (a list of (n, spheres)), F (B, n, 12, 12), G (B, n, 12, 6).  models: a list of B problems-style dicts (plan b takes model b)."""
    plan = np.asarray(plan, dtype=np.float64)
    B, n = plan.shape[:2]
    i1 = n - 1 if i1 is None else i1
    K = None if gains is None else orc.gains_to_kK(np.asarray(gains, dtype=np.float64))[1]
    Sg, rho = coeffs(sigma, tau_force_s, tau_torque_s, dt, held)
    mean = np.zeros(6) if mean is None else np.asarray(mean, dtype=np.float64)
    out = dict(cov=[], mean=[], cross=[], summary=[], pos=[], z=[], F=[], G=[])
    for b in range(B):
        mp = orc.model_params(**(models[b] if models is not None else model))
        F, G = np.full((n, 12, 12), np.nan), np.full((n, 12, 6), np.nan)
        for i in range(i0, i1):
            F[i], G[i] = knot_matrices(mp, integrator, plan[b, i], None if K is None else K[b, i], dt)
        cov, m, cross = recursion(F, G, state_sigma, Sg, rho, mean, i0, i1)
        words, pos, z = summary(cov, m, plan[b], None if K is None else K[b], dt, i0, i1, shared, None if own is None else own[b])
        for key, v in zip(("cov", "mean", "cross", "summary", "pos", "z", "F", "G"), (cov, m, cross, words, pos, z, F, G)):
            out[key].append(v)
    return {k: (v if k == "z" else np.stack(v)) for k, v in out.items()}


def margins(r, i0, i1):
    """how far the discrete words of the summaries are from flipping, relative to the value: (the least gap between the largest and the
    second largest sqrt(tr P) over a plan's knots, the least gap between the smallest and the second smallest z over its knots and spheres)"""
    gp, gz = np.inf, np.inf
    for b in range(len(r["pos"])):
        p = np.sort(r["pos"][b][i0:i1 + 1])
        if len(p) > 1:
            gp = min(gp, (p[-1] - p[-2]) / p[-1])
        z = np.sort(r["z"][b][i0:i1 + 1].ravel())
        z = z[np.isfinite(z)]
        if len(z) > 1:
            gz = min(gz, (z[1] - z[0]) / abs(z[0]))
    return gp, gz
