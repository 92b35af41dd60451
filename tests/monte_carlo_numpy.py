"""The Monte-Carlo kernels restated in NumPy from their definition (include/quadrotor_ilqr.h), sharing no text with the library:
Philox4x32-10 with the library's counter and key, two normals per call, the Gauss-Markov gust, the start states over the oracle's
state addition, and the per-plan summary.  Vectorised over draws.  The recursion's fused step is restated as a * b + c with two roundings (NumPy has no fma): within an ulp of g, far
inside the bound below; where a test asks for bits it compares the library with itself or with one product and one sum.

The bounds of tests/test_monte_carlo_cpu.py and tests/test_gpu_monte_carlo.py, derived and not tuned:
  a unit normal        atol 1e-12: |z| <= 8.58 and log, sqrt, sin, cos are good to a few ulp, so the error is below 1e-14; the bar leaves 100x
  a gust word          atol 1e-12 max(sigma_c, |mean_c|, 1): the recursion is a contraction (rho < 1), errors do not grow with n
  a state word         atol 1e-12 max(sigma_c, 1) for the velocities, 1e-12 for the pose words
  the mean cost        rtol 1e-12: costs are not negative, S <= 130 terms give at most S 2^-53 = 1.4e-14
  the deviation        rtol 1e-10, or atol 1e-12 mean where it is near zero
"""
import numpy as np

from oracle import oracle as orc

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_GUSTS, STREAM_STATES = 0, 1
NORMAL_ATOL = 1e-12
MEAN_RTOL, STD_RTOL = 1e-12, 1e-10


def philox(counter, key):
    """Philox4x32-10: counter (..., 4) and key (..., 2) of integers below 2^32 -> (..., 4) uint64 words below 2^32"""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) for k in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # (32 x 32 bits: no overflow in 64)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK), (k1 + np.uint64(W1)) & np.uint64(MASK)
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def words(seed, plan, sample, row, stream, pair):
    """the four words of draws (broadcast over the index arrays)"""
    plan, sample, row, stream, pair = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (plan, sample, row, stream, pair)))
    counter = np.stack([row, sample, plan, (stream << np.uint64(16)) | pair], axis=-1)
    key = np.array([int(seed) & MASK, int(seed) >> 32], dtype=np.uint64)
    return philox(counter, np.broadcast_to(key, counter.shape[:-1] + (2,)))


def normals(w):
    """(..., 4) words -> (z0, z1)"""
    w = np.asarray(w, dtype=np.uint64)
    a = (w[..., 0] >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w[..., 1] >> np.uint64(6)).astype(np.float64)
    u1 = (a + 1.0) * 2.0 ** -53
    t = ((w[..., 2] >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (w[..., 3] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * t), r * np.sin(2.0 * np.pi * t)


def draws(seed, plan, sample, row, stream, pair):
    return normals(words(seed, plan, sample, row, stream, pair))


def gust_coeffs(sigma, tau_force_s, tau_torque_s, dt):
    sigma = np.asarray(sigma, dtype=np.float64)
    tau = np.array([tau_force_s] * 3 + [tau_torque_s] * 3, dtype=np.float64)
    rho = np.where(tau > 0, np.exp(-dt / np.where(tau > 0, tau, 1.0)), 0.0)
    return rho, sigma * np.sqrt((1.0 - rho) * (1.0 + rho))


def gust_normals(seed, B, S, n_w, b0=0, s0=0):
    """xi[b, s, i, c]: normal c % 2 of pair c // 2 of row i"""
    b, s, i, j = np.meshgrid(np.arange(B) + b0, np.arange(S) + s0, np.arange(n_w), np.arange(3), indexing="ij")
    z0, z1 = draws(seed, b, s, i, STREAM_GUSTS, j)
    return np.stack([z0, z1], axis=-1).reshape(B, S, n_w, 6)


def gusts(seed, B, S, n_w, dt, sigma, mean=None, tau_force_s=0.0, tau_torque_s=0.0, b0=0, s0=0):
    """wrench (B, S, n_w, 6): g_0 = sigma xi_0, g_i = rho g_{i-1} + kappa xi_i, w_i = mean + g_i"""
    sigma = np.asarray(sigma, dtype=np.float64)
    mean = np.zeros(6) if mean is None else np.asarray(mean, dtype=np.float64)
    rho, kappa = gust_coeffs(sigma, tau_force_s, tau_torque_s, dt)
    xi = gust_normals(seed, B, S, n_w, b0, s0)
    out = np.empty_like(xi)
    g = sigma * xi[:, :, 0]
    out[:, :, 0] = mean + g
    for i in range(1, n_w):
        g = rho * g + kappa * xi[:, :, i]
        out[:, :, i] = mean + g
    return out


def state_normals(seed, B, S, b0=0, s0=0):
    """xi[b, s, c] over the 12 tangent words: stream 1, row 0, pairs 0..5"""
    b, s, j = np.meshgrid(np.arange(B) + b0, np.arange(S) + s0, np.arange(6), indexing="ij")
    z0, z1 = draws(seed, b, s, 0, STREAM_STATES, j)
    return np.stack([z0, z1], axis=-1).reshape(B, S, 12)


def states(seed, x_nom, S, sigma, b0=0, s0=0, first_is_nominal=False):
    """x0 (B, S, 13) = x_nom[b] (+) sigma xi through the oracle's state addition"""
    x_nom = np.asarray(x_nom, dtype=np.float64)
    B = x_nom.shape[0]
    delta = np.asarray(sigma, dtype=np.float64) * state_normals(seed, B, S, b0, s0)
    out = np.empty((B, S, 13))
    for b in range(B):
        for s in range(S):
            out[b, s] = x_nom[b] if (first_is_nominal and s0 + s == 0) else orc.state_add(x_nom[b], delta[b, s])
    return out


def summary(score):
    """(B, S, 4) -> (B, 8), each word by its definition, NumPy's own sums"""
    score = np.asarray(score, dtype=np.float64)
    B, S = score.shape[:2]
    out = np.empty((B, 8))
    for b in range(B):
        cost, clear, hits = score[b, :, 0], score[b, :, 1], score[b, :, 3]
        fin = np.isfinite(cost)
        if fin.any():
            mean = cost[fin].sum() / fin.sum()
            out[b, 0], out[b, 1] = mean, np.sqrt(((cost[fin] - mean) ** 2).sum() / fin.sum())
            out[b, 2] = cost[fin].max()
            out[b, 3] = np.flatnonzero(fin & (cost == out[b, 2]))[0]
        else:
            out[b, :3], out[b, 3] = np.nan, -1
        out[b, 4] = (hits > 0).sum() / S
        seen = ~np.isnan(clear) & (clear < np.inf)
        out[b, 5] = clear[seen].min() if seen.any() else np.inf
        out[b, 6] = np.flatnonzero(seen & (clear == out[b, 5]))[0] if seen.any() else -1
        out[b, 7] = (~fin).sum() / S
    return out


def extremes_are_unique(score):
    """the largest finite cost and the smallest clearance of every plan are attained once: the indices cannot depend on the order"""
    for b in range(score.shape[0]):
        cost, clear = score[b, :, 0], score[b, :, 1]
        fin = np.isfinite(cost)
        if fin.any() and (cost[fin] == cost[fin].max()).sum() != 1:
            return False
        seen = ~np.isnan(clear) & (clear < np.inf)
        if seen.any() and (clear[seen] == clear[seen].min()).sum() != 1:
            return False
    return True


def assert_summary(got, want, label=""):
    """words 2 .. 7 exactly; the mean to MEAN_RTOL; the deviation to STD_RTOL, or 1e-12 mean where it is near zero"""
    assert np.array_equal(got[:, 2:], want[:, 2:], equal_nan=True), (label, got[:, 2:], want[:, 2:])
    assert np.array_equal(np.isnan(got[:, :2]), np.isnan(want[:, :2])), label
    ok = ~np.isnan(want[:, 0])
    np.testing.assert_allclose(got[ok, 0], want[ok, 0], rtol=MEAN_RTOL, atol=0, err_msg=label)
    err = np.abs(got[ok, 1] - want[ok, 1])
    assert (err <= np.maximum(STD_RTOL * np.abs(want[ok, 1]), 1e-12 * np.abs(want[ok, 0]))).all(), (label, got[ok, 1], want[ok, 1])


def special_scores(B, S, seed):
    """(B, S, 4) scores as the scored flight writes them, with the rows a reduction has to get right: plan 0 ordinary, plan 1 with a NaN
    cost, a +inf cost and a NaN clearance, plan 2 without spheres (+inf clearances, knot -1) -- as far as S has room for them"""
    r = np.random.default_rng(seed)
    score = np.empty((B, S, 4))
    score[..., 0] = 50.0 + 100.0 * r.random((B, S))
    score[..., 1] = r.normal(0.3, 0.4, (B, S))
    score[..., 2] = r.integers(0, 24, (B, S))
    score[..., 3] = np.where(score[..., 1] < 0, r.integers(1, 5, (B, S)), 0)
    if B > 1:
        score[1, 0, 0] = np.nan
        if S > 2:
            score[1, 2, 0] = np.inf
        if S > 3:
            score[1, 3, 1] = np.nan
        if S > 66:
            score[1, 66, 0] = -np.inf
    if B > 2:
        score[2, :, 1], score[2, :, 2], score[2, :, 3] = np.inf, -1, 0
    return score
