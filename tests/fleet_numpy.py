"""Fleet deconfliction restated in plain NumPy from include/quadrotor_ilqr.h's words (qilqr_fleet_neighbours_device), including none of the
library's headers: brute-force pair distances, neighbours by np.lexsort((row, d2)), the line fit by its closed forms.  The sums here are
NumPy's (not fused, not sequential), so words that are computed agree with the library to rounding; words that are decided -- a partner, a
knot, a count -- agree exactly on inputs without near-ties (gaps)."""
import numpy as np

NBR, SUMMARY = 4, 8
COVER, YIELD_TO_LOWER = 1, 2


def pair_values(plan, V):
    """d2 (B, V): the smallest squared distance over the knots of row b to vehicle p of its fleet (+inf on the diagonal and where no knot
    has a finite one), and knot (B, V): the first knot that has it (-1)"""
    B, n = plan.shape[:2]
    d2, knot = np.full((B, V), np.inf), np.full((B, V), -1, dtype=np.int64)
    for g in range(B // V):
        p = plan[g * V:(g + 1) * V, :, 1:4]
        with np.errstate(invalid="ignore", over="ignore"):
            e = p[:, None] - p[None]
            d = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]  # (V, V, n)
        d = np.where(np.isnan(d), np.inf, d)
        d[np.arange(V), np.arange(V)] = np.inf
        k = d.argmin(axis=2)  # (the first on ties)
        m = np.take_along_axis(d, k[..., None], axis=2)[..., 0]
        d2[g * V:(g + 1) * V] = m
        knot[g * V:(g + 1) * V] = np.where(np.isfinite(m), k, -1)
    return d2, knot


def fit(plan, dt):
    """(c (B, 3), v (B, 3), residual (B)) of every vehicle's line through its knots"""
    p = plan[:, :, 1:4]
    n = p.shape[1]
    t = np.arange(n) * dt
    with np.errstate(invalid="ignore", over="ignore"):
        pbar = p.sum(axis=1) / n
        if n == 1:
            v = np.zeros_like(pbar)
            c = pbar.copy()
        else:
            tbar = (n - 1) * dt / 2.0
            stt = dt * dt * n * (n * n - 1.0) / 12.0
            v = ((t - tbar)[None, :, None] * (p - pbar[:, None])).sum(axis=1) / stt
            c = pbar - tbar * v
        r = p - (c[:, None] + t[None, :, None] * v[:, None])
        res = np.sqrt((r * r).sum(axis=2)).max(axis=1)
    return c, v, res


def gaps(plan, V):
    """the smallest relative distance of two consecutive sorted finite d2 over every ego (inf: nothing to compare): exact comparison of the
    decided words needs it well above the rounding of a d2"""
    d2, _ = pair_values(plan, V)
    worst = np.inf
    for b in range(len(d2)):
        s = np.sort(d2[b][np.isfinite(d2[b])])
        if len(s) > 1:
            worst = min(worst, float(((s[1:] - s[:-1]) / np.maximum(s[1:], 1e-300)).min()))
    return worst


def neighbours(plan, V, K, dt, radius, weight, range=np.inf, conflict=None, cover=False, yield_to_lower=False):
    """dict(summary (B, 8), nbr (B, K, 4), spheres (B, K, 8), counts (B) int32) as the header states them"""
    B = plan.shape[0]
    conflict = radius if conflict is None else conflict
    d2, knot = pair_values(plan, V)
    c, v, res = fit(plan, dt)
    ok = np.isfinite(c).all(axis=1) & np.isfinite(v).all(axis=1) & np.isfinite(res)
    summary, nbr = np.zeros((B, SUMMARY)), np.zeros((B, K, NBR))
    nbr[:, :, 0], nbr[:, :, 1], nbr[:, :, 2] = -1.0, np.inf, -1.0
    spheres, counts = np.zeros((B, K, 8)), np.zeros(B, dtype=np.int32)
    for b in np.arange(B):  # (`range` is the rule's here)
        g, ev = divmod(int(b), V)
        partners = np.array([p for p in np.arange(V) if p != ev], dtype=np.int64)
        cand = partners[partners < ev] if yield_to_lower else partners
        order = cand[np.lexsort((cand, d2[b, cand]))][:K] if len(cand) else cand
        kept, rmax, within = 0, 0.0, True
        for j, p in enumerate(order):
            row = g * V + p
            nbr[b, j] = [row, np.sqrt(d2[b, p]), knot[b, p], res[row]]
            within = within and np.isfinite(d2[b, p]) and np.sqrt(d2[b, p]) < range
            if within and ok[row]:
                r = radius + res[row] if cover else radius
                spheres[b, kept] = np.concatenate([c[row], v[row], [r, weight]])
                rmax, kept = max(rmax, r), kept + 1
        counts[b] = kept
        fin = partners[np.isfinite(d2[b, partners])] if len(partners) else partners
        if len(fin):
            p = fin[np.lexsort((fin, d2[b, fin]))][0]
            summary[b, :3] = [np.sqrt(d2[b, p]), knot[b, p], g * V + p]
        else:
            summary[b, :3] = [np.inf, -1.0, -1.0]
        summary[b, 3] = np.count_nonzero(np.sqrt(d2[b, partners]) < conflict) if len(partners) else 0
        summary[b, 4], summary[b, 5] = kept, rmax
    return dict(summary=summary, nbr=nbr, spheres=spheres, counts=counts)
