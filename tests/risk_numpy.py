"""The risk measures and the choice among candidate plans (quadrotorilqr_amd/csrc/risk_kernels.h), restated in NumPy from their
definitions in include/quadrotor_ilqr.h: NumPy's own sort (lexsort over (key, sample)), math.fsum for the tail, plain Python comparisons
for the choice.  Shared by tests/test_risk_cpu.py and tests/test_gpu_risk.py; nothing here is the kernels' text."""
import math

import numpy as np

COST, CLEARANCE = 0, 1
OBJECTIVES = {"mean": 0, "worst": 1, "var": 2, "cvar": 3}


def rank(level, S):
    """k = min(S - 1, max(0, ceil(level S) - 1)), in double"""
    return int(min(S - 1, max(0, math.ceil(float(level) * S) - 1)))


def keys(score, column):
    """(..., S, 4) -> (..., S): the cost, or minus the clearance; a NaN is +inf"""
    score = np.asarray(score, dtype=np.float64)
    k = score[..., 0].copy() if column == COST else -score[..., 1]
    k[np.isnan(k)] = np.inf
    return k


def order(key):
    """the permutation that sorts by (key, sample index)"""
    key = np.asarray(key)
    return np.lexsort((np.arange(len(key)), key))


def risk(score, levels, column):
    """(B, S, 4) -> words (B, L, 4) with word 1 from math.fsum, and the bound of word 1 (B, L): 2 (m + 1) 2^-53 mean|t_i| -- the
    first-order bound for m - 1 additions, a conversion and a division, doubled (inf where the tail holds an infinity: no error there)"""
    score = np.asarray(score, dtype=np.float64)
    B, S = score.shape[:2]
    out, bound = np.empty((B, len(levels), 4)), np.empty((B, len(levels)))
    sign = 1.0 if column == COST else -1.0
    for b in range(B):
        key = keys(score[b], column)
        perm = order(key)
        t_all = key[perm]
        for l, level in enumerate(levels):
            k = rank(level, S)
            t, m = t_all[k:], S - k
            if np.isposinf(t).any() and np.isneginf(t).any():
                mean = np.nan
            else:
                mean = math.fsum(t) / m
            out[b, l] = (sign * t[0], sign * mean, perm[k], m)
            bound[b, l] = 2.0 * (m + 1) * 2.0 ** -53 * np.abs(t).mean()
    return out, bound


def keys_are_unique(score, column):
    return all(len(np.unique(keys(score[b], column))) == score.shape[1] for b in range(score.shape[0]))


def assert_risk(got, score, levels, column, label=""):
    """words 0, 2 and 3 exactly; word 1 within its bound of math.fsum(t) / m (equal where it is infinite).  Returns the largest error of
    word 1 over its bound."""
    want, bound = risk(score, levels, column)
    got = np.asarray(got)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    for w in (0, 2, 3):
        assert np.array_equal(got[..., w], want[..., w]), (label, w, got[..., w], want[..., w])
    fin = np.isfinite(want[..., 1])
    assert np.array_equal(got[..., 1][~fin], want[..., 1][~fin], equal_nan=True), (label, got[..., 1], want[..., 1])
    if not fin.any():
        return 0.0
    err = np.abs(got[..., 1][fin] - want[..., 1][fin])
    assert (err <= bound[fin]).all(), (label, err, bound[fin])
    return float((err / bound[fin]).max())


def scores(B, S, seed, special=True):
    """(B, S, 4) scores as the scored flight writes them: log-normal costs, signed clearances.  With `special`, plan 1 has a NaN cost, a
    +inf cost and a NaN clearance and the last plan no spheres (+inf clearances), as far as B and S have room"""
    r = np.random.default_rng(seed)
    score = np.empty((B, S, 4))
    score[..., 0] = np.exp(r.normal(4.0, 1.0, (B, S)))
    score[..., 1] = r.normal(0.3, 0.4, (B, S))
    score[..., 2] = r.integers(0, 24, (B, S))
    score[..., 3] = np.where(score[..., 1] < 0, r.integers(1, 5, (B, S)), 0)
    if special and B > 1:
        score[1, S // 2, 0] = np.nan
        if S > 2:
            score[1, 0, 0] = np.inf
            score[1, S - 1, 1] = np.nan
    if special and B > 2:
        score[B - 1, :, 1] = np.inf
        score[B - 1, :, 2] = -1
        score[B - 1, :, 3] = 0
    return score


def select(summary, risk_words, C, objective="cvar", level=0, max_collision_fraction=1.0, max_diverged_fraction=1.0, min_clearance=-np.inf):
    """summary (C V, 8), risk_words (C V, L, 4) or None, candidate-major (plan b = c V + v) -> choice (V,) int32, info (V, 4)"""
    summary = np.asarray(summary, dtype=np.float64)
    V = summary.shape[0] // C
    o = OBJECTIVES[objective]
    choice, info = np.empty(V, dtype=np.int32), np.empty((V, 4))
    for v in range(V):
        rows = []
        for c in range(C):
            b = c * V + v
            obj = float(summary[b, 0] if o == 0 else summary[b, 2] if o == 1 else risk_words[b, level, o - 2])
            coll, clear, div = (float(summary[b, w]) for w in (4, 5, 7))
            ok = coll <= max_collision_fraction and div <= max_diverged_fraction and clear >= min_clearance and not math.isnan(obj)
            rows.append((obj, coll, div, ok, c))
        feasible = [r for r in rows if r[3]]
        if feasible:
            obj, coll, _, _, c = min(feasible, key=lambda r: (r[0], r[4]))
        else:
            obj, coll, _, _, c = min(rows, key=lambda r: (r[1], r[2], math.inf if math.isnan(r[0]) else r[0], r[4]))
        choice[v] = c
        info[v] = (obj, len(feasible), coll, 0.0 if feasible else 1.0)
    return choice, info
