"""References for the ridge alpha path (ops.ridge_loo_path, fit_translator_ridge_cv; csrc/ridge.hip and csrc/eigh.hip), numpy only, on top of
tests/ridge_translator_reference.py (rr), whose cases, inputs, wide closed form and bounds are used as they are.

wide(case)      per alpha of GRID, rr.closed_form(Z, M, alpha) in numpy.longdouble: the Cholesky route, independent of any eigendecomposition; plus
                sse = sum over the rows of (M - loo)^2 in the wide type.
eigen_path      the algebra the kernels implement, in float64 numpy on numpy.linalg.eigh: G = Xc^T Xc = V diag(lambda) V^T, lambda clamped at 0, P = Xc V,
                Q = V^T Xc^T Yc, h = 1 / N + sum_k P_k^2 / (lambda_k + alpha), Yhat = mbar + P diag(1 / (lambda + alpha)) Q, loo = M - (M - Yhat) / (1 - h).
bounds          rr.bounds(ref, M, c=C_PATH) for leverage, loo, r2, corr (the form c (N + d) 2^-53 kappa s, kappa that of Xc^T Xc + alpha I, unchanged); for sse
                the bound of the residual sum of squares as rr propagates it into r2, |d res| <= 2 e sum |y - p| + N e^2 with e the loo bound of the column,
                doubled for the second order, plus the rounding of the sum (N + 8) 2^-53 res.
C_PATH          rr's rule applied to eigen_path: four times the largest ratio it reaches against wide() with c = 1 over rr.CASES x GRID, rounded up to a power
                of two, at least 1.  Measured (tests/test_ridge_path_cpu.py re-measures and holds every line): the largest is 1.26 (loo at N2-d1-F1, where one
                rounding is most of the bound); every other case stays below 0.07.  So C_PATH = 8, section 25's constant: this evaluation (each term divided
                by lambda_k + alpha, the 1 / N added last) does not reach the 5.7 an earlier probe of another form of the algebra did, and the rule takes what
                the evaluation written here gives.
select          the alpha the path chooses, on any per-alpha outputs: "mse" the smallest mean of (M - loo)^2 over all rows and features, "r2" the largest mean
                leave-one-out R² over the features that are not constant; a tie takes the first.  margin: (runner-up - best) / |best| of the criterion, which the
                tests assert above 1e-6 on the wide reference alone.  The selection is checked on SELECT_GRID = {1, 100, 1e4}: on GRID the two
                best of N4500-d8-F2 are 5e-7 apart under "mse" (with 4500 rows on 8 dimensions no alpha below 1 matters); on SELECT_GRID every margin is above
                4e-4 and the choice is not always the same alpha.  At N = 2 every leave-one-out fit sees one row and predicts the
                other row's value whatever alpha is: a tie by construction, left out of the selection cases (SELECT_CASES)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ridge_translator_reference as rr  # noqa: E402

GRID = (1e-3, 1e-1, 1.0, 10.0, 1e3)
SELECT_GRID = (1.0, 100.0, 1e4)
SELECT_CASES = [c for c in rr.CASES + [rr.LONG_CASE] if c[0] > 2]
C_PATH = 8.0
KEYS = ("leverage", "loo", "r2", "corr", "sse")
_WIDE = {}


def sse_of(M, loo):
    return ((np.asarray(M).astype(loo.dtype) - loo) ** 2).sum(axis=0)


def wide(case, grid=GRID):
    """(Z, M, [rr.closed_form(Z, M, alpha) with "sse" added, for alpha in grid]), computed once per case and shared; nothing may write to it"""
    key = (case, tuple(grid))
    if key not in _WIDE:
        Z, M = rr.inputs(case)
        refs = []
        for alpha in grid:
            ref = rr.closed_form(Z, M, alpha)
            ref["sse"] = sse_of(M, ref["loo"])
            refs.append(ref)
        _WIDE[key] = (Z, M, refs)
    return _WIDE[key]


def eigen_path(Z, M, grid=GRID, dtype=np.float64):
    """the eigen route in `dtype` on numpy.linalg.eigh -> a list of dicts (leverage, loo, sse, r2, corr) per alpha, and the clamped eigenvalues"""
    Z, M = np.asarray(Z).astype(dtype), np.asarray(M).astype(dtype)
    N = Z.shape[0]
    zb, mb = Z.mean(axis=0), M.mean(axis=0)
    Xc, Yc = Z - zb, M - mb
    lam, V = np.linalg.eigh(Xc.T @ Xc)
    lam = np.maximum(lam, 0)
    P, Q = Xc @ V, V.T @ (Xc.T @ Yc)
    out = []
    for alpha in grid:
        shifted = lam + dtype(alpha)          # each term is divided, as in the kernels, not multiplied by a rounded reciprocal
        h = 1 / dtype(N) + (P * P / shifted).sum(axis=1)
        loo = M - (M - (mb + (P[:, :, None] * Q[None, :, :] / shifted[None, :, None]).sum(axis=1))) / (1 - h)[:, None]
        r2, corr = rr.ranking_stats(M, loo)
        out.append({"leverage": h, "loo": loo, "sse": sse_of(M, loo), "r2": r2, "corr": corr})
    return out, lam


def bounds(ref, M, c=None):
    """rr.bounds with c = C_PATH by default, and the bound of sse (see the module docstring)"""
    c = C_PATH if c is None else c
    b = rr.bounds(ref, M, c=c)
    M = np.asarray(M, dtype=np.float64)
    N = M.shape[0]
    P = np.asarray(ref["loo"], dtype=np.float64)
    e = np.asarray(b["loo"], dtype=np.float64).reshape(-1)
    res = ((M - P) ** 2).sum(axis=0)
    b["sse"] = 2 * (2 * e * np.abs(M - P).sum(axis=0) + N * e ** 2) + (N + 8) * rr.U * res
    return b


def ratios(got, ref, b):
    return {k: rr.max_ratio(got[k], ref[k], b[k]) for k in KEYS}


def scores(per_alpha, M, criterion):
    """the criterion of every alpha, smaller is better, in float64 from any per-alpha outputs"""
    M = np.asarray(M, dtype=np.float64)
    N, F = M.shape
    keep = M.max(axis=0) != M.min(axis=0)
    if criterion == "mse":
        return [float(np.asarray(o["sse"], dtype=np.float64).sum() / (N * F)) for o in per_alpha]
    return [-float(np.asarray(o["r2"], dtype=np.float64)[keep].sum() / keep.sum()) if keep.any() else 0.0 for o in per_alpha]


def select(per_alpha, M, criterion):
    """(the index of the chosen alpha, the relative margin of the best over the runner-up)"""
    s = scores(per_alpha, M, criterion)
    best = min(range(len(s)), key=lambda g: s[g])
    rest = [v for g, v in enumerate(s) if g != best]
    margin = (min(rest) - s[best]) / abs(s[best]) if rest and s[best] != 0 else np.inf
    return best, margin
