"""References for the latent translator (csrc/ridge.hip, causal_vae_amd/vit/translator.py), numpy only.

(a) naive_loo        the reference's own procedure (latent_translator/analysis.py:36-48) restated: N separate fits, each a centred normal-equation solve of
                     the N - 1 other rows in float64 (sklearn's Ridge(alpha, fit_intercept=True) solves the same system), and the prediction of the row left out.
(b) closed_form      the closed form the kernels implement, in numpy.longdouble (x87 extended, eps 1.08e-19; float64 if this machine's longdouble is no wider,
                     which PRECISION says) with a hand-written vectorised Cholesky and two substitutions:
                         Xc = Z - zbar, A = Xc^T Xc + alpha I = L L^T, W = A^-1 Xc^T (M - mbar), Yhat = mbar + Xc W,
                         h_i = 1 / N + |L^-1 xc_i|^2,  p_i = y_i - (y_i - yhat_i) / (1 - h_i)
                     closed_form_float(dtype) is the same algebra on numpy's own Cholesky and solves in float64 or float32.
(c) bootstrap        latent_translator/analysis.py:118-165 restated without pandas, plus what the tests assert on the reference alone (the top-k margin, the
                     presence of every group).

The bound of a device output has the standard forward-error form of a Cholesky solve, c (N + d) 2^-53 kappa s: kappa the 2-norm condition number of A
(eigvalsh), s the output's scale: coef: the feature's max |coef|; intercept: the feature's |intercept|; fitted: the column's max |fitted|; leverage: 1;
loo: the column's max |y - ybar| / (1 - max h).  N + d and not d: with d alone numpy's own float64 closed form reaches 1.34 of the bound at N = 2, d = 1.
C_BOUND is four times the largest ratio numpy's float64 closed form reaches against (b) over CASES with c = 1, rounded up to a power of two, at least 1;
the factor of four is for another summation order, FMA contraction and the MFMA's own accumulation order (tests/test_ridge_translator_cpu.py holds the
measured ratios and re-measures them).

r2 and corr are functions of the leave-one-out predictions; their bounds are propagated to first order from the loo bound e_j of the column, doubled for the
terms of second order, plus the rounding of the sums themselves, (N + 8) 2^-53 times the magnitudes involved:
    res = sum (y - p)^2:       |d res| <= 2 e sum |y - p| + N e^2
    r2 = 1 - res / syy:        |d r2| <= 2 |d res| / syy + (N + 8) 2^-53 (1 + res / syy)
    syp = sum dy dp, dp = p - pbar (|d dp| <= 2 e):   |d syp| <= 2 e sum |dy|;   spp = sum dp^2:  |d spp| <= 4 e sum |dp| + 4 N e^2
    corr = syp / sqrt(syy spp):  |d corr| <= 2 (|d syp| / sqrt(syy spp) + |corr| |d spp| / (2 spp)) + (N + 8) 2^-53 (1 + |corr|)
A constant truth column (syy == 0) has r2 and corr fixed by the rules, not by arithmetic: its bound is 0."""
import numpy as np

U = 2.0 ** -53
WIDE = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64
PRECISION = f"reference precision: {np.dtype(WIDE).name}, eps {float(np.finfo(WIDE).eps):.3e}" + ("" if WIDE is not np.float64 else
                                                                                               " (no wider longdouble on this machine: float64)")
C_BOUND = 8.0

# (N, d, F, alpha, constant column): the cases of tests/test_ridge_translator.py; the CPU test measures on the same ones
CASES = [(2, 1, 1, 1.0, False), (16, 512, 7, 1.0, False), (40, 8, 5, 1.0, True), (97, 64, 12, 1.0, False), (300, 130, 3, 1.0, False), (40, 8, 5, 1e-3, False)]


# beyond them, for the device test alone: N over 4096, where a row chunk grows to 512 rows (9 chunks, the last one ragged)
LONG_CASE = (4500, 8, 2, 1.0, False)


def case_id(case):
    N, d, F, alpha, const = case
    return f"N{N}-d{d}-F{F}-a{alpha:g}" + ("-const" if const else "")


def inputs(case, seed=None):
    """Z float32 standard normal; M float64 = Z B + noise with the noise level growing over the columns from 0.3 (so the leave-one-out R² of the columns
    differ), column 0 scaled by 1000 (so a per-column scale matters); with `const`, the last column is the constant 2.0 (sums of it are exact)."""
    N, d, F, alpha, const = case
    rng = np.random.RandomState(1000 + N + 7 * d + 13 * F if seed is None else seed)
    Z = rng.standard_normal((N, d)).astype(np.float32)
    B = rng.standard_normal((d, F)) / np.sqrt(d)
    M = Z.astype(np.float64) @ B + 0.3 * (1.0 + 0.5 * np.arange(F)) * rng.standard_normal((N, F))
    M[:, 0] *= 1000.0
    if const:
        M[:, -1] = 2.0
    return Z, M


def ranking_stats(Y, P):
    """analysis.py:55-68 in the dtype of the inputs: r2 (sklearn's r2_score, with its values for a constant truth) and the Pearson correlation, 0 where the
    population standard deviation of either side is below 1e-12"""
    N, F = Y.shape
    r2, corr = np.zeros(F, dtype=Y.dtype), np.zeros(F, dtype=Y.dtype)
    for j in range(F):
        y, p = Y[:, j], P[:, j]
        dy, dp = y - y.sum() / N, p - p.sum() / N
        res, syy, spp = ((y - p) ** 2).sum(), (dy ** 2).sum(), (dp ** 2).sum()
        r2[j] = (1.0 if res == 0 else 0.0) if syy == 0 else 1 - res / syy
        if np.sqrt(syy / N) < 1e-12 or np.sqrt(spp / N) < 1e-12:
            corr[j] = 0.0
        else:
            corr[j] = min(max((dy * dp).sum() / (np.sqrt(syy) * np.sqrt(spp)), -1.0), 1.0)
    return r2, corr


def naive_loo(Z, M, alpha):
    """(a): P [N, F] float64, row i predicted by the ridge fitted on the other N - 1 rows"""
    Z, M = np.asarray(Z, dtype=np.float64), np.asarray(M, dtype=np.float64)
    N, d = Z.shape
    P = np.zeros_like(M)
    for i in range(N):
        keep = np.arange(N) != i
        X, Y = Z[keep], M[keep]
        xb, yb = X.mean(axis=0), Y.mean(axis=0)
        Xc = X - xb
        Wm = np.linalg.solve(Xc.T @ Xc + alpha * np.eye(d), Xc.T @ (Y - yb))
        P[i] = yb + (Z[i] - xb) @ Wm
    return P


def cholesky_wide(A):
    """lower Cholesky factor, column by column, in A's dtype"""
    n = A.shape[0]
    Lm = np.zeros_like(A)
    for j in range(n):
        v = A[j:, j] - Lm[j:, :j] @ Lm[j, :j]
        Lm[j, j] = np.sqrt(v[0])
        Lm[j + 1:, j] = v[1:] / Lm[j, j]
    return Lm


def forward_sub(Lm, B):
    X = np.zeros_like(B)
    for k in range(Lm.shape[0]):
        X[k] = (B[k] - Lm[k, :k] @ X[:k]) / Lm[k, k]
    return X


def back_sub_t(Lm, B):
    """L^T X = B"""
    X = np.zeros_like(B)
    for k in range(Lm.shape[0] - 1, -1, -1):
        X[k] = (B[k] - Lm[k + 1:, k] @ X[k + 1:]) / Lm[k, k]
    return X


def _finish(Z, M, alpha, zb, mb, Xc, A, Wm, T):
    N = Z.shape[0]
    out = {"coef": Wm.T.copy(), "intercept": mb - zb @ Wm, "fitted": mb + Xc @ Wm, "leverage": 1 / Z.dtype.type(N) + (T ** 2).sum(axis=0)}
    out["loo"] = M - (M - out["fitted"]) / (1 - out["leverage"])[:, None]
    out["r2"], out["corr"] = ranking_stats(M, out["loo"])
    ev = np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))
    out["kappa"] = float(ev[-1] / ev[0])
    return out


def closed_form(Z, M, alpha, dtype=WIDE):
    """(b): every output of the fit in `dtype` (default: the widest this machine has), through cholesky_wide and the substitutions above"""
    Z, M = np.asarray(Z).astype(dtype), np.asarray(M).astype(dtype)
    N, d = Z.shape
    zb, mb = Z.sum(axis=0) / N, M.sum(axis=0) / N
    Xc, Yc = Z - zb, M - mb
    A = Xc.T @ Xc + dtype(alpha) * np.eye(d, dtype=dtype)
    Lm = cholesky_wide(A)
    T = forward_sub(Lm, Xc.T.copy())
    Wm = back_sub_t(Lm, forward_sub(Lm, Xc.T @ Yc))
    return _finish(Z, M, alpha, zb, mb, Xc, A, Wm, T)


def closed_form_float(Z, M, alpha, dtype=np.float64):
    """the same algebra on numpy's own Cholesky and solves in float64 (what sets C_BOUND) or float32 (what the reference's sklearn call computes in)"""
    Z, M = np.asarray(Z).astype(dtype), np.asarray(M).astype(dtype)
    N, d = Z.shape
    zb, mb = Z.mean(axis=0), M.mean(axis=0)
    Xc, Yc = Z - zb, M - mb
    A = Xc.T @ Xc + dtype(alpha) * np.eye(d, dtype=dtype)
    Lm = np.linalg.cholesky(A)
    T = np.linalg.solve(Lm, Xc.T)
    Wm = np.linalg.solve(Lm.T, np.linalg.solve(Lm, Xc.T @ Yc))
    return _finish(Z, M, alpha, zb, mb, Xc, A, Wm, T)


def predict_wide(ref, Znew):
    return ref["intercept"] + np.asarray(Znew).astype(ref["coef"].dtype) @ ref["coef"].T


KEYS = ("coef", "intercept", "fitted", "loo", "leverage", "r2", "corr")


def bounds(ref, M, c=None):
    """the bound of every output of KEYS (see the module docstring), broadcastable against the output; from the reference's values alone"""
    c = C_BOUND if c is None else c
    f = lambda a: np.asarray(a, dtype=np.float64)          # noqa: E731
    M = f(M)
    N, F = M.shape
    d = ref["coef"].shape[1]
    base = c * (N + d) * U * ref["kappa"]
    h = f(ref["leverage"])
    e_loo = base * np.abs(M - M.mean(axis=0)).max(axis=0) / (1.0 - h.max())
    out = {"coef": base * np.abs(f(ref["coef"])).max(axis=1)[:, None], "intercept": base * np.abs(f(ref["intercept"])),
           "fitted": base * np.abs(f(ref["fitted"])).max(axis=0)[None, :], "leverage": base * np.ones(N), "loo": e_loo[None, :]}
    P = f(ref["loo"])
    dy, dp = M - M.mean(axis=0), P - P.mean(axis=0)
    res, syy, spp = ((M - P) ** 2).sum(axis=0), (dy ** 2).sum(axis=0), (dp ** 2).sum(axis=0)
    round_ = (N + 8) * U
    d_res = 2 * e_loo * np.abs(M - P).sum(axis=0) + N * e_loo ** 2
    d_syp, d_spp = 2 * e_loo * np.abs(dy).sum(axis=0), 4 * e_loo * np.abs(dp).sum(axis=0) + 4 * N * e_loo ** 2
    const = syy == 0
    safe_syy, safe_spp = np.where(const, 1.0, syy), np.where(spp == 0, 1.0, spp)
    out["r2"] = np.where(const, 0.0, 2 * d_res / safe_syy + round_ * (1 + res / safe_syy))
    corr = np.abs(f(ref["corr"]))
    out["corr"] = np.where(const, 0.0, 2 * (d_syp / np.sqrt(safe_syy * safe_spp) + corr * d_spp / (2 * safe_spp)) + round_ * (1 + corr))
    return out


def predict_bound(ref, M, pred, c=None):
    """predict on new rows: the fit's bound at the scale of the predicted column"""
    c = C_BOUND if c is None else c
    N, d = np.asarray(M).shape[0], ref["coef"].shape[1]
    return c * (N + d) * U * ref["kappa"] * np.abs(np.asarray(pred, dtype=np.float64)).max(axis=0)[None, :]


def max_ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the values must be equal (ratio 0, else inf)"""
    err = np.abs(np.asarray(got).astype(WIDE) - np.asarray(ref).astype(WIDE)).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(r)) if r.size else 0.0


def ranking_order(r2):
    """indices by r2 descending, ties in input order"""
    return sorted(range(len(r2)), key=lambda j: -float(r2[j]))


def min_adjacent_gap(r2):
    s = np.sort(np.asarray(r2, dtype=np.float64))
    return float(np.min(np.diff(s))) if len(s) > 1 else np.inf


# ---- (c) the bootstrap ----
def group_means(arr, groups):
    """analysis.py:91-98: (groups in order of first appearance, their mean rows)"""
    uniq = list(dict.fromkeys(groups.tolist()))
    return uniq, np.stack([arr[groups == g].mean(axis=0) for g in uniq])


def bootstrap(groups, Z, coef, intercept, feature_names, scale=None, n_boot=200, top_k=10, seed=0):
    """analysis.py:118-165 in float64 without pandas -> dict(counts, total_slots, skipped, freq, min_margin, all_present).  A pair with a group absent from the
    draw (the reference crashes there) is skipped and counted in `skipped`.  min_margin: the smallest (|d|_(k) - |d|_(k+1)) / |d|_(k) over every counted
    (bootstrap, pair): how far the top-k set is from a tie."""
    groups = np.asarray([str(g) for g in np.asarray(groups).tolist()])
    Z, coef, intercept = np.asarray(Z, dtype=np.float64), np.asarray(coef, dtype=np.float64), np.asarray(intercept, dtype=np.float64)
    rng = np.random.RandomState(seed)
    uniq = sorted(set(groups.tolist()))
    pairs = [(uniq[i], uniq[j]) for i in range(len(uniq)) for j in range(i + 1, len(uniq))]
    counts = {fn: 0 for fn in feature_names}
    total_slots = skipped = 0
    min_margin, all_present = np.inf, True
    for _ in range(n_boot):
        idx = rng.randint(0, len(groups), size=len(groups))
        names, means = group_means(Z[idx], groups[idx])
        all_present = all_present and len(names) == len(uniq)
        for g1, g2 in pairs:
            if g1 not in names or g2 not in names:
                skipped += 1
                continue
            m1, m2 = intercept + coef @ means[names.index(g1)], intercept + coef @ means[names.index(g2)]
            dm = m2 - m1
            if scale is not None:
                dm = dm * np.asarray(scale, dtype=np.float64)
            order = np.argsort(-np.abs(dm))
            for i in order[:top_k]:
                counts[feature_names[i]] += 1
            total_slots += top_k
            if top_k < len(dm):
                a, b = abs(dm[order[top_k - 1]]), abs(dm[order[top_k]])
                min_margin = min(min_margin, (a - b) / a if a > 0 else 0.0)
    return dict(counts=counts, total_slots=total_slots, skipped=skipped, freq={k: v / max(total_slots, 1) for k, v in counts.items()}, min_margin=min_margin,
                all_present=all_present)
