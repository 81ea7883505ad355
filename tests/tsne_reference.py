"""Reference for the exact t-SNE (causal_vae_amd.vit.latent_tsne; csrc/tsne.hip), numpy only: sklearn's method="exact" pipeline in
numpy.longdouble (`wide`), and the same algebra in float64 (`dtype=numpy.float64`) for the constants' rule.

definitions     sqdist       D[i][j] = sum_k (z_ik - z_jk)^2 from differences, zero diagonal
                affinities   per row, d' = D - min_{j != i} D: e = exp(-beta d'), S = sum e, H = log S + beta sum d' e / S; sklearn's search for beta (from 1,
                             doubling / halving until bracketed, then midpoints), at most 100 steps, the first step with |H - log perplexity| <= tol is the last;
                             Pc = e / S with a zero diagonal.  The search of every row is recorded (`visited`: |H - log perplexity| of each step taken).
                joint        P = max((Pc + Pc^T) / sum, 2^-52) off the diagonal
                forces       w = 1 / (1 + |y_i - y_j|^2), Zs = sum_{i != j} w, grad_i = 4 sum_j (ex P_ij w - w^2 / Zs)(y_i - y_j),
                             KL = sum_{i != j} ex P log(ex P Zs / w)  (sklearn's clamp of Q at 2^-52 is dropped: it needs a span in the millions to act)
                step         sklearn's _gradient_descent element for element; fit: TSNE._tsne's two phases, with two stated differences: a gradient norm at or
                             below min_grad_norm ends the fit (sklearn goes on to the second phase and stops at its first check), and the KL reported is that of
                             P at the returned embedding (sklearn reports the one before the last update)
inputs          K Gaussian blobs (sigma 1) in float32, centres 4 sigma sqrt(d)-normal apart; the reference rounds D, P and every trajectory state to float64 and goes
                on from the rounded value, so a kernel handed those float64 arrays starts from exactly the reference's input.
bounds          c (terms) 2^-53 scale per output; the forms are in the functions below.  C_TSNE_* follow the rule of the other references:
                c = max(1, 2^ceil(log2(4 worst ratio))) with the worst ratio that the same algebra in float64 numpy reaches with c = 1 over CASES
                (tests/test_tsne_cpu.py re-measures and holds every line)."""
import math

import numpy as np

U = 2.0 ** -53
WIDE = np.longdouble
EPS = 2.0 ** -52
CHECK, EXPLORE, SEARCH_STEPS = 50, 250, 100
C_TSNE_D = 1.0
C_TSNE_AFF = 1.0
C_TSNE_FORCE = 1.0
C_TSNE_STEP = 4.0
C_TSNE_TRAJ = 256.0
TRAJ_STEPS = 8
STATE_ITERS = (0, 200, 400)
CASES = [(33, 7, 5.0), (96, 20, 30.0), (130, 512, 10.0), (300, 10, 50.0)]          # (N, d, perplexity)
DUPLICATE_CASE = (40, 6, 8.0)          # rows 2 k and 2 k + 1 equal
E2E_CASES = [CASES[1], CASES[3]]
E2E_K, E2E_MARGIN = 5, 1.25
_CACHE = {}


def case_id(case):
    return "N%d-d%d-p%g" % case


def inputs(case, duplicate=False):
    """(Z float32 [N, d], labels [N])"""
    N, d, perp = case
    rng = np.random.RandomState(900 + N + 7 * d)
    K = 4 + (N % 2)
    centres = 4.0 * rng.standard_normal((K, d))
    labels = np.arange(N) % K
    Z = (centres[labels] + rng.standard_normal((N, d))).astype(np.float32)
    if duplicate:
        Z[1::2] = Z[0::2]          # N is even
        labels[1::2] = labels[0::2]
    return Z, labels


def sqdist(Z, dtype=WIDE):
    Z = np.asarray(Z).astype(dtype)
    N = Z.shape[0]
    D = np.zeros((N, N), dtype=dtype)
    for i in range(N):
        diff = Z[i][None, :] - Z
        D[i] = (diff * diff).sum(axis=1)
    D[np.arange(N), np.arange(N)] = 0
    return D


def affinities(D, perplexity, tol=1e-5, dtype=WIDE):
    """all rows searched together: dict(beta, steps, Pc, S, dprime, visited [steps taken][N] with NaN once a row has stopped)"""
    D = np.asarray(D).astype(dtype)
    N = D.shape[0]
    off = ~np.eye(N, dtype=bool)
    dp = np.where(off, D - np.where(off, D, np.inf).min(axis=1)[:, None], 0)
    target = np.log(dtype(perplexity))
    beta, lo, hi = np.ones(N, dtype=dtype), np.full(N, -np.inf, dtype=dtype), np.full(N, np.inf, dtype=dtype)
    live = np.ones(N, dtype=bool)
    be, S, steps = beta.copy(), np.ones(N, dtype=dtype), np.zeros(N, dtype=np.int64)
    visited = []
    for step in range(SEARCH_STEPS):
        if not live.any():
            break
        r = np.nonzero(live)[0]
        b = beta[r]
        e = np.where(off[r], np.exp(-b[:, None] * dp[r]), 0)
        s = e.sum(axis=1)
        diff = (np.log(s) + b * (dp[r] * e).sum(axis=1) / s) - target
        be[r], S[r], steps[r] = b, s, step + 1
        rec = np.full(N, np.nan)
        rec[r] = np.abs(diff).astype(np.float64)
        visited.append(rec)
        stop = np.abs(diff) <= tol
        up = (diff > 0) & ~stop
        dn = ~(diff > 0) & ~stop
        ru, rd = r[up], r[dn]
        lo[ru] = b[up]
        beta[ru] = np.where(np.isinf(hi[ru]), b[up] * 2, (b[up] + hi[ru]) / 2)
        hi[rd] = b[dn]
        beta[rd] = np.where(np.isinf(lo[rd]), b[dn] / 2, (b[dn] + lo[rd]) / 2)
        live[r[stop]] = False
    Pc = np.where(off, np.exp(-be[:, None] * dp), 0) / S[:, None]
    return {"beta": be, "steps": steps, "Pc": Pc, "S": S, "dprime": dp, "visited": np.array(visited)}


def joint(Pc):
    V = Pc + Pc.T
    P = np.maximum(V / V.sum(), EPS)
    P[np.arange(len(P)), np.arange(len(P))] = 0
    return P


def forces(Y, P, ex, dtype=WIDE, scales=False, want_kl=True):
    """(kl, grad [N, 2]); with scales also (the sum of |terms| behind the KL, behind every gradient entry).  Without want_kl the KL is None (no logarithms)."""
    Y, P = np.asarray(Y).astype(dtype), np.asarray(P).astype(dtype, copy=False)
    x, y = Y[:, 0], Y[:, 1]
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    w = 1 / (1 + dx * dx + dy * dy)
    np.fill_diagonal(w, 0)
    Zs = w.sum()
    pw, ww = P * w, w * w
    A = np.stack([(pw * dx).sum(axis=1), (pw * dy).sum(axis=1)], axis=1)
    R = np.stack([(ww * dx).sum(axis=1), (ww * dy).sum(axis=1)], axis=1)
    grad = 4 * (ex * A - R / Zs)
    kl = None
    if want_kl or scales:
        off = ~np.eye(len(Y), dtype=bool)
        Po, wo = P[off], w[off]
        kl = (ex * Po * np.log(ex * Po * Zs / wo)).sum()
    if not scales:
        return kl, grad
    kls = (ex * Po * (np.abs(np.log(Po)) + np.abs(np.log(wo)) + abs(math.log(ex)) + np.abs(np.log(Zs)))).sum()
    gs = 4 * (ex * np.stack([(pw * np.abs(dx)).sum(axis=1), (pw * np.abs(dy)).sum(axis=1)], axis=1)
              + np.stack([(ww * np.abs(dx)).sum(axis=1), (ww * np.abs(dy)).sum(axis=1)], axis=1) / Zs)
    return kl, grad, float(kls), gs.astype(np.float64)


def step(Y, update, gains, P, ex, momentum, lr, dtype=WIDE, want_kl=True):
    """one iteration of sklearn's _gradient_descent: dict(Y, update, gains, kl, grad, gg, grad_norm, inc)"""
    kl, grad = forces(Y, P, ex, dtype, want_kl=want_kl)
    update, gains = np.asarray(update).astype(dtype), np.asarray(gains).astype(dtype)
    inc = update * grad < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01))
    gg = gains * grad
    update = dtype(momentum) * update - dtype(lr) * gg
    return {"Y": np.asarray(Y).astype(dtype) + update, "update": update, "gains": gains, "kl": kl, "grad": grad, "gg": gg, "grad_norm": np.sqrt((gg * gg).sum()),
            "inc": inc}


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def fit(P, Y0, early_exaggeration=12.0, learning_rate=None, max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, dtype=np.float64, keep=(),
        margins=None):
    """the schedule of the device's fit: dict(Y, kl, n_iter, reason, checks [(i, kl, grad_norm)], states {i: (Y, update, gains) before iteration i, float64}).
    margins: a list that receives, per iteration, the smallest |grad| / (its sum of |terms|) and |update| / (|momentum update| + |lr gains grad|)."""
    N = len(Y0)
    lr = auto_learning_rate(N, early_exaggeration) if learning_rate is None else learning_rate
    Y, P = np.asarray(Y0).astype(dtype), np.asarray(P).astype(dtype)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    states, checks, reason, last, nxt, stop = {}, [], 0, 0, 0, False
    for phase in range(2):
        if stop:
            break
        ex, momentum = (early_exaggeration, 0.5) if phase == 0 else (1.0, 0.8)
        end = min(EXPLORE, max_iter) if phase == 0 else max_iter
        limit = EXPLORE if phase == 0 else n_iter_without_progress
        best, best_iter = np.finfo(np.float64).max, nxt
        for i in range(nxt, end):
            if i in keep:          # the state goes on from its float64 rounding: a kernel handed it starts from the reference's own input
                Y, update, gains = (a.astype(np.float64).astype(dtype) for a in (Y, update, gains))
                states[i] = tuple(a.astype(np.float64) for a in (Y, update, gains))
            if margins is not None:
                _, g, _, gs = forces(Y, P, ex, dtype, scales=True)
            s = step(Y, update, gains, P, ex, momentum, lr, dtype, want_kl=(i + 1) % CHECK == 0)
            if margins is not None:
                us = np.abs(momentum * update) + np.abs(lr * s["gg"])
                nz = us > 0
                margins.append((float((np.abs(g) / gs).min()), float((np.abs(s["update"])[nz] / us[nz]).min())))
            Y, update, gains = s["Y"], s["update"], s["gains"]
            last, nxt = i, i + 1
            if (i + 1) % CHECK:
                continue
            err, gn = float(s["kl"]), float(s["grad_norm"])
            checks.append((i, err, gn))
            if err < best:
                best, best_iter = err, i
            elif i - best_iter > limit:
                reason = 2 if phase == 1 else reason
                break
            if gn <= min_grad_norm:
                reason, stop = 1, True
                break
    kl, _ = forces(Y, P, 1.0, dtype)
    return {"Y": Y, "kl": kl, "n_iter": last, "reason": reason, "checks": checks, "states": states}


def random_init(N, random_state=42):
    """sklearn's own draw for init="random" """
    return (1e-4 * np.random.RandomState(random_state).standard_normal((N, 2)).astype(np.float32)).astype(np.float64)


def wide(case, duplicate=False):
    """Z, labels and the wide affinities of a case at tol = 1e-5 and tol = 0, once; nothing may write to them.  D64 and P64 are the float64 roundings the later
    stages start from."""
    key = ("aff", case, duplicate)
    if key not in _CACHE:
        Z, labels = inputs(case, duplicate)
        D = sqdist(Z)
        D64 = D.astype(np.float64)
        out = {"Z": Z, "labels": labels, "D": D, "D64": D64}
        for name, tol in (("tol", 1e-5), ("tol0", 0.0)):
            a = affinities(D64, case[2], tol)
            a["P"] = joint(a["Pc"])
            out[name] = a
        out["P64"] = out["tol"]["P"].astype(np.float64)
        _CACHE[key] = out
    return _CACHE[key]


def trajectory(case, margins=False):
    """the wide run from init="random", random_state=42 to iteration 400, with the states before iterations 0, 200 and 400 and, wide, the Y after TRAJ_STEPS"""
    key = ("traj", case, margins)
    if key not in _CACHE:
        ref = wide(case)
        N = case[0]
        m = [] if margins else None
        run = fit(ref["P64"], random_init(N), max_iter=max(STATE_ITERS) + 1, dtype=WIDE, keep=STATE_ITERS, margins=m)
        short = fit(ref["P64"], random_init(N), max_iter=TRAJ_STEPS, dtype=WIDE)
        _CACHE[key] = {"states": run["states"], "short": short, "margins": m}
    return _CACHE[key]


def phase_of(i):
    """(exaggeration, momentum) of iteration i under the default schedule"""
    return (12.0, 0.5) if i < EXPLORE else (1.0, 0.8)


def e2e_reference(case):
    """float64 runs of the full schedule from random_init: the unperturbed one and E2E_K from the init moved by one ulp in random directions"""
    key = ("e2e", case)
    if key not in _CACHE:
        ref = wide(case)
        N = case[0]
        Y0 = random_init(N)
        rng = np.random.RandomState(4242 + N)
        runs = [fit(ref["P64"], Y0)]
        for _ in range(E2E_K):
            sign = rng.choice([-1.0, 1.0], size=Y0.shape)
            runs.append(fit(ref["P64"], np.nextafter(Y0, sign * np.inf)))
        _CACHE[key] = runs
    return _CACHE[key]


def nearest_neighbour_labels_agree(Y, labels):
    Y = np.asarray(Y, dtype=np.float64)
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=-1)
    D[np.arange(len(Y)), np.arange(len(Y))] = np.inf
    return bool((labels[D.argmin(axis=1)] == labels).all())


# ---- bounds ----
def _f(x):
    return np.asarray(x).astype(np.float64)


def bound_D(case, D, c=None):
    """a sum of d squares of differences: (d + 2) roundings relative to the entry"""
    c = C_TSNE_D if c is None else c
    return c * (case[1] + 2) * U * _f(D)


def bounds_affinities(case, a, c=None):
    """a: affinities() of the wide reference with its P.  With T = log2 N + 6 roundings per reduced sum:
    H within eH = c T U (1 + |log S| + beta E d'); beta within eH / (beta Var d') + c U beta (dH / dbeta = -beta Var_p d', the search's fixed point moves by the
    error of H over that slope); Pc within Pc (c T U (1 + beta d') + |d' - E d'| e_beta) and an underflow; P within (e_ij + e_ji) / sum + c T U P; sum P within c 2 T U of 1, plus 2^-52 for every
    clamped entry."""
    c = C_TSNE_AFF if c is None else c
    N = case[0]
    T = math.log2(N) + 6
    beta, S, dp, Pc = _f(a["beta"]), _f(a["S"]), _f(a["dprime"]), _f(a["Pc"])
    Ed = (Pc * dp).sum(axis=1)
    var = (Pc * (dp - Ed[:, None]) ** 2).sum(axis=1)
    eH = c * T * U * (1 + np.abs(np.log(S)) + beta * Ed)
    eb = eH / (beta * var) + c * U * beta
    ePc = Pc * (c * T * U * (1 + beta[:, None] * dp) + np.abs(dp - Ed[:, None]) * eb[:, None]) + c * 2.0 ** -1022          # and an underflow
    eP = (ePc + ePc.T) / (2.0 * N) + c * T * U * _f(a["P"])
    clamped = int((_f(a["P"]) == EPS).sum())          # every clamped entry lifts the sum by up to 2^-52: that is the definition, not an error
    return {"beta": eb, "Pc": ePc, "P": eP, "sumP": c * 2 * T * U + clamped * EPS}


def bounds_forces(case, kl_scale, grad_scale, c=None):
    """log2 N + 8 roundings relative to the sum of |terms| of each output"""
    c = C_TSNE_FORCE if c is None else c
    T = math.log2(case[0]) + 8
    return {"kl": c * 2 * T * U * kl_scale, "grad": c * T * U * grad_scale}


def bounds_step(case, s, update_in, momentum, lr, grad_bound, c=None):
    """s: step() of the wide reference.  gains: two roundings; gains grad: the gradient's bound times the gain and three roundings; the update: three roundings
    of its two terms and lr times that; Y: the update's and one rounding; the norm: the norm of the bounds and its own log2 N + 4 roundings."""
    c = C_TSNE_STEP if c is None else c
    g, gg = _f(s["gains"]), _f(s["gg"])
    e_gg = g * grad_bound + c * 3 * U * np.abs(gg)
    e_u = c * 3 * U * (np.abs(momentum * _f(update_in)) + lr * np.abs(gg)) + lr * e_gg
    return {"gains": c * 2 * U * g, "update": e_u, "Y": e_u + c * U * np.abs(_f(s["Y"])),
            "grad_norm": float(np.sqrt((e_gg ** 2).sum()) + c * (math.log2(case[0]) + 4) * U * float(s["grad_norm"]))}


def bound_trajectory(Y, c=None):
    """TRAJ_STEPS iterations of a map that stretches errors: c steps 2^-53 max |Y|, the constant from the rule like the others"""
    c = C_TSNE_TRAJ if c is None else c
    return c * TRAJ_STEPS * U * float(np.abs(_f(Y)).max())


def max_ratio(got, want, bound):
    got, want, bound = np.asarray(got), np.asarray(want), np.asarray(bound, dtype=np.float64)
    err = np.abs(got.astype(WIDE) - want).astype(np.float64)
    if not np.isfinite(np.asarray(got, dtype=np.float64)).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))
