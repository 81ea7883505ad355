"""Reference for the symmetric eigensolver (csrc/eigh.hip, cvae_eigh_f64), numpy only.

jacobi_eigh     a cyclic two-sided Jacobi method written out, in numpy.longdouble by default (x87 extended, eps 1.08e-19; float64 if this machine's longdouble
                is no wider, which PRECISION says): every pair (p, q) once per sweep, the disjoint pairs of a round-robin round rotated together (vectorised),
                Rutishauser's rotation, sweeps until one meets no |a_pq| above eps / 2 max |A|.  Eigenvalues ascending, ties by original index.
measures        what the tests assert of any (w, V), evaluated in the wide type, as ratios to bounds with c = 1:
                    residual  max |A V - V diag(w)|   / (n 2^-53 max |A|)
                    orth      max |V^T V - I|         / (n 2^-53)
                    trace     |sum w - tr A|          / (n 2^-53 sum |a_ii|)
                    eig       max |w - w_ref|         / (n 2^-53 ||A||_2)        (w_ref: the wide run, or eigvalsh at twice the bound where that is unaffordable)
C_EIGH          four times the largest of these ratios that two float64 evaluations reach over CASES (numpy.linalg.eigh, and jacobi_eigh run in float64), rounded
                up to a power of two, at least 1; the factor of four is for another pair order, FMA contraction and the rotation formula, as in
                ridge_translator_reference.  tests/test_eigh_cpu.py re-measures and holds every figure.  Measured: numpy.linalg.eigh reaches 1.17 (orth, n = 3), the
                float64 Jacobi 5.52 (orth at n = 512, after 12 sweeps of 511 rounds) and 2.54 below that size; residual, trace and eig stay below 1.1.
                So C_EIGH = 32."""
import numpy as np

U = 2.0 ** -53
WIDE = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64
PRECISION = f"reference precision: {np.dtype(WIDE).name}, eps {float(np.finfo(WIDE).eps):.3e}" + ("" if WIDE is not np.float64 else
                                                                                               " (no wider longdouble on this machine: float64)")
C_EIGH = 32.0
MAX_SWEEPS = 60

# name -> what the wide run can afford
CASES = ["n1", "n2", "n3-bye", "n5-identity-plus-rank-one", "n7-diagonal", "n2-angle-underflows", "n64", "n65", "n130", "gram-16x512"]
WIDE_AFFORDABLE = [c for c in CASES if c != "gram-16x512"]


def random_symmetric(n, seed):
    B = np.random.RandomState(seed).standard_normal((n, n))
    return (B + B.T) / 2.0


def gram_16x512():
    """the regime's own matrix: the centred Gram matrix of a 16 x 512 float32 standard normal Z, rank 15 with 497 zero eigenvalues"""
    Z = np.random.RandomState(16512).standard_normal((16, 512)).astype(np.float32).astype(np.float64)
    Xc = Z - Z.mean(axis=0)
    G = Xc.T @ Xc
    return (G + G.T) / 2.0


def matrix(name):
    """the float64 symmetric matrix of a case"""
    if name == "n1":
        return np.array([[-3.25]])
    if name == "n2":
        return random_symmetric(2, 2)
    if name == "n3-bye":
        return random_symmetric(3, 3)
    if name == "n5-identity-plus-rank-one":
        u = np.array([1.0, -2.0, 0.5, 3.0, 1.5])
        return np.eye(5) + np.outer(u, u)          # the eigenvalue 1 four times, 1 + |u|^2 once
    if name == "n7-diagonal":
        return np.diag([3.0, -1.0, 2.0, 2.0, 0.0, 7.5, -4.0])
    if name == "n2-angle-underflows":
        return np.array([[1.0, 1e-200], [1e-200, 2.0]])
    if name == "gram-16x512":
        return gram_16x512()
    n = int(name[1:])
    return random_symmetric(n, 100 + n)


def round_pairs(n, r):
    """the disjoint pairs (p < q < n) of round r of the round-robin order on n indices (an odd n: the index paired with n sits out)"""
    m = n + (n & 1)
    k = np.arange(1, m // 2)
    a = np.concatenate([[m - 1], (r + k) % (m - 1)])
    b = np.concatenate([[r], (r - k) % (m - 1)])
    p, q = np.minimum(a, b), np.maximum(a, b)
    keep = q < n
    return p[keep], q[keep]


def jacobi_eigh(A, dtype=None, max_sweeps=MAX_SWEEPS):
    """(w ascending, V with column k the eigenvector of w[k], sweeps) of the symmetric matrix whose lower triangle A holds, in `dtype` (default: WIDE)"""
    dtype = WIDE if dtype is None else dtype
    A = np.asarray(A).astype(dtype)
    n = A.shape[0]
    A = np.tril(A) + np.tril(A, -1).T
    Vt = np.eye(n, dtype=dtype)
    tol = dtype(np.finfo(dtype).eps) / 2 * (np.abs(A).max() if n else dtype(0))
    m = n + (n & 1)
    sweeps = 0
    one = dtype(1)
    while sweeps < max_sweeps:
        sweeps += 1
        off = dtype(0)
        for r in range(m - 1):
            p, q = round_pairs(n, r)
            if len(p) == 0:
                continue
            apq, app, aqq = A[p, q], A[p, p], A[q, q]
            off = max(off, np.abs(apq).max())
            nz = apq != 0
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                zeta = np.where(nz, (aqq - app) / np.where(nz, 2 * apq, one), one)
                t = np.where(nz, np.where(zeta >= 0, one, -one) / (np.abs(zeta) + np.sqrt(one + zeta * zeta)), dtype(0))
            c = one / np.sqrt(one + t * t)
            s = c * t
            cc, ss = c[:, None], s[:, None]
            for _side in range(2):          # rows: A <- J^T A; then the same on the transpose (A is symmetric): J^T (J^T A)^T = J^T A J.  Rows are contiguous.
                Ap, Aq = A[p], A[q]
                A[p], A[q] = cc * Ap - ss * Aq, ss * Ap + cc * Aq
                A = np.ascontiguousarray(A.T)
            A[p, p], A[q, q] = app - t * apq, aqq + t * apq
            A[p, q] = 0
            A[q, p] = 0
            Vp, Vq = Vt[p], Vt[q]          # V <- V J on the transpose
            Vt[p], Vt[q] = cc * Vp - ss * Vq, ss * Vp + cc * Vq
        if off <= tol:
            break
    w = np.diag(A).copy()
    order = np.argsort(w, kind="stable")
    return w[order], np.ascontiguousarray(Vt.T)[:, order], sweeps


def measures(A, w, V, w_ref=None):
    """the ratios of the module docstring with c = 1, from float64 (w, V) evaluated in the wide type; `eig` only with a reference spectrum"""
    Aw, ww, Vw = np.asarray(A).astype(WIDE), np.asarray(w).astype(WIDE), np.asarray(V).astype(WIDE)
    n = Aw.shape[0]
    amax, dsum = float(np.abs(Aw).max()), float(np.abs(np.diag(Aw)).sum())
    out = {"residual": float(np.abs(Aw @ Vw - Vw * ww[None, :]).max()) / (n * U * amax) if amax > 0 else 0.0,
           "orth": float(np.abs(Vw.T @ Vw - np.eye(n, dtype=WIDE)).max()) / (n * U),
           "trace": float(abs(ww.sum() - np.trace(Aw))) / (n * U * dsum) if dsum > 0 else 0.0}
    if w_ref is not None:
        norm2 = float(np.abs(np.asarray(w_ref).astype(WIDE)).max())
        out["eig"] = float(np.abs(ww - np.asarray(w_ref).astype(WIDE)).max()) / (n * U * norm2) if norm2 > 0 else 0.0
    return out
