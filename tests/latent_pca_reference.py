"""Reference for the latent PCA (causal_vae_amd.vit.latent_pca; csrc/eigh.hip and csrc/ridge.hip), numpy only.

inputs          Z = S B + 0.05 noise in float32 with a designed spectrum: S [N, r] standard normal with column scales 8, 4, 2, 1, 1/2, ... (r = k + 2), B [r, d] with
                orthonormal rows: the leading variances are about 64 : 16 : 4 : 1 ... apart, the rest is the noise floor.
wide            PCA in numpy.longdouble through tests/eigh_reference.py's Jacobi on whichever of Xc^T Xc [d, d] and Xc Xc^T [N, N] is smaller (for the dual,
                v = Xc^T u / sqrt(lambda)); the top k in descending order, sklearn >= 1.5's sign rule (each component's entry of largest |value| positive,
                lowest index on a tie), explained_variance = lambda / (N - 1), the ratio to the sum of all, singular values sqrt(lambda), scores = Xc V_k^T; and
                what the tests assert on the reference alone: rel_gap (the smaller neighbouring eigengap of every kept component over its eigenvalue, to be
                above 1e-3) and sign_lead (how far the sign-deciding entry leads the runner-up, relative, to be above 1e-6).
bounds          with delta_k the smaller neighbouring gap of component k (Davis-Kahan): eigenvalues within c (N + d) 2^-53 lambda_1 (so explained_variance
                within that over N - 1, singular values within that over 2 sqrt(lambda_k), the ratio within twice that over the sum); components within
                c (N + d) 2^-53 lambda_1 / delta_k; a row of transform within the component's bound times the row's centred norm, plus
                c (N + d) 2^-53 times that norm for the product itself.
C_PCA           the rule of the other references: four times the largest ratio that the same algebra in float64 numpy (numpy.linalg.eigh on Xc^T Xc) reaches
                with c = 1 over CASES, rounded up to a power of two, at least 1.  Measured (tests/test_latent_pca_cpu.py re-measures and holds every line): the largest is 0.017, so C_PCA = 1."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigh_reference as er  # noqa: E402

U, WIDE = er.U, er.WIDE
C_PCA = 1.0
CASES = [(16, 512, 4), (97, 64, 3), (300, 130, 5)]          # (N, d, k)
KEYS = ("mean", "components", "explained_variance", "explained_variance_ratio", "singular_values", "scores")
_WIDE = {}


def case_id(case):
    return "N%d-d%d-k%d" % case


def inputs(case):
    N, d, k = case
    rng = np.random.RandomState(500 + N + 3 * d + k)
    r = k + 2
    S = rng.standard_normal((N, r)) * (8.0 / 2.0 ** np.arange(r))
    B = np.linalg.qr(rng.standard_normal((d, r)))[0].T
    return (S @ B + 0.05 * rng.standard_normal((N, d)) + rng.standard_normal(d)).astype(np.float32)


def flip(components):
    """sklearn >= 1.5's svd_flip on V: each row's entry of largest |value| (lowest index on a tie) becomes positive"""
    lead = np.argmax(np.abs(components), axis=1)          # argmax returns the first of equals
    sign = np.where(components[np.arange(len(components)), lead] < 0, -1, 1).astype(components.dtype)
    return components * sign[:, None]


def _finish(Z, mean, Xc, lam_desc, comps, k):
    N = Z.shape[0]
    lam_k = lam_desc[:k]
    comps = flip(comps)
    return {"mean": mean, "components": comps, "explained_variance": lam_k / (N - 1), "explained_variance_ratio": lam_k / lam_desc.sum(),
            "singular_values": np.sqrt(lam_k), "scores": Xc @ comps.T, "lambda": lam_desc}


def wide(case):
    """(Z, the wide PCA of the case), computed once and shared; nothing may write to it"""
    if case not in _WIDE:
        Z = inputs(case)
        N, d, k = case
        Zw = Z.astype(WIDE)
        mean = Zw.sum(axis=0) / N
        Xc = Zw - mean
        if N < d:
            lam, Um, _ = er.jacobi_eigh(Xc @ Xc.T)
            lam = np.maximum(lam[::-1], 0)
            comps = (Xc.T @ Um[:, ::-1][:, :k] / np.sqrt(lam[:k])).T
            lam_desc = np.concatenate([lam, np.zeros(d - N, dtype=WIDE)])
        else:
            lam, V, _ = er.jacobi_eigh(Xc.T @ Xc)
            lam_desc = np.maximum(lam[::-1], 0)
            comps = V[:, ::-1][:, :k].T.copy()
        ref = _finish(Zw, mean, Xc, lam_desc, comps, k)
        lam64 = lam_desc.astype(np.float64)
        gaps = np.array([min(lam64[j - 1] - lam64[j] if j > 0 else np.inf, lam64[j] - lam64[j + 1]) for j in range(k)])
        ref["delta"] = gaps
        ref["rel_gap"] = gaps / lam64[:k]
        a = np.sort(np.abs(ref["components"].astype(np.float64)), axis=1)
        ref["sign_lead"] = (a[:, -1] - a[:, -2]) / a[:, -1]
        ref["row_norm"] = np.sqrt((Xc.astype(np.float64) ** 2).sum(axis=1))
        _WIDE[case] = (Z, ref)
    return _WIDE[case]


def pca_float(Z, k, dtype=np.float64):
    """the algebra of the device route in `dtype`: numpy.linalg.eigh on the centred Gram matrix"""
    Z = np.asarray(Z).astype(dtype)
    mean = Z.mean(axis=0)
    Xc = Z - mean
    lam, V = np.linalg.eigh(Xc.T @ Xc)
    return _finish(Z, mean, Xc, np.maximum(lam[::-1], 0), V[:, ::-1][:, :k].T.copy(), k)


def bounds(case, ref, c=None):
    c = C_PCA if c is None else c
    N, d, k = case
    lam = ref["lambda"].astype(np.float64)
    e_lam = c * (N + d) * U * lam[0]
    e_comp = e_lam / ref["delta"]
    return {"mean": c * (N + 8) * U * np.abs(ref["mean"].astype(np.float64)).max() * np.ones(d) + c * (N + 8) * U, "components": e_comp[:, None],
            "explained_variance": e_lam / (N - 1), "explained_variance_ratio": 2 * e_lam / lam.sum(), "singular_values": e_lam / (2 * np.sqrt(lam[:k])),
            "scores": (e_comp[None, :] + c * (N + d) * U) * ref["row_norm"][:, None]}


def ratios(got, ref, b):
    from ridge_translator_reference import max_ratio
    return {key: max_ratio(got[key], ref[key], b[key]) for key in KEYS}
