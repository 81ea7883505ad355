"""What the ridge alpha path (ops.ridge_loo_path, fit_translator_ridge_cv) rests on, checked without a GPU on tests/ridge_path_reference.py:
  identity      the eigen route in float64 numpy gives, for every alpha of the grid, the leave-one-out predictions of N separate fits (rr.naive_loo)
  the constant  C_PATH follows the rule from the ratios the float64 eigen route reaches against the wide Cholesky closed form with c = 1
  selection     on the wide reference alone, the best alpha of the grid leads the runner-up by more than 1e-6 under both criteria on every case; the float64
                eigen route chooses the same; sklearn's RidgeCV(alphas, fit_intercept=True).alpha_ agrees with "mse", where sklearn imports
  tie           at N = 2 every alpha gives the same leave-one-out predictions: why that case is left out of the selection cases
  refusals      every refusal of ops.ridge_loo_path and fit_translator_ridge_cv is raised without a device

Measured here, max |float64 eigen route - wide| / bound with c = 1, the largest over the grid {1e-3, 1e-1, 1, 10, 1e3} (the RATIO lines):
  N2-d1-F1        leverage 0.14 loo 1.3 r2 0.16 corr 0 sse 0.16
  N16-d512-F7     leverage 0.0028 loo 0.0057 r2 0.0012 corr 0.00031 sse 0.00098
  N40-d8-F5-const leverage 0.019 loo 0.065 r2 0.0039 corr 0.00076 sse 0.0044
  N97-d64-F12     leverage 0.0031 loo 0.0089 r2 0.00081 corr 0.00028 sse 0.0019
  N300-d130-F3    leverage 0.00099 loo 0.0052 r2 0.0002 corr 2.3e-05 sse 0.00074
  N40-d8-F5       leverage 0.019 loo 0.065 r2 0.0039 corr 0.0014 sse 0.0081
The largest is 1.256: four times that, rounded up to a power of two, is C_PATH = 8.
Selection on SELECT_GRID = {1, 100, 1e4}, the wide reference's choice and margin, "mse" then "r2": N16-d512-F7 100 (9.2e-4), 1 (0.14); N40-d8-F5 1 (7.2), 1 (0.61);
N97-d64-F12 1 (0.56), 100 (1.1); N300-d130-F3 1 (0.43), 1 (0.014); N4500-d8-F2 1 (1.8e-3), 1 (4.3e-4)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ridge_path_reference as rp  # noqa: E402
import ridge_translator_reference as rr  # noqa: E402


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_eigen_route_equals_n_separate_fits(case):
    Z, M, refs = rp.wide(case)
    got, lam = rp.eigen_path(Z, M)
    assert (lam >= 0).all() and (np.diff(lam) >= 0).all()
    for alpha, o, ref in zip(rp.GRID, got, refs):
        ratio = rr.max_ratio(o["loo"], rr.naive_loo(Z, M, alpha), rp.bounds(ref, M)["loo"])
        print(f"RATIO eigen-vs-naive {rr.case_id(case)} alpha {alpha:g} loo {ratio:.4g}")
        assert ratio <= 1.0


def test_bound_constant_follows_its_rule():
    print(rr.PRECISION)
    worst = 0.0
    for case in rr.CASES:
        Z, M, refs = rp.wide(case)
        got, _lam = rp.eigen_path(Z, M)
        per_key = {k: 0.0 for k in rp.KEYS}
        for o, ref in zip(got, refs):
            for k, v in rp.ratios(o, ref, rp.bounds(ref, M, c=1.0)).items():
                per_key[k] = max(per_key[k], v)
        print(f"RATIO numpy-float64 eigen route c=1 {rr.case_id(case)} " + " ".join(f"{k} {v:.2g}" for k, v in per_key.items()))
        worst = max(worst, max(per_key.values()))
    rule = max(1.0, 2.0 ** math.ceil(math.log2(4.0 * worst)))
    print(f"largest ratio {worst:.4g}: c = {rule:g}")
    assert rp.C_PATH == rule


@pytest.mark.parametrize("case", rp.SELECT_CASES, ids=rr.case_id)
def test_the_grid_has_a_clear_best_alpha_and_float64_finds_it(case):
    Z, M, refs = rp.wide(case, rp.SELECT_GRID)
    got, _lam = rp.eigen_path(Z, M, rp.SELECT_GRID)
    for criterion in ("mse", "r2"):
        best, margin = rp.select(refs, M, criterion)
        print(f"SELECT {rr.case_id(case)} {criterion}: alpha {rp.SELECT_GRID[best]:g}, margin {margin:.3g}")
        assert margin > 1e-6
        assert rp.select(got, M, criterion)[0] == best


@pytest.mark.parametrize("case", [rr.CASES[2], rr.CASES[3]], ids=rr.case_id)
def test_sklearn_ridgecv_chooses_the_same_alpha(case):
    lm = pytest.importorskip("sklearn.linear_model")
    Z, M, refs = rp.wide(case, rp.SELECT_GRID)
    model = lm.RidgeCV(alphas=rp.SELECT_GRID, fit_intercept=True).fit(Z.astype(np.float64), M)
    assert float(model.alpha_) == rp.SELECT_GRID[rp.select(refs, M, "mse")[0]]


def test_two_rows_are_a_tie_by_construction():
    """N = 2: each leave-one-out fit sees one row, whose centred latent is 0, and predicts the other row's value whatever alpha is"""
    Z, M, refs = rp.wide(rr.CASES[0])
    assert rr.CASES[0][0] == 2 and rr.CASES[0] not in rp.SELECT_CASES
    for ref in refs:
        assert rr.max_ratio(ref["loo"], M[::-1].astype(rr.WIDE), 64 * rr.U * np.abs(M).max(axis=0)[None, :]) <= 1.0


def test_refusals_need_no_device():
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import fit_translator_ridge_cv
    Z, M = torch.zeros(6, 4), torch.zeros(6, 3, dtype=torch.float64)
    for bad, pattern in [([], "alphas is empty"), ([1.0, 0.0], "positive and finite"), ([-1.0], "positive and finite"), ([float("nan")], "positive and finite"),
                         ([float("inf")], "positive and finite"), ([1.0] * 65, "at most 64 alphas"), (3.0, "sequence of numbers")]:
        with pytest.raises(CvaeError, match=pattern):
            ops.ridge_loo_path(Z, M, bad)
        with pytest.raises(CvaeError, match=pattern):
            fit_translator_ridge_cv(Z.numpy(), M.numpy(), alphas=bad)
    for z, m, pattern in [(torch.zeros(6), M, r"Z \[N, d\] and M \[N, F\] expected"), (Z.to(torch.float16), M, "float32 or float64"), (Z, M[:5], "Z has 6 rows, M has 5"),
                          (Z[:1], M[:1], "at least 2 samples"), (torch.zeros(6, 1025), M, "1 <= d <= 1024"), (torch.zeros(6, 0), M, "1 <= d <= 1024"),
                          (Z, M[:, :0], "at least one feature column")]:
        with pytest.raises(CvaeError, match=pattern):
            ops.ridge_loo_path(z, m, rp.GRID)
    with pytest.raises(CvaeError, match='select must be "mse" or "r2"'):
        fit_translator_ridge_cv(Z.numpy(), M.numpy(), select="aic")
    with pytest.raises(CvaeError, match="feature_names has 2 entries for 3 feature columns"):
        fit_translator_ridge_cv(Z.numpy(), M.numpy(), feature_names=("a", "b"))
    with pytest.raises(CvaeError, match="MI355X only"):          # and with everything in order, the CPU tensors themselves are refused: no fallback
        ops.ridge_loo_path(Z, M, rp.GRID)
