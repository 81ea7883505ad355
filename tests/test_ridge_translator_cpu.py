"""What the latent translator's kernels (csrc/ridge.hip) rest on, checked without a GPU on tests/ridge_translator_reference.py's cases:
  identity      the closed-form leave-one-out prediction (b, numpy.longdouble) equals N separate fits (a, float64) within the bound on every case; so does
                sklearn's Ridge(alpha, fit_intercept=True) on float64 inputs, where sklearn imports
  the constant  C_BOUND follows the rule of the reference module from the ratios numpy's own float64 closed form reaches against (b)
  float32       the float32 evaluation the reference actually performs misses the bound at N = 16, d = 512 by orders of magnitude: the bound tells fp64 from fp32
  refusals      the argument checks of ops.ridge_fit_loo / ops.group_means_resampled / fit_translator_ridge that need no device
  bootstrap     the restatement of the reference's bootstrap against a case small enough to check by hand, and the host-side helpers of vit/translator.py

Measured here, max |numpy float64 - (b)| / bound with c = 1 (the RATIO lines), per case over coef, intercept, fitted, loo, leverage, r2, corr:
  N2-d1-F1       coef 0.68 intercept 0.20 fitted 0.21 loo 1.15 leverage 0.19 r2 0.078 corr 0
  N16-d512-F7    coef 0.021 intercept 0.0042 fitted 2.4e-05 loo 4.5e-05 leverage 4.8e-05 r2 3.4e-06 corr 1.7e-06
  N40-d8-F5      coef 0.033 intercept 0.34 fitted 0.021 loo 0.019 leverage 0.0090 r2 0.00062 corr 0.00042   (alpha 1e-3: 0.033 0.15 0.022 0.017 0.0066 0.00074 0.00044)
  N97-d64-F12    coef 0.0032 intercept 0.18 fitted 0.0017 loo 0.0012 leverage 0.00066 r2 3.8e-05 corr 2.4e-05
  N300-d130-F3   coef 0.0042 intercept 0.013 fitted 0.0010 loo 0.00097 leverage 0.00061 r2 1.3e-05 corr 3.7e-06
The largest is 1.15 (N = 2, d = 1, where one rounding is most of the bound): four times that, rounded up to a power of two, is C_BOUND = 8.
(a) against (b), loo, with c = 8: at most 0.0022 of the bound.  float32 at N = 16, d = 512 with c = 8: coef 3.6e5, loo 2.9e3, leverage 4.0e3 bounds."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ridge_translator_reference as rr  # noqa: E402

_REF = {}


def reference(case):
    """the inputs and (b) of a case, computed once and shared"""
    if case not in _REF:
        Z, M = rr.inputs(case)
        _REF[case] = (Z, M, rr.closed_form(Z, M, case[3]))
    return _REF[case]


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_closed_form_equals_n_separate_fits(case):
    Z, M, ref = reference(case)
    print(rr.PRECISION)
    ratio = rr.max_ratio(rr.naive_loo(Z, M, case[3]), ref["loo"], rr.bounds(ref, M)["loo"])
    print(f"RATIO naive-vs-closed {rr.case_id(case)} loo {ratio:.4g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_sklearn_ridge_equals_the_naive_form(case):
    lm = pytest.importorskip("sklearn.linear_model")
    Z, M, ref = reference(case)
    Z64 = Z.astype(np.float64)
    P = np.zeros_like(M)
    for i in range(len(Z)):
        keep = np.arange(len(Z)) != i
        P[i] = lm.Ridge(alpha=case[3], fit_intercept=True).fit(Z64[keep], M[keep]).predict(Z64[i:i + 1]).reshape(-1)
    b = rr.bounds(ref, M)
    full = lm.Ridge(alpha=case[3], fit_intercept=True).fit(Z64, M)
    ratios = {"loo-vs-naive": rr.max_ratio(P, rr.naive_loo(Z, M, case[3]), b["loo"]), "loo": rr.max_ratio(P, ref["loo"], b["loo"]),
              "coef": rr.max_ratio(full.coef_.reshape(ref["coef"].shape), ref["coef"], b["coef"]),          # sklearn drops the axis of a single target
              "fitted": rr.max_ratio(full.predict(Z64).reshape(M.shape), ref["fitted"], b["fitted"])}
    print(f"RATIO sklearn {rr.case_id(case)} " + " ".join(f"{k} {v:.4g}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_bound_constant_follows_its_rule():
    worst = 0.0
    for case in rr.CASES:
        Z, M, ref = reference(case)
        got, b = rr.closed_form_float(Z, M, case[3], np.float64), rr.bounds(ref, M, c=1.0)
        ratios = {k: rr.max_ratio(got[k], ref[k], b[k]) for k in rr.KEYS}
        print(f"RATIO numpy-float64 c=1 {rr.case_id(case)} " + " ".join(f"{k} {v:.4g}" for k, v in ratios.items()))
        worst = max(worst, max(ratios.values()))
    rule = max(1.0, 2.0 ** math.ceil(math.log2(4.0 * worst)))
    print(f"largest ratio {worst:.4g}: c = {rule:g}")
    assert rr.C_BOUND == rule


def test_float32_misses_the_bound_by_orders_of_magnitude():
    case = rr.CASES[1]
    assert case[:3] == (16, 512, 7)
    Z, M, ref = reference(case)
    got, b = rr.closed_form_float(Z, M, case[3], np.float32), rr.bounds(ref, M)
    ratios = {k: rr.max_ratio(got[k], ref[k], b[k]) for k in ("coef", "fitted", "loo", "leverage")}
    print(f"RATIO numpy-float32 {rr.case_id(case)} " + " ".join(f"{k} {v:.4g}" for k, v in ratios.items()))
    assert min(ratios.values()) > 100.0, ratios
    lm = pytest.importorskip("sklearn.linear_model")
    model = lm.Ridge(alpha=case[3], fit_intercept=True).fit(Z, M.astype(np.float32))          # what the reference hands sklearn
    assert model.coef_.dtype == np.float32
    assert rr.max_ratio(model.coef_.reshape(ref["coef"].shape), ref["coef"], b["coef"]) > 100.0


def test_reference_ranking_is_far_from_a_tie():
    for case in rr.CASES:
        _, _, ref = reference(case)
        assert rr.min_adjacent_gap(ref["r2"]) > 1e-6, rr.case_id(case)


def test_refusals_that_need_no_device():
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import fit_translator_ridge
    z, m = torch.zeros(4, 3), torch.zeros(4, 2)
    for args, word in (((torch.zeros(1, 3), torch.zeros(1, 2), 1.0), "at least 2 samples"), ((torch.zeros(4, 0), m, 1.0), "1 <= d <= 1024"),
                       ((torch.zeros(4, 1025), m, 1.0), "1 <= d <= 1024"), ((z, torch.zeros(4, 0), 1.0), "at least one feature"),
                       ((z, torch.zeros(5, 2), 1.0), "Z has 4 rows, M has 5"), ((z, m, 0.0), "alpha must be positive"), ((z, m, -1.0), "alpha must be positive"),
                       ((z, m, float("nan")), "alpha must be positive"), ((z, m, float("inf")), "alpha must be positive"),
                       ((z.to(torch.int32), m, 1.0), "float32 or float64"), ((torch.zeros(4), m, 1.0), r"Z \[N, d\] and M \[N, F\]")):
        with pytest.raises(CvaeError, match=word):
            ops.ridge_fit_loo(*args)
    with pytest.raises(CvaeError, match="no CPU fallback"):          # every argument in order: the device is asked for last
        ops.ridge_fit_loo(z, m, 1.0)
    with pytest.raises(CvaeError, match=r"codes \[N\] and idx"):
        ops.group_means_resampled(z, torch.zeros(3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), 2)
    with pytest.raises(CvaeError, match="integer codes"):
        ops.group_means_resampled(z, torch.zeros(4), torch.zeros(2, 4, dtype=torch.int32), 2)
    with pytest.raises(CvaeError, match="1 <= G"):
        ops.group_means_resampled(z, torch.zeros(4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), 0)
    with pytest.raises(CvaeError, match="no CPU fallback"):
        ops.group_means_resampled(z, torch.zeros(4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), 2)
    with pytest.raises(CvaeError, match="3 entries for 2 feature columns"):
        fit_translator_ridge(z.numpy(), m.numpy(), feature_names=("a", "b", "c"))
    with pytest.raises(CvaeError, match="Z has 4 rows, M has 5"):
        fit_translator_ridge(z.numpy(), np.zeros((5, 2)))


def test_entry_points_refuse_before_any_launch():
    """the C entries' own checks answer with the header's codes without touching a device"""
    from causal_vae_amd._lib import lib
    BADSHAPE, NULLPTR, UNSUPPORTED, WORKSPACE = -1, -6, -3, -4
    p = 1 << 12          # a non-null, 8-byte-aligned value: no check that passes it reaches a launch below
    assert lib.cvae_ridge_gram_f64(p, 3, p, p, 2, p, 1, 3, 2, 1.0, p, p, p, 1 << 20, None) == BADSHAPE           # N < 2
    assert lib.cvae_ridge_gram_f64(p, 3, p, p, 2, p, 4, 1025, 2, 1.0, p, p, p, 1 << 20, None) == BADSHAPE        # d > 1024
    assert lib.cvae_ridge_gram_f64(p, 3, p, p, 2, p, 4, 3, 2, 0.0, p, p, p, 1 << 20, None) == BADSHAPE           # alpha
    assert lib.cvae_ridge_gram_f64(p, 3, p, p, 2, p, 4, 3, 2, float("nan"), p, p, p, 1 << 20, None) == BADSHAPE
    assert lib.cvae_ridge_gram_f64(p, 2, p, p, 2, p, 4, 3, 2, 1.0, p, p, p, 1 << 20, None) == BADSHAPE           # a row stride below the row
    assert lib.cvae_ridge_gram_f64(p, 3, p, None, 2, p, 4, 3, 2, 1.0, p, p, p, 1 << 20, None) == NULLPTR
    assert lib.cvae_ridge_gram_f64(p + 4, 3, p, p, 2, p, 4, 3, 2, 1.0, p, p, p, 1 << 20, None) == UNSUPPORTED
    assert lib.cvae_ridge_gram_f64_workspace_bytes(4, 3, 2) == 3 * 5 * 8 and lib.cvae_ridge_gram_f64_workspace_bytes(300, 130, 3) == 2 * 130 * 133 * 8
    assert lib.cvae_ridge_gram_f64(p, 3, p, p, 2, p, 4, 3, 2, 1.0, p, p, p, 3 * 5 * 8 - 1, None) == WORKSPACE
    assert lib.cvae_chol_f64(p, 0, p, None) == BADSHAPE and lib.cvae_chol_f64(p, 1025, p, None) == BADSHAPE and lib.cvae_chol_f64(p, 4, None, None) == NULLPTR
    assert lib.cvae_trsm_f64(p, 3, p, 5, 1, None, p, 5, 4, 5, 0, None) == BADSHAPE                                 # ldl < d
    assert lib.cvae_trsm_f64(p, 4, p, 5, 1, None, p, 5, 4, 5, 2, None) == UNSUPPORTED                              # the flag is 0 or 1
    assert lib.cvae_trsm_f64(p, 4, p, 1, 5, None, p, 5, 4, 5, 0, None) == UNSUPPORTED                              # in place only element for element
    assert lib.cvae_col_means_f64(p, 0, 3, 3, p, p, 64, None) == BADSHAPE and lib.cvae_col_means_f64(p, 4, 3, 3, p, None, 64, None) == NULLPTR
    assert lib.cvae_ridge_loo_f64(p, 3, p, p, 2, p, p, p, 4, 3, 2, p, p, None, p, p, None) == NULLPTR
    assert lib.cvae_ridge_predict_f64(p, 3, p, p, 0, 3, 2, p, None) == 0 and lib.cvae_ridge_predict_f64(p, 2, p, p, 4, 3, 2, p, None) == BADSHAPE
    assert lib.cvae_ranking_stats_f64(p, 1, p, 2, 4, 2, p, p, None) == BADSHAPE
    assert lib.cvae_group_means_resampled_f64(p, 3, p, p, 4, 3, 2, 0, p, p, None) == 0
    assert lib.cvae_group_means_resampled_f64(p, 3, p, p, 4, 3, 0, 5, p, p, None) == BADSHAPE
    assert lib.cvae_group_means_resampled_f64(p, 3, p + 2, p, 4, 3, 2, 5, p, p, None) == UNSUPPORTED


def test_bootstrap_restatement_on_a_hand_checked_case():
    """Two groups whose members share one latent each: whatever the draw, the group means are (0, 0) and (1, 0), the predicted difference is the first column of
    coef, (3, -1, 0.1), so with top_k = 2 features f0 and f1 are counted once in every bootstrap that drew both groups and f2 never; the other bootstraps
    are skipped.  Which bootstraps those are is read off the draws themselves."""
    groups = np.array(["b", "a", "a", "a"])
    Z = np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    coef, intercept = np.array([[3.0, 5.0], [-1.0, 5.0], [0.1, 5.0]]), np.array([7.0, 8.0, 9.0])
    rng = np.random.RandomState(3)
    both = sum(len(set(groups[rng.randint(0, 4, size=4)])) == 2 for _ in range(12))
    assert 0 < both < 12          # seed 3 draws both kinds
    got = rr.bootstrap(groups, Z, coef, intercept, ["f0", "f1", "f2"], n_boot=12, top_k=2, seed=3)
    assert got["counts"] == {"f0": both, "f1": both, "f2": 0} and got["skipped"] == 12 - both and got["total_slots"] == 2 * both
    assert got["freq"]["f0"] == 0.5 and not got["all_present"]
    assert abs(got["min_margin"] - 0.9) < 1e-12          # (|-1| - |0.1|) / |-1|
    scaled = rr.bootstrap(groups, Z, coef, intercept, ["f0", "f1", "f2"], scale=[0.1, 1.0, 100.0], n_boot=12, top_k=2, seed=3)
    assert scaled["counts"] == {"f0": 0, "f1": both, "f2": both}          # (0.3, -1, 10)


def test_host_side_helpers():
    from causal_vae_amd.vit import compute_group_means, contrast_delta, pairwise_contrasts, topk_features
    arr = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 9.0]])
    groups = np.array(["y", "x", "y", "x"])
    uniq, means = compute_group_means(arr, groups)
    assert uniq == ["y", "x"] and np.array_equal(means, [[3.0, 4.0], [5.0, 6.5]])          # order of first appearance
    ref_uniq, ref_means = rr.group_means(arr, groups)
    assert uniq == ref_uniq and np.array_equal(means, ref_means)
    assert pairwise_contrasts(["a", "b", "c"]) == [("a", "b"), ("a", "c"), ("b", "c")]
    delta = contrast_delta(uniq, means, "y", "x")
    assert delta.dtype == np.float32 and np.array_equal(delta, [2.0, 2.5])
    assert topk_features(np.array([0.5, -3.0, 2.0]), ["a", "b", "c"], k=2) == [("b", -3.0), ("c", 2.0)]
