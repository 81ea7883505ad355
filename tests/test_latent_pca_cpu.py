"""What the latent PCA's tests (causal_vae_amd.vit.latent_pca) rest on, checked without a GPU on tests/latent_pca_reference.py:
  the inputs    on the wide reference alone: every kept component's relative eigengap is above 1e-3 and its sign-deciding entry leads the runner-up by more
                than 1e-6, so neither an order nor a sign is a coin toss
  the constant  C_PCA follows the rule from the ratios the same algebra in float64 numpy reaches with c = 1
  sklearn       sklearn.decomposition.PCA(k, svd_solver="full") on float64 inputs agrees within the bounds, signs included, where sklearn imports
  refusals      k = 0, k > min(N - 1, d), d > 1024 and a non-integer k are CvaeErrors raised without a device

Measured here with c = 1 (the RATIO lines; mean, components, explained_variance, explained_variance_ratio, singular_values, scores):
  N16-d512-k4     0 0.0045 0.0049 0.017 0.0022 0.0029
  N97-d64-k3      0.0052 0.011 0.0088 0.0073 0.011 0.012
  N300-d130-k5    0.0017 0.0055 0.0047 0.0014 0.0043 0.0098
The largest is 0.017 (the form (N + d) 2^-53 lambda_1 is a generous one for LAPACK): four times that is below 1, so C_PCA = 1."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import latent_pca_reference as pr  # noqa: E402


@pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)
def test_the_inputs_have_clear_gaps_and_signs(case):
    Z, ref = pr.wide(case)
    print(f"PCA {pr.case_id(case)} lambda {ref['lambda'][:case[2] + 1].astype(np.float64)} rel_gap {ref['rel_gap']} sign_lead {ref['sign_lead']}")
    assert (ref["rel_gap"] > 1e-3).all() and (ref["sign_lead"] > 1e-6).all()
    assert float(ref["explained_variance_ratio"].sum()) < 1.0
    comps = ref["components"].astype(np.float64)
    assert np.abs(comps @ comps.T - np.eye(case[2])).max() < 1e-15          # the dual route's v = Xc^T u / sqrt(lambda) are orthonormal


def test_bound_constant_follows_its_rule():
    worst = 0.0
    for case in pr.CASES:
        Z, ref = pr.wide(case)
        r = pr.ratios(pr.pca_float(Z, case[2]), ref, pr.bounds(case, ref, c=1.0))
        print(f"RATIO numpy-float64 c=1 {pr.case_id(case)} " + " ".join(f"{k} {v:.2g}" for k, v in r.items()))
        worst = max(worst, max(r.values()))
    rule = max(1.0, 2.0 ** math.ceil(math.log2(4.0 * worst)))
    print(f"largest ratio {worst:.4g}: c = {rule:g}")
    assert pr.C_PCA == rule


@pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)
def test_sklearn_pca_agrees(case):
    dec = pytest.importorskip("sklearn.decomposition")
    Z, ref = pr.wide(case)
    model = dec.PCA(n_components=case[2], svd_solver="full").fit(Z.astype(np.float64))
    got = {"mean": model.mean_, "components": pr.flip(model.components_), "explained_variance": model.explained_variance_,
           "explained_variance_ratio": model.explained_variance_ratio_, "singular_values": model.singular_values_}
    got["scores"] = (Z.astype(np.float64) - got["mean"]) @ got["components"].T
    r = pr.ratios(got, ref, pr.bounds(case, ref, c=4.0 * pr.C_PCA))          # another algorithm (an SVD of Xc): the rule's factor of four on top
    print(f"RATIO sklearn {pr.case_id(case)} " + " ".join(f"{k} {v:.2g}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


def test_refusals_need_no_device():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import latent_pca
    Z = np.zeros((6, 4), dtype=np.float32)
    for k in (0, -1, 5, 6, 1.5):          # min(N - 1, d) = 4
        with pytest.raises(CvaeError, match=r"1 <= n_components <= min\(N - 1, d\) = 4"):
            latent_pca(Z, k)
    with pytest.raises(CvaeError, match=r"1 <= n_components <= min\(N - 1, d\) = 2"):
        latent_pca(np.zeros((3, 8)), 3)
    with pytest.raises(CvaeError, match="1 <= d <= 1024"):
        latent_pca(np.zeros((6, 1025)), 2)
    with pytest.raises(CvaeError, match="must be a matrix"):
        latent_pca(np.zeros(6), 1)
    with pytest.raises(CvaeError, match="MI355X only"):          # everything in order: the CPU tensor itself is refused, there is no fallback
        latent_pca(torch.zeros(6, 4), 2, device="cpu")
