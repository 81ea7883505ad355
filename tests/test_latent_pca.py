"""The latent PCA on the device (causal_vae_amd.vit.latent_pca / pca_vit_latents; cvae_eigh_f64, cvae_centered_gram_f64, cvae_pca_components_f64 and
cvae_centered_matmul_f64) against tests/latent_pca_reference.py: PCA in numpy.longdouble on the smaller of Xc^T Xc and Xc Xc^T, and the
Davis-Kahan bounds derived there with c = C_PCA = 1 (tests/test_latent_pca_cpu.py shows where it comes from and that the inputs have clear gaps and signs).

Cases (N, d, k): (16, 512, 4) the reference's regime, N < d, rank 15; (97, 64, 3) ragged against every tile; (300, 130, 5) d ragged, N over one 256-row chunk.
  fit          mean_, components_ (signs included), explained_variance_, explained_variance_ratio_, singular_values_ and transform(Z) within their bounds;
               the ratios sum below 1; transform(Z) has column means within the bound of 0
  forms        numpy in numpy out, a device tensor in a device tensor out, a CPU tensor in a CPU tensor out, float32 and float64 inputs, a second run: equal bits
  new rows     transform of rows the fit has not seen, against the wide projection
  from a model pca_vit_latents on a ViTVAEEncoder at 64 x 96: Z is extract_vit_latents' bits, the rest latent_pca(Z)'s

Measured on the MI355X with c = 1 (the RATIO lines of the run):
  N16-d512-k4     mean 0       components 0.0579 explained_variance 0.141  explained_variance_ratio 0.0168  singular_values 0.142  scores 0.209
  N97-d64-k3      mean 0.00521 components 0.0962 explained_variance 0.0499 explained_variance_ratio 0.00723 singular_values 0.0537 scores 0.187
  N300-d130-k5    mean 0.00172 components 0.121  explained_variance 0.0164 explained_variance_ratio 0.00646 singular_values 0.0145 scores 0.218
  transform of new rows, N97-d64-k3: 0.119
No ratio is above 0.22."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import latent_pca_reference as pr  # noqa: E402
from ridge_translator_reference import max_ratio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_FIT = {}


def fitted(case):
    """latent_pca of a case on the device and its transform of the training rows, once"""
    if case not in _FIT:
        from causal_vae_amd.vit import latent_pca
        Z, _ = pr.wide(case)
        pca = latent_pca(Z, case[2], device=DEV)
        _FIT[case] = (pca, pca.transform(Z))
    return _FIT[case]


def outputs(pca, scores):
    return {"mean": pca.mean_, "components": pca.components_, "explained_variance": pca.explained_variance_,
            "explained_variance_ratio": pca.explained_variance_ratio_, "singular_values": pca.singular_values_, "scores": scores}


@pytest.mark.parametrize("case", pr.CASES, ids=pr.case_id)
def test_fit_against_the_wide_reference(case):
    N, d, k = case
    Z, ref = pr.wide(case)
    pca, scores = fitted(case)
    assert pca.mean_.shape == (d,) and pca.components_.shape == (k, d) and pca.explained_variance_.shape == (k,) and scores.shape == (N, k)
    assert all(v.dtype == np.float64 for v in outputs(pca, scores).values()) and pca.n_components_ == k and pca.n_samples_ == N
    assert (ref["rel_gap"] > 1e-3).all() and (ref["sign_lead"] > 1e-6).all()          # on the reference alone
    b = pr.bounds(case, ref)
    r = pr.ratios(outputs(pca, scores), ref, b)
    print(f"RATIO pca {pr.case_id(case)} " + " ".join(f"{key} {v:.3g}" for key, v in r.items()))
    for key, v in r.items():
        assert v <= 1.0, (pr.case_id(case), key, v)
    assert float(pca.explained_variance_ratio_.sum()) < 1.0 and (np.diff(pca.explained_variance_) < 0).all()
    lead = np.argmax(np.abs(pca.components_), axis=1)
    assert (pca.components_[np.arange(k), lead] > 0).all()
    assert (np.abs(scores.mean(axis=0)) <= b["scores"].max(axis=0)).all()


@pytest.mark.parametrize("case", [pr.CASES[0], pr.CASES[2]], ids=pr.case_id)
def test_input_forms_and_runs_give_equal_bits(case):
    from causal_vae_amd.vit import latent_pca
    Z, _ = pr.wide(case)
    pca, scores = fitted(case)
    for label, z in {"float64 numpy": Z.astype(np.float64), "a device tensor": torch.as_tensor(Z).to(DEV), "float32 numpy again": Z}.items():
        again = latent_pca(z, case[2], device=DEV)
        for key, v in outputs(again, again.transform(Z)).items():
            assert np.array_equal(v, outputs(pca, scores)[key]), (label, key)
    on_dev = pca.transform(torch.as_tensor(Z).to(DEV))
    assert torch.is_tensor(on_dev) and on_dev.is_cuda and on_dev.dtype == torch.float64 and np.array_equal(on_dev.cpu().numpy(), scores)
    on_cpu = pca.transform(torch.as_tensor(Z.astype(np.float64)))
    assert torch.is_tensor(on_cpu) and not on_cpu.is_cuda and np.array_equal(on_cpu.numpy(), scores)


def test_transform_of_new_rows():
    case = pr.CASES[1]
    Z, ref = pr.wide(case)
    pca, _ = fitted(case)
    Znew = (Z[:9] * 1.5 + 0.25).astype(np.float32)
    xc = Znew.astype(pr.WIDE) - ref["mean"]
    want = xc @ ref["components"].T
    norm = np.sqrt((xc.astype(np.float64) ** 2).sum(axis=1))
    b = pr.bounds(case, ref)
    bound = (b["components"].reshape(1, -1) + pr.C_PCA * sum(case[:2]) * pr.U) * norm[:, None] + np.sqrt(case[1]) * b["mean"].max()
    ratio = max_ratio(pca.transform(Znew), want, bound)
    print(f"RATIO pca transform-new {pr.case_id(case)} {ratio:.3g}")
    assert ratio <= 1.0


def test_pca_vit_latents_is_extract_then_pca():
    from causal_vae_amd.vit import ViTVAEEncoder, extract_vit_latents, latent_pca, pca_vit_latents
    torch.manual_seed(3)
    model = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=16).to(DEV).eval()
    loader = [{"x": torch.randn(2, 1, 64, 96)} for _ in range(3)]
    Z, pca, scores = pca_vit_latents(model, loader, 2, DEV)
    assert Z.dtype == np.float32 and Z.shape == (6, 16) and np.array_equal(Z, extract_vit_latents(model, loader, DEV))
    again = latent_pca(Z, 2, device=DEV)
    for key, v in outputs(again, again.transform(Z)).items():
        assert np.array_equal(v, outputs(pca, scores)[key]), key
    assert scores.shape == (6, 2) and scores.dtype == np.float64
