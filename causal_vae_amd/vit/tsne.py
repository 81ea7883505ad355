"""Latent t-SNE: the reference's sklearn.manifold.TSNE calls (mnist_test/01_baseline_causal_vae/visualize.py:125, :172, :179 and :256, and their
06_model_experiment twins) as the exact O(N^2) method in float64 on the kernels of csrc/tsne.hip: squared distances, the perplexity search,
the joint affinities and the gradient descent of TSNE._tsne, all on the device.  latent_tsne embeds a matrix; tsne_vit_latents a model's latents, which never
leave the device."""
import numpy as np
import torch

from .. import ops
from .._lib import CvaeError

PCA_INIT_STD = 1e-4          # sklearn >= 1.2 scales the PCA start so that its first column has this standard deviation


class LatentTSNE:
    """What sklearn's fitted TSNE is to the reference, under its names: embedding_ [N, 2] (float64 numpy), kl_divergence_ (of the joint affinities from the
    embedding's Q, at the returned embedding), n_iter_ (the index of the last iteration run), learning_rate_; stop_reason_ says why the descent ended; with
    keep_affinities also affinities_ [N, N] and betas_ [N] (float64 numpy)."""

    def __init__(self, fit, learning_rate, affinities=None, betas=None):
        self.embedding_ = fit.Y.cpu().numpy()
        self.kl_divergence_, self.n_iter_, self.learning_rate_ = fit.kl, fit.n_iter, learning_rate
        self.stop_reason_ = ops.TSNE_STOP_REASONS[fit.reason]
        self.n_checks_ = fit.checks
        self.affinities_, self.betas_ = affinities, betas


def _as_tensor(a):
    return a.detach() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def _pca_start(Zd):
    """sklearn's init="pca": the first two principal components' scores, scaled so that the first column's population standard deviation is 1e-4"""
    fit = ops.pca_fit_f64(Zd, 2)
    scores = ops.pca_transform_f64(Zd, fit["mean"], fit["components"])
    return scores / scores[:, 0].std(unbiased=False) * PCA_INIT_STD


def _fit(what, X, N, lr, device, perplexity, early_exaggeration, max_iter, n_iter_without_progress, min_grad_norm, init, random_state, tol, distances,
         keep_affinities):
    """X on the device: the latents, or with distances the squared distances"""
    D = X.to(torch.float64).contiguous() if distances else ops.tsne_sqdist_f64(X)
    P, _pc, beta, _steps = ops.tsne_affinities_f64(D, perplexity, tol)
    if isinstance(init, str):
        if init == "pca":
            Y0 = _pca_start(X)
        else:
            Y0 = torch.as_tensor(1e-4 * np.random.RandomState(random_state).standard_normal((N, 2)).astype(np.float32)).to(device=device, dtype=torch.float64)
    else:
        Y0 = _as_tensor(init).to(device=device, dtype=torch.float64)
    fit = ops.tsne_fit_f64(P, Y0.contiguous(), early_exaggeration, lr, max_iter, n_iter_without_progress, min_grad_norm)
    return LatentTSNE(fit, lr, P.cpu().numpy() if keep_affinities else None, beta.cpu().numpy() if keep_affinities else None)


def latent_tsne(Z, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7, init="pca",
                random_state=None, tol=1e-5, distances=None, device="cuda", n_components=2, keep_affinities=False):
    """sklearn's TSNE(method="exact", ...).fit(Z) -> a LatentTSNE.  Z [N, d]: a numpy array or a tensor on any device, float32 or float64, 3 <= N <= 4096; or
    Z = None and distances [N, N], squared distances computed elsewhere (init="pca" is refused then, as in sklearn).  init: "pca" (through latent_pca's
    kernels, with its limits), "random" (sklearn's own draw from numpy.random.RandomState(random_state), made on the host) or an array [N, 2], used as given.
    tol is the perplexity search's tolerance on the entropy.  Every refusal (ops.tsne_args) comes before the first copy to the device; a CPU device is
    refused, there is no fallback."""
    what = "latent_tsne"
    use_d = distances is not None
    if use_d and Z is not None:
        raise CvaeError(f"{what}: give Z or distances, not both")
    X = _as_tensor(distances if use_d else Z)
    N, lr = ops.tsne_args(what, X, perplexity, n_components, early_exaggeration, learning_rate, max_iter, init, tol, n_iter_without_progress, distances=use_d)
    if isinstance(init, str) and init == "pca":
        ops.pca_args(what, X, 2)          # latent_pca's limits, with their messages
    return _fit(what, X.to(device), N, lr, device, perplexity, early_exaggeration, max_iter, n_iter_without_progress, min_grad_norm, init, random_state, tol,
                use_d, keep_affinities)


@torch.no_grad()
def tsne_vit_latents(model, loader, device, **kw):
    """(Z, tsne): pca_vit_latents' protocol (eval mode, mu of every batch["x"], the per-batch mu staying on the device) into latent_tsne.  Z [N, latent_dim]
    float32 numpy, copied to the host once; tsne: the LatentTSNE.  model: a ViTVAE or a ViTVAEEncoder; kw: latent_tsne's keywords."""
    what = "tsne_vit_latents"
    if kw.get("distances") is not None:
        raise CvaeError(f"{what}: the distances come from the model's latents; distances= is latent_tsne's")
    model.eval()
    zs = [model.encode(batch["x"].to(device))[0] for batch in loader]
    if not zs:
        raise CvaeError(f"{what}: the loader gave no batch")
    Zd = torch.cat(zs, dim=0)
    a = dict(perplexity=30.0, n_components=2, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, init="pca", tol=1e-5, n_iter_without_progress=300)
    a.update({k: v for k, v in kw.items() if k in a})
    N, lr = ops.tsne_args(what, Zd, **a)
    if isinstance(a["init"], str) and a["init"] == "pca":
        ops.pca_args(what, Zd, 2)
    tsne = _fit(what, Zd, N, lr, device, a["perplexity"], a["early_exaggeration"], a["max_iter"], a["n_iter_without_progress"], kw.get("min_grad_norm", 1e-7),
                a["init"], kw.get("random_state"), a["tol"], False, kw.get("keep_affinities", False))
    return Zd.cpu().numpy(), tsne
