"""Latent PCA: the reference's PCA(n_components=2).fit_transform(z_all) (mnist_test/01_baseline_causal_vae/visualize.py:164-167, 06_model_experiment/
visualize.py:165-167) on the float64 kernels of csrc/eigh.hip and csrc/ridge.hip: column means, the centred Gram matrix, its symmetric
eigendecomposition, the top components in descending order with sklearn's sign rule, and the projection, all on the device.  latent_pca fits from a matrix;
pca_vit_latents from a model and a loader, the latents never leaving the device."""
import torch

from .. import ops
from .._lib import CvaeError
from .translator import _matrix, _to_device


class LatentPCA:
    """What sklearn's fitted PCA is to the reference, under its names, float64 numpy: mean_ [d], components_ [k, d] (rows in descending order of variance, each
    signed so that its entry of largest |value| is positive, lowest index on a tie: sklearn >= 1.5's svd_flip on V), explained_variance_ [k] = lambda / (N - 1),
    explained_variance_ratio_ [k] = lambda / sum lambda, singular_values_ [k] = sqrt(lambda), n_components_, n_samples_.  transform(Z) = (Z - mean_) components_^T
    on the device in float64: numpy in, numpy out; a tensor in, a tensor (on its device) out."""

    def __init__(self, fit, n_samples, device="cuda"):
        host = {k: v.cpu().numpy() for k, v in fit.items()}
        self.mean_, self.components_ = host["mean"], host["components"]
        self.explained_variance_, self.explained_variance_ratio_ = host["explained_variance"], host["explained_variance_ratio"]
        self.singular_values_ = host["singular_values"]
        self.n_components_, self.n_samples_ = self.components_.shape[0], int(n_samples)
        self.device = device
        self._dev = (fit["mean"], fit["components"])

    def _params(self, device):
        if self._dev[0].device != torch.device(device):
            self._dev = (torch.as_tensor(self.mean_).to(device), torch.as_tensor(self.components_).to(device))
        return self._dev

    def transform(self, Z):
        if torch.is_tensor(Z) and Z.is_cuda:
            return ops.pca_transform_f64(Z, *self._params(Z.device))
        z, was_numpy = _to_device(Z, self.device, "Z")
        out = ops.pca_transform_f64(z, *self._params(z.device))
        return out.cpu().numpy() if was_numpy else out.to(Z.device)


def latent_pca(Z, n_components, device="cuda"):
    """sklearn's PCA(n_components).fit(Z) -> a LatentPCA.  Z [N, d]: a numpy array or a tensor on any device, float32 or float64 (anything else is converted to
    float64).  1 <= n_components <= min(N - 1, d) and d <= 1024, anything else is a CvaeError, raised before the first copy to the device."""
    Zh = _matrix(Z, "Z")[0]
    k = ops.pca_args("latent_pca", Zh, n_components)
    return LatentPCA(ops.pca_fit_f64(Zh.to(device), k), Zh.shape[0], device=device)


@torch.no_grad()
def pca_vit_latents(model, loader, n_components, device):
    """(Z, pca, scores): translate_vit_latents' protocol (eval mode, mu of every batch["x"], the per-batch mu staying on the device) into latent_pca.
    Z [N, latent_dim] float32 numpy, copied to the host once; pca: the LatentPCA; scores [N, n_components] float64 numpy = pca.transform(Z), the reference's
    fit_transform.  model: a ViTVAE or a ViTVAEEncoder."""
    model.eval()
    zs = [model.encode(batch["x"].to(device))[0] for batch in loader]
    if not zs:
        raise CvaeError("pca_vit_latents: the loader gave no batch")
    Zd = torch.cat(zs, dim=0)
    k = ops.pca_args("pca_vit_latents", Zd, n_components)
    pca = LatentPCA(ops.pca_fit_f64(Zd, k), Zd.shape[0], device=device)
    return Zd.cpu().numpy(), pca, pca.transform(Zd).cpu().numpy()
