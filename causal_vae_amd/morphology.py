"""The image side of the reference's MNIST analyses: its 12 morphology features measured on the device.

extract_refined_features (mnist_test/01_baseline_causal_vae/dataset.py:11-99 and its 06_model_experiment twin) is skimage regionprops and scipy's distance
transform on one image at a time on the host.  Here ops.morph_features12 (csrc/morphology.hip) measures a whole batch in one launch, so that what a decode
produced is measured where it lies:
  measure_morphology        [B, H, W] or [B, 1, H, W] -> [B, 12]
  extract_refined_features  the reference's signature: one [1, H, W] image on any device -> float32 [12] on the CPU
  morph_mnist12             MorphMNIST12.__init__'s cache (dataset.py:101-126) from arrays: (x [N, 1, 28, 28] in [0, 1], m [N, 12], t_onehot [N, 10])
  measure_counterfactual    the [B, F, V, 1, H, W] of counterfactual.batched_counterfactual -> [B, F, V, 12]
  measured_sensitivity      03_measurement_approach/analyze_counterfactual.py:38-110: decode every z under every class, measure, std over the classes
  measured_pair_contrast    phase 2 of 04_phase_comparison/analyze_pairwise_importance.py:51-74: mean |features(t_a) - features(t_b)| and its 0-100 scale
Nothing leaves the device before the final small result.  Two deliberate departures from the libraries, both in DESIGN §28: a mask without a background pixel
has a NaN thickness (scipy returns an artefact of its sentinel), and the convex area counts pixel centres on the hull's boundary exactly."""
import numpy as np
import torch

from . import _lib as L
from . import ops
from .mnist_baseline.config import FEATURE_NAMES

FEATURE_NAMES_12 = tuple(FEATURE_NAMES)
__all__ = ["FEATURE_NAMES_12", "measure_morphology", "extract_refined_features", "morph_mnist12", "measure_counterfactual", "measured_sensitivity",
           "measured_pair_contrast"]


def measure_morphology(x, threshold=0.2, norms=ops.MORPH_NORMS, return_raw=False):
    """[B, 12] float32 on x's device (ops.morph_features12)."""
    return ops.morph_features12(x, threshold, norms, return_raw)


def extract_refined_features(img_tensor, device=None):
    """The reference's call: one image [1, H, W] (or [H, W]) on any device -> torch.float32 [12] on the CPU."""
    x = torch.as_tensor(img_tensor)
    if x.dim() < 2 or x.numel() != x.shape[-2] * x.shape[-1]:
        raise L.CvaeError(f"extract_refined_features: one image [1, H, W] expected, got {tuple(x.shape)}")
    if not x.is_cuda:
        x = x.to(device if device is not None else "cuda")
    return ops.morph_features12(x.reshape(1, x.shape[-2], x.shape[-1]))[0].cpu()


def morph_mnist12(images, labels, device, limit_count=None, chunk=16384):
    """(x [N, 1, H, W] float32 in [0, 1], m [N, 12], t_onehot [N, 10]) on `device`: what MorphMNIST12.__init__ caches item by item.  images: [N, H, W] or
    [N, 1, H, W], a numpy array or a tensor; uint8 is divided by 255 (ToTensor), floats are taken as they are.  labels: [N] integers 0 .. 9.  limit_count: only
    the first that many, as there.  M comes from one launch per `chunk` images."""
    x, t = torch.as_tensor(images), torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).long()
    if x.dim() == 3:
        x = x[:, None]
    if x.dim() != 4 or x.shape[1] != 1 or t.dim() != 1 or t.shape[0] != x.shape[0]:
        raise L.CvaeError(f"morph_mnist12: images [N, H, W] or [N, 1, H, W] and labels [N] expected, got {tuple(x.shape)} and {tuple(t.shape)}")
    if limit_count is not None and limit_count < x.shape[0]:
        x, t = x[:limit_count], t[:limit_count]
    if t.numel() and (int(t.min()) < 0 or int(t.max()) > 9):
        raise L.CvaeError("morph_mnist12: labels 0 .. 9 expected")
    x = x.to(device)
    if x.dtype == torch.uint8:          # ToTensor's v / 255 from a table divided on the host: a device kernel may multiply by 1 / 255 instead, which is not the same float
        x = (torch.arange(256, dtype=torch.float32) / 255).to(device)[x.long()]
    x = x.float()
    m = torch.cat([ops.morph_features12(x[i:i + chunk]) for i in range(0, x.shape[0], chunk)])
    return x, m, torch.nn.functional.one_hot(t.to(device), 10).float()


def measure_counterfactual(images, threshold=0.2, norms=ops.MORPH_NORMS):
    """[B, F, V, 12]: the features of every image of a sweep [B, F, V, 1, H, W] (counterfactual.batched_counterfactual's result), rows in its order."""
    if not torch.is_tensor(images) or images.dim() != 6 or images.shape[3] != 1:
        got = tuple(images.shape) if torch.is_tensor(images) else type(images).__name__
        raise L.CvaeError(f"measure_counterfactual: a sweep [B, F, V, 1, H, W] expected, got {got}")
    B, F, V = images.shape[:3]
    return ops.morph_features12(images.reshape(B * F * V, *images.shape[-2:]), threshold, norms).view(B, F, V, 12)


def _one_hot_rows(t_idx, n, t_dim, like):
    t = like.new_zeros(n, t_dim)
    t[:, t_idx] = 1.0
    return t


def _decode_morph(model, m_hat, z):
    if hasattr(model, "decode"):
        return model.decode(m_hat, z)
    return model.dec_conv(model.dec_fc(ops.cat([m_hat, z])).view(-1, 64, 7, 7))          # analyze_counterfactual.py:57-68; the Gaussian variant has no decode()


def _decode_class(model, z, t_idx, t_dim):
    """the images of every row of z under class t_idx: through morph_predictor where the model has one, through decode(z, t) otherwise (ConditionalVAE)"""
    t = _one_hot_rows(t_idx, z.shape[0], t_dim, z)
    if hasattr(model, "morph_predictor"):
        return _decode_morph(model, model.morph_predictor(t), z)
    return model.decode(z, t)


def _ranking(values, key):
    vals = [float(v) for v in values]
    order = sorted(range(len(vals)), key=lambda i: (vals[i] != vals[i], -vals[i] if vals[i] == vals[i] else 0.0))          # descending, NaN last (as pandas sorts)
    return [{"feature": FEATURE_NAMES_12[i], key: vals[i]} for i in order]


@torch.no_grad()
def measured_sensitivity(model, z, t_dim=10, threshold=0.2, norms=ops.MORPH_NORMS, keep_images=False):
    """analyze_counterfactual.py:38-110 for the samples z [N, Z]: for every class t, m_hat = morph_predictor(onehot t), decode every z with it, measure the
    images.  Returns {"measured" [N, t_dim, 12] float32, "std_per_sample" [N, 12] float64 (the population standard deviation over the classes),
    "sensitivity" [12] float64 (its mean over the samples), all on the device, and "ranking": [{"feature", "sensitivity"}] sorted as the reference's DataFrame};
    keep_images adds "images" [N, t_dim, 1, H, W], what was measured."""
    L.require_gpu(z)
    images = [_decode_class(model, z, t, t_dim) for t in range(t_dim)]
    measured = torch.stack([ops.morph_features12(im, threshold, norms) for im in images], dim=1)
    std = measured.double().std(dim=1, unbiased=False)
    sens = std.mean(dim=0)
    out = {"measured": measured, "std_per_sample": std, "sensitivity": sens, "ranking": _ranking(sens.cpu().tolist(), "sensitivity")}
    if keep_images:
        out["images"] = torch.stack(images, dim=1)
    return out


@torch.no_grad()
def measured_pair_contrast(model, z, t_a, t_b, t_dim=10, threshold=0.2, norms=ops.MORPH_NORMS, keep_images=False):
    """Phase 2 of analyze_pairwise_importance.py:51-74: decode every z [N, Z] under class t_a and under class t_b (CausalMorphVAE12 and its Gaussian variant
    through morph_predictor, ConditionalVAE through its decode(z, t)), measure both.  Returns {"diff" [12] float64 = mean |feat_a - feat_b| over the samples,
    "normalized" [12] = diff / (max diff + 1e-9) * 100 (the max skips NaN), on the device, and "ranking": [{"feature", "importance"}] by the normalised value}; keep_images adds "images_a", "images_b" [N, 1, H, W]."""
    L.require_gpu(z)
    xa, xb = _decode_class(model, z, t_a, t_dim), _decode_class(model, z, t_b, t_dim)
    fa, fb = ops.morph_features12(xa, threshold, norms), ops.morph_features12(xb, threshold, norms)
    diff = (fa - fb).abs().double().mean(dim=0)
    top = torch.where(diff.isnan(), torch.full_like(diff, -float("inf")), diff).max()
    norm = diff / (top + 1e-9) * 100
    out = {"diff": diff, "normalized": norm, "ranking": _ranking(norm.cpu().tolist(), "importance")}
    if keep_images:
        out["images_a"], out["images_b"] = xa, xb
    return out
