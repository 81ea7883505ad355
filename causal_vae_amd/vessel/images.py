"""Vessel image preparation on the device: from a stack or a projected image to a model's input without a host step in between.

The reference prepares one image at a time on the host, inside its datasets, and training repeats that for every sample of every epoch:
  prepare_vessel_images       VesselDataset.__getitem__ (vessel_analysis/00_core/dataset.py:192-237): antialiased bilinear resize to 768 x 1280, the four flip
                              variants, per-image min-max, mask = v > mean(v).  The input of CausalVesselVAE / CausalViTVAE.
  prepare_translator_images   ImageTableDataset.__getitem__ (latent_translator/utils.py:18-60, dataset.py:57-70): maximum-intensity projection, percentile
                              clip and scale to [0, 1], plain bilinear resize to 384 x 640.  The input of the latent translator's ViT-VAE.
Both take a tensor [B, Hs, Ws] (projected images) or [B, D, Hs, Ws] (stacks, projected first: ops.mip_max), uint16 or float32, on the host (moved to the
device as it is, before any arithmetic) or on the device, a numpy array of the same kinds, or a list of per-image arrays / tensors [Hs, Ws] or [D, Hs, Ws],
which is grouped by shape and dtype, one pass per group, the output in the list's order.  Reading the files stays on the host (volume_io.read_tiff_stack).
Kernels: csrc/image_prep.hip through ops.mip_max, ops.resize_bilinear_aa, ops.minmax_binarise, ops.percentile_clip_scale, and the existing bilinear
kernel (cvae_upsample_linear_fwd) for the translator's resize.
"""
import numpy as np
import torch

from .. import _lib as L
from .. import ops

__all__ = ["prepare_vessel_images", "prepare_translator_images"]


def _to_device(what, a, device):
    """one array / tensor -> a device tensor of uint16 or float32 (other integer and float kinds are converted to float32 on the device)"""
    if isinstance(a, np.ndarray):
        if a.dtype not in (np.uint16, np.float32):
            if a.dtype.kind not in "uif":
                raise L.CvaeError(f"{what}: uint16 or float32 images expected, got a numpy array of {a.dtype}")
            a = a.astype(np.float32)
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not torch.is_tensor(a):
        raise L.CvaeError(f"{what}: a tensor, a numpy array or a list of them expected, got {type(a).__name__}")
    if a.dtype not in (torch.uint16, torch.float32):
        if a.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise L.CvaeError(f"{what}: uint16 or float32 images expected, got {a.dtype}")
        a = a.to(device).float()
    return a.to(device)


def _stack(items):
    if items[0].dtype == torch.uint16:          # torch moves uint16 but does not compute on it: stack the same bits as int16
        return torch.stack([a.view(torch.int16) for a in items]).view(torch.uint16)
    return torch.stack(items)


def _groups(what, src, device):
    """src -> [(positions in the output, device tensor [b, Hs, Ws] or [b, D, Hs, Ws])], one entry per shape and dtype"""
    if isinstance(src, (list, tuple)):
        if not src:
            raise L.CvaeError(f"{what}: an empty list of images")
        items = [_to_device(what, a, device) for a in src]
        for a in items:
            if a.dim() not in (2, 3):
                raise L.CvaeError(f"{what}: a list holds single images [Hs, Ws] or stacks [D, Hs, Ws], got {tuple(a.shape)}")
        keys = {}
        for i, a in enumerate(items):
            keys.setdefault((tuple(a.shape), a.dtype), []).append(i)
        return [(idx, _stack([items[i] for i in idx])) for idx in keys.values()], len(items)
    a = _to_device(what, src, device)
    if a.dim() not in (3, 4):
        raise L.CvaeError(f"{what}: images [B, Hs, Ws] or stacks [B, D, Hs, Ws] expected, got {tuple(a.shape)}")
    return [(list(range(a.shape[0])), a)], a.shape[0]


def _projected(a):
    """[b, D, Hs, Ws] -> float32 [b, Hs, Ws] by the maximum over D; [b, Hs, Ws] as float32"""
    if a.dim() == 4:
        return ops.mip_max(a)
    return a if a.dtype == torch.float32 else a.float()


def _device(device):
    return torch.device("cuda" if device is None else device)


def prepare_vessel_images(src, size=(768, 1280), augment=False, dtype=torch.float32, return_stats=False, device=None):
    """The reference's VesselDataset transform for a batch: masks [B * A, 1, H, W] of exactly 0 / 1 in `dtype` (float32 or bfloat16), contiguous, on the device.
    augment: A = 4 and source i's variants stand at 4 i + a (a = 0 none, 1 horizontal flip, 2 vertical, 3 both), the reference's dataset index
    real_idx * 4 + aug_mode; the statistics are those of the unflipped image (the reference recomputes them per variant and finds the same extremes).
    return_stats: (masks, [ops.BinariseStats per shape group, with its source positions as .index])."""
    what = "prepare_vessel_images"
    A = 4 if augment else 1
    groups, n = _groups(what, src, _device(device))
    out, stats = None, []
    for idx, a in groups:
        masks, st = ops.minmax_binarise(ops.resize_bilinear_aa(_projected(a), size), augment, dtype)
        st.index = idx
        stats.append(st)
        if len(groups) == 1:
            out = masks
            break
        if out is None:
            out = torch.empty((n * A,) + tuple(masks.shape[1:]), dtype=dtype, device=masks.device)
        pos = (torch.tensor(idx, device=masks.device)[:, None] * A + torch.arange(A, device=masks.device)).flatten()
        out[pos] = masks
    return (out, stats) if return_stats else out


def prepare_translator_images(src, size=(384, 640), clip_percentile=99.5, device=None):
    """The reference's ImageTableDataset transform for a batch: float32 [B, 1, H, W] on the device, each image projected (stacks), clipped to its
    [100 - p, p] percentiles and scaled to [0, 1] in float64 exactly as numpy does it (ops.percentile_clip_scale), then resized with plain bilinear
    interpolation.  An image with a NaN or an infinity raises (the reference would return an all-NaN image); that one look at the flag words happens after
    everything is enqueued."""
    what = "prepare_translator_images"
    H, W = ops._prep_size(what, size)
    groups, n = _groups(what, src, _device(device))
    out, flags = None, []
    for idx, a in groups:
        y = _projected(a)
        b, Hs, Ws = y.shape
        v, st = ops.percentile_clip_scale(y, clip_percentile, check_finite=False)
        flags.append((idx, st.flags))
        r = torch.empty((b, 1, H, W), dtype=torch.float32, device=v.device)
        L.check(L.lib.cvae_upsample_linear_fwd(L.ptr(v), L.ptr(r), b, 1, Hs, Ws, 1, H, W, 1, L.F32, L.stream()), what)
        if len(groups) == 1:
            out = r
            break
        if out is None:
            out = torch.empty((n, 1, H, W), dtype=torch.float32, device=r.device)
        out[torch.tensor(idx, device=r.device)] = r
    for idx, f in flags:
        bad = [idx[i] for i in torch.nonzero(f.cpu() & ops.PREP_NONFINITE).flatten().tolist()]
        if bad:
            raise L.CvaeError(f"{what}: image(s) {bad} hold a NaN or an infinity; the percentiles of such an image are not defined")
    return out
