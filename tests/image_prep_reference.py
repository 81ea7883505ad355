"""Float64 references of csrc/image_prep.hip in numpy and torch on the CPU, shared by tests/test_image_prep_cpu.py and tests/test_image_prep.py.

  aa_matrix(n_in, n_out)        torch's antialiased bilinear weights of one axis as a dense float64 matrix [n_out, n_in] and the tap count of every output:
                                scale = n_in / n_out, support = max(scale, 1), c = scale (i + 1/2), taps max(0, int(c - support + 1/2)) .. min(int(c + support
                                + 1/2), n_in), w_j = max(0, 1 - |(j - c + 1/2) / support|) over their sum
  resize_aa(x, size)            (ref, err): Wh x Ww^T and the bound 4 2^-24 (sqrt Kw + sqrt Kh) (|Wh| |x| |Ww|^T) by the rule of oracle/conv64.py (C sqrt(K) U sum
                                |terms| per product-sum, K the real tap counts; the two passes add)
  binarise(y)                   the tail of VesselDataset.__getitem__ on given float32 input: v in float32 (two operations), the EXACT mean (math.fsum), the mask,
                                and how far the nearest v lies from the mean in units of the float64 summation bound n 2^-53 thr
  vessel_pipeline(x, size)      the whole transform A in float64 with the exclusion band tau of every pixel
  normalize(arr, p)             normalize_image (np.percentile itself, clip and division in float64, one rounding); translator(arr, size, p) adds F.interpolate
Inputs are made here, seeded: images(...) = rand^6 3000 + 100 with bright strokes (dim background, few bright vessels: the distribution of a projected stack).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
C = 4.0
# (Hs, Ws, H, W): a plain downscale, one with taps that straddle tiles, an upscale, equal sizes (a copy), ratio 32 along H (a row window wider than any
# tile), many tiles
RESIZE_CASES = [(75, 131, 32, 64), (37, 53, 32, 32), (20, 30, 32, 64), (32, 64, 32, 64), (257, 40, 8, 32), (200, 333, 96, 160)]
RESIZE_BATCHES = (1, 3)
MAX_EXCLUDED_PER_IMAGE, MAX_EXCLUDED_OVERALL = 0.005, 0.0002


def case_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}x{c[3]}"


def images(B, Hs, Ws, seed):
    """float32 [B, Hs, Ws]: rand^6 * 3000 + 100 and a few bright strokes"""
    g = np.random.default_rng(seed)
    x = g.random((B, Hs, Ws)) ** 6 * 3000.0 + 100.0
    for b in range(B):
        for _ in range(3):
            r0, c0 = g.integers(0, Hs), g.integers(0, Ws)
            dr, dc = g.uniform(-1, 1), g.uniform(-1, 1)
            for s in range(max(Hs, Ws)):
                r, c = int(round(r0 + s * dr)), int(round(c0 + s * dc))
                if not (0 <= r < Hs and 0 <= c < Ws):
                    break
                x[b, r, c] = 3500.0 + 500.0 * g.random()
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ antialiased resize
def aa_window(i, n_in, n_out):
    scale = n_in / n_out
    support = max(scale, 1.0)
    c = scale * (i + 0.5)
    return max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)


def aa_matrix(n_in, n_out):
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / support
    Wm = np.zeros((n_out, n_in), dtype=np.float64)
    K = np.zeros(n_out, dtype=np.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = aa_window(i, n_in, n_out)
        w = np.array([max(0.0, 1.0 - abs((j - c + 0.5) * inv)) for j in range(lo, hi)], dtype=np.float64)
        Wm[i, lo:hi] = w / w.sum()
        K[i] = hi - lo
    return Wm, K


def resize_aa(x, size):
    """x [B, Hs, Ws] (any float) -> (ref, err) float64 [B, H, W]"""
    x = np.asarray(x, dtype=np.float64)
    H, W = size
    Wh, Kh = aa_matrix(x.shape[1], H)
    Ww, Kw = aa_matrix(x.shape[2], W)
    ref = np.einsum("ij,bjk,lk->bil", Wh, x, Ww)
    mag = np.einsum("ij,bjk,lk->bil", np.abs(Wh), np.abs(x), np.abs(Ww))
    err = C * U * (np.sqrt(Kw)[None, None, :] + np.sqrt(Kh)[None, :, None]) * mag
    return ref, err


def torch_resize_aa(x, size, dtype=np.float32):
    """torch's own CPU operator in float32 (what the reference runs) or float64 (the same operator with its weights formed in float64)"""
    return F.interpolate(torch.from_numpy(np.asarray(x, dtype=dtype))[:, None], size=tuple(size), mode="bilinear", antialias=True, align_corners=False)[:, 0].numpy()


def max_ratio(got, ref, err):
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, d / np.maximum(err, 1e-300), np.where(d > 0, np.inf, 0.0))
    return float(r.max())


# ------------------------------------------------------------------------------------------------ min-max and the mean threshold
def flip_variant(mask, a):
    """variant a of [..., H, W]: 1 flips W, 2 flips H, 3 both (the dataset's aug_mode)"""
    if a & 1:
        mask = mask[..., :, ::-1]
    if a & 2:
        mask = mask[..., ::-1, :]
    return mask


def binarise(y):
    """y float32 [H, W] -> dict(mn, mx, v float32, thr = exact mean of v as a float, mask bool, ones, clearance): clearance = min |v - thr| / (n 2^-53 thr), which has to
    be above 1 for a float64 sum in any order to decide every pixel as the exact mean does.  A constant image: zeros, thr 0."""
    y = np.asarray(y, dtype=np.float32)
    mn, mx = y.min(), y.max()
    if not mx > mn:
        return dict(mn=mn, mx=mx, v=np.zeros_like(y), thr=0.0, mask=np.zeros(y.shape, dtype=bool), ones=0, clearance=math.inf)
    v = (y - mn) / np.float32(mx - mn)
    assert v.dtype == np.float32
    thr = math.fsum(v.ravel().tolist()) / v.size
    v64 = v.astype(np.float64)
    mask = v64 > thr
    clearance = float(np.abs(v64 - thr).min() / (v.size * 2.0 ** -53 * thr))
    return dict(mn=mn, mx=mx, v=v, thr=thr, mask=mask, ones=int(mask.sum()), clearance=clearance)


# (B, H, W), seed of the binarise test: a width that is no multiple of 4 on one chunk, the vector path on one chunk, several chunks on each path
BINARISE_CASES = [((3, 37, 53), 31), ((2, 32, 64), 32), ((2, 96, 160), 33), ((3, 75, 131), 34)]


def binarise_inputs(shape, seed):
    """float32 [B, H, W] for the binarise test: resized-looking images (smooth values, no ties with the mean).  test_image_prep_cpu.py holds every one of them
    clear of the mean."""
    B, H, W = shape
    return torch_resize_aa(images(B, 2 * H + 3, 2 * W + 5, seed), (H, W))


def vessel_pipeline(x, size):
    """transform A in float64 for x [B, Hs, Ws]: dict(mask bool [B, H, W], v, thr [B], tau [B, H, W]).  tau: the resize bound e pushed through v = (r - mn) / (mx - mn):
    the pixel's own e plus mn's and mx's (twice the image's largest) over the range, 4 U for the two float32 operations, and the mean of the same for the threshold."""
    r, e = resize_aa(x, size)
    mn, mx = r.min(axis=(1, 2), keepdims=True), r.max(axis=(1, 2), keepdims=True)
    rng = mx - mn
    v = (r - mn) / rng
    thr = v.mean(axis=(1, 2), keepdims=True)
    tv = (e + 2.0 * e.max(axis=(1, 2), keepdims=True)) / rng + C * U
    tau = tv + tv.mean(axis=(1, 2), keepdims=True)
    return dict(mask=v > thr, v=v, thr=thr[:, 0, 0], tau=tau, band=np.abs(v - thr) <= tau)


def torch_vessel_pipeline(x, size):
    """the reference's own float32 sequence on the CPU (VesselDataset.__getitem__ without the flips), bool [B, H, W]"""
    out = []
    for img in torch.from_numpy(np.asarray(x, dtype=np.float32)):
        t = F.interpolate(img[None, None], size=tuple(size), mode="bilinear", antialias=True, align_corners=False)[0]
        t = (t - t.min()) / (t.max() - t.min()) if t.max() > t.min() else torch.zeros_like(t)
        out.append((t > t.mean())[0].numpy())
    return np.stack(out)


def band_check(mask, ref):
    """(excluded share of the worst image, excluded share overall, mismatches outside the band) of mask bool [B, H, W] against vessel_pipeline's dict"""
    band = ref["band"]
    wrong = (np.asarray(mask, dtype=bool) != ref["mask"]) & ~band
    per_image = band.reshape(band.shape[0], -1).mean(axis=1)
    return float(per_image.max()), int(band.sum()), band.size, int(wrong.sum())


# ------------------------------------------------------------------------------------------------ percentile clip and scale
def normalize(arr, p=99.5):
    """normalize_image on a float32 array of any shape -> (float32 result, vmin, vmax): the percentiles are float64 scalars, so the clip and the division run in
    float64 and the result is rounded once"""
    arr = np.asarray(arr, dtype=np.float32)
    vmin, vmax = np.percentile(arr, [100 - p, p])
    assert vmin.dtype == np.float64
    c = np.clip(arr, vmin, vmax)
    denom = vmax - vmin
    if denom == 0:
        denom = 1e-5
    out = (c - vmin) / denom
    assert out.dtype == np.float64
    return out.astype(np.float32), float(vmin), float(vmax)


def translator(arr, size, p=99.5):
    """transform B for one image or stack: float32 [1, H, W] by torch's CPU bilinear, and the normalised source it was resized from"""
    arr = np.asarray(arr)
    if arr.ndim == 3:
        arr = np.max(arr, axis=0)
    v, _, _ = normalize(arr.astype(np.float32), p)
    t = F.interpolate(torch.from_numpy(v)[None, None], size=tuple(size), mode="bilinear", align_corners=False)[0]
    return t.numpy(), v


def percentile_inputs(kind, n, seed):
    """float32 [n]: 'ties' integer-valued with few distinct values, 'equal' one value, 'signed' both signs and both zeros, 'smooth' distinct values"""
    g = np.random.default_rng(seed)
    if kind == "ties":
        return g.integers(0, 7, n).astype(np.float32) * 100.0
    if kind == "equal":
        return np.full(n, 417.0, dtype=np.float32)
    if kind == "signed":
        x = g.standard_normal(n).astype(np.float32) * 50.0
        x[g.random(n) < 0.2] = 0.0
        x[g.random(n) < 0.2] = -0.0
        return x
    return (g.random(n) ** 6 * 3000.0 + 100.0).astype(np.float32)
