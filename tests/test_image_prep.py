"""csrc/image_prep.hip and causal_vae_amd.vessel.images on the MI355X against the references of tests/image_prep_reference.py (the references
themselves are held to torch and numpy in tests/test_image_prep_cpu.py).
  MIP         bit for bit np.max (a NaN for a NaN): uint16 and float32, D = 1, 2, 7, a planted NaN, pixel counts that are and are not multiples of the 8-pixel vector.
  resize      within 4 2^-24 (sqrt Kw + sqrt Kh) (|Wh| |x| |Ww|^T) of the float64 restatement on the case list (`RATIO resize_aa` is printed), B = 1 and 3; equal
              sizes copy the bits; two runs give the same bits, and an image's bits do not depend on the batch around it.
  binarise    on given float32 input: the mask of the exact mean (math.fsum), no pixel excused (the inputs are clear of the mean: the CPU file), count, extremes,
              the four flips, float32 and bfloat16 alike, a constant image and a NaN with their flags.
  percentile  outputs, vmin and vmax equal to numpy's (==) at N = 1, 2, 200, 50 x 70 and 300 x 500, ties, all-equal, both signs and both zeros, p = 99.5 and 90; an
              infinity raises.
  end to end  prepare_vessel_images (augment) against the float64 pipeline outside the exclusion band, the band's share limited; prepare_translator_images within
              the existing bilinear kernel's bound on the same normalised input; the masks feed CausalViTVAE.forward.
Measured on the MI355X: see DESIGN §30."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_prep_reference as ipr  # noqa: E402
from causal_vae_amd import ops, prepare_translator_images, prepare_vessel_images  # noqa: E402
from causal_vae_amd._lib import CvaeError  # noqa: E402
from oracle import plumbing64 as p64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want):
    """bit-exact, a NaN for a NaN"""
    return np.array_equal(got, want, equal_nan=True)


# ------------------------------------------------------------------------------------------------ MIP
@pytest.mark.parametrize("hw", [(48, 50), (37, 53)], ids=["vector", "odd"])
@pytest.mark.parametrize("D", [1, 2, 7])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_mip_max(dtype, D, hw):
    g = np.random.default_rng(D)
    x = (g.random((2, D, *hw)) ** 6 * 60000).astype(dtype)
    if dtype == np.float32:
        x -= 20000.0
        x[1, D // 2, 5, 7] = np.nan
        x[0, 0, 0, 0] = np.nan
        x[0, D - 1, hw[0] - 1, hw[1] - 1] = np.nan
    got = ops.mip_max(dev(x)).cpu().numpy()
    want = np.stack([np.max(s, axis=0) for s in x]).astype(np.float32)
    assert got.dtype == np.float32 and same_bits(got, want)
    if dtype == np.float32:
        assert np.isnan(got[1, 5, 7]) and np.isnan(got[0, 0, 0]) and np.isnan(got[0, -1, -1]) and np.isnan(got).sum() == 3


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("B", ipr.RESIZE_BATCHES)
@pytest.mark.parametrize("case", ipr.RESIZE_CASES, ids=ipr.case_id)
def test_resize_bilinear_aa(case, B):
    Hs, Ws, H, W = case
    x = ipr.images(B, Hs, Ws, 7)
    ref, err = ipr.resize_aa(x, (H, W))
    xd = dev(x)
    got = ops.resize_bilinear_aa(xd, (H, W)).cpu().numpy()
    ratio = ipr.max_ratio(got, ref, err)
    print(f"RATIO resize_aa {ipr.case_id(case)} B{B} {ratio:.4f}")
    assert ratio <= 1.0
    assert same_bits(got, ops.resize_bilinear_aa(xd, (H, W)).cpu().numpy()), "two runs gave different bits"
    if (Hs, Ws) == (H, W):
        assert same_bits(got, x), "equal sizes must copy"
    if B > 1:
        alone = ops.resize_bilinear_aa(xd[B - 1:], (H, W)).cpu().numpy()
        assert same_bits(alone[0], got[B - 1]), "an image's bits depend on the batch around it"


# ------------------------------------------------------------------------------------------------ binarise
@pytest.mark.parametrize("case", ipr.BINARISE_CASES, ids=[str(c[0]) for c in ipr.BINARISE_CASES])
def test_minmax_binarise(case):
    (B, H, W), seed = case
    y = ipr.binarise_inputs((B, H, W), seed)
    refs = [ipr.binarise(img) for img in y]
    yd = dev(y)
    m1, st1 = ops.minmax_binarise(yd)
    m4, st4 = ops.minmax_binarise(yd, augment=True)
    b4, _ = ops.minmax_binarise(yd, augment=True, dtype=torch.bfloat16)
    assert m1.shape == (B, 1, H, W) and m4.shape == (4 * B, 1, H, W) and m1.dtype == torch.float32 and b4.dtype == torch.bfloat16
    assert m1.is_contiguous() and m4.is_contiguous()
    m1n, m4n = m1.cpu().numpy(), m4.cpu().numpy()
    assert same_bits(b4.float().cpu().numpy(), m4n), "bfloat16 and float32 masks differ"
    assert set(np.unique(m4n)) <= {0.0, 1.0}
    for b, r in enumerate(refs):
        want = r["mask"].astype(np.float32)
        assert same_bits(m1n[b, 0], want), f"image {b}: {int((m1n[b, 0] != want).sum())} pixels differ from the mask of the exact mean"
        for a in range(4):
            assert same_bits(m4n[4 * b + a, 0], ipr.flip_variant(want, a)), f"image {b} variant {a} is not the flip of variant 0"
        for st in (st1, st4):
            assert int(st.ones[b]) == r["ones"] and int(st.flags[b]) == 0
            assert float(st.mn[b]) == float(r["mn"]) and float(st.mx[b]) == float(r["mx"])
            assert abs(float(st.thr[b]) - r["thr"]) <= y[b].size * 2.0 ** -53 * r["thr"]
    assert torch.equal(st1.thr, st4.thr)
    alone, _ = ops.minmax_binarise(yd[B - 1:])
    assert torch.equal(alone[0], m1[B - 1]), "an image's mask depends on the batch around it"


def test_minmax_binarise_constant_and_nonfinite():
    y = ipr.binarise_inputs((4, 37, 53), 41)
    y[1] = 7.25
    y[2, 30, 2] = np.nan
    y[3, 0, 52] = np.inf
    for dtype in (torch.float32, torch.bfloat16):
        m, st = ops.minmax_binarise(dev(y), augment=True, dtype=dtype)
        m = m.float().cpu().numpy()
        assert st.flags.tolist() == [0, ops.PREP_CONSTANT, ops.PREP_NONFINITE, ops.PREP_NONFINITE]
        assert same_bits(m[0, 0], ipr.binarise(y[0])["mask"].astype(np.float32))
        assert not m[4:].any() and st.ones.tolist()[1:] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ percentile clip and scale
PERCENTILE_SHAPES = [(1,), (2,), (200,), (50, 70), (300, 500)]


@pytest.mark.parametrize("p", [99.5, 90.0])
@pytest.mark.parametrize("shape", PERCENTILE_SHAPES, ids=[str(s) for s in PERCENTILE_SHAPES])
def test_percentile_clip_scale(shape, p):
    n = int(np.prod(shape))
    kinds = ("ties", "equal", "signed", "smooth")
    x = np.stack([ipr.percentile_inputs(k, n, 11 + i).reshape(shape) for i, k in enumerate(kinds)])
    got, st = ops.percentile_clip_scale(dev(x), p)
    assert got.shape == x.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    for i, k in enumerate(kinds):
        want, vmin, vmax = ipr.normalize(x[i], p)
        assert float(st.vmin[i]) == vmin and float(st.vmax[i]) == vmax, (k, float(st.vmin[i]), vmin, float(st.vmax[i]), vmax)
        assert (got[i] == want).all(), f"{k}: {int((got[i] != want).sum())} of {n} outputs differ from numpy's"
        assert int(st.flags[i]) == 0
    alone, _ = ops.percentile_clip_scale(dev(x[3:]), p)
    assert same_bits(alone.cpu().numpy()[0], got[3]), "an image's bits depend on the batch around it"


def test_percentile_clip_scale_raises_for_an_infinity():
    x = np.stack([ipr.percentile_inputs("smooth", 3500, 3).reshape(50, 70) for _ in range(3)])
    x[1, 20, 20] = np.inf
    with pytest.raises(CvaeError, match=r"\[1\]"):
        ops.percentile_clip_scale(dev(x))
    out, st = ops.percentile_clip_scale(dev(x), check_finite=False)
    assert st.flags.tolist() == [0, ops.PREP_NONFINITE, 0]
    assert (out[0].cpu().numpy() == ipr.normalize(x[0])[0]).all()
    x[1, 20, 20] = np.nan
    with pytest.raises(CvaeError, match="NaN"):
        prepare_translator_images(x, size=(24, 40))


# ------------------------------------------------------------------------------------------------ end to end
def test_prepare_vessel_images_end_to_end():
    band = total = 0
    for case in ipr.RESIZE_CASES:
        Hs, Ws, H, W = case
        for B in ipr.RESIZE_BATCHES:
            x = ipr.images(B, Hs, Ws, 100 + B)
            ref = ipr.vessel_pipeline(x, (H, W))
            masks, stats = prepare_vessel_images(x, size=(H, W), augment=True, return_stats=True)
            assert masks.shape == (4 * B, 1, H, W) and masks.dtype == torch.float32 and masks.is_contiguous() and masks.is_cuda
            m = masks.cpu().numpy()[:, 0]
            assert set(np.unique(m)) <= {0.0, 1.0}
            worst, n_band, n, wrong = ipr.band_check(m[0::4] > 0.5, ref)
            print(f"BAND {ipr.case_id(case)} B{B}: {n_band}/{n} in the band, worst image {worst:.5f}, wrong outside {wrong}")
            assert wrong == 0 and worst <= ipr.MAX_EXCLUDED_PER_IMAGE
            for b in range(B):
                for a in range(1, 4):          # the dataset's index real_idx * 4 + aug_mode: flips of the reference wherever it is decided, exact flips of variant 0
                    assert same_bits(m[4 * b + a], ipr.flip_variant(m[4 * b], a))
                    keep = ~ipr.flip_variant(ref["band"][b], a)
                    assert ((m[4 * b + a] > 0.5) == ipr.flip_variant(ref["mask"][b], a))[keep].all()
            assert torch.equal(stats[0].ones.cpu(), torch.from_numpy((m[0::4] > 0.5).reshape(B, -1).sum(1)))
            band, total = band + n_band, total + n
    assert band <= ipr.MAX_EXCLUDED_OVERALL * total, (band, total)


def test_prepare_vessel_images_takes_stacks_lists_and_bf16():
    g = np.random.default_rng(3)
    stacks = (g.random((3, 4, 40, 56)) ** 6 * 3000 + 100).astype(np.uint16)
    want = prepare_vessel_images(np.max(stacks, axis=1).astype(np.float32), size=(32, 32))
    assert torch.equal(prepare_vessel_images(stacks, size=(32, 32)), want)
    assert torch.equal(prepare_vessel_images(torch.from_numpy(stacks).to(DEV), size=(32, 32), dtype=torch.bfloat16).float(), want)
    other = ipr.images(1, 37, 53, 9)[0]
    mixed = prepare_vessel_images([stacks[0], other, stacks[1], torch.from_numpy(stacks[2])], size=(32, 32), augment=True)
    assert mixed.shape == (16, 1, 32, 32)
    assert torch.equal(mixed[0::4][[0, 2, 3]], want) and torch.equal(mixed[4:8], prepare_vessel_images(other[None], size=(32, 32), augment=True))


@pytest.mark.parametrize("case", [((75, 131), (32, 64), 99.5), ((40, 56), (80, 112), 90.0), ((50, 70), (24, 40), 99.5)], ids=["down", "exact-2x-p90", "down-small"])
def test_prepare_translator_images_end_to_end(case):
    (Hs, Ws), (H, W), p = case
    g = np.random.default_rng(Hs)
    stacks = (g.random((3, 3, Hs, Ws)) ** 6 * 3000 + 100).astype(np.uint16)
    got = prepare_translator_images(stacks, size=(H, W), clip_percentile=p)
    assert got.shape == (3, 1, H, W) and got.dtype == torch.float32 and got.is_contiguous()
    src = np.stack([ipr.translator(s, (H, W), p)[1] for s in stacks])          # the reference's normalised images: what the device resizes, bit for bit
    ref, err = p64.resize_fwd(torch.from_numpy(src).reshape(3, 1, Hs, Ws, 1), (1, H, W))
    ratio = p64.max_ratio(got.cpu().reshape(3, 1, H, W, 1), ref["dst"], err["dst"])
    print(f"RATIO translator {Hs}x{Ws}->{H}x{W} {ratio:.4f}")
    assert ratio <= 1.0
    lst = prepare_translator_images([stacks[2], stacks[0]], size=(H, W), clip_percentile=p)
    assert torch.equal(lst, got[[2, 0]])


def test_masks_feed_causal_vit_vae():
    from causal_vae_amd.vit import CausalViTVAE
    torch.manual_seed(3)
    model = CausalViTVAE(img_size=(64, 96), depth=1).to(DEV).eval()
    x = prepare_vessel_images(ipr.images(1, 150, 211, 5), size=(64, 96), augment=True)
    assert x.shape == (4, 1, 64, 96) and x.dtype == torch.float32 and x.is_contiguous()
    assert set(torch.unique(x).tolist()) == {0.0, 1.0}
    m, t = torch.randn(4, model.m_dim, device=DEV), torch.nn.functional.one_hot(torch.arange(4, device=DEV), model.t_dim).float()
    recon = model(x, m, t)[0]
    assert recon.shape == x.shape and bool(torch.isfinite(recon).all())
