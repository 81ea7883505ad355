"""The references of tests/image_prep_reference.py held against torch and numpy themselves, and every refusal of the image preparation ops, without a
device.  tests/test_image_prep.py runs the kernels against the same references.
  * the float64 restatement of the antialiased resize agrees with torch's CPU operator within the bound the kernel is held to, on the kernel's case list.  The
    operator is run on float64 input, where it forms its weights in float64 as the restatement and the kernel do (ratios around 1e-9).  On float32 input torch forms
    scale, centre and weights in float32, an error that grows with the coordinate and that the bound (roundings of the two sums only) does not model: the float32
    operator sits at 0.22 - 0.50 of the bound on five cases and at 39 times the bound at 200 x 333 -> 96 x 160, whose scales are not binary fractions (printed);
  * the restatement of the translator transform equals the literal numpy / torch sequence of normalize_image + interpolate, bit for bit;
  * ops.percentile_ranks and numpy's lerp reproduce np.percentile's bits from a sorted array (what the kernel's radix select + finish computes);
  * every refusal of ops.mip_args / resize_aa_args / binarise_args / percentile_args is met on CPU tensors, the device being asked about last;
  * the exclusion band of the end-to-end test is a fair one: torch's own float32 pipeline leaves out at most 0.5 % of any image and 0.02 % of all pixels on the case
    list, and never disagrees with float64 outside the band."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_prep_reference as ipr  # noqa: E402
from causal_vae_amd import ops  # noqa: E402
from causal_vae_amd._lib import CvaeError  # noqa: E402


@pytest.mark.parametrize("case", ipr.RESIZE_CASES, ids=ipr.case_id)
def test_resize_restatement_agrees_with_torch(case):
    Hs, Ws, H, W = case
    x = ipr.images(3, Hs, Ws, 7)
    ref, err = ipr.resize_aa(x, (H, W))
    ratio = ipr.max_ratio(ipr.torch_resize_aa(x, (H, W), np.float64), ref, err)
    ratio32 = ipr.max_ratio(ipr.torch_resize_aa(x, (H, W)), ref, err)
    print(f"RATIO torch-cpu resize_aa {ipr.case_id(case)} float64 operator {ratio:.2e}, float32 operator {ratio32:.4f}")
    assert ratio <= 1.0
    if (Hs, Ws) == (H, W):
        assert np.array_equal(ref, x.astype(np.float64))


def test_resize_windows_of_the_ops_module_are_the_reference_windows():
    for Hs, Ws, H, W in ipr.RESIZE_CASES:
        for n_in, n_out in ((Hs, H), (Ws, W)):
            assert [ops._aa_window(i, n_in, n_out) for i in range(n_out)] == [ipr.aa_window(i, n_in, n_out) for i in range(n_out)]
    assert ops.aa_lds_bytes(2160, 3600, 768, 1280) < 48 * 1024


@pytest.mark.parametrize("p", [99.5, 90.0])
def test_translator_restatement_equals_the_literal_sequence(p):
    g = np.random.default_rng(5)
    stack = (g.random((3, 50, 70)) ** 6 * 3000 + 100).astype(np.uint16)
    # the reference, literally: load_image_any's projection and cast, normalize_image, ImageTableDataset's interpolate
    arr = np.max(stack, axis=0).astype(np.float32)
    vmin, vmax = np.percentile(arr, [100 - p, p])
    a = np.clip(arr, vmin, vmax)
    denom = vmax - vmin
    if denom == 0:
        denom = 1e-5
    a = (a - vmin) / denom
    img = torch.from_numpy(a).float().unsqueeze(0)
    img = F.interpolate(img.unsqueeze(0), size=(24, 40), mode="bilinear", align_corners=False).squeeze(0)
    got, v = ipr.translator(stack, (24, 40), p)
    assert got.dtype == np.float32 and np.array_equal(got, img.numpy())
    assert isinstance(vmin, np.float64) and a.dtype == np.float64          # the percentiles are float64 scalars: the clip and the division run in float64


def lerp_like_numpy(a, b, t):
    d = np.float64(np.float32(b) - np.float32(a))
    return np.float64(b) - d * (1 - t) if t >= 0.5 else np.float64(a) + d * t


@pytest.mark.parametrize("p", [99.5, 90.0, 100.0, 50.0])
@pytest.mark.parametrize("n", [1, 2, 3, 200, 3500, 150000])
def test_ranks_and_lerp_reproduce_numpy_percentile(n, p):
    for kind in ("smooth", "ties", "signed"):
        x = ipr.percentile_inputs(kind, n, n + 1)
        s = np.sort(x)
        (k0, k1, k2, k3), (t0, t1) = ops.percentile_ranks(n, p)
        assert 0 <= k0 <= k1 < n and 0 <= k2 <= k3 < n
        want = np.percentile(x, [100 - p, p])
        got = [lerp_like_numpy(s[k0], s[k1], t0), lerp_like_numpy(s[k2], s[k3], t1)]
        assert got[0] == want[0] and got[1] == want[1], (kind, n, p, got, want)


def refused(fn, *args, match):
    with pytest.raises(CvaeError, match=match):
        fn("op", *args)


def test_every_refusal_without_a_device():
    f32, u16 = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.uint16)
    # mip_max
    refused(ops.mip_args, np.zeros((2, 3, 8, 8), dtype=np.float32), match="tensor")
    refused(ops.mip_args, f32[0], match=r"\[B, D, Hs, Ws\]")
    refused(ops.mip_args, f32.double(), match="uint16 or float32")
    refused(ops.mip_args, f32[:, :0], match="empty")
    refused(ops.mip_args, torch.zeros(1, 1, 1, 1).expand(65536, 1, 1, 1), match="65535")
    refused(ops.mip_args, f32, match="MI355X only")
    refused(ops.mip_args, u16, match="MI355X only")
    # resize_bilinear_aa
    img = f32[:, 0]
    refused(ops.resize_aa_args, f32, (4, 4), match=r"\[B, Hs, Ws\]")
    refused(ops.resize_aa_args, img.half(), (4, 4), match="float32")
    refused(ops.resize_aa_args, img[:, :, :0], (4, 4), match="empty")
    refused(ops.resize_aa_args, img, 4, match="size")
    refused(ops.resize_aa_args, img, (4, 0), match="size")
    refused(ops.resize_aa_args, img, (4, 4, 4), match="size")
    refused(ops.resize_aa_args, torch.zeros(1, 1, 1).expand(1, 4096, 8), (8, 8), match="LDS")          # ratio 512: the row window of a tile cannot be staged
    refused(ops.resize_aa_args, img, (4, 4), match="MI355X only")
    # minmax_binarise
    refused(ops.binarise_args, f32, match=r"\[B, H, W\]")
    refused(ops.binarise_args, img.to(torch.bfloat16), match="float32")
    refused(ops.binarise_args, img[:0], match="empty")
    refused(ops.binarise_args, img, False, torch.float16, match="float32 or bfloat16")
    refused(ops.binarise_args, img, True, torch.bfloat16, match="MI355X only")
    # percentile_clip_scale
    refused(ops.percentile_args, torch.zeros(8), match=r"\[B, N\]")
    refused(ops.percentile_args, torch.zeros(2, 8, dtype=torch.float64), match="float32")
    refused(ops.percentile_args, torch.zeros(2, 0), match="empty")
    refused(ops.percentile_args, torch.zeros(2, 8), 40.0, match="percentile")
    refused(ops.percentile_args, torch.zeros(2, 8), 100.5, match="percentile")
    refused(ops.percentile_args, torch.zeros(2, 8), "high", match="percentile")
    refused(ops.percentile_args, torch.zeros(2, 8), match="MI355X only")
    refused(ops.percentile_args, img, 99.5, match="MI355X only")


def test_c_entries_refuse_before_any_launch():
    """the codes include/cvae_hip.h states for the four entries, each returned before anything is launched (there is no device here)"""
    import ctypes as C
    from causal_vae_amd import _lib as L
    lib, P = L.lib, C.c_void_p(4096)          # never dereferenced: every call below is refused
    BADSHAPE, DTYPE, UNSUPPORTED, WORKSPACE, NULLPTR = -1, -2, -3, -4, -6
    assert lib.cvae_mip_max(P, P, 1, 0, 8, 8, L.F32, None) == BADSHAPE
    assert lib.cvae_mip_max(P, P, 1, 2, 8, 8, L.BF16, None) == DTYPE
    assert lib.cvae_mip_max(P, P, 1, 2, 8, 8, 77, None) == DTYPE
    assert lib.cvae_mip_max(P, P, 65536, 2, 8, 8, L.U16, None) == UNSUPPORTED
    assert lib.cvae_mip_max(P, P, 1, 2, 65536, 32768, L.U16, None) == UNSUPPORTED
    assert lib.cvae_mip_max(None, P, 1, 2, 8, 8, L.U16, None) == NULLPTR
    assert lib.cvae_resize_bilinear_aa_f32(P, P, 1, 8, 8, 0, 4, None) == BADSHAPE
    assert lib.cvae_resize_bilinear_aa_f32(P, P, 1, 4096, 8, 8, 8, None) == UNSUPPORTED          # ratio 512: the same shape ops.resize_aa_args refuses
    assert lib.cvae_resize_bilinear_aa_f32(P, None, 1, 8, 8, 4, 4, None) == NULLPTR
    need = lib.cvae_minmax_binarise_workspace_bytes(2, 37, 53)
    assert need > 0 and lib.cvae_minmax_binarise_workspace_bytes(0, 37, 53) == 0
    assert lib.cvae_minmax_binarise(P, P, P, 2, 0, 53, 0, L.F32, P, need, None) == BADSHAPE
    assert lib.cvae_minmax_binarise(P, P, P, 2, 37, 53, 0, L.FP8, P, need, None) == DTYPE
    assert lib.cvae_minmax_binarise(P, P, P, 2, 37, 53, 0, 77, P, need, None) == DTYPE
    assert lib.cvae_minmax_binarise(P, P, P, 65536, 37, 53, 0, L.F32, P, need, None) == UNSUPPORTED
    assert lib.cvae_minmax_binarise(P, P, None, 2, 37, 53, 1, L.BF16, P, need, None) == NULLPTR
    assert lib.cvae_minmax_binarise(P, P, P, 2, 37, 53, 1, L.BF16, P, need - 1, None) == WORKSPACE
    assert lib.cvae_minmax_binarise(P, P, P, 2, 37, 53, 1, L.BF16, None, need, None) == WORKSPACE
    need = lib.cvae_percentile_clip_scale_workspace_bytes(2, 3500)
    ranks, t = (C.c_int64 * 4)(17, 18, 3481, 3482), (C.c_double * 2)(0.5, 0.5)
    assert need > 0
    assert lib.cvae_percentile_clip_scale(P, P, P, 2, 0, ranks, t, P, need, None) == BADSHAPE
    assert lib.cvae_percentile_clip_scale(P, P, P, 2, 3482, ranks, t, P, need, None) == BADSHAPE          # a rank outside [0, N)
    assert lib.cvae_percentile_clip_scale(P, P, P, 65536, 3500, ranks, t, P, need, None) == UNSUPPORTED
    assert lib.cvae_percentile_clip_scale(P, P, P, 2, 3500, None, t, P, need, None) == NULLPTR
    assert lib.cvae_percentile_clip_scale(P, P, P, 2, 3500, ranks, t, P, need - 1, None) == WORKSPACE


def test_exclusion_band_is_fair_to_torch_float32():
    """the condition of test_image_prep.py's end-to-end test, met by the reference's own float32 arithmetic: few pixels in the band, none wrong outside it"""
    band = total = 0
    for case in ipr.RESIZE_CASES:
        Hs, Ws, H, W = case
        for B in ipr.RESIZE_BATCHES:
            x = ipr.images(B, Hs, Ws, 100 + B)
            ref = ipr.vessel_pipeline(x, (H, W))
            worst, n_band, n, wrong = ipr.band_check(ipr.torch_vessel_pipeline(x, (H, W)), ref)
            print(f"BAND torch-cpu {ipr.case_id(case)} B{B}: {n_band}/{n} in the band, worst image {worst:.5f}, wrong outside {wrong}")
            assert wrong == 0 and worst <= ipr.MAX_EXCLUDED_PER_IMAGE
            band, total = band + n_band, total + n
    assert band <= ipr.MAX_EXCLUDED_OVERALL * total, (band, total)


def test_binarise_inputs_are_clear_of_the_mean():
    """the inputs of test_image_prep.py's binarise test: no v within n 2^-53 thr of the exact mean, so a float64 sum in any order decides every pixel alike"""
    for shape, seed in ipr.BINARISE_CASES:
        for y in ipr.binarise_inputs(shape, seed):
            assert ipr.binarise(y)["clearance"] > 1.0
