"""GPU cases for the launch layer's multi-axis dispatch (csrc/common.h: with_dtype, with_nd, with_bool nested): one case per template instance that the rest of
the suite does not select, each through ops at the smallest shape that selects it.  Nothing new is measured here: every case is judged by the float64
reference and the derived bound of the kernel's own test file (tests/test_conv_reference.py: oracle/conv64.py; tests/test_vit_encoder_grad.py:
tests/vit_encoder_grad_reference.py), or — the streamed 2x resize — by that kernel's existing bit-equality with the launches below the streaming size.

  wgrad_c1_kernel<T, TL, ND, LSUM, VEC>   B = 1, Cs = 32.  2D image 16 x 16 (bf16 rows of whole 16-byte vectors: VEC), 16 x 12 (bf16: element form; fp32 image:
      whole vectors), 16 x 10 (element form for an fp32 image too), 3D 8 x 16 x 16 and 4 x 8 x 12 (3D element form); gradient / image bf16 / bf16, fp32 / fp32
      and bf16 / fp32 (the mixed form), each with the ConvTranspose bias sum (LSUM; the mixed form has none: ops refuses it) and with the Conv bias sum instead.
  vit_gemm_bwd_data_kernel<T, TG, TO>     the five forms (fp32; bf16 with a bf16 / fp32 gradient and a bf16 / fp32 result) at M = 130 rows (one full 128-row tile
      and a ragged one) for the four supported (K, N).
  vit_gemm_wgrad_kernel<T, TG>            the three forms (fp32; bf16 input with a bf16 / fp32 gradient), same rows and shapes.
  up2x_tile_kernel<float, NT>, up2x_block_kernel<float, 4>   the streamed resize of an fp32 source (tests/test_hip_ops.py runs the bf16 one)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from causal_vae_amd import ops  # noqa: E402
from oracle import conv64 as c64  # noqa: E402
import vit_reference as vr  # noqa: E402
from test_conv_reference import wgrad_check  # noqa: E402
from test_vit_encoder_grad import rand, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}

# ---- wgrad_c1 -------------------------------------------------------------------------------------------------------------------------------------
IMAGES = [(2, (16, 16)), (2, (16, 12)), (2, (16, 10)), (3, (8, 16, 16)), (3, (4, 8, 12))]
FORMS = [("bf16", "bf16", 1), ("bf16", "bf16", 0), ("f32", "f32", 1), ("f32", "f32", 0), ("bf16", "f32", 0)]      # gradient dtype, image dtype, dbias side


@pytest.mark.parametrize("sdt,ldt,side", FORMS, ids=[f"{s}-{ld}-side{k}" for s, ld, k in FORMS])
@pytest.mark.parametrize("nd,image", IMAGES, ids=["x".join(map(str, im)) for _nd, im in IMAGES])
def test_wgrad_single_channel_forms(nd, image, sdt, ldt, side):
    i = IMAGES.index((nd, image))
    c = c64.make_case("wgrad", 1100 + i, nd, 1, 1, 32, tuple(v // 2 for v in image), DT[sdt])
    assert c["l_dims"][-nd:] == image
    if ldt != sdt:                                           # the fp32 image is rounded to bf16 on the way into LDS
        img = torch.randn(c["L"].shape, generator=torch.Generator().manual_seed(i))
        c["L"], c["L_dev"] = img.to(BF16).float(), img
    wgrad_check(f"wgrad-c1-{sdt}-{ldt}-{'x'.join(map(str, image))}", c, side, l_dtype=DT[ldt])


# ---- token GEMMs ----------------------------------------------------------------------------------------------------------------------------------
M = 130
KN = [(256, 768), (256, 256), (256, 512), (512, 256)]
_CASE = {}


def gemm_case(K, N):
    """bf16-exact operands of one shape, shared by every form, and their float64 copies"""
    if (K, N) not in _CASE:
        c = lambda t: t.double()
        g, x, W = rand(F32, M, N, seed=K + N), rand(F32, M, K, seed=K), rand(F32, N, K, seed=11, scale=0.2)
        _CASE[K, N] = dict(g=g, x=x, W=W, g64=c(g), x64=c(x), W64=c(W), Wb64=c(vr.round_bf16(W)))
    return _CASE[K, N]


BWD_DATA = [(F32, F32, F32), (BF16, BF16, BF16), (BF16, BF16, F32), (BF16, F32, BF16), (BF16, F32, F32)]      # arithmetic, gradient dtype, result dtype


@pytest.mark.parametrize("mode,gdt,odt", BWD_DATA, ids=["f32", "bf16", "bf16-out32", "bf16-g32", "bf16-g32-out32"])
@pytest.mark.parametrize("K,N", KN)
def test_token_gemm_bwd_data_forms(K, N, mode, gdt, odt):
    c = gemm_case(K, N)
    Wd = c["Wb64"] if mode == BF16 else c["W64"]
    dx = ops.token_gemm_bwd_data(c["g"].to(gdt).to(DEV), c["W"].to(DEV), mode, out_dtype=odt)
    assert dx.dtype == odt
    ref = c["g64"] @ Wd
    within(dx, ref, (N + 2) * vr.U32 * (c["g64"].abs() @ Wd.abs()) + (vr.UBF * ref.abs() if odt == BF16 else 0), f"bwd_data {mode} g {gdt} out {odt} K{K} N{N}")


@pytest.mark.parametrize("xdt,gdt", [(F32, F32), (BF16, BF16), (BF16, F32)], ids=["f32", "bf16", "bf16-g32"])
@pytest.mark.parametrize("K,N", KN)
def test_token_gemm_wgrad_forms(K, N, xdt, gdt):
    c = gemm_case(K, N)
    dW, db = ops.token_gemm_wgrad(c["g"].to(gdt).to(DEV), c["x"].to(xdt).to(DEV))
    within(dW, c["g64"].T @ c["x64"], (M + 2) * vr.U32 * (c["g64"].abs().T @ c["x64"].abs()), f"wgrad dW x {xdt} g {gdt} K{K} N{N}")
    within(db, c["g64"].sum(0), (4 + M * 2.0 ** -20) * vr.U32 * c["g64"].abs().sum(0), f"wgrad db x {xdt} g {gdt} K{K} N{N}")


# ---- streamed 2x resize of an fp32 source ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,src", [(32, (64, 64, 64)), (64, (64, 64, 32))], ids=["tile-kernel", "block-kernel"])
def test_up2x_streaming_outputs_equal_the_small_launches_fp32(B, src):
    """tests/test_hip_ops.py::test_up2x_streaming_outputs_equal_the_small_launches for an fp32 source: the same arithmetic as the launches below 256 MB,
    which test_upsample_linear ties to F.interpolate, so the bits must agree chunk by chunk"""
    x = torch.randn(B, *src, 1, generator=torch.Generator().manual_seed(9)).to(DEV)
    dst = tuple(2 * v for v in src)
    assert B * dst[0] * dst[1] * dst[2] * 4 >= 256 << 20
    with torch.no_grad():
        big = ops.UpsampleLinear.apply(x, dst)
        for b0 in range(0, B, 8):
            assert torch.equal(big[b0:b0 + 8], ops.UpsampleLinear.apply(x[b0:b0 + 8].contiguous(), dst)), b0
