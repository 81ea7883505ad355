"""The k4 / s2 / p1 convolution kernels (csrc/conv_mfma.hip, csrc/conv_c1.hip) against the float64 reference oracle/conv64.py: ONE launch, ONE comparison
with an elementwise bound derived from the sum (C sqrt(K) U (|A| . |B| + |bias|), C = 4, U = 2^-24, plus half a bf16 / e4m3 ulp on a bf16 / fp8 result);
masks are independent random tensors.  tests/test_conv_reference_cpu.py shows that the bounds are neither loose nor wrong.

Form -> cases (tile extents in positions of the GATHERED side: S for `down` / wgrad, the parity lattice ceil(l / 2) for `up`):
  down, 64-channel tiles, Tile<3,128> 4x4x8 / Tile<2,128> 8x16     conv_data_kernel<float, 2x2 waves> (f32) / <bf16, K-split waves> (bf16)
      DOWN3D: one tile, +-1 voxel per axis, 2 / 3 voxels, odd L (9, 8, 11), Cl 16 (minimum, ksplit 1) / 96 / 128 / 256 (ksplit 6 / 8 / 16 = cap),
      Cs 64 / 192; every case with split-K on and off.  DOWN2D: the same seams, B = 3 and 5 with XB = 2 forced (DOWN_VARIANT = 1) and off,
      B = 32 x Cs 256 (128 workgroups: ksplit 3 of 6 chunks), B = 64 x Cs 256 (256 workgroups: ksplit 1).
  up, 64-channel tiles                                              conv_data_kernel<UP>: f32; bf16 KH = 2 (Cs >= 128) and KH = 1 (Cs 64 / 96)
      UP3D / UP2D: the seams above on the parity lattice, l = 2 s and l = 2 s + 1, XB = 2 forced with odd B (3D: rows <= 4 wide; 2D: <= 8 wide).
      `up` never splits K (pick_ksplit returns 1 for it): the SPLIT_K switch is run on and off all the same and must not change anything.
  up, 32-channel tiles (Cl % 64 != 0), Tile<3,256> 4x8x8 / <2,256> 16x16   conv_up_full_kernel (bf16, upfull = 1; it exists for 3D Cs 64 and 2D Cs 64 / 128 only:
      whole_k_exists) and conv_data_kernel (upfull = 0; f32; every other Cs)
  Cl == 1 (Cs == 32)   down_c1_kernel (f32; bf16 with lw % 8 != 0), down_c1_vec_kernel (bf16 image MS 2 / 4, fp32 image -> bf16 S, masked),
      up_c1_kernel (f32), up_c1_mfma_kernel (bf16), up_c1_mfma_walk_kernel (bf16, c1_walk_units forced: whole columns, even segments, a short last segment: walk_plan), wgrad_c1_kernel (f32; bf16 vector and plain; fp32
      image with bf16 S; S-side and L-side bias sum)
  wgrad                conv_wgrad_kernel + wgrad_reduce_kernel through cvae_conv_wgrad (own launch) and cvae_conv_wgrad_multi (3 / 5 layers of unequal size,
      dbias_side 0 and 1), f32 and bf16, ragged and odd extents, Cl 32 / 96, Cs 64 / 192
  fp8                  cvae_conv_fp8 down (bf16 / dual / codes output, split-K on and off), up wide and 32-channel, xpair; cvae_conv_up_c1_fp8in
Every family also runs STRUCTURED cases (small-integer inputs; one-hot weight for down / up / fp8, integer S and L for wgrad: the result must be exact, so a
wrong index is a named coordinate).  relu_bits_out of cvae_conv_fp8 is NOT compared with the bound: with the fp8 MFMA's truncation term more than 0.1 % of a case's
pre-activations are undecided.  Kernel names of one run of this file (rocprofv3 --kernel-trace --stats): profiles/conv_reference_kernel_names.txt.

ReLU masks as bits: relu_bits_out must equal pre > 0 wherever |pre| > its bound; at most 0.1 % of a case may be undecided.

Measured on the MI355X, max |got - ref| / err per family (the CPU fp32 aten stand-in of tests/test_conv_reference_cpu.py in brackets):
  down 64-ch tiles   f32 3D 0.001 - 0.026, 2D 0.002 - 0.067 [0.02 - 0.04];  bf16 3D 0.79 - 0.98, 2D 0.92 - 0.99 (XB = 2: 0.94 - 0.98) [0.92 - 0.96]
  up 64-ch tiles     f32 3D 0.017 - 0.077, 2D 0.031 - 0.108 [0.06 - 0.07];  bf16 0.95 - 0.99, XB = 2 alike [0.97 - 0.98]
  up 32-ch tiles     f32 0.017 - 0.057;  bf16 conv_data_kernel 0.96 - 0.99, whole-K kernel 0.96 - 0.99 [0.99]
  Cl == 1            down f32 0.07 - 0.21 [0.16], bf16 and fp32-image forms 0.98 - 0.995 [0.99];  up f32 0.010 - 0.027, bf16 0.56 - 0.97, walking 0.97 - 0.98 [0.98]
  wgrad              dW f32 0.002 - 0.40, bf16 0.001 - 0.31, grouped launch 0.004 - 0.37 [0.02 - 0.11];  dbias <= 0.10 [<= 0.01];  Cl == 1 dW <= 0.10 [0.01]
  ReLU bits          0 wrong bits, 0 undecided elements in every case; the results 0.003 - 0.05 (f32), 0.92 - 0.99 (bf16)
  fp8                bf16 result 0.48 - 0.73, code result 0.91 - 0.97 with the truncation term of the fp8 MFMA in the bound (see test_conv_fp8);  without it 0.89 - 1.017, 0.99 - 1.00 [0.998 - 0.999];  cvae_conv_up_c1_fp8in 0.90 - 0.99
(a bf16 / e4m3 result sits just under 1 by construction: the half ulp of the stored value is nearly the whole bound and is reached by some element.)
Found by this file and fixed with it: cvae_conv_fp8 `down` with split-K and a code output scaled BY VALUE (out8_inv_scale, no dscale) quantised the codes with
scale 1 in conv_splitk_finish_kernel (test_conv_fp8[1]: 3D, 128 -> 256 channels at 8^3, 8361 of 16384 codes wrong, max ratio 31.5).
"""
import ctypes as C

import pytest
import torch

from causal_vae_amd import _lib as L
from causal_vae_amd import ops
from oracle import conv64 as c64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
ACTS = [None, "relu", "sigmoid", "leaky02"]


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(t, dtype):
    return None if t is None else t.to(DEV).to(dtype).contiguous()


def report(family, got, ref, err):
    r = c64.max_ratio(got, ref, err)
    print(f"RATIO {family} {r:.3f}")
    bad = c64.compare({"y": got}, {"y": ref}, {"y": err})
    assert not bad, family + ": " + "\n".join(bad)


class hooks:
    """ops' test switches for one launch, restored afterwards"""

    def __init__(self, split_k=True, up=None, down=None):
        self.new = (split_k, up, down)

    def __enter__(self):
        self.old = (ops.SPLIT_K, ops.UP_VARIANT, ops.DOWN_VARIANT)
        ops.SPLIT_K, ops.UP_VARIANT, ops.DOWN_VARIANT = self.new

    def __exit__(self, *a):
        ops.SPLIT_K, ops.UP_VARIANT, ops.DOWN_VARIANT = self.old


def variety(i):
    """epilogue of case i: the activation cycles through all four, bias and mask come and go with different periods"""
    return ACTS[i % 4], (i % 3) != 2, (i % 5) in (1, 3)


def launch(c, act, split_k=True, up=None, down=None, l_dtype=None, want_bits=None, mask_bits=None):
    """the case through ops._conv_down / ops._conv_up: one launch.  l_dtype: dtype the single-channel image is stored in (mixed form)."""
    dt, nd = c["dtype"], c["nd"]
    b, m = dev(c["bias"], F32), dev(c["mask"], dt)
    with hooks(split_k, up, down):
        if c["kind"] == "down":
            wp = ops.pack_weight(c["w"].to(DEV), nd, False, dt)
            x = dev(c["L"], l_dtype or dt)
            return ops._conv_down(x, wp, b, m, c["Cs"], nd, act, out_dtype=dt if l_dtype else None, want_bits=want_bits, mask_bits=mask_bits)
        wp = ops.pack_weight(c["w"].to(DEV), nd, True, dt)
        return ops._conv_up(dev(c["S"], dt), wp, b, m, c["Cl"], nd, act, l_dims=c["l_dims"], want_bits=want_bits, mask_bits=mask_bits)


def check(family, c, act, **kw):
    ref, err, _, _ = c64.reference(c, act)
    ref, err = c64.out_bound(ref, err, "bf16" if c["dtype"] == BF16 else "f32")
    got = launch(c, act, **kw)
    torch.cuda.synchronize()
    report(family, got, ref, err)
    return got


def check_structured(family, kind, nd, B, Cl, Cs, size, dtype, **kw):
    c = c64.make_case(kind, 0, nd, B, Cl, Cs, size, dtype, bias=False, structure=True, odd_l=kw.pop("odd_l", False))
    ref = c64.reference(c)[0]
    got = launch(c, None, **kw).double().cpu()
    diff = torch.nonzero(got != ref)
    assert diff.numel() == 0, f"{family}: {diff.shape[0]} wrong; first at (b, z, y, x, c) = {diff[0].tolist()}: got {float(got[tuple(diff[0])])} want {float(ref[tuple(diff[0])])}"


# ------------------------------------------------------------------------------------------------ down, 64-channel tiles
DOWN3D = [  # B, Cl, Cs, large extent
    (1, 32, 64, (8, 8, 16)), (2, 32, 64, (10, 8, 16)), (1, 32, 64, (8, 10, 16)), (1, 32, 64, (8, 8, 18)), (2, 32, 64, (6, 8, 16)), (1, 32, 64, (8, 6, 16)),
    (1, 32, 64, (8, 8, 14)), (3, 48, 64, (4, 6, 4)), (2, 64, 128, (6, 4, 6)), (1, 32, 64, (9, 8, 11)), (2, 16, 64, (8, 8, 16)), (1, 96, 192, (8, 10, 8)),
    (1, 128, 64, (4, 4, 8)), (1, 256, 64, (4, 6, 4)), (5, 32, 64, (5, 7, 9)),
]
DOWN2D = [
    (1, 32, 64, (16, 32)), (2, 32, 64, (18, 32)), (1, 32, 64, (16, 34)), (3, 32, 64, (14, 32)), (1, 32, 64, (16, 30)), (2, 48, 64, (4, 6)), (3, 96, 192, (14, 14)),
    (5, 64, 128, (6, 16)), (2, 16, 64, (13, 9)), (32, 96, 256, (8, 16)), (64, 32, 256, (4, 8)), (1, 256, 64, (16, 32)),
]


@pytest.mark.parametrize("split_k", [True, False], ids=["splitk", "unsplit"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(DOWN3D)))
def test_down_3d(i, dt, split_k):
    B, Cl, Cs, size = DOWN3D[i]
    act, bias, masked = variety(i)
    check(f"down3d-{dt}", c64.make_case("down", 100 + i, 3, B, Cl, Cs, size, DT[dt], bias=bias, masked=masked), act, split_k=split_k)


# two samples per tile (XB = 2): rows at most 8 wide, B >= 2; forced once per case, with split-K on
DOWN2D_ARMS = [(i, dt, xb, sk) for i, (B, _, _, size) in enumerate(DOWN2D) for dt in ("f32", "bf16") for xb in (0, 1) for sk in (True, False)
               if not (xb and (size[1] // 2 > 8 or B < 2 or not sk or dt == "f32"))]            # XB = 2 exists for 2-byte operands only (DataForm::XPAIR)


@pytest.mark.parametrize("i,dt,xb,split_k", DOWN2D_ARMS)
def test_down_2d(i, dt, xb, split_k):
    B, Cl, Cs, size = DOWN2D[i]
    act, bias, masked = variety(i + 1)
    check(f"down2d-{dt}" + ("-xb2" if xb else ""), c64.make_case("down", 200 + i, 2, B, Cl, Cs, size, DT[dt], bias=bias, masked=masked), act, split_k=split_k, down=xb)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_down_structured(dt):
    for nd, B, Cl, Cs, size, kw in [(3, 2, 96, 192, (10, 8, 18), {}), (3, 2, 96, 192, (10, 8, 18), dict(split_k=False)), (2, 3, 96, 192, (18, 14), dict(down=1)),
                                    (2, 3, 96, 192, (18, 34), {})]:
        if dt == "f32" and kw.get("down"):
            continue                                         # XB = 2: bf16 only
        check_structured(f"down{nd}d-{dt}", "down", nd, B, Cl, Cs, size, DT[dt], **kw)


# ------------------------------------------------------------------------------------------------ up
UP3D = [  # B, Cl, Cs, small extent, odd_l — 64-channel tiles: Tile<3,128> 4x4x8 on the parity lattice
    (1, 64, 64, (4, 4, 8), False), (2, 64, 128, (5, 4, 8), False), (1, 64, 128, (4, 5, 8), False), (1, 64, 64, (4, 4, 9), False), (2, 64, 128, (3, 4, 8), False),
    (1, 64, 64, (4, 3, 7), False), (3, 64, 128, (2, 3, 2), False), (1, 64, 64, (4, 4, 5), True), (2, 128, 256, (2, 2, 4), True), (3, 192, 96, (3, 4, 4), False),
    (5, 64, 128, (2, 4, 3), False), (1, 64, 16, (4, 4, 8), False), (1, 64, 64, (4, 3, 8), False), (1, 64, 128, (4, 4, 7), False),       # a tile minus one voxel in h alone, in w alone
]
UP2D = [
    (1, 64, 64, (8, 16), False), (2, 64, 128, (9, 16), False), (1, 64, 64, (8, 17), False), (3, 64, 128, (7, 15), False), (2, 64, 64, (2, 3), False),
    (3, 64, 64, (3, 3), True), (2, 64, 64, (6, 4), True), (5, 192, 96, (7, 7), False), (3, 128, 256, (3, 8), False), (1, 64, 16, (8, 16), False),
]


# two samples per tile (XB = 2): bf16, rows at most 4 wide, B >= 2.  `up` never splits K: the switch is exercised on every third case
UP3D_ARMS = [(i, dt, xb, sk) for i, (B, _, _, size, odd) in enumerate(UP3D) for dt in ("f32", "bf16") for xb in (0, 1) for sk in (True, False)
             if not (xb and (size[2] + (1 if odd else 0) > 4 or B < 2 or dt == "f32" or not sk)) and not (not sk and i % 3)]


@pytest.mark.parametrize("i,dt,xb,split_k", UP3D_ARMS)
def test_up_3d_wide(i, dt, xb, split_k):
    B, Cl, Cs, size, odd = UP3D[i]
    act, bias, masked = variety(i + 2)
    check(f"up3d-{dt}" + ("-xb2" if xb else ""), c64.make_case("up", 300 + i, 3, B, Cl, Cs, size, DT[dt], bias=bias, masked=masked, odd_l=odd), act, split_k=split_k, up=(-1, xb, 0))


UP2D_ARMS = [(i, dt, xb) for i, (B, _, _, size, odd) in enumerate(UP2D) for dt in ("f32", "bf16") for xb in (0, 1)
             if not (xb and (size[1] + (1 if odd else 0) > 8 or B < 2 or dt == "f32"))]      # XB = 2: bf16, rows at most 8 wide, B >= 2


@pytest.mark.parametrize("i,dt,xb", UP2D_ARMS)
def test_up_2d_wide(i, dt, xb):
    B, Cl, Cs, size, odd = UP2D[i]
    act, bias, masked = variety(i + 3)
    check(f"up2d-{dt}" + ("-xb2" if xb else ""), c64.make_case("up", 400 + i, 2, B, Cl, Cs, size, DT[dt], bias=bias, masked=masked, odd_l=odd), act, up=(-1, xb, 0))


UP32 = [  # nd, B, Cl, Cs, small extent, odd_l — 32-channel tiles: Tile<3,256> 4x8x8, Tile<2,256> 16x16
    (3, 1, 32, 64, (4, 8, 8), False), (3, 2, 32, 128, (5, 8, 8), False), (3, 1, 32, 256, (4, 9, 8), False), (3, 1, 32, 64, (4, 8, 9), False), (3, 2, 32, 64, (3, 7, 7), False),
    (3, 3, 96, 128, (2, 3, 2), False), (3, 1, 32, 64, (4, 4, 5), True), (3, 2, 96, 96, (3, 4, 5), False), (2, 1, 32, 64, (16, 16), False), (2, 2, 96, 128, (17, 15), False),
    (2, 3, 32, 256, (7, 7), False), (2, 2, 32, 64, (6, 4), True), (2, 1, 32, 64, (2, 3), False),
    (3, 1, 32, 64, (4, 7, 8), False), (3, 1, 32, 64, (4, 8, 7), False), (3, 2, 32, 64, (3, 8, 8), False), (2, 2, 32, 128, (15, 16), False), (2, 1, 32, 128, (16, 15), False),   # a tile minus one voxel per axis, alone
]


def whole_k_exists(nd, Cs):
    """conv_up_full_kernel is bf16 and exists where the halo of ALL input channels fits the 160 KiB of LDS (launch_up_full): 3D Cs 64 (136 KB; 128: 261 KB),
    2D Cs 64 / 128 (68 / 131 KB; 256: 256 KB).  Elsewhere cvae_conv_up(upfull = 1) runs conv_data_kernel, which the data-kernel arm covers already."""
    return Cs == 64 or (nd == 2 and Cs == 128)


UP32_ARMS = [(i, dt, uf) for i, c in enumerate(UP32) for dt in ("f32", "bf16") for uf in (0, 1) if not (uf and (dt == "f32" or not whole_k_exists(c[0], c[3])))]


@pytest.mark.parametrize("i,dt,upfull", UP32_ARMS)
def test_up_32_channel_tiles(i, dt, upfull):
    nd, B, Cl, Cs, size, odd = UP32[i]
    act, bias, masked = variety(i)
    check(f"up32-{dt}-" + ("wholek" if upfull else "data"), c64.make_case("up", 500 + i, nd, B, Cl, Cs, size, DT[dt], bias=bias, masked=masked, odd_l=odd), act, up=(upfull, -1, 0))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_up_structured(dt):
    for nd, B, Cl, Cs, size, kw in [(3, 2, 192, 96, (5, 4, 9), {}), (3, 3, 192, 128, (3, 4, 4), dict(up=(-1, 1, 0))), (3, 2, 96, 64, (5, 9, 8), dict(up=(1, -1, 0))),
                                    (3, 2, 96, 128, (5, 9, 8), dict(up=(0, -1, 0))), (2, 2, 96, 128, (17, 15), dict(up=(1, -1, 0))), (2, 3, 192, 96, (9, 7), dict(up=(-1, 1, 0))), (2, 2, 96, 64, (17, 15), dict(up=(1, -1, 0))),
                                    (3, 1, 192, 96, (4, 4, 5), dict(odd_l=True))]:
        if dt == "f32" and kw.get("up", (0,))[0] == 1:
            continue
        check_structured(f"up{nd}d-{dt}", "up", nd, B, Cl, Cs, size, DT[dt], **kw)


# ------------------------------------------------------------------------------------------------ ReLU masks as bits
BITS = c64.BIT_CASES        # the CPU file asserts the 0.1 % condition on exactly these cases


@pytest.mark.parametrize("kind,nd,B,Cl,Cs,size,dt,split_k", BITS)
def test_relu_bits_out(kind, nd, B, Cl, Cs, size, dt, split_k):
    c = c64.make_case(kind, c64.BIT_SEED, nd, B, Cl, Cs, size, DT[dt], bits=True)
    ref, err, pre, e_pre = c64.reference(c, "relu")
    assert c64.undecided_fraction(pre, e_pre) <= 1e-3
    y, bits = launch(c, "relu", split_k=split_k, want_bits=True)
    assert bits is not None and bits.numel() * 32 == y.numel()
    wrong, undecided, total = c64.relu_bits(bits, pre, e_pre)
    assert wrong == 0 and undecided <= 1e-3 * total, (wrong, undecided, total)
    report(f"bits-{kind}{nd}d-{dt}", y, *c64.out_bound(ref, err, "bf16" if dt == "bf16" else "f32"))


def pack_bits(mask):
    """a 0 / 1 tensor -> the int32 words a launch reads as mask_bits (element 32 i + j = bit j of word i)"""
    w = ((mask.reshape(-1, 32) > 0).long() << torch.arange(32)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).to(DEV)


@pytest.mark.parametrize("kind,nd,B,Cl,Cs,size,dt,split_k", [
    ("down", 3, 2, 32, 64, (8, 10, 18), "bf16", True), ("down", 3, 1, 128, 256, (8, 8, 8), "f32", True), ("down", 3, 1, 128, 256, (8, 8, 8), "bf16", False), ("down", 2, 3, 32, 64, (30, 44), "f32", True),
    ("up", 3, 2, 64, 128, (3, 4, 9), "bf16", True), ("up", 2, 3, 32, 64, (7, 7), "f32", True), ("up", 3, 1, 96, 64, (4, 4, 5), "bf16", True), ("down", 3, 2, 1, 32, (8, 16, 32), "bf16", True)])
def test_mask_given_as_bits(kind, nd, B, Cl, Cs, size, dt, split_k):
    """mask_bits in place of the mask tensor (conv_data_kernel, conv_splitk_finish_kernel, down_c1_vec_kernel): an independent random mask, packed here; where
    the launch can, it leaves the bits of its own (masked) result too"""
    odd = kind == "up" and size == (4, 4, 5)
    c = c64.make_case(kind, 650, nd, B, Cl, Cs, size, DT[dt], masked=True, bits=True, odd_l=odd)
    ref, err, pre, e_pre = c64.reference(c, "relu")
    mb = pack_bits(c["mask"])
    before = ops.BITS_STATS["consumed"]
    y, bits = launch(dict(c, mask=None), "relu", split_k=split_k, want_bits=True, mask_bits=mb)
    assert ops.BITS_STATS["consumed"] == before + 1, "the launch did not take the bit form of the mask"
    report(f"maskbits-{kind}{nd}d-{dt}", y, *c64.out_bound(ref, err, "bf16" if dt == "bf16" else "f32"))
    if bits is not None:
        assert c64.undecided_fraction(pre, e_pre) <= 1e-3
        wrong, undecided, total = c64.relu_bits(bits, pre, e_pre, mask=c["mask"])
        assert wrong == 0, (wrong, undecided, total)


@pytest.mark.parametrize("nd,B,size", [(3, 2, (8, 16, 32)), (3, 1, (6, 18, 40)), (2, 3, (34, 28))])
def test_image_layer_relu_bits(nd, B, size):
    """cvae_conv_down_image_f8: relu_bits_out of the single-channel layer (fp32 image, bf16 S)"""
    c = c64.make_case("down", 660, nd, B, 1, 32, size, BF16, bits=True)
    ref, err, pre, e_pre = c64.reference(c, "relu")
    assert c64.undecided_fraction(pre, e_pre) <= 1e-3
    y, bits = ops._conv_down(dev(c["L"], F32), c["w"].to(DEV), dev(c["bias"], F32), None, 32, nd, "relu", out_dtype=BF16, want_bits=True)
    assert bits is not None
    report("image-bits", y, *c64.out_bound(ref, err, "bf16"))
    wrong, undecided, total = c64.relu_bits(bits, pre, e_pre)
    assert wrong == 0 and undecided <= 1e-3 * total, (wrong, undecided, total)


# ------------------------------------------------------------------------------------------------ Cl == 1
C1_DOWN = [  # nd, B, large extent, image dtype, S dtype — TileC1<3> 4x8x8, TileC1<2> 16x16; TileC1V<3, MS> (MS/2)x8x32, TileC1V<2> 32x16
    (3, 2, (8, 16, 16), "f32", "f32"), (3, 1, (10, 16, 18), "f32", "f32"), (3, 2, (6, 14, 14), "f32", "f32"), (3, 1, (4, 6, 4), "f32", "f32"), (2, 3, (32, 32), "f32", "f32"),
    (2, 2, (34, 30), "f32", "f32"), (3, 2, (6, 20, 10), "bf16", "bf16"), (2, 3, (28, 28), "bf16", "bf16"),
    (3, 2, (4, 16, 64), "bf16", "bf16"), (3, 1, (6, 18, 72), "bf16", "bf16"), (3, 3, (2, 14, 56), "bf16", "bf16"), (2, 2, (64, 32), "bf16", "bf16"), (2, 3, (66, 40), "bf16", "bf16"),
    (3, 2, (4, 16, 64), "f32", "bf16"), (3, 1, (6, 18, 68), "f32", "bf16"), (2, 2, (62, 28), "f32", "bf16"), (3, 16, (32, 64, 128), "f32", "bf16"),     # 1024 tiles: MS = 4 in 3D
    (3, 16, (32, 64, 128), "bf16", "bf16"),    # the same for the bf16 image
]


@pytest.mark.parametrize("i", range(len(C1_DOWN)))
def test_down_single_channel(i):
    nd, B, size, ldt, sdt = C1_DOWN[i]
    act, bias, masked = variety(i)
    act = act if act != "sigmoid" else "relu"                # the image kernels' epilogues: none / ReLU / LeakyReLU
    c = c64.make_case("down", 700 + i, nd, B, 1, 32, size, DT[sdt], bias=bias, masked=masked)
    if ldt != sdt:                                           # fp32 image whose values are NOT bf16 values: the kernel rounds them on the way into LDS
        img = torch.randn(c["L"].shape, generator=torch.Generator().manual_seed(i))
        c["L"], c["L_dev"] = img.to(BF16).float(), img
    ref, err, _, _ = c64.reference(c, act)
    ref, err = c64.out_bound(ref, err, "bf16" if sdt == "bf16" else "f32")
    x = dev(c.get("L_dev", c["L"]), DT[ldt])
    got = ops._conv_down(x, c["w"].to(DEV), dev(c["bias"], F32), dev(c["mask"], DT[sdt]), 32, nd, act, out_dtype=DT[sdt] if ldt != sdt else None)
    report(f"down-c1-{ldt}-{sdt}", got, ref, err)


C1_UP = [(3, 2, (2, 8, 16), 0), (3, 1, (3, 9, 17), 0), (3, 3, (1, 7, 15), 0), (3, 2, (2, 3, 2), 0), (3, 2, (6, 9, 17), 1), (3, 1, (5, 8, 16), 1), (2, 2, (16, 16), 0),
         (2, 3, (17, 15), 0), (2, 1, (2, 3), 0), (3, 1, (9, 8, 16), 2), (3, 2, (11, 7, 15), 4), (3, 1, (9, 9, 17), 8)]


def walk_plan(B, size, units):
    """cvae_conv_up_c1's choice for a bf16 3D launch with c1_walk_units = units (TileC1U<3> 2 x 8 x 16): (walk, segments per z column), or None when it does
    not walk (fewer than 2 x units tiles, or one tile deep)"""
    if not units or len(size) != 3:
        return None
    tiles_d, tiles_h, tiles_w = (size[0] + 1) // 2, (size[1] + 7) // 8, (size[2] + 15) // 16
    ntiles = B * tiles_d * tiles_h * tiles_w
    if ntiles < 2 * units or tiles_d <= 1:
        return None
    walk = min(ntiles // units, tiles_d)
    return walk, (tiles_d + walk - 1) // walk


def test_walking_cases_reach_their_seams():
    """the walking arms really walk: whole columns (one segment), several even segments, and a last segment shorter than the walk"""
    plans = [walk_plan(B, size, w) for nd, B, size, w in C1_UP if w]
    assert None not in plans
    assert (3, 1) in plans and (3, 2) in plans and (2, 3) in plans, plans          # (9, ..): 5 tiles deep in walks of 2: segments of 2, 2, 1


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(C1_UP)))
def test_up_single_channel(i, dt):
    """TileC1U<3> 2x8x16, TileC1U<2> 16x16; walk > 0: up_c1_mfma_walk_kernel with that many units (bf16, 3D)"""
    nd, B, size, walk = C1_UP[i]
    act, bias, masked = variety(i)
    c = c64.make_case("up", 800 + i, nd, B, 1, 32, size, DT[dt], bias=bias, masked=masked)
    walks = dt == "bf16" and walk_plan(B, size, walk) is not None
    assert walks == (dt == "bf16" and walk > 0)
    check(f"up-c1-{dt}" + ("-walk" if walks else ""), c, act, up=(-1, -1, walk) if walk else None)


def test_single_channel_structured():
    check_structured("down-c1-bf16", "down", 3, 2, 1, 32, (6, 18, 72), BF16)
    check_structured("down-c1-f32", "down", 2, 3, 1, 32, (34, 30), F32)
    check_structured("up-c1-bf16", "up", 3, 2, 1, 32, (3, 9, 17), BF16)
    check_structured("up-c1-walk", "up", 3, 2, 1, 32, (6, 9, 17), BF16, up=(-1, -1, 1))
    check_structured("up-c1-walk-segments", "up", 3, 1, 1, 32, (9, 9, 17), BF16, up=(-1, -1, 8))       # walks of 2 over 5 tiles: 3 segments, the last one short
    check_structured("up-c1-f32", "up", 2, 3, 1, 32, (17, 15), F32)


# ------------------------------------------------------------------------------------------------ wgrad
def wgrad_check(family, c, side, s_dtype=None, l_dtype=None):
    ref, err = c64.reference(c, dbias_side=side)
    S, Lt = dev(c["S"], s_dtype or c["dtype"]), dev(c.get("L_dev", c["L"]), l_dtype or c["dtype"])
    wshape = (c["Cs"], c["Cl"], *([4] * c["nd"]))
    out = ops._conv_wgrad(S, Lt, c["nd"], wshape, want_sbias=side == 0, want_lbias=side == 1)
    got = {"dW": out[0], "dbias": out[1]} if side is not None else {"dW": out}
    for k in got:
        print(f"RATIO {family}-{k} {c64.max_ratio(got[k], ref[k], err[k]):.3f}")
    bad = c64.compare(got, ref, err)
    assert not bad, family + ": " + "\n".join(bad)


WGRAD = [  # nd, B, Cl, Cs, small extent, odd_l, dbias_side — Tile<3,128> 4x4x8, Tile<2,128> 8x16
    (3, 2, 32, 64, (4, 4, 8), False, 0), (3, 1, 32, 64, (5, 4, 8), False, 1), (3, 1, 32, 64, (4, 5, 9), False, None), (3, 3, 32, 64, (3, 3, 7), False, 1), (3, 2, 96, 192, (2, 3, 2), False, 0),
    (3, 1, 32, 64, (4, 4, 5), True, 1), (3, 3, 64, 128, (8, 8, 8), False, 1), (3, 1, 128, 256, (2, 2, 2), False, 0), (2, 2, 32, 64, (8, 16), False, 0), (2, 3, 32, 64, (9, 17), False, 1),
    (2, 5, 96, 192, (7, 7), False, 1), (2, 2, 64, 64, (6, 4), True, 1), (2, 1, 32, 64, (2, 3), False, None), (2, 5, 32, 64, (32, 24), False, 0),
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(WGRAD)))
def test_wgrad_own_launch(i, dt):
    nd, B, Cl, Cs, size, odd, side = WGRAD[i]
    wgrad_check(f"wgrad{nd}d-{dt}", c64.make_case("wgrad", 900 + i, nd, B, Cl, Cs, size, DT[dt], odd_l=odd), side)


C1_WGRAD = [  # nd, B, small extent, S dtype, image dtype, side — tile 2x2x32 (3D), 8x16 (2D); bf16 vector form needs lw % 8 == 0
    (3, 2, (2, 2, 32), "f32", "f32", 0), (3, 1, (3, 3, 33), "f32", "f32", 1), (2, 3, (8, 16), "f32", "f32", 0), (3, 2, (2, 2, 32), "bf16", "bf16", 0), (3, 3, (3, 1, 36), "bf16", "bf16", 1),
    (3, 1, (3, 10, 5), "bf16", "bf16", 0), (2, 2, (9, 17), "bf16", "bf16", 1), (2, 3, (14, 14), "bf16", "bf16", 0), (3, 2, (4, 6, 34), "bf16", "f32", 0), (2, 2, (12, 20), "bf16", "f32", 0),
    (3, 1, (2, 3, 3), "bf16", "f32", None),
]


@pytest.mark.parametrize("i", range(len(C1_WGRAD)))
def test_wgrad_single_channel(i):
    nd, B, size, sdt, ldt, side = C1_WGRAD[i]
    c = c64.make_case("wgrad", 1000 + i, nd, B, 1, 32, size, DT[sdt])
    if ldt != sdt:                                           # the fp32 image is rounded to bf16 on the way into LDS
        img = torch.randn(c["L"].shape, generator=torch.Generator().manual_seed(i))
        c["L"], c["L_dev"] = img.to(BF16).float(), img
    wgrad_check(f"wgrad-c1-{sdt}-{ldt}", c, side, l_dtype=DT[ldt])


MULTI = [  # nd, [(B, Cl, Cs, small extent, odd_l, dbias_side or None)]
    (3, [(2, 32, 64, (8, 8, 8), False, 0), (2, 64, 128, (4, 4, 4), False, 1), (2, 128, 256, (2, 2, 2), False, None)]),
    (3, [(1, 96, 192, (2, 3, 2), False, 1), (3, 32, 64, (4, 5, 9), False, 0), (1, 32, 64, (4, 4, 5), True, 0), (2, 64, 64, (3, 3, 7), False, 1), (1, 32, 128, (5, 4, 8), False, None)]),
    (2, [(3, 32, 64, (7, 7), False, 1), (2, 64, 128, (9, 17), False, 0), (5, 96, 192, (3, 8), False, 1), (2, 32, 64, (6, 4), True, 0)]),
    (3, [(2, 32, 64, (4, 4, 9), False, 1), (1, 64, 64, (2, 3, 2), False, 0)]),
    (2, [(1, 32, 64, (8, 16), False, 0), (2, 32, 64, (9, 17), False, 1), (3, 64, 64, (7, 7), False, None), (1, 96, 64, (2, 3), False, 1), (2, 32, 128, (8, 15), False, 0),
         (1, 64, 128, (16, 16), False, 1), (5, 32, 192, (3, 8), False, 0), (2, 32, 64, (6, 4), True, 0)]),
]


def run_multi(nd, cases, sides, dt):
    """one cvae_conv_wgrad_multi call over `cases`; returns the list of {'dW', 'dbias'} results"""
    k = len(cases)
    S, Lt = [dev(c["S"], DT[dt]) for c in cases], [dev(c["L"], DT[dt]) for c in cases]
    dW = [torch.full((c["Cs"], c["Cl"], *([4] * nd)), float("nan"), device=DEV) for c in cases]
    db = [None if s is None else torch.full((c["Cl"] if s else c["Cs"],), float("nan"), device=DEV) for c, s in zip(cases, sides)]
    nb = [L.lib.cvae_conv_wgrad_workspace_bytes(c["Cs"], c["Cl"], nd) for c in cases]
    ws = [torch.empty(n // 4, dtype=F32, device=DEV) for n in nb]
    vp = lambda ts: (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts])
    dims = (C.c_int64 * (9 * k))(*[v for c in cases for v in (c["B"], *c["s_dims"], c["Cs"], *c["l_dims"], c["Cl"])])
    rc = L.lib.cvae_conv_wgrad_multi(k, vp(S), vp(Lt), vp(dW), vp(db), (C.c_int * k)(*[int(s or 0) for s in sides]), vp(ws), (C.c_size_t * k)(*nb), dims, nd,
                                     L.dtype_code(DT[dt]), ops.stream())
    assert rc == 0, L.lib.cvae_strerror(rc)
    torch.cuda.synchronize()
    return [{"dW": dW[j]} if sides[j] is None else {"dW": dW[j], "dbias": db[j]} for j in range(k)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(MULTI)))
def test_wgrad_multi(i, dt):
    """cvae_conv_wgrad_multi: 2 .. 8 (the table's limit) layers of unequal size in one main + one reduce launch, dbias on either side or absent"""
    nd, layers = MULTI[i]
    cases = [c64.make_case("wgrad", 1100 + 10 * i + j, nd, B, Cl, Cs, size, DT[dt], odd_l=odd) for j, (B, Cl, Cs, size, odd, _) in enumerate(layers)]
    sides = [l[5] for l in layers]
    results = run_multi(nd, cases, sides, dt)
    for j, c in enumerate(cases):
        ref, err = c64.reference(c, dbias_side=sides[j])
        got = results[j]
        for key in got:
            print(f"RATIO wgrad-multi{nd}d-{dt}-{key} {c64.max_ratio(got[key], ref[key], err[key]):.3f}")
        bad = c64.compare(got, ref, err)
        assert not bad, f"layer {j}: " + "\n".join(bad)


# ------------------------------------------------------------------------------------------------ fp8
def decode(codes):
    return codes.cpu().view(torch.float8_e4m3fn).float()


FP8 = [  # up, nd, B, Cl, Cs, extent of the input, output ('bf16' / 'codes' / 'dual'), split_k, xpair
    (False, 3, 2, 32, 64, (8, 8, 16), "bf16", True, -1), (False, 3, 1, 128, 256, (8, 8, 8), "dual", True, -1), (False, 3, 1, 128, 256, (8, 8, 8), "dual", False, -1),
    (False, 3, 1, 96, 192, (9, 8, 11), "codes", True, -1), (False, 2, 3, 32, 64, (14, 14), "dual", True, 1), (False, 2, 2, 64, 128, (18, 34), "bf16", True, -1),
    (True, 3, 2, 128, 256, (4, 4, 4), "codes", True, 1), (True, 3, 3, 64, 128, (5, 4, 9), "bf16", True, 0), (True, 3, 1, 32, 64, (4, 9, 8), "dual", True, -1),
    (True, 3, 3, 96, 96, (2, 3, 2), "bf16", True, -1), (True, 2, 2, 32, 64, (17, 15), "codes", True, -1), (True, 2, 3, 64, 128, (7, 7), "dual", True, 1),
]


@pytest.mark.parametrize("i", range(len(FP8)))
def test_conv_fp8(i):
    """The products run on v_mfma_scale_f32_32x32x64_f8f6f4, which truncates each product to 2^-13 of the largest product of its group of 8 (measured:
    tools/probes/mfma_f8_sum_probe.hip): the reference carries that term (conv64, f8_mfma).  Without it case 8 (`up`, 3D, 64 -> 32 channels, S 4 x 9 x 8) had
    1 of 73728 bf16 elements at 1.017 x its bound, and among the elements whose bound is not the bf16 half ulp the fp8 kernels sat at a median of 0.13 - 0.2
    and a maximum of 0.6 - 1.5 of the fp32 bound, where the bf16 kernels reach 0.4 at most."""
    up, nd, B, Cl, Cs, size, out, split_k, xpair = FP8[i]
    act, bias, _ = variety(i)
    act = act if act != "sigmoid" else "relu"
    c = c64.make_case("up" if up else "down", 1200 + i, nd, B, Cl, Cs, size, BF16, bias=bias)
    key = "S" if up else "L"
    x = c[key].abs()
    sx, sw = float(x.max()) / 448.0, float(c["w"].abs().max()) / 448.0
    xq = ops.quantize_fp8(dev(x, BF16), sx)
    wq = ops.pack_weight_fp8(c["w"].to(DEV), nd, up, sw)
    c[key], c["w_ref"] = decode(xq).double() * sx, decode(ops.quantize_fp8(c["w"].to(DEV), sw)).double() * sw      # code x scale, exact in float64
    ref, err, _, _ = c64.reference(c, act, f8_mfma=True)
    so = 0.75 * float(ref.abs().max()) / 448.0                                    # the top quarter of the range saturates
    cout = Cl if up else Cs
    with hooks(split_k, (-1, xpair, 0) if xpair >= 0 else None, None):
        res = ops.conv_fp8(up, xq, wq, dev(c["bias"], F32), cout, nd, act, acc_scale=sx * sw, out8_scale=None if out == "bf16" else so, codes_only=out == "codes")
    y, y8 = (res, None) if out == "bf16" else ((None, res) if out == "codes" else res)
    fam = f"fp8-{'up' if up else 'down'}{nd}d"
    if y is not None:
        report(fam + "-bf16", y, *c64.out_bound(ref, err, "bf16"))
    if y8 is not None:
        report(fam + "-codes", decode(y8) * so, *c64.out_bound(ref, err, "e4m3", so))


@pytest.mark.parametrize("B,size,act", [(2, (2, 8, 16), None), (3, (3, 9, 17), "sigmoid"), (1, (2, 3, 2), None), (2, (6, 7, 15), "relu")])
def test_up_single_channel_from_fp8_codes(B, size, act):
    c = c64.make_case("up", 1300, 3, B, 1, 32, size, BF16)
    sx = float(c["S"].abs().max()) / 448.0
    xq = ops.quantize_fp8(dev(c["S"].abs(), BF16), sx)
    c["S"] = decode(xq).double() * sx
    ref, err, _, _ = c64.reference(c, act)
    got = ops.conv_up_c1_fp8in(xq, c["w"].to(DEV), dev(c["bias"], F32), sx, 3, act)
    report("up-c1-fp8in", got, *c64.out_bound(ref, err, "bf16"))


# ------------------------------------------------------------------------------------------------ structured cases of wgrad and fp8
def exact(family, got, ref, names):
    """integer inputs: every sum is an integer below 2^24, exact in fp32 in ANY order — the result must equal the reference, and a mismatch names (cs, cl, tap..)"""
    g = got.double().cpu().reshape(ref.shape)
    diff = torch.nonzero(g != ref)
    assert diff.numel() == 0, f"{family}: {diff.shape[0]} wrong; first at {names} = {diff[0].tolist()}: got {float(g[tuple(diff[0])])} want {float(ref[tuple(diff[0])])}"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wgrad_structured(dt):
    """S and L both small integers f(b, z, y, x, c) (|v| <= 15: exact in bf16; |sum| <= 225 B positions < 2^24): own launch, grouped launch, Cl == 1"""
    mk = lambda nd, B, Cl, Cs, size, odd=False: c64.make_case("wgrad", 0, nd, B, Cl, Cs, size, DT[dt], structure=True, odd_l=odd)
    for nd, B, Cl, Cs, size, odd, side in [(3, 2, 96, 192, (5, 4, 9), False, 0), (3, 1, 32, 64, (4, 4, 5), True, 1), (2, 3, 96, 192, (9, 17), False, 1), (3, 2, 1, 32, (3, 3, 40), False, 0),
                                           (2, 3, 1, 32, (9, 17), False, 1)]:
        c = mk(nd, B, Cl, Cs, size, odd)
        ref, _ = c64.reference(c, dbias_side=side)
        out = ops._conv_wgrad(dev(c["S"], DT[dt]), dev(c["L"], DT[dt]), nd, (Cs, Cl, *([4] * nd)), want_sbias=side == 0, want_lbias=side == 1)
        exact(f"wgrad{nd}d-{dt} Cl {Cl}", out[0], ref["dW"], "(cs, cl, k..)")
        exact(f"wgrad{nd}d-{dt} Cl {Cl} dbias", out[1], ref["dbias"], "(c)")
    cases = [mk(3, 2, 96, 192, (2, 3, 2)), mk(3, 1, 32, 64, (5, 4, 9)), mk(3, 3, 64, 128, (4, 4, 4))]
    sides = [1, 0, None]
    for c, side, got in zip(cases, sides, run_multi(3, cases, sides, dt)):
        ref, _ = c64.reference(c, dbias_side=side)
        for key in got:
            exact(f"wgrad-multi-{dt} {key}", got[key], ref[key], "(cs, cl, k..)" if key == "dW" else "(c)")


def test_fp8_structured():
    """integers up to 15 and a one-hot weight are exact e4m3 codes (scales 1): every result is ONE input element, exact in bf16 and as a code"""
    for up, nd, B, Cl, Cs, size, kw in [(False, 3, 2, 96, 192, (10, 8, 18), {}), (False, 3, 1, 128, 256, (8, 8, 8), dict(split_k=False)), (False, 2, 3, 96, 192, (18, 14), dict(up=(-1, 1, 0))),
                                        (True, 3, 2, 192, 96, (5, 4, 9), {}), (True, 3, 3, 64, 128, (3, 4, 4), dict(up=(-1, 1, 0))), (True, 3, 2, 96, 64, (5, 9, 8), {}), (True, 2, 3, 96, 64, (9, 7), {})]:
        c = c64.make_case("up" if up else "down", 0, nd, B, Cl, Cs, size, BF16, bias=False, structure=True)
        x = c["S" if up else "L"]
        xq, wq = ops.quantize_fp8(dev(x, BF16), 1.0), ops.pack_weight_fp8(c["w"].to(DEV), nd, up, 1.0)
        assert torch.equal(decode(xq), x)
        ref = c64.reference(c)[0]
        with hooks(kw.get("split_k", True), kw.get("up"), None):
            y, y8 = ops.conv_fp8(up, xq, wq, None, Cl if up else Cs, nd, None, acc_scale=1.0, out8_scale=1.0)
        exact(f"fp8-{'up' if up else 'down'}{nd}d bf16", y, ref, "(b, z, y, x, c)")
        exact(f"fp8-{'up' if up else 'down'}{nd}d codes", decode(y8), ref.float().to(torch.float8_e4m3fn).double(), "(b, z, y, x, c)")     # two inputs meet where Cs > Cl: integers above 16 round
    c = c64.make_case("up", 0, 3, 2, 1, 32, (5, 9, 17), BF16, bias=False, structure=True)
    xq = ops.quantize_fp8(dev(c["S"], BF16), 1.0)
    exact("up-c1-fp8in", ops.conv_up_c1_fp8in(xq, c["w"].to(DEV), None, 1.0, 3, None), c64.reference(c)[0], "(b, z, y, x, c)")
