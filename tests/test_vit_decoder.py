"""GPU tests of the ViT-VAE decoder (csrc/conv_s1.hip, the decoder's fold kinds, causal_vae_amd/vit.ViTVAE): every new kernel against float64 on the same
operands with the local bound c u sum|terms| of tests/vit_decoder_reference.py (c = the products the kernel issues per output + the epilogue's few
operations, u = 2^-24; bf16: float64 on bf16-rounded operands, + 2^-8 |y| for a bf16 result), the whole decoder against the goldens captured from the
reference ViTVAE, and the interface contracts.

Whole decoder, fp32: every collected stage and the image within vit_decoder_reference.composed_bound of the float64 restatement and within twice it of the
fp32 golden.  Whole decoder, bf16: rel-L2 of the 768 x 1280 image against plain float64 at most 2 x the gap between the rounding oracle and plain float64
(the factor allows for accumulation order, as in tests/test_vit_encoder.py).  No fitted tolerance."""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as dr  # noqa: E402
from test_vit_decoder_cpu import CASES, NAMES, reference_state, check_against_golden, subpixel_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
ACTS = {None: lambda v: v, "leaky02": lambda v: F.leaky_relu(v, 0.2), "leaky001": lambda v: F.leaky_relu(v, 0.01)}


def ops():
    from causal_vae_amd import ops as o
    return o


def within(got, ref, err, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = float(((got.detach().cpu().double() - ref).abs() / err).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


def bf16_exact(*shape, seed, scale=1.0):
    """fp32 values that are bf16 numbers: the same operands serve both arithmetic modes and no rounding hides in the packing"""
    return vr.round_bf16(scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def to_cl(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(device=DEV, dtype=dtype)


def gemm_matrix(w, kind, dtype):
    """the kernel's weight matrix through the library's own fold (no BatchNorm: the plain transform) and pack"""
    o = ops()
    (m, _b), = o.fold_bn_conv([(w.to(DEV), kind, None, None)])
    return m if dtype == F32 else o.conv_s1_pack_weights([m])[0]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,B,H,W,act,resid", [(32, 1, 11, 19, "leaky02", False), (32, 3, 8, 16, None, True), (64, 2, 13, 37, None, True),
                                               (64, 1, 5, 3, "leaky001", False), (128, 1, 9, 17, "leaky02", True), (128, 2, 16, 32, None, False)])
def test_conv_s1_k3_against_float64(dtype, C, B, H, W, act, resid):
    o = ops()
    x, w = bf16_exact(B, C, H, W, seed=C + H), bf16_exact(C, C, 3, 3, seed=C + W, scale=0.1)
    b, r = torch.randn(C, generator=torch.Generator().manual_seed(3)), bf16_exact(B, C, H, W, seed=9)
    got = o.conv_s1(to_cl(x, dtype), gemm_matrix(w, o.FOLD_CONV_K3S1, dtype), b.to(DEV), o.CONV_S1_K3, act, resid=to_cl(r, dtype) if resid else None)
    pre = F.conv2d(x.double(), w.double(), b.double(), padding=1) + (r.double() if resid else 0.0)
    terms = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1) + (r.double().abs() if resid else 0.0)
    ref = ACTS[act](pre)
    err = (dr.kernel_terms("res", C) + 6) * vr.U32 * terms + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
    within(got.permute(0, 3, 1, 2), ref, err, f"conv_s1 k3 {dtype} C{C} B{B} {H}x{W} {act} resid={resid}")
    again = o.conv_s1(to_cl(x, dtype), gemm_matrix(w, o.FOLD_CONV_K3S1, dtype), b.to(DEV), o.CONV_S1_K3, act, resid=to_cl(r, dtype) if resid else None)
    assert torch.equal(got, again)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Cin,B,H,W,act,resid", [(32, 1, 11, 19, "leaky001", False), (32, 2, 8, 16, None, True), (16, 3, 13, 21, "leaky001", False),
                                                 (16, 1, 24, 40, "leaky02", True)])
def test_conv_s1_subpixel_against_float64(dtype, Cin, B, H, W, act, resid):
    o = ops()
    x, w = bf16_exact(B, Cin, H, W, seed=Cin + H), bf16_exact(Cin, 16, 3, 3, seed=Cin + W, scale=0.2)
    b, r = torch.randn(16, generator=torch.Generator().manual_seed(4)), bf16_exact(B, 16, 2 * H, 2 * W, seed=10)
    got = o.conv_s1(to_cl(x, dtype), gemm_matrix(w, o.FOLD_CONVT_K3S2_SUBPIXEL, dtype), b.to(DEV), o.CONV_S1_SUBPIXEL, act, resid=to_cl(r, dtype) if resid else None)
    ct = lambda a, ww, bb: F.conv_transpose2d(a, ww, bb, stride=2, padding=1, output_padding=1)
    pre = ct(x.double(), w.double(), b.double()) + (r.double() if resid else 0.0)
    terms = ct(x.double().abs(), w.double().abs(), b.double().abs()) + (r.double().abs() if resid else 0.0)
    ref = ACTS[act](pre)
    err = (dr.kernel_terms("up", Cin) + 6) * vr.U32 * terms + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
    within(got.permute(0, 3, 1, 2), ref, err, f"conv_s1 subpixel {dtype} Cin{Cin} B{B} {H}x{W} {act} resid={resid}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,H,W,act", [(1, 7, 12, None), (3, 9, 10, "leaky02"), (2, 32, 64, "leaky001")])
def test_conv_s1_c1_against_float64(dtype, B, H, W, act):
    """The weight is NOT bf16-exact: in bf16 mode the kernel rounds it on its way into LDS, and the float64 reference uses the rounded weight."""
    o = ops()
    x = bf16_exact(B, 16, H, W, seed=H)
    w = 0.3 * torch.randn(1, 16, 3, 3, generator=torch.Generator().manual_seed(W))
    assert not torch.equal(w, vr.round_bf16(w))
    b = torch.tensor([0.37])
    got = o.conv_s1_c1(to_cl(x, dtype), w.to(DEV), b.to(DEV), act)
    wd = (vr.round_bf16(w) if dtype == BF16 else w).double()
    ref = ACTS[act](F.conv2d(x.double(), wd, b.double(), padding=1))
    err = (144 + 3) * vr.U32 * F.conv2d(x.double().abs(), wd.abs(), b.double().abs(), padding=1)
    assert got.dtype == F32
    within(got, ref, err, f"conv_s1_c1 {dtype} B{B} {H}x{W} {act}")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_conv_s1_k3_zero_padded_columns_do_not_leak_non_finite_values(dtype):
    """C = 32 pads K from 288 to 320: the padded products must be exact zeros, so an Inf activation reaches only the outputs whose window holds it."""
    o = ops()
    x, w = bf16_exact(1, 32, 12, 20, seed=1), bf16_exact(32, 32, 3, 3, seed=2, scale=0.1)
    x[0, 5, 6, 9] = float("inf")
    got = o.conv_s1(to_cl(x, dtype), gemm_matrix(w, o.FOLD_CONV_K3S1, dtype), torch.zeros(32).to(DEV), o.CONV_S1_K3, None).permute(0, 3, 1, 2).cpu().float()
    bad = ~torch.isfinite(got)
    window = torch.zeros_like(bad)
    window[:, :, 5:8, 8:11] = True
    assert bool(bad.any()) and not bool((bad & ~window).any())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("K,B,P", [(128, 1, 6), (128, 19, 6), (512, 4, 80), (32, 3, 5)])
def test_latent_to_grid_against_float64(dtype, K, B, P):
    o = ops()
    g = torch.Generator().manual_seed(K + B)
    z, W, b = torch.randn(B, K, generator=g), torch.randn(256 * P, K, generator=g) * 0.1, torch.randn(256 * P, generator=g)
    got = o.latent_to_grid(z.to(DEV), W.to(DEV), b.to(DEV), 256, dtype)
    ref = (z.double() @ W.double().T + b.double()).view(B, 256, P).transpose(1, 2)
    err = (K + 2) * vr.U32 * (z.double().abs() @ W.double().abs().T + b.double().abs()).view(B, 256, P).transpose(1, 2)
    err = err + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
    within(got, ref, err, f"latent_to_grid {dtype} K{K} B{B} P{P}")
    one = o.latent_to_grid(z[B - 1:].to(DEV), W.to(DEV), b.to(DEV), 256, dtype)                    # a row's bits do not depend on the rows it travels with
    assert torch.equal(one[0], got[B - 1])


def seeded_bn(c, seed):
    bn = nn.BatchNorm2d(c)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(c, generator=g)); bn.bias.copy_(0.1 * torch.randn(c, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(c, generator=g)); bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
    return bn.to(DEV).eval()


def test_decoder_fold_kinds_against_float64():
    o = ops()
    torch.manual_seed(3)
    ct, ct2, cv = nn.ConvTranspose2d(64, 32, 3, 2, 1, 1).to(DEV), nn.ConvTranspose2d(32, 16, 3, 2, 1, 1).to(DEV), nn.Conv2d(32, 32, 3, 1, 1).to(DEV)
    bns = seeded_bn(32, 1), seeded_bn(16, 2), seeded_bn(32, 3)
    with torch.no_grad():
        (w4, b4), (ms, bs), (mk, bk) = o.fold_bn_conv([(ct.weight, o.FOLD_CONVT_K3S2, ct.bias, bns[0]), (ct2.weight, o.FOLD_CONVT_K3S2_SUBPIXEL, ct2.bias, bns[1]),
                                                        (cv.weight, o.FOLD_CONV_K3S1, cv.bias, bns[2])])
    scale = lambda bn: (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu()
    tol = lambda want: 3 * vr.U32 * float(want.abs().max())
    # zero-embedded transposed k4 weight, scaled per Cout (dimension 1); the embedded row and column are exact zeros
    want = torch.zeros(64, 32, 4, 4, dtype=torch.float64)
    want[:, :, :3, :3] = ct.weight.detach().double().cpu() * scale(bns[0])[None, :, None, None]
    assert w4.shape == (64, 32, 4, 4) and float((w4.cpu().double() - want).abs().max()) <= tol(want)
    assert float(w4[:, :, 3].abs().max()) == 0.0 and float(w4[:, :, :, 3].abs().max()) == 0.0
    for bn, conv, bo in ((bns[0], ct, b4), (bns[1], ct2, bs), (bns[2], cv, bk)):
        wb = (conv.bias.detach().double().cpu() - bn.running_mean.double().cpu()) * scale(bn) + bn.bias.detach().double().cpu()
        assert float((bo.cpu().double() - wb).abs().max()) <= 4 * vr.U32 * float(wb.abs().max() + 1)
    # sub-pixel matrix [4 Cout][KT = 128]: the layout of test_vit_decoder_cpu.subpixel_matrix, zeros where a parity has no tap
    want = subpixel_matrix(ct2.weight.detach().double().cpu() * scale(bns[1])[None, :, None, None])
    assert ms.shape == (64, 128) and float((ms.cpu().double() - want).abs().max()) <= tol(want)
    assert torch.equal(ms.cpu() == 0, want == 0)
    # 3 x 3 matrix [Cout][KT = 320]: k = (ky 3 + kx) Cin + ci, 32 zero columns behind
    want = torch.zeros(32, 320, dtype=torch.float64)
    want[:, :288] = (cv.weight.detach().double().cpu() * scale(bns[2])[:, None, None, None]).permute(0, 2, 3, 1).reshape(32, 288)
    assert mk.shape == (32, 320) and float((mk.cpu().double() - want).abs().max()) <= tol(want) and float(mk[:, 288:].abs().max()) == 0.0
    # the zero-embedded weight through cvae_conv_up computes the k3 transposed conv
    with torch.no_grad():
        x = torch.randn(2, 64, 6, 9, device=DEV)
        y = o.ConvUp.apply(x.permute(0, 2, 3, 1).contiguous().view(2, 1, 6, 9, 64), w4, b4, 2, "leaky001", False, False, None)
    w3 = ct.weight.detach().double().cpu() * scale(bns[0])[None, :, None, None]
    t = lambda a, ww, bb: F.conv_transpose2d(a, ww, bb, stride=2, padding=1, output_padding=1)
    ref = F.leaky_relu(t(x.double().cpu(), w3, b4.double().cpu()), 0.01)
    err = (16 * 64 + 5) * vr.U32 * t(x.double().cpu().abs(), w3.abs(), b4.double().cpu().abs())
    within(y.view(2, 12, 18, 32).permute(0, 3, 1, 2), ref, err, "ConvTranspose2d k3 op1 as zero-embedded k4 + leaky001")


def build(golden, name, dtype=F32):
    g = golden(name)
    model, sd, z, grid = reference_state(g)
    return g, model.to(DEV).eval().set_compute_dtype(dtype), sd, z, grid


def collected(model, z):
    col = {}
    image, _saved = model._decode_walk(z.to(DEV), save=False, collect=col)
    got = {"grid": col["grid"].permute(0, 3, 1, 2), "image": image}
    got.update({f"stage{i}": s.permute(0, 3, 1, 2) for i, s in enumerate(col["stages"])})
    assert len(col["stages"]) == 8
    return got


@pytest.mark.parametrize("name", CASES)
def test_whole_decoder_fp32_every_stage(golden, name):
    g, model, sd, z, grid = build(golden, name)
    got = collected(model, z)
    bound, ref = dr.composed_bound(sd, z, grid, key=name)
    for k in NAMES:
        ratio = vr.fro_ratio(got[k], ref[k], bound[k])
        print(f"{name} {k}: ||HIP fp32 - float64|| / bound = {ratio:.2e} (rel-L2 {vr.rel_l2(got[k].cpu(), ref[k]):.3e})")
        assert ratio <= 1.0, (k, ratio)
        if g.has("out/" + k):
            assert vr.fro_ratio(got[k], g.t("out/" + k).double(), 2 * bound[k]) <= 1.0, (k, "against the fp32 golden")
    check_against_golden(g, name, {k: v.cpu() for k, v in got.items()}, bound, ref, factor=2.0)
    assert torch.equal(got["image"], model.decode(z.to(DEV)))                            # two runs: the same bits


def test_whole_decoder_bf16_within_twice_the_rounding_oracle_gap(golden):
    g, model, sd, z, grid = build(golden, CASES[2], BF16)
    plain = dr.decode_ref(sd, z, grid)["image"]
    orac = dr.decode_ref(sd, z, grid, rnd=vr.round_bf16)["image"]
    image = model.decode(z.to(DEV))
    gap, mine = vr.rel_l2(orac, plain), vr.rel_l2(image.cpu(), plain)
    print(f"bf16 image: rounding oracle vs float64 {gap:.3e}; HIP bf16 vs float64 {mine:.3e}; HIP vs oracle {vr.rel_l2(image.cpu(), orac):.3e}")
    assert image.dtype == F32 and mine <= 2.0 * gap, (mine, gap)
    assert torch.equal(image, model.decode(z.to(DEV)))


def test_batch_of_one_equals_row_of_a_batch_of_four(golden):
    g, model, sd, z, grid = build(golden, CASES[1])
    z4 = dr.dec_inputs(4, 128, 77).to(DEV)
    for dt in (F32, BF16):
        model.set_compute_dtype(dt)
        assert torch.equal(model.decode(z4)[:1], model.decode(z4[:1].contiguous())), dt


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_decode_under_graph_capture_equals_eager(golden, dtype):
    g, model, sd, z, grid = build(golden, CASES[1], dtype)
    zd = z.to(DEV)
    eager = model.decode(zd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.decode(zd)                                                                # warm-up on the side stream: allocations, kernel attributes
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.decode(zd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_forward_and_reconstruct_compose_encode_and_decode(golden):
    g, model, sd, z, grid = build(golden, CASES[1])
    x = vr.vit_inputs(2, 256, 320, 31).to(DEV)
    mu, lv = model.encode(x)
    torch.manual_seed(123)
    recons, x_out, mu2, lv2 = model(x)
    torch.manual_seed(123)
    std = torch.exp(0.5 * lv)
    by_hand = model.decode(mu + torch.randn_like(std) * std)
    assert x_out is x and torch.equal(mu, mu2) and torch.equal(lv, lv2) and torch.equal(recons, by_hand)
    assert recons.shape == (2, 1, 256, 320) and recons.dtype == F32
    assert torch.equal(model.reconstruct(x), model.decode(mu))
    assert not torch.equal(recons, model.decode(mu))


def test_train_mode_raises_and_checkpoint_round_trip(golden, tmp_path):
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAE, load_vitvae_state_dict
    g, model, sd, z, grid = build(golden, CASES[0])
    zd = z.to(DEV)
    want = model.decode(zd)
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train().decode(zd)
    model.eval()
    with pytest.raises(CvaeError):
        model.decode(zd[:, :64].contiguous())
    torch.save(model.state_dict(), tmp_path / "vitvae.pt")
    other = ViTVAE(img_size=(64, 96), depth=1)
    assert load_vitvae_state_dict(other, torch.load(tmp_path / "vitvae.pt", map_location="cpu")) == []
    assert torch.equal(other.to(DEV).eval().decode(zd), want)
    assert model.decode(zd[:0]).shape == (0, 1, 64, 96)
