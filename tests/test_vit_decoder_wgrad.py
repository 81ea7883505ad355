"""GPU tests of the ViT-VAE decoder's weight gradients (csrc/conv_s1.hip's wgrad entries, cvae_fold_bn_conv_bwd, ViTVAE.train_decoder / decode_with_grad,
CausalViTVAE.train_adapters(decoder=True)).

Every new kernel alone against float64 on the same operands, the cotangent already gated with the SAME gate on both sides (a planted exact zero in the gate
takes the slope), element-wise within c u sum|terms| with the c of tests/vit_decoder_wgrad_reference.py's docstring; and with a cotangent that is zero
outside one pixel, where every element of dW is ONE product: a flipped tap or a missing [Cin][Cout] transposition moves it.

Whole decoder at 64 x 96 (a 2 x 3 grid, the smallest the model builds), B = 2 and 3, random running statistics, the masks of the HIP forward's own activations,
per parameter tensor: fp32 rel-L2 from float64 at most 4 x that of the fp32 CPU evaluation of the same restatement; bf16 at most 2 x the rounding-oracle gap.

Ratios measured on an MI355X (worst parameter tensor of each run): see DESIGN §15."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as dr  # noqa: E402
import vit_decoder_grad_reference as gr  # noqa: E402
import vit_decoder_wgrad_reference as wr  # noqa: E402
from test_vit_decoder_cpu import CASES, reference_state  # noqa: E402
from test_vit_decoder_grad_cpu import cotangent  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


def ops():
    from causal_vae_amd import ops as o
    return o


def within(got, ref, err, what):
    assert got.shape == ref.shape and got.dtype == F32, (what, got.shape, ref.shape, got.dtype)
    bad = (got.detach().cpu().double() - ref).abs() > err
    ratio = float(((got.detach().cpu().double() - ref).abs() / err.clamp_min(1e-300)).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert not bool(bad.any()), (what, ratio)


def bf16_exact(*shape, seed, scale=1.0):
    return vr.round_bf16(scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def gated(g, seed, slope):
    """g * act'(gate) with exact zeros planted in the gate (torch's rule gives them the slope), rounded to bf16 ONCE, on the host: both sides read this tensor"""
    gate = bf16_exact(*g.shape, seed=seed)
    gate[torch.rand(*g.shape, generator=torch.Generator().manual_seed(seed + 1)) < 0.1] = 0.0
    assert bool((gate == 0).any())
    return vr.round_bf16(g * torch.where(gate > 0, 1.0, slope))


def to_cl(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(device=DEV, dtype=dtype)


def one_pixel(g, b, y, x):
    out = torch.zeros_like(g)
    out[b, :, y, x] = g[b, :, y, x]
    return out


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C", [16, 128])
@pytest.mark.parametrize("H,W", [(8, 16), (11, 19)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv_s1_wgrad_k3_against_float64(dtype, C, B, H, W):
    """11 x 19: partial tiles and halo on every side, four tiles per sample"""
    o = ops()
    x = bf16_exact(B, C, H, W, seed=C + H)
    g = gated(bf16_exact(B, C, H, W, seed=C + W), seed=5, slope=0.2)
    n = B * H * W
    for what, gg in (("random", g), ("one pixel", one_pixel(g, B - 1, H - 2, W - 3))):
        dW, db = o.conv_s1_wgrad(to_cl(x, dtype), to_cl(gg, dtype), o.CONV_S1_K3)
        ref = conv2d_weight(x.double(), (C, C, 3, 3), gg.double(), padding=1)
        err = (n + 1) * vr.U32 * conv2d_weight(x.double().abs(), (C, C, 3, 3), gg.double().abs(), padding=1)
        within(dW, ref, err, f"conv_s1_wgrad k3 {what} {dtype} C{C} B{B} {H}x{W}")
        within(db, gg.double().sum((0, 2, 3)), n * vr.U32 * gg.double().abs().sum((0, 2, 3)), f"conv_s1_wgrad k3 dbias {what} {dtype} C{C} B{B} {H}x{W}")
        assert float(ref.abs().max()) > 0
    assert torch.equal(dW, o.conv_s1_wgrad(to_cl(x, dtype), to_cl(gg, dtype), o.CONV_S1_K3)[0])      # two runs: the same bits


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Cin", [32, 16])
def test_conv_s1_wgrad_subpixel_against_float64(dtype, Cin):
    """ConvTranspose2d(Cin, 16, 3, 2, 1, output_padding 1): dW [Cin][16][3][3] — Cin = 16 makes a missing channel swap a wrong value, not a wrong shape"""
    o = ops()
    B, H, W = 2, 5, 7
    x = bf16_exact(B, Cin, H, W, seed=Cin)
    g = gated(bf16_exact(B, 16, 2 * H, 2 * W, seed=Cin + 1), seed=9, slope=0.01)
    n = B * H * W
    for what, gg in (("random", g), ("one pixel", one_pixel(g, 1, 2 * H - 1, 4)), ("one pixel, even row", one_pixel(g, 0, 4, 2 * W - 1))):
        dW, db = o.conv_s1_wgrad(to_cl(x, dtype), to_cl(gg, dtype), o.CONV_S1_SUBPIXEL)
        ref = conv2d_weight(gg.double(), (Cin, 16, 3, 3), x.double(), stride=2, padding=1)
        err = (n + 1) * vr.U32 * conv2d_weight(gg.double().abs(), (Cin, 16, 3, 3), x.double().abs(), stride=2, padding=1)
        within(dW, ref, err, f"conv_s1_wgrad subpixel {what} {dtype} Cin{Cin}")
        within(db, gg.double().sum((0, 2, 3)), 4 * n * vr.U32 * gg.double().abs().sum((0, 2, 3)), f"conv_s1_wgrad subpixel dbias {what} {dtype} Cin{Cin}")
        assert float(ref.abs().max()) > 0
    # the reference form itself: autograd through conv_transpose2d
    w = torch.zeros(Cin, 16, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv_transpose2d(x.double(), w, stride=2, padding=1, output_padding=1) * g.double()).sum().backward()
    assert float((w.grad - conv2d_weight(g.double(), (Cin, 16, 3, 3), x.double(), stride=2, padding=1)).abs().max()) <= 1e-9


# ---- more tiles than slabs: a workgroup walks several tiles (the LDS re-stage, MFMA and bias sums carried across tiles, the finish at the slab cap): the path
# every 768 x 1280 layer takes.  Shapes: the smallest that pass the cap (cvae_conv_s1_wgrad: 512 slabs below C = 64, 64 at C = 128; the output conv: 1024
# workgroups x 256 pixels), with partial tiles at the right and bottom.
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,H,W,form", [(16, 196, 340, "k3"), (32, 180, 370, "k3"), (128, 75, 140, "k3"), (16, 196, 340, "sub"), (32, 180, 370, "sub")])
def test_conv_s1_wgrad_walks_several_tiles(dtype, C, H, W, form):
    o = ops()
    sub = form == "sub"
    tiles = ((H + 7) // 8) * ((W + 15) // 16)
    assert tiles > (64 if C == 128 else 512) and H % 8 and W % 16
    x = bf16_exact(1, C, H, W, seed=C + H)
    g = gated(bf16_exact(1, 16, 2 * H, 2 * W, seed=W) if sub else bf16_exact(1, C, H, W, seed=W), seed=6, slope=0.01)
    xd, gd, n = to_cl(x, dtype), to_cl(g, dtype), H * W
    dW, db = o.conv_s1_wgrad(xd, gd, o.CONV_S1_SUBPIXEL if sub else o.CONV_S1_K3)
    if sub:
        ref = conv2d_weight(g.double(), (C, 16, 3, 3), x.double(), stride=2, padding=1)
        terms = conv2d_weight(g.double().abs(), (C, 16, 3, 3), x.double().abs(), stride=2, padding=1)
    else:
        ref = conv2d_weight(x.double(), (C, C, 3, 3), g.double(), padding=1)
        terms = conv2d_weight(x.double().abs(), (C, C, 3, 3), g.double().abs(), padding=1)
    within(dW, ref, (n + 1) * vr.U32 * terms, f"conv_s1_wgrad {form} {tiles} tiles {dtype} C{C} {H}x{W}")
    within(db, g.double().sum((0, 2, 3)), (4 if sub else 1) * n * vr.U32 * g.double().abs().sum((0, 2, 3)), f"conv_s1_wgrad {form} dbias {tiles} tiles {dtype} C{C}")
    again = o.conv_s1_wgrad(xd, gd, o.CONV_S1_SUBPIXEL if sub else o.CONV_S1_K3)
    assert torch.equal(dW, again[0]) and torch.equal(db, again[1])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_conv_s1_c1_wgrad_walks_several_pixels_per_thread(dtype):
    """521 x 517 = 269 357 pixels against 1024 workgroups x 256 threads: the grid-stride walk with the 145 sums carried from pixel to pixel"""
    o = ops()
    B, H, W = 1, 521, 517
    assert B * H * W > 1024 * 256
    x, g = bf16_exact(B, 16, H, W, seed=13), cotangent(B, H, W, 14)
    xd, gd, n = to_cl(x, dtype), g.to(DEV), B * H * W
    dW, db = o.conv_s1_c1_wgrad(xd, gd)
    ref = conv2d_weight(x.double(), (1, 16, 3, 3), g.double(), padding=1)
    within(dW, ref, (n + 1) * vr.U32 * conv2d_weight(x.double().abs(), (1, 16, 3, 3), g.double().abs(), padding=1), f"conv_s1_c1_wgrad {n} pixels {dtype}")
    within(db, g.double().sum().view(1), n * vr.U32 * g.double().abs().sum().view(1), f"conv_s1_c1_wgrad dbias {n} pixels {dtype}")
    again = o.conv_s1_c1_wgrad(xd, gd)
    assert torch.equal(dW, again[0]) and torch.equal(db, again[1])


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_conv_s1_c1_wgrad_against_float64(dtype):
    o = ops()
    B, H, W = 2, 9, 17
    x = bf16_exact(B, 16, H, W, seed=3)
    g = cotangent(B, H, W, 4)
    n = B * H * W
    for what, gg in (("random", g), ("one pixel", one_pixel(g, 1, 0, W - 1))):
        dW, db = o.conv_s1_c1_wgrad(to_cl(x, dtype), gg.to(DEV))
        ref = conv2d_weight(x.double(), (1, 16, 3, 3), gg.double(), padding=1)
        err = (n + 1) * vr.U32 * conv2d_weight(x.double().abs(), (1, 16, 3, 3), gg.double().abs(), padding=1)
        within(dW, ref, err, f"conv_s1_c1_wgrad {what} {dtype}")
        within(db, gg.double().sum().view(1), n * vr.U32 * gg.double().abs().sum().view(1), f"conv_s1_c1_wgrad dbias {what} {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_latent_to_grid_wgrad_against_float64(dtype, B):
    o = ops()
    K, P, C = 512, 6, 256
    g, z = bf16_exact(B, P, C, seed=B), torch.randn(B, K, generator=torch.Generator().manual_seed(B + 1))
    g[0, 0, :7] = 0.0
    dW, db = o.latent_to_grid_wgrad(g.to(device=DEV, dtype=dtype), z.to(DEV))
    G = g.double().transpose(1, 2).reshape(B, C * P)                     # row c P + p, as nn.Linear's output viewed [B, C, gh, gw]
    within(dW, G.T @ z.double(), (B + 1) * vr.U32 * (G.abs().T @ z.double().abs()), f"latent_to_grid_wgrad {dtype} B{B}")
    within(db, G.sum(0), B * vr.U32 * G.abs().sum(0), f"latent_to_grid_wgrad dbias {dtype} B{B}")
    if B == 1:
        assert bool((dW[:7 * P:P] == 0).all()) and bool((dW != 0).any())
    again = o.latent_to_grid_wgrad(g.to(device=DEV, dtype=dtype), z.to(DEV))
    assert torch.equal(dW, again[0]) and torch.equal(db, again[1])


# ---- the whole decoder -----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def whole(golden, dtype, B):
    """One HIP pass with weight gradients and its float64 companions per (dtype, B), shared by the tests below."""
    key = (dtype, B)
    if key in _CACHE:
        return _CACHE[key]
    model, sd, _z, grid = reference_state(golden(CASES[0]))
    sd = {k: v.clone() for k, v in sd.items()}
    model = model.to(DEV).eval().set_compute_dtype(dtype).train_decoder()
    z, cot = dr.dec_inputs(B, 128, 300 + B), cotangent(B, 64, 96, 400 + B)
    col = {}
    model.zero_grad(set_to_none=True)
    zg = z.to(DEV).requires_grad_(True)
    image = model.decode_with_grad(zg, collect=col)
    image.backward(cot.to(DEV))
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu().double()
    stages = {f"stage{i}": nchw(s) for i, s in enumerate(col["stages"])}
    masks = gr.masks_of(stages, [nchw(y) for y in col["res_inner"]])
    names = wr.decoder_param_names(sd)
    grads = {k: dict(model.named_parameters())[k].grad.detach().clone() for k in names}
    res = dict(model=model, sd=sd, z=z, cot=cot, grid=grid, image=image.detach(), dz=zg.grad.clone(), masks=masks, names=names, grads=grads,
               ref=wr.decoder_wgrad_ref(sd, z, cot, grid, masks))
    _CACHE[key] = res
    return res


def fp32_yardstick(r):
    if "yard" not in r:
        cpu = wr.decoder_wgrad_ref(r["sd"], r["z"], r["cot"], r["grid"], r["masks"], dtype=F32)
        r["yard"] = {k: vr.rel_l2(cpu[k].double(), r["ref"][k]) for k in r["names"]}
    return r["yard"]


def check_ratios(r, yard, factor, label, elementwise=None):
    """elementwise: name -> an element-wise bound for a gradient whose yardstick is zero (a ratio to zero says nothing): it must be listed, nothing else may be"""
    worst, elementwise = 0.0, elementwise or {}
    assert sorted(k for k in r["names"] if yard[k] == 0) == sorted(elementwise)
    for k in r["names"]:
        ref, got = r["ref"][k], r["grads"][k].cpu().double()
        assert got.shape == ref.shape and r["grads"][k].dtype == F32 and bool(torch.isfinite(got).all()), k
        assert float(ref.norm()) > 0, k                                  # eval-mode BatchNorm: no db or dbeta is zero in exact arithmetic here
        if k in elementwise:
            worst_el = float(((got - ref).abs() / elementwise[k]).max())
            print(f"{label} {k}: yardstick 0; max |HIP - float64| / element-wise bound = {worst_el:.4f}")
            continue
        mine = vr.rel_l2(got, ref)
        print(f"{label} {k}: yardstick {yard[k]:.3e}; HIP vs float64 {mine:.3e}; ratio {mine / yard[k]:.2f}")
        worst = max(worst, mine / yard[k])
    print(f"{label}: worst ratio {worst:.2f} (allowed {factor})")
    for k in r["names"]:
        got = r["grads"][k].cpu().double()
        if k in elementwise:
            assert bool(((got - r["ref"][k]).abs() <= elementwise[k]).all()), k
        else:
            assert vr.rel_l2(got, r["ref"][k]) <= factor * yard[k], k


@pytest.mark.parametrize("B", [2, 3])
def test_whole_decoder_wgrad_fp32(golden, B):
    r = whole(golden, F32, B)
    check_ratios(r, fp32_yardstick(r), 4.0, f"wgrad fp32 B{B}")


@pytest.mark.parametrize("B", [2, 3])
def test_whole_decoder_wgrad_bf16_within_twice_the_rounding_oracle_gap(golden, B):
    r = whole(golden, BF16, B)
    orac = wr.decoder_wgrad_ref(r["sd"], r["z"], r["cot"], r["grid"], r["masks"], rnd=vr.round_bf16)
    # the output conv's bias gradient is the sum of the fp32 cotangent: no bf16 rounding enters, the oracle's gap is exactly zero, and the kernel is held to
    # cvae_conv_s1_c1_wgrad's own fp32 bound n u sum |g| (tests/vit_decoder_wgrad_reference.py)
    exact = {"decoder.18.bias": r["cot"].numel() * vr.U32 * r["cot"].double().abs().sum().view(1)}
    check_ratios(r, {k: vr.rel_l2(orac[k], r["ref"][k]) for k in r["names"]}, 2.0, f"wgrad bf16 B{B}", exact)


def test_what_the_wgrad_comparison_refuses(golden):
    """The restatement with the 16 -> 16 transposed conv's gradient left unswapped, or with dgamma missing its bias term, must fail the fp32 comparison the
    HIP result passes."""
    r = whole(golden, F32, 2)
    yard = fp32_yardstick(r)
    for mutate, keys in (("no_swap", ["decoder.15.weight", "decoder.16.weight"]), ("no_bias_term", ["decoder.1.weight", "decoder.3.conv.4.weight", "decoder.16.weight"])):
        wrong = wr.decoder_wgrad_ref(r["sd"], r["z"], r["cot"], r["grid"], r["masks"], mutate=mutate)
        for k in keys:
            hip = r["grads"][k].cpu().double()
            assert vr.rel_l2(hip, r["ref"][k]) <= 4.0 * yard[k], k
            gap = vr.rel_l2(hip, wrong[k])
            print(f"{mutate} {k}: rel-L2 of HIP against the wrong restatement / (4 x yardstick) = {gap / (4 * yard[k]):.1f}")
            assert gap > 4.0 * yard[k], (mutate, k)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_bits_and_accumulation(golden, dtype):
    """image = decode's; dz = the frozen path's; two runs agree; .grad after two backward calls is the sum; zero_grad clears"""
    r = whole(golden, dtype, 2)
    model, zd, cot = r["model"], r["z"].to(DEV), r["cot"].to(DEV)
    params = dict(model.named_parameters())
    assert torch.equal(r["image"], model.decode(zd))
    model.zero_grad(set_to_none=True)
    zg = zd.clone().requires_grad_(True)
    model.decode_with_grad(zg).backward(cot)
    assert torch.equal(zg.grad, r["dz"])
    for k in r["names"]:
        assert torch.equal(params[k].grad, r["grads"][k]), k
    model.decode_with_grad(zd).backward(cot)                             # z asks for nothing: the parameters still do
    for k in r["names"]:
        assert torch.equal(params[k].grad, r["grads"][k] + r["grads"][k]), k
    model.zero_grad(set_to_none=True)
    assert all(params[k].grad is None for k in r["names"])
    model.freeze_decoder()
    zf = zd.clone().requires_grad_(True)
    image = model.decode_with_grad(zf)
    image.backward(cot)
    assert torch.equal(image, r["image"]) and torch.equal(zf.grad, r["dz"]) and all(params[k].grad is None for k in r["names"])
    model.train_decoder()
    image = model.decode_with_grad(zd)
    with torch.no_grad():
        params["decoder.18.bias"].add_(1.0)                              # a parameter rewritten between forward and backward: autograd's version check
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        image.backward(cot)
    with torch.no_grad():
        params["decoder.18.bias"].sub_(1.0)
    model.zero_grad(set_to_none=True)


def test_causal_vit_trains_heads_and_decoder():
    from causal_vae_amd.vessel.train import loss_function, total_loss
    from causal_vae_amd.vit import CausalViTVAE
    torch.manual_seed(5)
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    dr.randomize_decoder_bn(model.backbone.decoder, 6)
    model = model.to(DEV)
    params = model.train_adapters(decoder=True)
    gen = torch.Generator().manual_seed(8)
    B = 3
    x = torch.rand(B, 1, 64, 96, generator=gen).to(DEV)
    m, t = torch.randn(B, model.m_dim, generator=gen).to(DEV), torch.randn(B, model.t_dim, generator=gen).to(DEV)
    eps = torch.randn(B, model.my_z_dim, generator=gen).to(DEV)
    seen = {}
    decode_with_grad = model.backbone.decode_with_grad
    model.backbone.decode_with_grad = lambda z: seen.setdefault("image", decode_with_grad(seen.setdefault("z", z)))
    out = model.forward_train(x, m, t, eps=eps)
    out[0].register_hook(lambda g: seen.setdefault("cot", g.clone()))
    total_loss(*loss_function(out[0], x, out[1], m, *out[2:])).backward()              # the vessel loss: recon + kld + morph + sparsity
    del model.backbone.decode_with_grad
    dec = {k: p for k, p in model.backbone.named_parameters() if k.startswith(("decoder_input.", "decoder."))}
    assert len(dec) == 48 and len(params) == len(model.head_parameters()) + 48
    for k, p in list(dec.items()) + [(f"head{i}", p) for i, p in enumerate(model.head_parameters())]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    assert all(p.grad is None for k, p in model.backbone.named_parameters() if k not in dec)
    got = {k: p.grad.clone() for k, p in dec.items()}
    model.zero_grad(set_to_none=True)
    model.backbone.decode_with_grad(seen["z"].detach()).backward(seen["cot"])
    for k, p in dec.items():
        assert torch.equal(p.grad, got[k]), k
