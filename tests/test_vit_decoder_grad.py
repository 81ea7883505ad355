"""GPU tests of the ViT-VAE decoder's latent gradient (csrc/conv_s1.hip's backward entries, the fold's _GRAD kinds, ViTVAE.decode_with_grad / decode_vjp,
vit.fit_latent).

Every new kernel alone against float64 on the same operands and the SAME gate tensor, with the element-wise bound c u sum|terms| of tests/test_vit_decoder.py
(c = the products the kernel issues per output + the epilogue's few operations, u = 2^-24; bf16: bf16-exact operands, + 2^-8 |y| for a bf16 result).

Whole decoder: dz of decode_vjp against the fixed-mask float64 restatement tests/vit_decoder_grad_reference.py with the masks of the HIP forward's own
activations.  fp32: rel-L2 at most 4 x the rel-L2 gap between an fp32 CPU evaluation of the same fixed-mask map and float64 (HIP is another independent fp32
evaluation, with its own accumulation order and 64-element chunks).  bf16: at most 2 x the gap between the rounding oracle and float64.  Nothing fitted."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as dr  # noqa: E402
import vit_decoder_grad_reference as gr  # noqa: E402
from test_vit_decoder_cpu import CASES, reference_state  # noqa: E402
from test_vit_decoder_grad_cpu import cotangent, k3_grad_matrix, subpixel_t_matrix  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SLOPE = {None: 1.0, "leaky02": 0.2, "leaky001": 0.01}


def ops():
    from causal_vae_amd import ops as o
    return o


def within(got, ref, err, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = float(((got.detach().cpu().double() - ref).abs() / err).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


def bf16_exact(*shape, seed, scale=1.0):
    return vr.round_bf16(scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed)))


def gate_like(*shape, seed):
    """an activation output with exact zeros in it (torch's rule gives them the slope)"""
    t = bf16_exact(*shape, seed=seed)
    t[torch.rand(*shape, generator=torch.Generator().manual_seed(seed + 1)) < 0.1] = 0.0
    assert bool((t == 0).any())
    return t


def to_cl(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(device=DEV, dtype=dtype)


def grad_matrix(w, kind, dtype):
    """the backward matrix through the library's own fold (no BatchNorm) and pack"""
    o = ops()
    (_m, _b, mg), = o.fold_bn_conv([(w.to(DEV), kind, None, None)])
    return mg if dtype == F32 else o.conv_s1_pack_weights([mg])[0]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("C,B,H,W", [(32, 1, 11, 19), (64, 2, 13, 37), (128, 1, 8, 16), (32, 3, 8, 16)])
def test_conv_s1_bwd_k3_against_float64(dtype, fused, C, B, H, W):
    o = ops()
    g, w = bf16_exact(B, C, H, W, seed=C + H), bf16_exact(C, C, 3, 3, seed=C + W, scale=0.1)
    r, gate = bf16_exact(B, C, H, W, seed=9), gate_like(B, C, H, W, seed=21)
    act = "leaky02" if C == 64 else "leaky001"
    got = o.conv_s1_bwd_data(to_cl(g, dtype), grad_matrix(w, o.FOLD_CONV_K3S1_GRAD, dtype), o.CONV_S1_K3, resid=to_cl(r, dtype) if fused else None,
                             gate=to_cl(gate, dtype) if fused else None, gate_act=act if fused else None)
    fac = torch.where(gate > 0, 1.0, SLOPE[act]).double() if fused else 1.0
    ref = (F.conv_transpose2d(g.double(), w.double(), padding=1) + (r.double() if fused else 0.0)) * fac
    terms = (F.conv_transpose2d(g.double().abs(), w.double().abs(), padding=1) + (r.double().abs() if fused else 0.0)) * fac
    err = (dr.kernel_terms("res", C) + 6) * vr.U32 * terms + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
    within(got.permute(0, 3, 1, 2), ref, err, f"conv_s1_bwd k3 {dtype} C{C} B{B} {H}x{W} fused={fused}")
    if fused:
        assert bool(((gate == 0) & (ref != 0)).any())                    # zeros in the gate take the slope, not 1 and not 0


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("Cin,B,H,W", [(32, 1, 11, 19), (16, 3, 13, 21), (32, 2, 8, 16)])
def test_conv_s1_bwd_subpixel_t_against_float64(dtype, Cin, B, H, W):
    o = ops()
    g, w = bf16_exact(B, 16, 2 * H, 2 * W, seed=Cin + H), bf16_exact(Cin, 16, 3, 3, seed=Cin + W, scale=0.2)
    gate = gate_like(B, Cin, H, W, seed=33)
    mat = grad_matrix(w, o.FOLD_CONVT_K3S2_SUBPIXEL_GRAD, dtype)
    for act in ("leaky001", None):
        got = o.conv_s1_bwd_data(to_cl(g, dtype), mat, o.CONV_S1_SUBPIXEL_T, cin=Cin, gate=to_cl(gate, dtype) if act else None, gate_act=act)
        fac = torch.where(gate > 0, 1.0, SLOPE[act]).double() if act else 1.0
        ref = F.conv2d(g.double(), w.double(), stride=2, padding=1) * fac
        terms = F.conv2d(g.double().abs(), w.double().abs(), stride=2, padding=1) * fac
        err = (256 + 6) * vr.U32 * terms + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
        within(got.permute(0, 3, 1, 2), ref, err, f"conv_s1_bwd subpixel_t {dtype} Cin{Cin} B{B} {H}x{W} {act}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,H,W", [(1, 7, 12), (3, 9, 10), (2, 32, 64)])
def test_conv_s1_c1_bwd_against_float64(dtype, B, H, W):
    """The cotangent is fp32 and the weight is NOT bf16-exact: in bf16 mode the kernel rounds the weight as the forward does, and so does the reference."""
    o = ops()
    g = cotangent(B, H, W, H)
    w = 0.3 * torch.randn(1, 16, 3, 3, generator=torch.Generator().manual_seed(W))
    gate = gate_like(B, 16, H, W, seed=44)
    got = o.conv_s1_c1_bwd_data(g.to(DEV), w.to(DEV), to_cl(gate, dtype), "leaky001", dtype)
    wd = (vr.round_bf16(w) if dtype == BF16 else w).double()
    fac = torch.where(gate > 0, 1.0, 0.01).double()
    ref = F.conv_transpose2d(g.double(), wd, padding=1) * fac
    err = (9 + 3) * vr.U32 * F.conv_transpose2d(g.double().abs(), wd.abs(), padding=1) * fac + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
    assert got.dtype == dtype
    within(got.permute(0, 3, 1, 2), ref, err, f"conv_s1_c1_bwd {dtype} B{B} {H}x{W}")
    plain = o.conv_s1_c1_bwd_data(g.to(DEV), w.to(DEV), None, None, dtype)
    within(plain.permute(0, 3, 1, 2), ref / fac, err / fac, f"conv_s1_c1_bwd {dtype} B{B} {H}x{W} no gate")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("K,B,P", [(128, 1, 6), (128, 19, 6), (512, 4, 80), (32, 3, 5)])
def test_latent_to_grid_bwd_against_float64(dtype, K, B, P):
    o = ops()
    gen = torch.Generator().manual_seed(K + B)
    g, W = bf16_exact(B, P, 256, seed=K + P), torch.randn(256 * P, K, generator=gen) * 0.1
    got = o.latent_to_grid_bwd(g.to(device=DEV, dtype=dtype), W.to(DEV))
    G = g.double().transpose(1, 2).reshape(B, 256 * P)                   # row c P + p, as nn.Linear's output viewed [B, C, gh, gw]
    ref = G @ W.double()
    err = (256 * P + 2) * vr.U32 * (G.abs() @ W.double().abs())
    assert got.dtype == F32
    within(got, ref, err, f"latent_to_grid_bwd {dtype} K{K} B{B} P{P}")
    one = o.latent_to_grid_bwd(g[B - 1:].contiguous().to(device=DEV, dtype=dtype), W.to(DEV))     # a row's bits do not depend on the rows it travels with
    assert torch.equal(one[0], got[B - 1])
    assert torch.equal(got, o.latent_to_grid_bwd(g.to(device=DEV, dtype=dtype), W.to(DEV)))


def test_grad_fold_kinds_against_float64():
    from causal_vae_amd.vit import ViTVAE
    o = ops()
    torch.manual_seed(3)
    model = ViTVAE(img_size=(64, 64), depth=1)
    dr.randomize_decoder_bn(model.decoder, 5)
    model = model.to(DEV).eval()
    cv, bn_cv, ct, bn_ct, ct2, bn_ct2 = model.decoder[7].conv[0], model.decoder[7].conv[1], model.decoder[12], model.decoder[13], model.decoder[15], model.decoder[16]
    with torch.no_grad():
        table = [(cv.weight, cv.bias, bn_cv), (ct.weight, ct.bias, bn_ct), (ct2.weight, ct2.bias, bn_ct2)]
        grad = o.fold_bn_conv([(w, k, b, bn) for (w, b, bn), k in zip(table, (o.FOLD_CONV_K3S1_GRAD, o.FOLD_CONVT_K3S2_SUBPIXEL_GRAD, o.FOLD_CONVT_K3S2_SUBPIXEL_GRAD))])
        fwd = o.fold_bn_conv([(w, k, b, bn) for (w, b, bn), k in zip(table, (o.FOLD_CONV_K3S1, o.FOLD_CONVT_K3S2_SUBPIXEL, o.FOLD_CONVT_K3S2_SUBPIXEL))])
    for (m, b, _mg), (m0, b0) in zip(grad, fwd):
        assert torch.equal(m, m0) and torch.equal(b, b0)                 # the forward part: the bits of kinds 5 / 6
    scale = lambda bn: (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu()
    tol = lambda want: 3 * vr.U32 * float(want.abs().max())
    s = scale(bn_cv)
    assert float((s - 1).abs().max()) > 0.1                              # non-trivial statistics
    want = torch.zeros(64, 576, dtype=torch.float64)
    want[:, :576] = k3_grad_matrix(cv.weight.detach().double().cpu() * s[:, None, None, None])
    mg = grad[0][2]
    assert mg.shape == (64, 576) and float((mg.cpu().double() - want).abs().max()) <= tol(want)
    for (conv, bn), (_m, _b, mg) in zip(((ct, bn_ct), (ct2, bn_ct2)), grad[1:]):
        want = subpixel_t_matrix(conv.weight.detach().double().cpu() * scale(bn)[None, :, None, None])
        assert mg.shape == (32, 256) and float((mg.cpu().double() - want).abs().max()) <= tol(want)
        assert torch.equal(mg.cpu() == 0, want == 0)


# ---- the whole decoder -----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def whole(golden, name, dtype, B):
    """One HIP pass and its float64 companions per (golden, dtype), shared by the tests below."""
    key = (name, dtype)
    if key in _CACHE:
        return _CACHE[key]
    g = golden(name)
    model, sd, z, grid = reference_state(g)
    model = model.to(DEV).eval().set_compute_dtype(dtype).freeze_decoder()
    z_full = z
    z = z[:B].contiguous()
    assert z.shape[0] == B
    H, W = model.img_height, model.img_width
    cot = cotangent(B, H, W, 71)
    col = {}
    image = model.decode_with_grad(z.to(DEV), collect=col)
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu().double()
    stages = {f"stage{i}": nchw(s) for i, s in enumerate(col["stages"])}
    masks = gr.masks_of(stages, [nchw(y) for y in col["res_inner"]])
    dz = model.decode_vjp(z.to(DEV), cot.to(DEV))
    ref = gr.decode_vjp_ref(sd, cot, grid, masks)
    res = dict(model=model, sd=sd, z=z, z_full=z_full, grid=grid, cot=cot, image=image, stages=stages, masks=masks, dz=dz, ref=ref)
    _CACHE[key] = res
    return res


def fp32_yardstick(r):
    if "yard" not in r:
        r["yard"] = vr.rel_l2(gr.decode_vjp_ref(r["sd"], r["cot"], r["grid"], r["masks"], dtype=F32).double(), r["ref"])
    return r["yard"]


@pytest.mark.parametrize("name,B", [(CASES[0], 2), (CASES[1], 2), (CASES[2], 1)])
def test_whole_decoder_dz_fp32(golden, name, B):
    r = whole(golden, name, F32, B)
    yard, mine = fp32_yardstick(r), vr.rel_l2(r["dz"].cpu().double(), r["ref"])
    print(f"{name} dz fp32: fp32 CPU vs float64 {yard:.3e}; HIP fp32 vs float64 {mine:.3e}; ratio {mine / yard:.2f}")
    assert r["dz"].shape == r["z"].shape and r["dz"].dtype == F32
    assert mine <= 4.0 * yard, (mine, yard)


@pytest.mark.parametrize("name,B", [(CASES[0], 2), (CASES[1], 2), (CASES[2], 1)])
def test_whole_decoder_dz_bf16_within_twice_the_rounding_oracle_gap(golden, name, B):
    r = whole(golden, name, BF16, B)
    orac = gr.decode_vjp_ref(r["sd"], r["cot"], r["grid"], r["masks"], rnd=vr.round_bf16)
    gap, mine = vr.rel_l2(orac, r["ref"]), vr.rel_l2(r["dz"].cpu().double(), r["ref"])
    print(f"{name} dz bf16: rounding oracle vs float64 {gap:.3e}; HIP bf16 vs float64 {mine:.3e}; ratio {mine / gap:.2f}")
    assert mine <= 2.0 * gap, (mine, gap)


@pytest.mark.parametrize("name,B", [(CASES[0], 2), (CASES[1], 2)])
def test_hip_masks_differ_from_float64_only_within_the_bound(golden, name, B):
    """A condition, not a tolerance.  Where the sign of a gate activation differs between the HIP fp32 forward and float64, the two values lie on opposite
    sides of zero, so |h64| <= |h64 - h_hip| <= ||h64 - h_hip||_F <= composed_bound[stage] (the bound tests/test_vit_decoder.py holds the forward to): a flip at
    an element larger than that would be a wrong mask, not rounding.  The ResBlocks' inner activations have no entry in composed_bound and are not
    covered here."""
    r = whole(golden, name, F32, B)
    bound, ref = dr.composed_bound(r["sd"], r["z_full"], r["grid"], key=name)
    flips = 0
    for i in gr.GATES:
        h64 = ref[f"stage{i}"][:B]
        diff = (h64 > 0) != r["masks"][f"stage{i}"]
        flips += int(diff.sum())
        if bool(diff.any()):
            worst = float(h64[diff].abs().max())
            print(f"{name} stage{i}: {int(diff.sum())} of {diff.numel()} signs differ, largest |h64| there {worst:.3e}, bound {bound[f'stage{i}']:.3e}")
            assert worst <= bound[f"stage{i}"], (i, worst)
    print(f"{name}: {flips} gate signs differ between HIP fp32 and float64")


def test_what_the_dz_bound_refuses(golden):
    """The restatement with a wrong ResBlock slope, without the residual path, or shifted by one pixel must fail the comparison the HIP result passes."""
    r = whole(golden, CASES[0], F32, 2)
    yard = fp32_yardstick(r)
    hip = r["dz"].cpu().double()
    assert vr.rel_l2(hip, r["ref"]) <= 4.0 * yard
    for mutate in ("slope", "no_residual", "shift"):
        wrong = gr.decode_vjp_ref(r["sd"], r["cot"], r["grid"], r["masks"], mutate=mutate)
        gap = vr.rel_l2(hip, wrong)
        print(f"{mutate}: rel-L2 of HIP against the wrong restatement / (4 x yardstick) = {gap / (4 * yard):.1f}")
        assert gap > 4.0 * yard, mutate
    assert vr.rel_l2(hip * (1 + 2.0 ** -9), r["ref"]) > 4.0 * yard


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_decode_with_grad_bits(golden, dtype):
    """the image is decode's; backward is decode_vjp's; two runs agree; the saved set is the eight activations of DESIGN §13"""
    r = whole(golden, CASES[0], dtype, 2)
    model, zd, cot = r["model"], r["z"].to(DEV), r["cot"].to(DEV)
    assert torch.equal(r["image"], model.decode(zd))
    zg = zd.clone().requires_grad_(True)
    image = model.decode_with_grad(zg)
    assert image.requires_grad and torch.equal(image, r["image"])
    image.backward(cot)
    assert torch.equal(zg.grad, r["dz"]) and torch.equal(model.decode_vjp(zd, cot), r["dz"])
    _img, (steps, _out_conv, out_gate) = model._decode_walk(zd, save=True)
    gates = [s.gate_in for s in steps[1:]] + [out_gate]                  # entry i: the output of stage i where something downstream is gated by it
    assert [i for i, t in enumerate(gates) if t is not None] == [0, 2, 4, 6, 7] and steps[0].gate_in is None
    assert sum(s.inner is not None for s in steps) == 3 and sum(len(s.mats) for s in steps) == 8 and sum(s.k4 is not None for s in steps) == 3
    with pytest.raises(RuntimeError):
        torch.autograd.grad(model.decode_with_grad(zg).sum(), zg, create_graph=True)[0].sum().backward()      # once differentiable
    assert model.decode_vjp(zd[:0], cot[:0]).shape == (0, 128)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_decode_and_decode_with_grad_agree_at_every_stage(golden, dtype):
    """One walk issues both: the grid, all 8 stage activations and the image of decode and of decode_with_grad are the same bits, not the image alone."""
    r = whole(golden, CASES[0], dtype, 2)
    model, zd = r["model"], r["z"].to(DEV)
    assert CASES[0] == "vitvae_dec_64x96" and zd.shape[0] == 2 and model.compute_dtype == dtype
    plain, grad = {}, {}
    image = model.decode(zd, collect=plain)
    image_g = model.decode_with_grad(zd, collect=grad)
    assert len(plain["stages"]) == 8 and len(grad["stages"]) == 8
    assert torch.equal(plain["grid"], grad["grid"])
    for i, (a, b) in enumerate(zip(plain["stages"], grad["stages"])):
        assert torch.equal(a, b), i
    assert torch.equal(image, image_g)


def test_row_of_a_batch_of_four_equals_the_row_alone(golden):
    r = whole(golden, CASES[1], F32, 2)
    model = r["model"]
    z4, c4 = dr.dec_inputs(4, 128, 77).to(DEV), cotangent(4, 256, 320, 78).to(DEV)
    for dt in (F32, BF16):
        model.set_compute_dtype(dt)
        assert torch.equal(model.decode_vjp(z4, c4)[:1], model.decode_vjp(z4[:1].contiguous(), c4[:1].contiguous())), dt
    model.set_compute_dtype(F32)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_decode_vjp_under_graph_capture_equals_eager(golden, dtype):
    r = whole(golden, CASES[0], dtype, 2)
    model, zd, cot = r["model"], r["z"].to(DEV), r["cot"].to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.decode_vjp(zd, cot)                                        # warm-up on the side stream: allocations, kernel attributes
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.decode_vjp(zd, cot)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, r["dz"])


def test_sse_through_decode_with_grad_and_fit_latent(golden):
    from causal_vae_amd.vit import fit_latent
    o = ops()
    r = whole(golden, CASES[0], F32, 2)
    model, sd, grid = r["model"], r["sd"], r["grid"]
    zstar = r["z"].to(DEV)
    x = model.decode(zstar)
    z0 = (r["z"] + 0.3 * torch.randn(2, 128, generator=torch.Generator().manual_seed(5))).to(DEV)
    # z.grad of sse(decode_with_grad(z), x): the cotangent is 2 (image - x), the map the fixed-mask one with this pass's masks
    zg = z0.clone().requires_grad_(True)
    col = {}
    image = model.decode_with_grad(zg, collect=col)
    loss0 = o.sse(image, x)
    loss0.backward()
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu().double()
    masks = gr.masks_of({f"stage{i}": nchw(s) for i, s in enumerate(col["stages"])}, [nchw(y) for y in col["res_inner"]])
    cot = (2.0 * (image.detach() - x)).cpu()
    ref = gr.decode_vjp_ref(sd, cot, grid, masks)
    yard = vr.rel_l2(gr.decode_vjp_ref(sd, cot, grid, masks, dtype=F32).double(), ref)
    mine = vr.rel_l2(zg.grad.cpu().double(), ref)
    print(f"z.grad of sse: fp32 CPU vs float64 {yard:.3e}; HIP vs float64 {mine:.3e}")
    assert mine <= 4.0 * yard, (mine, yard)
    z0_copy = z0.clone()
    for kind in ("sse", "vessel"):
        z, losses = fit_latent(model, x, z0, steps=20 if kind == "sse" else 3, lr=0.05, loss=kind)
        print(f"fit_latent {kind}: loss {losses[0]:.4e} -> {losses[-1]:.4e}")
        assert z.shape == z0.shape and not z.requires_grad and losses[-1] < losses[0] and torch.equal(z0, z0_copy)
        if kind == "sse":
            assert len(losses) == 20 and losses[0] == float(loss0.detach())       # the first step starts from z0: the gradient checked above
