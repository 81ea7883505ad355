"""GPU tests of the ViT-VAE encoder (csrc/vit.hip, causal_vae_amd/vit): every kernel against float64 on the same operands with the local bounds of
tests/vit_reference.py (c u sum|terms|, c = accumulation length, u = 2^-24; bf16: float64 on bf16-rounded operands, + 2^-8 |y| for a bf16 result, + 2 x 2^-8
p|v| for the rounding of P), the whole model against the goldens captured from the reference ViTVAE, and the interface contracts.

Whole model, fp32: every stage within vit_reference.composed_bound of the float64 restatement (the per-layer fp32 bounds composed over depth: Jacobian
action, worst-case magnitudes, independent signs, three sigma; relative size 2e-4 .. 1e-3, stem 6.5e-3), and within twice that bound of the fp32 golden
(two fp32 evaluations, each inside the bound of the same float64 value).  No fitted tolerance is left.
Whole model, bf16: rel-L2 of mu and cls_out against plain float64 at most 2 x the gap between the rounding oracle (float64 with bf16 rounding at the kernels'
rounding points) and plain float64 on the 961-token case; the factor allows for accumulation order.  Oracle gap measured on the CPU: mu 1.05e-3, cls_out
1.06e-3 (printed by test_rounding_oracle_gap_is_what_the_gpu_test_uses); HIP bf16 vs float64 on the MI355X: 1.08e-3 / 1.07e-3."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


def ops():
    from causal_vae_amd import ops as o
    return o


def operands(dtype, *shapes, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ts = [scale * torch.randn(*s, generator=g) for s in shapes]
    return [t.to(dtype) for t in ts]


def within(got, ref, err, what):
    ratio = float(((got.detach().cpu().double() - ref).abs() / err).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layernorm_against_float64(dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(333, 256, generator=g) * 3 + 0.7
    gam, bet = torch.randn(256, generator=g), torch.randn(256, generator=g)
    y = ops().layernorm256(x.to(DEV), gam.to(DEV), bet.to(DEV), 1e-5, dtype)
    ref, err = vr.layernorm_b(x.double(), torch.zeros(333, 256, dtype=torch.float64), gam.double(), bet.double(), 1e-5, out_u=vr.UBF if dtype == BF16 else 0.0)
    within(y, ref, err, f"layernorm {dtype}")
    xs = torch.randn(5, 7, 256, generator=g).to(DEV)                       # strided rows: the CLS rows of a [B, N, 256] stream
    assert torch.equal(ops().layernorm256(xs[:, 0], gam.to(DEV), bet.to(DEV), 1e-5, dtype), ops().layernorm256(xs[:, 0].contiguous(), gam.to(DEV), bet.to(DEV), 1e-5, dtype))


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("K,N,epi", [(256, 768, None), (256, 256, "residual"), (256, 512, "gelu"), (512, 256, "residual"), (256, 512, None)])
def test_token_gemm_against_float64(dtype, K, N, epi):
    M = 3 * 81 + 5
    (x,) = operands(dtype, (M, K), seed=K + N)
    W, b, res = operands(F32, (N, K), (N,), (M, N), seed=7, scale=0.2)
    got = ops().token_gemm(x.to(DEV), W.to(DEV), b.to(DEV), epi, resid=res.to(DEV).clone() if epi == "residual" else None)
    Wd = (vr.round_bf16(W) if dtype == BF16 else W).double()
    out_u = vr.UBF if (dtype == BF16 and epi != "residual") else 0.0
    ref, err = vr.linear_b(x.double(), torch.zeros(M, K, dtype=torch.float64), Wd, b.double())
    if epi == "gelu":
        ref, err = vr.gelu_b(ref, err)
    if epi == "residual":
        ref, err = ref + res.double(), err + vr.U32 * (ref + res.double()).abs()
    err = err + out_u * (ref.abs() + err)
    within(got, ref, err, f"token_gemm {dtype} K{K} N{N} {epi}")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("N,nq", [(81, None), (241, None), (961, None), (100, None), (961, 1)])
def test_attention_against_float64(dtype, N, nq):
    B = 2
    (qkv,) = operands(dtype, (B, N, 768), seed=N, scale=1.5)
    d = qkv.to(DEV)
    got = ops().mhsa(d[:, :, :256], d[:, :, 256:512], d[:, :, 512:], n_query_rows=nq)
    q, k, v = qkv.double().split(256, dim=-1)
    z = torch.zeros_like(k)
    bf = dtype == BF16
    ref, err = vr.attention_b(q, z, k, z, v, z, n_query_rows=nq, rnd=vr.round_bf16 if bf else None, p_u=vr.UBF if bf else 0.0, out_u=vr.UBF if bf else 0.0)
    assert got.shape == ref.shape
    within(got, ref, err, f"attention {dtype} N{N} nq{nq}")
    assert torch.equal(got, ops().mhsa(d[:, :, :256], d[:, :, 256:512], d[:, :, 512:], n_query_rows=nq))          # fixed-order sums: same bits


def test_fold_k3s2_and_leaky001_against_float64():
    import torch.nn as nn
    import torch.nn.functional as F
    from causal_vae_amd import ops as o
    torch.manual_seed(3)
    conv, bn = nn.Conv2d(32, 64, 3, 2, 1), nn.BatchNorm2d(64)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.1); bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5)
    conv, bn = conv.to(DEV), bn.to(DEV).eval()
    with torch.no_grad():
        (w4, b4), = o.fold_bn_conv([(conv.weight, o.FOLD_CONV_K3S2, conv.bias, bn)])
        s = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu()
        want = torch.zeros(64, 32, 4, 4, dtype=torch.float64)
        want[:, :, :3, :3] = conv.weight.double().cpu() * s[:, None, None, None]
        assert w4.shape == (64, 32, 4, 4) and float((w4.cpu().double() - want).abs().max()) <= 3 * vr.U32 * float(want.abs().max())
        assert float(w4[:, :, 3].abs().max()) == 0.0 and float(w4[:, :, :, 3].abs().max()) == 0.0
        x = torch.randn(2, 32, 16, 24, device=DEV)
        y = o.ConvDown.apply(x.permute(0, 2, 3, 1).contiguous().view(2, 1, 16, 24, 32), w4, b4, 2, "leaky001", False, False, None)
        ref = F.leaky_relu(F.conv2d(x.double().cpu(), want[:, :, :3, :3], b4.double().cpu(), stride=2, padding=1), 0.01)
        err = (16 * 32 + 5) * vr.U32 * F.conv2d(x.double().cpu().abs(), want[:, :, :3, :3].abs(), b4.double().cpu().abs(), stride=2, padding=1)
        within(y.view(2, 8, 12, 64).permute(0, 3, 1, 2), ref, err, "stem layer k3s2 + leaky001")


def build(golden, name, dtype=F32):
    from test_vit_reference_cpu import reference_state
    g = golden(name)
    model, sd, x, depth = reference_state(g)
    return g, model.to(DEV).eval().set_compute_dtype(dtype), sd, x, depth


def fp32_checks(g, name, got, sd, x, depth):
    bound, ref = vr.composed_bound(sd, x, depth, key=name)
    for k, v in got.items():
        ratio = vr.fro_ratio(v, ref[k], bound[k])
        print(f"{name} {k}: ||HIP fp32 - float64|| / bound = {ratio:.2e} (rel-L2 {vr.rel_l2(v.cpu(), ref[k]):.3e})")
        assert ratio <= 1.0, (k, ratio)
        if g.has("out/" + k):
            assert vr.fro_ratio(v, g.t("out/" + k).double(), 2 * bound[k]) <= 1.0, (k, "against the fp32 golden")
        else:
            g.check("out", k, v, rtol=2 * bound[k] / float(ref[k].norm()), atol=2 * bound[k] / 20)      # digest: as in tests/test_vit_reference_cpu.py


def test_small_model_every_stored_intermediate(golden):
    name = "vitvae_enc_256x320"
    g, model, sd, x, depth = build(golden, name)
    model._cls_only_last_block = False
    col = {}
    cls_out = model._cls_features(x.to(DEV), collect=col)
    mu, lv = model.encode(x.to(DEV))
    B = x.shape[0]
    got = {"stem": col["stem"].view(B, 8, 10, 256).permute(0, 3, 1, 2), "cls_out": cls_out, "mu": mu, "log_var": lv}
    got.update({f"tokens{i}": col["tokens"][i] for i in range(depth)})
    got.update({f"cls_row{i}": col["cls_rows"][i] for i in range(depth)})
    fp32_checks(g, name, got, sd, x, depth)


def test_large_model_fp32_against_golden_and_cls_only_equals_full(golden):
    name = "vitvae_enc_768x1280"
    g, model, sd, x, depth = build(golden, name)
    xd = x.to(DEV)
    col = {}
    cls_out = model._cls_features(xd, collect=col)
    mu, lv = model.encode(xd)
    assert len(col["tokens"]) == depth - 1                                      # the last block ran for the CLS row only
    assert torch.equal(cls_out, model.cls_features(xd))
    got = {"cls_out": cls_out, "mu": mu, "log_var": lv}
    got.update({f"cls_row{i}": col["cls_rows"][i] for i in range(depth)})
    fp32_checks(g, name, got, sd, x, depth)
    mu2, lv2 = model.encode(xd)
    assert torch.equal(mu, mu2) and torch.equal(lv, lv2)                        # two runs: the same bits
    model._cls_only_last_block = False
    mu_full, lv_full = model.encode(xd)
    assert torch.equal(mu, mu_full) and torch.equal(lv, lv_full)                # CLS-only last block == full last block on the CLS row, bit for bit


def test_large_model_bf16_within_twice_the_rounding_oracle_gap(golden):
    g, model, sd, x, depth = build(golden, "vitvae_enc_768x1280", BF16)
    plain = vr.flat(vr.encode_ref(sd, x, depth), depth)
    orac = vr.flat(vr.encode_ref(sd, x, depth, rnd=vr.round_bf16), depth)
    xd = x.to(DEV)
    cls_out = model.cls_features(xd)
    mu, lv = model.encode(xd)
    for k, v in (("mu", mu), ("cls_out", cls_out)):
        gap, mine = vr.rel_l2(orac[k], plain[k]), vr.rel_l2(v.cpu(), plain[k])
        print(f"bf16 {k}: rounding oracle vs float64 {gap:.3e}; HIP bf16 vs float64 {mine:.3e}; HIP vs oracle {vr.rel_l2(v.cpu(), orac[k]):.3e}")
        assert mine <= 2.0 * gap, (k, mine, gap)
    assert torch.equal(mu, model.encode(xd)[0])
    model._cls_only_last_block = False
    assert torch.equal(mu, model.encode(xd)[0])


def test_batch_of_one_equals_row_of_a_batch_of_four(golden):
    """Bit-equal, both dtypes: every transformer kernel computes a row from that row's operands alone in a fixed order (its tile geometry does not depend
    on the batch), and the conv launch layer's tile forms — which may differ between B = 1 and B = 4 — compute the same products in the same order
    (include/cvae_hip.h).  Zero is inside any fp32 bound."""
    g, model, sd, x, depth = build(golden, "vitvae_enc_256x320")
    x4 = vr.vit_inputs(4, 256, 320, 77).to(DEV)
    for dt in (F32, BF16):
        model.set_compute_dtype(dt)
        mu4, lv4 = model.encode(x4)
        mu1, lv1 = model.encode(x4[:1].contiguous())
        assert torch.equal(mu4[:1], mu1) and torch.equal(lv4[:1], lv1), dt


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_token_assembly_equals_torch(dtype):
    (stem,) = operands(dtype, (3, 1, 4, 5, 256), seed=4)
    cls, pos = operands(F32, (1, 1, 256), (21, 256), seed=5)
    got = ops().vit_tokens(stem.to(DEV), cls.to(DEV), pos.to(DEV))
    want = torch.cat([cls.expand(3, -1, -1), stem.float().view(3, 20, 256)], dim=1) + pos          # one fp32 add per element: exact agreement
    assert got.dtype == F32 and torch.equal(got.cpu(), want)


def test_training_mode_and_unsupported_shapes_raise_before_any_launch(golden):
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAEEncoder
    m = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=16).to(DEV)
    x = torch.zeros(2, 1, 64, 96, device=DEV)
    with pytest.raises(RuntimeError, match="eval mode"):
        m.train().encode(x)
    m.eval()
    with pytest.raises(CvaeError):
        m.encode(torch.zeros(2, 1, 64, 128, device=DEV))
    with pytest.raises(CvaeError):
        m.encode(torch.zeros(2, 3, 64, 96, device=DEV))
    with pytest.raises(CvaeError):
        ops().token_gemm(torch.zeros(8, 128, device=DEV), torch.zeros(256, 128, device=DEV), torch.zeros(256, device=DEV))
    assert m.encode(x)[0].shape == (2, 16)


def test_load_full_checkpoint_and_extract_latents():
    import torch.nn as nn
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAEEncoder, extract_vit_latents, load_vitvae_state_dict
    torch.manual_seed(11)
    src = ViTVAEEncoder(img_size=(128, 160), depth=2, latent_dim=32)
    vr.randomize_stem_bn(src.stem, 5)

    class Full(nn.Module):                                       # a full checkpoint's keys: the encoder's + decoder_input.* + decoder.*
        def __init__(self):
            super().__init__()
            self.decoder_input = nn.Linear(32, 64)
            self.decoder = nn.Sequential(nn.ConvTranspose2d(8, 4, 3, 2, 1, 1), nn.BatchNorm2d(4))
    full = {**src.state_dict(), **Full().state_dict()}
    dst = ViTVAEEncoder(img_size=(128, 160), depth=2, latent_dim=32)
    dropped = load_vitvae_state_dict(dst, full)
    assert dropped and all(k.startswith(("decoder_input.", "decoder.")) for k in dropped) and len(dropped) == len(Full().state_dict())
    for k, v in src.state_dict().items():
        assert torch.equal(v, dst.state_dict()[k]), k
    with pytest.raises(CvaeError):
        load_vitvae_state_dict(dst, {**full, "stray.weight": torch.zeros(1)})
    half = ViTVAEEncoder(img_size=(64, 96), depth=2, latent_dim=32)                # another grid (4 x 5 -> 2 x 3): the position embedding is resized
    with pytest.raises(CvaeError, match="src_grid"):
        load_vitvae_state_dict(half, full)
    load_vitvae_state_dict(half, full, src_grid=(4, 5))
    assert half.pos_embedding.shape == (1, 7, 256) and torch.equal(half.pos_embedding[:, 0], src.pos_embedding[:, 0])
    assert half.eval().to(DEV).encode(vr.vit_inputs(1, 64, 96, 9).to(DEV))[0].shape == (1, 32)
    dst = dst.to(DEV).eval()
    xs = [vr.vit_inputs(2, 128, 160, 20 + i) for i in range(3)]
    lat = extract_vit_latents(dst, [{"x": x} for x in xs], DEV)
    assert isinstance(lat, np.ndarray) and lat.shape == (6, 32)
    for i, x in enumerate(xs):
        assert np.array_equal(lat[2 * i:2 * i + 2], dst.encode(x.to(DEV))[0].cpu().numpy())
