"""CPU tests of the yardstick of tests/test_vit_encoder_grad.py (tests/vit_encoder_grad_reference.py) and of the mode switches that need no GPU.

The float64 restatement of the transformer's vector-Jacobian product equals torch.autograd through the model's own nn.MultiheadAttention / nn.LayerNorm /
nn.Linear modules (eval mode, composed as the reference's ViTBlock.forward composes them) to 1e-12 of each tensor's largest element, with and without the
CLS-only last block.  What the yardstick refuses: two deliberately wrong restatements miss the fp32 comparison (rel-L2 from float64 at most 4 x that of the
fp32 evaluation) by the factors recorded in test_the_yardstick_refuses_wrong_restatements.  The k bias (zero in exact arithmetic) of the fp32 evaluation sits
inside its element-wise bound."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_encoder_grad_reference as gr  # noqa: E402

F64 = torch.float64


def make(img, cls=None, seed=0):
    from causal_vae_amd.vit.models import ViTVAE, ViTVAEEncoder
    torch.manual_seed(seed)
    return (cls or ViTVAEEncoder)(img_size=img, depth=2, latent_dim=128).eval()


def autograd_side(model, stem, gm, gl, cls_only):
    """mu, log_var and their gradients through the model's own torch modules in float64, composed as ViTBlock.forward (x = x + attn(norm1(x)); x = x + mlp(norm2(x)))"""
    m = model.double()
    B = stem.shape[0]
    t = torch.cat([m.cls_token.expand(B, -1, -1), stem], 1) + m.pos_embedding
    for i, blk in enumerate(m.transformer):
        y = blk.norm1(t)
        if cls_only and i == m.depth - 1:
            t = t[:, :1] + blk.attn(y[:, :1], y, y, need_weights=False)[0]
        else:
            t = t + blk.attn(y, y, y, need_weights=False)[0]
        t = t + blk.mlp(blk.norm2(t))
    c = m.to_latent(t[:, 0])
    mu, lv = m.fc_mu(c), m.fc_var(c)
    named = m._transformer_named()
    return dict(zip([k for k, _p in named], torch.autograd.grad([mu, lv], [p for _k, p in named], [gm, gl]))), mu, lv


def case(img, cls_only, B=3):
    model = make(img)
    g = torch.Generator().manual_seed(3)
    Np = (img[0] // 32) * (img[1] // 32)
    stem = torch.randn(B, Np, 256, generator=g, dtype=F64)
    gm, gl = torch.randn(B, 128, generator=g, dtype=F64), torch.randn(B, 128, generator=g, dtype=F64)
    return model, stem, gm, gl


@pytest.mark.parametrize("cls_only", [False, True])
@pytest.mark.parametrize("img", [(64, 96), (256, 320)])
def test_restatement_equals_autograd_in_float64(img, cls_only):
    model, stem, gm, gl = case(img, cls_only)
    assert stem.shape[1] + 1 in (7, 81)
    want, mu, lv = autograd_side(model, stem, gm, gl, cls_only)
    got, out = gr.transformer_vjp(model.state_dict(), stem, 2, gm, gl, cls_only_last=cls_only)
    assert float((out["mu"] - mu).abs().max()) <= 1e-12 * float(mu.abs().max()) and float((out["log_var"] - lv).abs().max()) <= 1e-12 * float(lv.abs().max())
    for k, w in want.items():
        err = float((got[k] - w).abs().max()) / float(w.abs().max())
        assert err <= 1e-12, (k, err)


def test_the_yardstick_refuses_wrong_restatements():
    """dk formed from P instead of dS, and dgamma without xhat: each misses the fp32 rule on the tensors it touches by the factor printed here.
    Recorded (81 tokens, B = 3, depth 2): dk from P: transformer.0.attn.in_proj_weight 1.3e+07 x the allowance; dgamma without xhat: transformer.0.norm1.weight 2.6e+06 x."""
    model, stem, gm, gl = case((256, 320), False)
    sd = model.state_dict()
    r64 = gr.transformer_vjp(sd, stem, 2, gm, gl)[0]
    r32 = gr.transformer_vjp(sd, stem, 2, gm, gl, dtype=torch.float32)[0]
    for wrong, key in (("dk_from_p", "transformer.0.attn.in_proj_weight"), ("dgamma_no_xhat", "transformer.0.norm1.weight")):
        bad = gr.transformer_vjp(sd, stem, 2, gm, gl, wrong=wrong)[0]
        allowance = 4 * gr.rel_l2(r32[key], r64[key])
        factor = gr.rel_l2(bad[key], r64[key]) / allowance
        print(f"{wrong}: {key} misses the fp32 rule by a factor {factor:.3g}")
        assert factor > 1e3, (wrong, factor)
        clean = [k for k in r64 if k != "k_bias_parts" and gr.rel_l2(bad[k], r64[k]) > 4 * max(gr.rel_l2(r32[k], r64[k]), 1e-300)]
        assert key in clean


@pytest.mark.parametrize("cls_only", [False, True])
def test_k_bias_of_the_fp32_evaluation_sits_inside_its_bound(cls_only):
    model, stem, gm, gl = case((256, 320), cls_only)
    sd = model.state_dict()
    r64 = gr.transformer_vjp(sd, stem, 2, gm, gl, cls_only_last=cls_only, want_parts=True)[0]
    r32 = gr.transformer_vjp(sd, stem, 2, gm, gl, dtype=torch.float32, cls_only_last=cls_only)[0]
    for i in range(2):
        k = f"transformer.{i}.attn.in_proj_bias"
        bound = gr.k_bias_bound(r64["k_bias_parts"][i], False)
        ratio = float((r32[k][256:512].double().abs() / bound).max())
        print(f"{k}[256:512] fp32 CPU evaluation: max |value| / bound = {ratio:.4f}; float64: {float(r64[k][256:512].abs().max()):.2e}")
        assert ratio <= 1.0 and float(r64[k][256:512].abs().max()) <= 1e-12 * float(r64[k].abs().max())


# ---- mode switches -------------------------------------------------------------------------------------------------------------------------------------
NAMED = ("pos_embedding", "cls_token", "transformer.", "to_latent.", "fc_mu.", "fc_var.")


def test_train_transformer_returns_exactly_the_named_set():
    from causal_vae_amd.vit.models import ViTVAE
    model = make((64, 96), ViTVAE)
    with pytest.raises(RuntimeError, match="stem.0.weight"):
        model.train_transformer()                                           # a fresh model's stem asks for gradients
    model.requires_grad_(False)
    params = model.train_transformer()
    want = [(k, p) for k, p in model.named_parameters() if k.startswith(NAMED)]
    assert len(params) == len(want) == 2 + 2 * 12 + 2 + 4 and all(a is b for a, (_k, b) in zip(params, want))
    live = {k for k, p in model.named_parameters() if p.requires_grad}
    assert live == {k for k, _p in want}                                    # the stem and the decoder stay frozen
    model.freeze_transformer()
    assert not any(p.requires_grad for p in model.parameters())
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train_transformer()


def test_train_adapters_default_is_unchanged():
    from causal_vae_amd.vit.causal import CausalViTVAE
    torch.manual_seed(0)
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    heads = model.head_parameters()
    params = model.train_adapters()
    assert len(params) == len(heads) and all(a is b for a, b in zip(params, heads))
    assert not any(p.requires_grad for p in model.backbone.parameters()) and not model.backbone.training
    both = model.train_adapters(decoder=True)
    dec = list(model.backbone.decoder_input.parameters()) + list(model.backbone.decoder.parameters())
    assert len(both) == len(heads) + len(dec) and all(a is b for a, b in zip(both, heads + dec))
    full = model.train_adapters(decoder=True, transformer=True)
    tr = [p for k, p in model.backbone.named_parameters() if k.startswith(NAMED[:4])]      # fc_mu / fc_var are not on CausalViTVAE's path: frozen, not returned
    assert len(full) == len(heads) + len(tr) + len(dec) and all(a is b for a, b in zip(full, heads + tr + dec))
    assert not any(p.requires_grad for p in model.backbone.stem.parameters()) and not model.backbone.training
    assert {k for k, p in model.backbone.named_parameters() if p.requires_grad} == {k for k, _p in model.backbone.named_parameters() if k.startswith(NAMED[:4] + ("decoder",))}
    assert len(model.train_adapters()) == len(heads) and not any(p.requires_grad for p in model.backbone.parameters())


# ---- the golden: gradients captured from the reference ViTVAE class ------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_class_gradients(golden):
    """tests/golden/vitvae_enc_grad_64x96.npz (tools/make_golden.py vitvae_grad): one fp32 CPU backward through the reference ViTVAE in eval mode.  Per stored
    tensor (small ones whole, a fixed row subset of each weight matrix) the float64 restatement lies within twice the fp32 CPU evaluation's own distance from
    float64: the golden is one fp32 evaluation, the restatement's fp32 run another, of the same float64 value."""
    import numpy as np
    from test_vit_reference_cpu import reference_state
    g = golden("vitvae_enc_grad_64x96")
    _model, sd, _x, depth = reference_state(g)
    z = g.z
    stem = torch.from_numpy(z["out/stem"]).flatten(2).transpose(1, 2)
    gm, gl = torch.from_numpy(z["in/g_mu"]), torch.from_numpy(z["in/g_lv"])
    r64, out = gr.transformer_vjp(sd, stem.double(), depth, gm, gl)
    r32 = gr.transformer_vjp(sd, stem, depth, gm, gl, dtype=torch.float32)[0]
    assert gr.rel_l2(out["mu"], torch.from_numpy(z["out/mu"])) < 1e-5
    names = sorted(k[5:] for k in z.files if k.startswith("grad/") and not k.endswith("#rows"))
    assert names == sorted(k for k in r64 if k != "dstem")                  # every transformer-side parameter, nothing else
    worst = 0.0
    for k in names:
        want = torch.from_numpy(z["grad/" + k]).double()
        rows = torch.from_numpy(z[f"grad/{k}#rows"]) if f"grad/{k}#rows" in z.files else None
        a, b = (r64[k], r32[k].double()) if rows is None else (r64[k][rows], r32[k].double()[rows])
        assert a.shape == want.shape, k
        if k.endswith("attn.in_proj_bias"):                                 # the k bias is rounding noise on both sides (its own test above)
            keep = torch.ones(768, dtype=torch.bool)
            keep[256:512] = False
            a, b, want = a[keep], b[keep], want[keep]
        dist, own = float((a - want).norm()), float((a - b).norm())
        print(f"{k}: |float64 - golden| {dist:.3e}, |float64 - fp32 evaluation| {own:.3e}, ratio {dist / own:.3f}")
        worst = max(worst, dist / own)
        assert dist <= 2 * own, (k, dist, own)
    print("worst ratio", worst)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vitvae_enc_grad_64x96.npz")) <= max(
        os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f != "vitvae_enc_grad_64x96.npz")
