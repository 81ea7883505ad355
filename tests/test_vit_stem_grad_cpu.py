"""CPU tests of the yardstick of tests/test_vit_stem_grad.py (tests/vit_stem_grad_reference.py) and of the switches that need no GPU.

The float64 restatement of the stem's vector-Jacobian product in the FOLDED form equals torch.autograd through the model's own nn.Conv2d / nn.BatchNorm2d /
nn.LeakyReLU stack (eval mode, unfolded) to 1e-12 of each tensor's largest element, on inputs whose pre-activations take both signs at every layer.  It
matches the stem gradients captured from the reference ViTVAE class (the golden) by the rule of tests/test_vit_encoder_grad_cpu.py.  What the yardstick
refuses: two deliberately wrong restatements miss the fp32 comparison by the factors recorded in test_the_yardstick_refuses_wrong_restatements."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_stem_grad_reference as sr  # noqa: E402

F64 = torch.float64


def make(img, cls=None, seed=0):
    from causal_vae_amd.vit.models import ViTVAEEncoder
    torch.manual_seed(seed)
    model = (cls or ViTVAEEncoder)(img_size=img, depth=2, latent_dim=128).eval()
    vr.randomize_stem_bn(model.stem, seed + 1)
    return model


def case(img, B):
    model = make(img)
    x = vr.vit_inputs(B, *img, seed=5)
    g = torch.Generator().manual_seed(3)
    dstem = torch.randn(B, (img[0] // 32) * (img[1] // 32), 256, generator=g, dtype=F64)
    return model, x, dstem


@pytest.mark.parametrize("img,B", [((64, 96), 2), ((256, 320), 3)])
def test_restatement_equals_autograd_in_float64(img, B):
    model, x, dstem = case(img, B)
    m = model.double()
    h = x.double()
    for j in range(5):                                                       # the unfolded stack, layer by layer: both signs in front of every LeakyReLU
        pre = m.stem[3 * j + 1](m.stem[3 * j](h))
        assert float(pre.detach().min()) < 0.0 < float(pre.detach().max()), j
        h = m.stem[3 * j + 2](pre)
    y = m.stem(x.double())
    assert torch.equal(y, h)
    named = list(m.stem.named_parameters())
    want = torch.autograd.grad(y, [p for _k, p in named], dstem.transpose(1, 2).reshape(y.shape))
    got = sr.stem_vjp(model.state_dict(), x, dstem)
    assert [f"stem.{k}" for k, _p in named] == list(sr.STEM_KEYS) and len(got) == 20
    for (k, _p), w in zip(named, want):
        err = float((got[f"stem.{k}"] - w).abs().max()) / float(w.abs().max())
        assert err <= 1e-12, (k, err)


def test_the_yardstick_refuses_wrong_restatements():
    """The gate read off the layer's own output instead of its input's producer, and dgamma without the (bias - mean) term: each misses the fp32 rule (rel-L2
    from float64 at most 4 x that of the fp32 evaluation) on the tensors it touches by the factor printed here.
    Recorded (256 x 320, B = 3): gate from the output: stem.9.weight 4.3e+05 x the allowance; dgamma without (bias - mean): stem.13.weight 1.0e+06 x."""
    model, x, dstem = case((256, 320), 3)
    sd = model.state_dict()
    r64 = sr.stem_vjp(sd, x, dstem)
    r32 = sr.stem_vjp(sd, x, dstem, dtype=torch.float32)
    for wrong, key in (("gate_from_output", "stem.9.weight"), ("dgamma_no_bias", "stem.13.weight")):
        bad = sr.stem_vjp(sd, x, dstem, wrong=wrong)
        allowance = 4 * sr.rel_l2(r32[key], r64[key])
        factor = sr.rel_l2(bad[key], r64[key]) / allowance
        print(f"{wrong}: {key} misses the fp32 rule by a factor {factor:.3g}")
        assert factor > 1e3, (wrong, factor)
    last = [k for k in sr.STEM_KEYS if k.startswith(("stem.12.", "stem.13."))]     # the last layer's g is gated the same way in both: untouched by the wrong gate
    bad = sr.stem_vjp(sd, x, dstem, wrong="gate_from_output")
    assert all(torch.equal(bad[k], r64[k]) for k in last)


def test_restatement_matches_the_reference_class_gradients(golden):
    """tests/golden/vitvae_stem_grad_64x96.npz (tools/make_golden.py vitvae_stem_grad): one fp32 CPU backward through the reference ViTVAE in eval mode.  Per
    stored tensor (small ones whole, a fixed row subset of each conv weight's gradient) the float64 restatement lies within twice the fp32 CPU evaluation's own
    distance from float64: the golden is one fp32 evaluation, the restatement's fp32 run another, of the same float64 value."""
    from test_vit_reference_cpu import reference_state
    g = golden("vitvae_stem_grad_64x96")
    _model, sd, x, _depth = reference_state(g)
    z = g.z
    dstem = torch.from_numpy(z["out/dstem"]).flatten(2).transpose(1, 2)
    r64 = sr.stem_vjp(sd, x, dstem.double())
    r32 = sr.stem_vjp(sd, x, dstem, dtype=torch.float32)
    names = sorted(k[5:] for k in z.files if k.startswith("grad/") and not k.endswith("#rows"))
    assert names == sorted(sr.STEM_KEYS)                                    # every stem tensor, nothing else
    worst = 0.0
    for k in names:
        want = torch.from_numpy(z["grad/" + k]).double()
        rows = torch.from_numpy(z[f"grad/{k}#rows"]) if f"grad/{k}#rows" in z.files else None
        assert (rows is not None) == (r64[k].dim() == 4), k
        a, b = (r64[k], r32[k].double()) if rows is None else (r64[k][rows], r32[k].double()[rows])
        assert a.shape == want.shape, k
        dist, own = float((a - want).norm()), float((a - b).norm())
        print(f"{k}: |float64 - golden| {dist:.3e}, |float64 - fp32 evaluation| {own:.3e}, ratio {dist / own:.3f}")
        worst = max(worst, dist / own)
        assert dist <= 2 * own, (k, dist, own)
    print("worst ratio", worst)
    size = lambda f: os.path.getsize(os.path.join(ROOT, "tests", "golden", f))
    assert size("vitvae_stem_grad_64x96.npz") <= 0.75 * size("vitvae_enc_grad_64x96.npz")


# ---- switches ------------------------------------------------------------------------------------------------------------------------------------------
def test_train_stem_and_freeze_stem():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit.models import ViTVAE
    model = make((64, 96), ViTVAE)
    model.requires_grad_(False)
    params = model.train_stem()
    want = [(k, p) for k, p in model.named_parameters() if k.startswith("stem.")]
    assert len(params) == len(want) == 20 and all(a is b for a, (_k, b) in zip(params, want))
    assert [k for k, _p in want] == list(sr.STEM_KEYS)
    assert {k for k, p in model.named_parameters() if p.requires_grad} == set(sr.STEM_KEYS)       # the stem alone: no transformer, no decoder
    assert not model.training and all(not m.training for m in model.stem)                           # BatchNorm2d stays on its running statistics
    both = model.train_transformer()                                        # a live stem is admitted once train_stem() was called
    assert all(p.requires_grad for p in params) and len(both) == 2 + 2 * 12 + 2 + 4
    model.freeze_stem()
    assert not any(p.requires_grad for p in model.stem.parameters()) and not model._stem_grads
    assert all(p.requires_grad for p in both)                               # freeze_stem leaves the transformer alone
    model.freeze_transformer()
    model.stem[0].weight.requires_grad_(True)                               # a live stem parameter without train_stem(): an error, not a gradient that stays None
    x = torch.zeros(1, 1, 64, 96)
    with pytest.raises(CvaeError, match="train_stem"):
        model.cls_features_with_grad(x)
    with pytest.raises(CvaeError, match="train_stem"):
        model.encode_with_grad(x)
    with pytest.raises(RuntimeError, match="stem.0.weight"):
        model.train_transformer()
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train_stem()


def test_train_all_returns_every_parameter():
    from causal_vae_amd.vit.models import ViTVAE
    model = make((64, 96), ViTVAE)
    model.requires_grad_(False)
    params = model.train_all()
    assert len(params) == len(list(model.parameters())) and all(a is b for a, b in zip(params, model.parameters()))
    assert all(p.requires_grad for p in params) and model._stem_grads and model._transformer_grads and model._decoder_grads and not model.training


def test_train_adapters_stem_switch():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit.causal import CausalViTVAE
    torch.manual_seed(0)
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    with pytest.raises(CvaeError, match="transformer=True"):
        model.train_adapters(stem=True)
    with pytest.raises(CvaeError, match="transformer=True"):
        model.train_adapters(decoder=True, stem=True)
    heads = model.head_parameters()
    base = model.train_adapters(decoder=True, transformer=True)
    assert not any(p.requires_grad for p in model.backbone.stem.parameters())
    full = model.train_adapters(decoder=True, transformer=True, stem=True)
    stem = list(model.backbone.stem.parameters())
    assert len(full) == len(base) + 20 and len({id(p) for p in full}) == len(full)
    assert all(a is b for a, b in zip(full, heads + stem + base[len(heads):]))
    assert all(p.requires_grad for p in stem) and not model.backbone.training
    assert len(model.train_adapters()) == len(heads) and not any(p.requires_grad for p in model.backbone.parameters())     # the default call starts frozen again


def test_vit_vae_loss_is_the_reference_expression():
    """On host tensors vit_vae_loss takes torch's mse_loss for the image term — the expression it is compared with — so what this test holds is the KLD
    term, beta and the composition; the GPU form of the image term, ops.sse / numel, is held to the same expression by
    tests/test_vit_stem_grad.py::test_vitvae_trains_end_to_end."""
    import torch.nn.functional as F
    from causal_vae_amd.vit import vit_vae_loss
    g = torch.Generator().manual_seed(9)
    recons, x = torch.randn(3, 1, 64, 96, generator=g), torch.rand(3, 1, 64, 96, generator=g)
    mu, log_var = torch.randn(3, 128, generator=g), 0.3 * torch.randn(3, 128, generator=g)
    for beta in (1.0, 0.25):
        want = F.mse_loss(recons, x, reduction="mean") + beta * (-0.5 * torch.mean(1 + log_var - mu.pow(2) - log_var.exp()))
        got = vit_vae_loss(recons, x, mu, log_var, beta=beta)
        assert got.shape == () and abs(float(got) - float(want)) <= 1e-6 * abs(float(want))
    assert float(vit_vae_loss(recons, x, mu, log_var)) == float(vit_vae_loss(recons, x, mu, log_var, beta=1.0))


def test_header_and_library_export_the_new_entry():
    from causal_vae_amd import _lib, vit
    text = open(os.path.join(ROOT, "include", "cvae_hip.h")).read()
    assert "int cvae_conv_down_bwd_data(" in text and "CVAE_FOLD_CONV_K3S2 (the ViT-VAE stem)" in text
    assert "const void* gate, int gate_act, int64_t B, int64_t n_patches" in text           # cvae_vit_tokens_bwd's optional gate
    assert hasattr(_lib.lib, "cvae_conv_down_bwd_data") and _lib.lib.cvae_conv_down_bwd_data.argtypes is not None
    for name in ("vit_vae_loss", "train_vit_vae", "ViTVAE", "ViTVAEEncoder"):
        assert hasattr(vit, name), name
