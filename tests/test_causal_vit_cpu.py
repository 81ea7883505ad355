"""CausalViTVAE without a GPU: the constructor draws the reference's weights (digests and key list of tests/golden/causal_vitvae_768x1280.npz), the float64
restatement (tests/causal_vit_reference.py) reproduces the fp32 reference's recorded outputs within the composed fp32 bound, the rounding-oracle gap of the
bf16 backbone is printed (tests/test_causal_vit.py asserts against twice that gap), the entry points raise in training mode and on wrong shapes,
pretrained_path loads a backbone checkpoint strictly, and batched_counterfactual's precision= reaches the model's compute dtype."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as dr  # noqa: E402
import causal_vit_reference as cr  # noqa: E402

NAME = "causal_vitvae_768x1280"
WHOLE = ("cls_out", "mu", "logvar", "z", "m_mu", "m_logvar", "z_vit", "recon_crop")


def reference_state(g):
    """(model, state_dict, (x, m, t, eps), crop) of the golden: the seed's draws + the seeded BatchNorm statistics, checked against the stored digests."""
    from causal_vae_amd.vit import CausalViTVAE
    B, H, W, seed_model, seed_bn, seed_dec_bn, seed_head_bn, seed_data = (int(v) for v in g.z["in/seed"])
    torch.manual_seed(seed_model)
    model = CausalViTVAE(img_size=(H, W))
    vr.randomize_stem_bn(model.backbone.stem, seed_bn)
    dr.randomize_decoder_bn(model.backbone.decoder, seed_dec_bn)
    cr.randomize_head_bn(model, seed_head_bn)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g.z["sd0_keys"]]
    for k, v in sd.items():
        g.check("sd0", k, v, rtol=0, atol=0)
    x, m, t, eps = cr.causal_inputs(B, H, W, seed_data)
    assert np.array_equal(np.packbits(x.numpy().astype(np.uint8).reshape(-1)), g.z["in/x_bits"])
    for k, v in (("m", m), ("t", t), ("eps", eps)):
        assert torch.equal(v, g.t("in/" + k)), k
    return model, sd, (x, m, t, eps), tuple(int(v) for v in g.z["in/crop"])


def test_constructor_reproduces_the_reference_state_dict(golden):
    model, sd, _inp, _crop = reference_state(golden(NAME))
    assert [k for k in sd if not k.startswith("backbone.")][:3] == ["enc_adapter.0.weight", "enc_adapter.0.bias", "enc_adapter.1.weight"]
    assert {"dec_adapter.1.running_var", "morph_predictor_shared.2.bias", "morph_predictor_logvar.weight", "backbone.decoder_input.weight"} <= set(sd)
    assert sd["backbone.decoder_input.weight"].shape == (256 * 24 * 40, 512) and sd["enc_adapter.0.weight"].shape == (512, 287)
    assert sd["dec_adapter.3.weight"].shape == (512, 256) and type(model).decode_signature == "z_m"


def test_float64_restatement_matches_golden(golden):
    g = golden(NAME)
    _model, sd, (x, m, t, eps), crop = reference_state(g)
    bound, ref = cr.composed_bound(sd, x, m, t, eps, 6, key=NAME, crop=crop)
    for k in WHOLE:
        want = g.t("out/" + k).double()
        ratio, rel = vr.fro_ratio(want, ref[k], bound[k]), bound[k] / float(ref[k].norm())
        print(f"{k}: ||golden - float64|| / bound = {ratio:.2e}; bound / ||value|| = {rel:.2e}")
        assert 0.0 < rel < 2e-2, (k, rel, "the bound must be finite and a small fraction of the values it guards")
        assert ratio <= 1.0, (k, ratio)
    g.check("out", "recon_x", ref["recon_x"].float(), rtol=bound["recon_x"] / float(ref["recon_x"].norm()), atol=bound["recon_x"] / 20)
    # the rounding-oracle gap of the bf16 backbone (what tests/test_causal_vit.py allows twice of)
    orac = cr.forward_ref(sd, x, m, t, eps, 6, rnd=vr.round_bf16, crop=crop)
    for k in ("mu", "z_vit", "recon_x"):
        print(f"bf16 rounding oracle vs float64, {k}: rel-L2 {vr.rel_l2(orac[k], ref[k]):.3e}")


def test_what_the_heads_bound_refuses(golden):
    """A head port's structural mistakes must fall outside the bound: [z | m] where [m | z] belongs, the BatchNorm mean left out, slope 0.01 for 0.2.  The
    element-wise worst case carried through up to four layers is coarse next to the Frobenius bounds (it guards structure; the kernel's own test prints how
    far inside it the kernel sits), but it stays a small fraction of the values."""
    g = golden(NAME)
    _model, sd, (x, m, t, eps), _crop = reference_state(g)
    cls_out = g.t("out/cls_out").double()
    vals, bounds = cr.heads_ref(sd, cls_out, m, t, eps, want_bound=True)
    inside = lambda k, v: bool(((v - vals[k]).abs() <= bounds[k]).all())
    for k in cr.HEAD_NAMES:
        assert inside(k, vals[k]) and bool((bounds[k] < 0.05 * vals[k].abs().max()).all()), k
    get = lambda k: sd[k].double()
    z = vals["z"]
    layers = cr.adapter_layers(get, "dec_adapter")
    assert not inside("z_vit", cr.head_b(torch.cat([z, m.double()], 1), None, layers)[0])
    W, b, (gam, bet, mean, var, e), slope = layers[0]
    assert not inside("z_vit", cr.head_b(torch.cat([m.double(), z], 1), None, [(W, b, (gam, bet, 0 * mean, var, e), slope), layers[1]])[0])
    assert not inside("z_vit", cr.head_b(torch.cat([m.double(), z], 1), None, [(W, b, (gam, bet, mean, var, e), 0.01), layers[1]])[0])
    # the golden's own head outputs from its own cls_out: the fp32 reference sits inside the element-wise bound
    for k in cr.HEAD_NAMES:
        assert inside(k, g.t("out/" + k).double()), k


def test_training_mode_and_wrong_shapes_raise():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import AdapterMLP, CausalViTVAE
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    x, m, t, eps = cr.causal_inputs(2, 64, 96, 5)
    z = torch.zeros(2, 128)
    assert model.training
    for call in (lambda: model(x, m, t), lambda: model.encode(x, m, t), lambda: model.decode(z, m), lambda: model.predict_morph(t),
                 lambda: model.reparameterize(z, z, eps), lambda: model.dec_adapter(torch.cat([m, z], 1))):
        with pytest.raises(RuntimeError, match="eval mode"):
            call()
    model.eval()
    for call in (lambda: model.encode(x, m[:, :11], t), lambda: model.encode(x, m, t[:1]), lambda: model.decode(z[:, :64], m), lambda: model.decode(z, m.double()),
                 lambda: model.predict_morph(t[:, :18]), lambda: model(x, m, t, eps[:, :5]), lambda: model.reparameterize(z, z[:1])):
        with pytest.raises(CvaeError, match="must be a float32"):
            call()
    with pytest.raises(CvaeError, match="MI355X only"):          # right shapes on the CPU: there is no fallback
        model.predict_morph(t)
    with pytest.raises(RuntimeError, match="predict_morph"):
        model.morph_predictor_shared(t)
    assert isinstance(model.enc_adapter, AdapterMLP) and list(model.enc_adapter.state_dict())[4] == "1.running_mean"


def test_heads_entry_point_limits():
    """cvae_mlp_heads_fwd's argument checks come before any launch: they answer without a GPU."""
    import ctypes as C
    from causal_vae_amd import _lib as L
    assert L.lib.cvae_version() >= 203
    pan = (L.HeadsPanel * 3)(*[L.HeadsPanel(None, w, w) for w in (256, 12, 19)])
    lay = (L.HeadsLayer * 3)()
    lay[0].out = lay[0].out_first = 512
    lay[1].out = lay[1].out_first = 256
    call = lambda npan, nlay, split, B, z=None: L.lib.cvae_mlp_heads_fwd(pan, npan, lay, nlay, split, None, None, None, 128, None, 128, None, 128, z, 128, B, None)
    assert call(3, 2, 128, 0) == 0                                            # B == 0: nothing is launched
    assert call(3, 2, 128, 4) == -6                                           # null pointers
    assert call(4, 2, 128, 0) == -3 and call(3, 4, 128, 0) == -3 and call(0, 2, 128, 0) == -3
    assert call(3, 2, 0, 0) == -1 and call(3, 2, 257, 0) == -1
    assert call(3, 2, 64, 0, z=C.c_void_p(16)) == -1                          # z needs out == 2 split
    lay[1].out = lay[1].out_first = 513
    assert call(3, 2, 128, 0) == -3                                           # wider than CVAE_HEADS_MAX_WIDTH
    lay[1].out, lay[1].out_first = 256, 128
    lay[2].out = lay[2].out_first = 24
    assert call(3, 2, 128, 0) == 0 and call(3, 3, 12, 0) == -3                # two weight tensors: the last layer only
    pan[0].width = pan[0].stride = 512
    assert call(3, 2, 128, 0) == -3                                           # concatenated input wider than the limit
    pan[0].width, pan[0].stride = 256, 255
    assert call(3, 2, 128, 0) == -1


def test_pretrained_path_loads_the_backbone_strictly(tmp_path):
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import CausalViTVAE
    torch.manual_seed(1)
    src = CausalViTVAE(img_size=(64, 96), depth=1)
    vr.randomize_stem_bn(src.backbone.stem, 2)
    good = src.backbone.state_dict()
    torch.save(good, tmp_path / "backbone.pt")
    torch.manual_seed(9)                                                      # other draws: what is equal afterwards was loaded
    model = CausalViTVAE(str(tmp_path / "backbone.pt"), img_size=(64, 96), depth=1)
    got = model.backbone.state_dict()
    assert list(got) == list(good) and all(torch.equal(got[k], good[k]) for k in good)
    assert not torch.equal(model.enc_adapter[0].weight, src.enc_adapter[0].weight)          # the heads are not in a backbone checkpoint
    # the reference's strict=False would pass all three over in silence
    extra = dict(good, stray=torch.zeros(1))
    missing = {k: v for k, v in good.items() if k != "fc_mu.bias"}
    misshaped = dict(good, **{"fc_mu.bias": torch.zeros(7)})
    for name, sd, word in (("extra", extra, "stray"), ("missing", missing, "fc_mu.bias"), ("misshaped", misshaped, "fc_mu.bias")):
        torch.save(sd, tmp_path / (name + ".pt"))
        with pytest.raises(CvaeError, match=word):
            CausalViTVAE(str(tmp_path / (name + ".pt")), img_size=(64, 96), depth=1)
    # the loader's one exception: a pos_embedding of another patch grid is resized; the decoder_input of that grid is still a shape error
    torch.manual_seed(1)
    torch.save(CausalViTVAE(img_size=(128, 192), depth=1).backbone.state_dict(), tmp_path / "grid.pt")
    with pytest.raises(CvaeError, match="decoder_input.weight"):
        CausalViTVAE(str(tmp_path / "grid.pt"), img_size=(64, 96), depth=1)


def test_batched_counterfactual_precision_reaches_the_model():
    """precision= decides the dtype the sweep's decode runs in, and the model's own choice is put back (the decode itself is replaced: no GPU here)."""
    from causal_vae_amd.counterfactual import batched_counterfactual
    from causal_vae_amd.vit import CausalViTVAE
    seen = []

    class Spy(CausalViTVAE):
        def decode(self, z, m):
            seen.append(self.compute_dtype)
            return torch.zeros(z.shape[0], 1, 2, 2)

    model = Spy(img_size=(64, 96), depth=1).eval()
    z, m = torch.zeros(2, 128), torch.zeros(2, 12)
    for own in (torch.float32, torch.bfloat16):
        model.set_compute_dtype(own)
        for precision, want in ((None, torch.float32), ("fp32", torch.float32), ("bf16", torch.bfloat16), ("model", own)):
            del seen[:]
            out = batched_counterfactual(model, z, m, [0, 3], [-1.0, 1.0, 2.0], precision=precision, chunk_rows=5)
            assert out.shape == (2, 2, 3, 1, 2, 2) and seen == [want] * 3, (own, precision, seen)
            assert model.compute_dtype == own, (own, precision)
