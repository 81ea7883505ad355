"""CPU tests of the decoder's weight-gradient path: the float64 restatement tests/vit_decoder_wgrad_reference.py against torch.autograd through the restated
decoder (tests/vit_decoder_reference.py), the fold's way back alone, the library's exports, and the flags of ViTVAE.train_decoder /
CausalViTVAE.train_adapters(decoder=True).  No GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_decoder_reference as dr  # noqa: E402
import vit_decoder_grad_reference as gr  # noqa: E402
import vit_decoder_wgrad_reference as wr  # noqa: E402
from test_vit_decoder_cpu import CASES, reference_state  # noqa: E402
from test_vit_decoder_grad_cpu import cotangent  # noqa: E402

NEW_ENTRIES = ("cvae_conv_s1_wgrad_workspace_bytes", "cvae_conv_s1_wgrad", "cvae_conv_s1_c1_wgrad_workspace_bytes", "cvae_conv_s1_c1_wgrad",
               "cvae_latent_to_grid_wgrad", "cvae_fold_bn_conv_bwd")


def test_restatement_equals_autograd_for_every_parameter(golden):
    """float64's own masks: the fixed-mask decoder IS the decoder, so its weight VJP is autograd's, for all 48 parameters, BatchNorm weight and bias and
    non-trivial running statistics included"""
    _model, sd, _z, grid = reference_state(golden(CASES[0]))
    z, cot = dr.dec_inputs(3, 128, 41), cotangent(3, 64, 96, 42).double()
    names = wr.decoder_param_names(sd)
    assert len(names) == 48 and "decoder.3.conv.4.weight" in names and "decoder.1.bias" in names
    assert float((sd["decoder.1.running_var"] - 1).abs().max()) > 0.1 and float(sd["decoder.1.running_mean"].abs().max()) > 0.01
    live = {k: (v.double().requires_grad_(True) if k in names else v.double()) for k, v in sd.items() if v.is_floating_point()}
    ref = dr.decode_ref(live, z, grid)
    (ref["image"] * cot).sum().backward()
    stages = {k: v.detach() for k, v in ref.items()}
    masks = gr.masks_of(stages, gr.res_inner_ref(sd, stages))
    got = wr.decoder_wgrad_ref(sd, z, cot, grid, masks)
    assert sorted(got) == sorted(names)
    for k in names:
        want = live[k].grad
        assert got[k].shape == want.shape, k
        err = float((got[k] - want).abs().max()) / float(want.abs().max())
        assert float(want.abs().max()) > 0 and err <= 1e-12, (k, err)
    for mutate, key in (("no_swap", "decoder.15.weight"), ("no_bias_term", "decoder.1.weight")):
        wrong = wr.decoder_wgrad_ref(sd, z, cot, grid, masks, mutate=mutate)
        assert float((wrong[key] - live[key].grad).abs().max()) > 1e-3 * float(live[key].grad.abs().max()), mutate


@pytest.mark.parametrize("transposed", [False, True])
def test_fold_backward_formulas_equal_autograd(transposed):
    gen = torch.Generator().manual_seed(7 + transposed)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    cout, cin = 6, 4
    w = (rnd(cin, cout, 3, 3) if transposed else rnd(cout, cin, 3, 3)).requires_grad_(True)
    b, gamma, beta = (rnd(cout).requires_grad_(True) for _ in range(3))
    mean, var = 0.3 * rnd(cout), 0.5 + torch.rand(cout, generator=gen, dtype=torch.float64)
    sd = {"c.weight": w, "c.bias": b, "n.weight": gamma, "n.bias": beta, "n.running_mean": mean, "n.running_var": var}
    wf, bf = dr.fold(lambda k: sd[k], "c", "n", transposed)
    dwf, dbf = rnd(*wf.shape), rnd(cout)
    ((wf * dwf).sum() + (bf * dbf).sum()).backward()
    got = wr.fold_backward_ref(w.detach(), b.detach(), gamma.detach(), mean, var, dwf, dbf, transposed)
    for name, mine, want in zip(("dw", "db", "dgamma", "dbeta"), got, (w.grad, b.grad, gamma.grad, beta.grad)):
        assert float((mine - want).abs().max()) <= 1e-12 * float(want.abs().max()), name


def test_library_exports_the_weight_gradient_entries():
    from causal_vae_amd import _lib as L
    from causal_vae_amd import ops
    for name in NEW_ENTRIES:
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert L.lib.cvae_version() >= 205
    header = open(os.path.join(ROOT, "include", "cvae_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name + "(" in header, name
    for name in ("conv_s1_wgrad", "conv_s1_c1_wgrad", "latent_to_grid_wgrad", "fold_bn_conv_bwd"):
        assert callable(getattr(ops, name))
    wb = L.lib.cvae_conv_s1_wgrad_workspace_bytes
    assert wb(8, 96, 160, 128, ops.CONV_S1_K3) == 64 * (16 * 9 * 1024 + 2 * 128) * 4         # 64 slabs of 147 456 sums + the bias partials
    assert wb(1, 8, 16, 16, ops.CONV_S1_K3) == (9 * 1024 + 2 * 32) * 4 and wb(1, 8, 16, 48, ops.CONV_S1_K3) == 0
    assert wb(2, 5, 7, 32, ops.CONV_S1_SUBPIXEL) == 2 * (2 * 4 * 1024 + 2 * 64) * 4 and wb(2, 5, 7, 64, ops.CONV_S1_SUBPIXEL) == 0 and wb(0, 8, 16, 32, ops.CONV_S1_K3) == 0


def test_train_decoder_and_train_adapters_set_the_flags():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import CausalViTVAE, ViTVAE
    torch.manual_seed(1)
    model = ViTVAE(img_size=(64, 96), depth=1).eval()
    dec = lambda m: list(m.decoder_input.parameters()) + list(m.decoder.parameters())
    assert model.freeze_decoder() is model and not model._decoder_grads and not any(p.requires_grad for p in dec(model))
    assert model.train_decoder() is model and model._decoder_grads and all(p.requires_grad for p in dec(model)) and not model.training
    assert len(model._decoder_params()) == 48 == len(dec(model)) and {id(p) for p in model._decoder_params()} == {id(p) for p in dec(model)}
    assert not model.freeze_decoder()._decoder_grads
    # the default paths raise as before: live decoder parameters without train_decoder()
    model.decoder.requires_grad_(True)
    with pytest.raises(CvaeError, match="freeze_decoder"):
        model.decode_with_grad(torch.zeros(1, 128))
    with pytest.raises(CvaeError):                                       # and with it, a CPU tensor is still refused: no fallback
        model.train_decoder().decode_with_grad(torch.zeros(1, 128))

    cm = CausalViTVAE(img_size=(64, 96), depth=1)
    heads = cm.train_adapters()
    assert len(heads) == len(cm.head_parameters()) and not any(p.requires_grad for p in cm.backbone.parameters()) and not cm.backbone._decoder_grads
    both = cm.train_adapters(decoder=True)
    assert len(both) == len(heads) + 48 and cm.backbone._decoder_grads and not cm.backbone.training and cm.enc_adapter.training
    live = {k for k, p in cm.backbone.named_parameters() if p.requires_grad}
    assert live and all(k.startswith(("decoder_input.", "decoder.")) for k in live) and len(live) == 48
    cm.backbone.fc_mu.weight.requires_grad_(True)                        # a live encoder parameter still raises, naming train_adapters()
    with pytest.raises(RuntimeError, match="train_adapters"):
        cm.forward_train(torch.zeros(2, 1, 64, 96), torch.zeros(2, cm.m_dim), torch.zeros(2, cm.t_dim))
    cm.train_adapters()                                                  # the default call: everything in the backbone frozen again
    assert not any(p.requires_grad for p in cm.backbone.parameters()) and not cm.backbone._decoder_grads
    cm.backbone.decoder.requires_grad_(True)
    with pytest.raises(RuntimeError, match="train_adapters"):
        cm.forward_train(torch.zeros(2, 1, 64, 96), torch.zeros(2, cm.m_dim), torch.zeros(2, cm.t_dim))
