"""The training-mode heads without a GPU: tests/heads_grad_reference.py (float64, its own masks) against torch.autograd through the equivalent
nn.Sequential in .train() mode, the new C entries' argument checks (they come before any launch), and CausalViTVAE.train_adapters / forward_train's guards."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import heads_grad_reference as hr  # noqa: E402

F64 = torch.float64


def make_layers(widths, bn_at, seed, pair=False):
    """random float64 layers K0 -> widths..; BatchNorm1d behind the layers in bn_at; LeakyReLU(0.2) behind every hidden layer"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    out = []
    for l in range(1, len(widths)):
        K, N = widths[l - 1], widths[l]
        bn = None
        if l - 1 in bn_at:
            bn = dict(gamma=0.5 + torch.rand(N, generator=g, dtype=F64), beta=0.1 * r(N), eps=1e-5, momentum=0.1, running_mean=0.1 * r(N),
                      running_var=0.5 + torch.rand(N, generator=g, dtype=F64), num_batches_tracked=3)
        out.append((r(N, K) / K ** 0.5, 0.1 * r(N), bn, 0.2 if l < len(widths) - 1 else None))
    return out


def autograd_head(x, layers, split, clamp0, clamp1, noise):
    seq = hr.sequential_of(layers)
    x = x.clone().requires_grad_(True)
    pc = seq(x)
    first = pc[:, :split] if clamp0 is None else pc[:, :split].clamp(*clamp0)
    second = None if split == pc.shape[1] else (pc[:, split:] if clamp1 is None else pc[:, split:].clamp(*clamp1))
    z = None if noise is None else first + noise * torch.exp(0.5 * second)
    return seq, x, first, second, z


def same(a, b, what="", tol=1e-12, floor=1e-300):
    """max |a - b| <= tol max |b| (the convention of tests/test_vit_decoder_grad_cpu.py); floor: the scale of a quantity that is zero in exact arithmetic"""
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * max(float(b.abs().max()), floor), (what, float((a - b).abs().max()), float(b.abs().max()))


def check_against_autograd(seq, x, got, layers, tol=1e-12):
    lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
    bns = {}
    i = -1
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            i += 1
        elif isinstance(m, torch.nn.BatchNorm1d):
            bns[i] = m
    close = lambda a, b, what: same(a, b, what, tol)
    for l, m in enumerate(lin):
        close(got[f"dW{l}"], m.weight.grad, f"dW{l}")
        # the bias in front of a BatchNorm layer has no gradient in exact arithmetic (the mean is subtracted): both sides hold rounding noise of dW's scale
        same(got[f"db{l}"], m.bias.grad, f"db{l}", tol, float(m.weight.grad.abs().max()) if l in bns else 1e-300)
    for l, m in bns.items():
        close(got[f"dgamma{l}"], m.weight.grad, f"dgamma{l}")
        close(got[f"dbeta{l}"], m.bias.grad, f"dbeta{l}")
    close(got["dx"], x.grad, "dx")
    return bns


CASES = {"enc": ((287, 512, 256), (0,), 128, (-100.0, 100.0), (-10.0, 10.0), True), "dec": ((140, 256, 512), (0,), 512, None, None, False),
         "morph": ((19, 64, 64, 24), (), 12, None, (-10.0, 10.0), False)}


@pytest.mark.parametrize("kind", sorted(CASES))
def test_float64_restatement_equals_autograd(kind):
    widths, bn_at, split, c0, c1, reparam = CASES[kind]
    B = 5
    g = torch.Generator().manual_seed(7)
    layers = make_layers(widths, bn_at, 11)
    W, b, bn, s = layers[-1]
    layers[-1] = (W * 40.0, b, bn, s)                                   # the clamps bite on some values
    x = torch.randn(B, widths[0], generator=g, dtype=F64)
    noise = torch.randn(B, split, generator=g, dtype=F64) if reparam else None
    N = widths[-1]
    cot = (torch.randn(B, split, generator=g, dtype=F64), torch.randn(B, N - split, generator=g, dtype=F64) if split < N else None,
           torch.randn(B, split, generator=g, dtype=F64) if reparam else None)
    fw = hr.head_forward(x, layers, split, c0, c1, noise)
    masks = hr.own_masks(fw)
    if c1 is not None:
        assert bool(masks["clamp"].any()) and not bool(masks["clamp"].all())
    got = hr.head_vjp(fw, layers, cot, masks)
    seq, xa, first, second, z = autograd_head(x, layers, split, c0, c1, noise)
    total = (first * cot[0]).sum() + (0 if second is None else (second * cot[1]).sum()) + (0 if z is None else (z * cot[2]).sum())
    total.backward()
    same(fw["first"], first.detach())
    if z is not None:
        same(fw["z"], z.detach())
    bns = check_against_autograd(seq, xa, got, layers)
    for l, m in bns.items():
        same(fw["running_mean"][l], m.running_mean)
        same(fw["running_var"][l], m.running_var)
        assert fw["nbt"][l] == int(m.num_batches_tracked) == 4
        biased = hr.head_forward(x, layers, split, c0, c1, noise, biased_running=True)
        assert float((biased["running_var"][l] - m.running_var).abs().max()) > 1e-4         # the unbiased variance is what torch stores
    # a wrong slope and a missing clamp mask are visible
    assert hr.rel_l2(hr.head_vjp(fw, layers, cot, masks, slope_override=0.01)["dW0"], got["dW0"]) > 1e-3
    if c1 is not None:
        assert hr.rel_l2(hr.head_vjp(fw, layers, cot, masks, use_clamp_mask=False)["dW0"], got["dW0"]) > 1e-3


def test_chained_enc_z_dec_equals_autograd():
    """enc_adapter -> (mu, logvar, z) -> dec_adapter([m | z]): the dz link between the two heads' VJPs, with cotangents on mu, logvar and z_vit"""
    B = 6
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    enc, dec = make_layers((287, 512, 256), (0,), 21), make_layers((140, 256, 512), (0,), 22)
    xin, m, noise = r(B, 287), r(B, 12), r(B, 128)
    c_mu, c_lv, c_out = r(B, 128), r(B, 128), r(B, 512)
    fe = hr.head_forward(xin, enc, 128, (-100.0, 100.0), (-10.0, 10.0), noise)
    fd = hr.head_forward(torch.cat([m, fe["z"]], 1), dec, 512)
    gd = hr.head_vjp(fd, dec, (c_out, None, None), hr.own_masks(fd))
    ge = hr.head_vjp(fe, enc, (c_mu, c_lv, gd["dx"][:, 12:]), hr.own_masks(fe))
    se, xe, mu, lv, z = autograd_head(xin, enc, 128, (-100.0, 100.0), (-10.0, 10.0), noise)
    sd = hr.sequential_of(dec)
    out = sd(torch.cat([m, z], 1))
    ((out * c_out).sum() + (mu * c_mu).sum() + (lv * c_lv).sum()).backward()
    check_against_autograd(se, xe, ge, enc)
    lin = [mod for mod in sd if isinstance(mod, torch.nn.Linear)]
    for l, mod in enumerate(lin):
        same(gd[f"dW{l}"], mod.weight.grad)
    same(gd["dgamma0"], sd[1].weight.grad)


def test_training_entry_point_limits():
    """cvae_mlp_heads_train_fwd / cvae_mlp_heads_bwd and their workspace queries check their arguments before any launch: they answer without a GPU."""
    from causal_vae_amd import _lib as L
    assert L.lib.cvae_version() >= 204
    one = ctypes.c_void_p(16)                                                    # a non-null pointer that is never read: every case below ends before a launch

    def head(widths=(287, 512, 256), bn=True, panel_stride=287, wptr=one):
        pan = (L.HeadsPanel * 1)(L.HeadsPanel(one, widths[0], panel_stride))
        lay = (L.HeadsLayer * (len(widths) - 1))()
        for i, n in enumerate(widths[1:]):
            lay[i].W, lay[i].b, lay[i].out, lay[i].out_first = wptr, wptr, n, n
        if bn:
            lay[0].bn_weight, lay[0].bn_bias, lay[0].leaky, lay[0].slope = one, one, 1, 0.2
        return pan, lay, len(widths) - 1

    def fwd(pan, lay, n, B, split=128, saved=one, nbytes=1 << 40, out0=one, z=None, bnst=True):
        st = (L.HeadsBnTrain * n)() if bnst else None
        return L.lib.cvae_mlp_heads_train_fwd(pan, 1, lay, n, st, split, None, None, None, 128, out0, 128, one, 128, z, 128, B, saved, nbytes, None)

    def bwd(pan, lay, n, B, grads="ok", split=128, ws=one, gz=None, pg_stride=None):
        gr = None
        if grads is not None:
            gr = (L.HeadsLayerGrad * n)()
            for i in range(n):
                gr[i].dW, gr[i].db, gr[i].dgamma, gr[i].dbeta = one, one, one, one
                if grads == "no_dW":
                    gr[i].dW = None
        pg = ps = None
        if pg_stride is not None:
            pg, ps = (ctypes.c_void_p * 1)(one), (ctypes.c_int64 * 1)(pg_stride)
        return L.lib.cvae_mlp_heads_bwd(pan, 1, pg, ps, lay, n, gr, split, None, None, None, 128, one, 128, one, 128, gz, 128, B, one, 1 << 40, ws, 1 << 40, None)

    pan, lay, n = head()
    query = L.lib.cvae_mlp_heads_train_workspace_bytes
    assert query(pan, 1, lay, n, 8) == 4 * (2 * 512 + 3 * 8 * 512 + 8 * 256)
    assert L.lib.cvae_mlp_heads_bwd_workspace_bytes(pan, 1, lay, n, 8) == 4 * 8 * (512 + 256)
    assert fwd(*head(bn=False), 0) == 0 and bwd(*head(bn=False), 0) == 0         # B == 0 without BatchNorm: nothing is launched
    assert fwd(pan, lay, n, 0) == -1 and bwd(pan, lay, n, 0) == -1               # .. with BatchNorm: no batch to take statistics of
    assert fwd(pan, lay, n, 1) == -1 and bwd(pan, lay, n, 1) == -1 and query(pan, 1, lay, n, 1) == 0       # batch statistics of one row
    assert fwd(*head(bn=False), 1, saved=None) == -6                             # .. is fine without BatchNorm, and then asks for its buffers
    assert fwd(pan, lay, n, 8, saved=None) == -6 and fwd(pan, lay, n, 8, out0=None) == -6 and fwd(pan, lay, n, 8, z=one) == -6      # z without eps
    assert fwd(pan, lay, n, 8, bnst=False) == -6
    assert fwd(pan, lay, n, 8, nbytes=64) == -4
    assert fwd(pan, lay, n, 8, split=0) == -1 and fwd(pan, lay, n, 8, split=100, z=one) == -1
    assert fwd(*head(wptr=None), 8) == -6
    assert fwd(*head(widths=(287, 513, 256)), 8) == -3 and fwd(*head(widths=(600, 512, 256), panel_stride=600), 8) == -3
    assert fwd(*head(panel_stride=286), 8) == -1 and bwd(*head(panel_stride=286), 8) == -1
    assert L.lib.cvae_mlp_heads_train_fwd(None, 1, lay, n, None, 128, None, None, None, 128, one, 128, one, 128, None, 128, 8, one, 1 << 40, None) == -6
    assert L.lib.cvae_mlp_heads_train_fwd(pan, 4, lay, n, None, 128, None, None, None, 128, one, 128, one, 128, None, 128, 8, one, 1 << 40, None) == -3
    p2, l2, n2 = head()
    l2[1].leaky = 1                                                              # the last layer is a plain Linear
    assert fwd(p2, l2, n2, 8) == -3 and bwd(p2, l2, n2, 8) == -3
    assert bwd(pan, lay, n, 8, grads=None) == -6 and bwd(pan, lay, n, 8, grads="no_dW") == -6 and bwd(pan, lay, n, 8, ws=None) == -6
    assert bwd(pan, lay, n, 8, gz=one) == -6                                     # a z cotangent without eps
    assert bwd(pan, lay, n, 8, split=100, gz=one) == -1 and bwd(pan, lay, n, 8, pg_stride=100) == -1
    assert bwd(*head(widths=(287, 513, 256)), 8) == -3


FAULTS = {  # name -> (panel (width, stride) list, n_panels passed, layer (out, out_first) list, n_layers passed, split, the code include/cvae_hip.h gives it)
    "no_panel": ([(19, 19)], 0, [(64, 64), (24, 24)], 2, 12, -3),
    "four_panels": ([(19, 19)] * 4, 4, [(64, 64), (24, 24)], 2, 12, -3),
    "four_layers": ([(19, 19)], 1, [(64, 64)] * 3 + [(24, 24)], 4, 12, -3),
    "stride_below_width": ([(19, 18)], 1, [(64, 64), (24, 24)], 2, 12, -1),
    "layer_above_512": ([(19, 19)], 1, [(513, 513), (24, 24)], 2, 12, -3),
    "input_above_512": ([(300, 300), (213, 213)], 2, [(64, 64), (24, 24)], 2, 12, -3),
    "out_first_zero": ([(19, 19)], 1, [(64, 64), (24, 0)], 2, 12, -1),
    "out_first_above_out": ([(19, 19)], 1, [(64, 64), (24, 25)], 2, 12, -1),
    "pair_on_hidden_layer": ([(19, 19)], 1, [(64, 32), (24, 24)], 2, 12, -3),
    "split_zero": ([(19, 19)], 1, [(64, 64), (24, 12)], 2, 0, -1),
    "split_above_width": ([(19, 19)], 1, [(64, 64), (24, 12)], 2, 25, -1),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_three_entries_refuse_a_faulty_head_alike(fault):
    """One faulty description, three entries (cvae_mlp_heads_fwd, cvae_mlp_heads_train_fwd, cvae_mlp_heads_bwd): the same code from each.  The head has no
    BatchNorm and every pointer is a non-null dummy that is never read: each case ends in the shape checks, before a launch."""
    from causal_vae_amd import _lib as L
    panels, n_panels, layers, n_layers, split, code = FAULTS[fault]
    one, B = ctypes.c_void_p(16), 8
    pan = (L.HeadsPanel * len(panels))(*[L.HeadsPanel(one, w, s) for w, s in panels])
    lay = (L.HeadsLayer * len(layers))()
    gr = (L.HeadsLayerGrad * len(layers))()
    for i, (out, out_first) in enumerate(layers):
        lay[i].W, lay[i].b, lay[i].W2, lay[i].b2, lay[i].out, lay[i].out_first = one, one, one, one, out, out_first
        if i < len(layers) - 1:
            lay[i].leaky, lay[i].slope = 1, 0.2
        gr[i].dW, gr[i].db, gr[i].dW2, gr[i].db2 = one, one, one, one
    st = (L.HeadsBnTrain * len(layers))()
    big = 1 << 40
    got = {"fwd": L.lib.cvae_mlp_heads_fwd(pan, n_panels, lay, n_layers, split, None, None, None, 0, one, 512, one, 512, None, 0, B, None),
           "train_fwd": L.lib.cvae_mlp_heads_train_fwd(pan, n_panels, lay, n_layers, st, split, None, None, None, 0, one, 512, one, 512, None, 0, B, one, big, None),
           "bwd": L.lib.cvae_mlp_heads_bwd(pan, n_panels, None, None, lay, n_layers, gr, split, None, None, None, 0, one, 512, one, 512, None, 0, B, one, big,
                                           one, big, None)}
    assert got == {"fwd": code, "train_fwd": code, "bwd": code}, (fault, got)


def test_forward_train_guards_and_frozen_backbone():
    from causal_vae_amd.vit import CausalViTVAE
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    x, m, t = torch.zeros(2, 1, 64, 96), torch.zeros(2, 12), torch.zeros(2, 19)
    model.train()
    assert model.backbone.training                                               # the override does nothing before train_adapters()
    with pytest.raises(RuntimeError, match="train_adapters"):
        model.forward_train(x, m, t)
    model.eval()
    with pytest.raises(RuntimeError, match="train_adapters"):                    # eval mode, but backbone parameters still ask for gradients
        model.forward_train(x, m, t)
    params = model.train_adapters()
    assert not model.backbone.training and not any(p.requires_grad for p in model.backbone.parameters())
    model.train()
    assert model.training and model.enc_adapter.training and not model.backbone.training
    assert not any(mod.training for mod in model.backbone.modules())
    head_names = {k for k, _ in model.named_parameters() if not k.startswith("backbone.")}
    assert len(params) == len(head_names) == 20 and all(p.requires_grad for p in params)
    assert {id(p) for p in params} == {id(p) for k, p in model.named_parameters() if k in head_names}
    with pytest.raises(RuntimeError, match="eval mode"):                         # the inference entries keep their contract
        model(x, m, t)
