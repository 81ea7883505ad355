"""The batch-statistics decoder without a GPU: the argument checks of cvae_bn2d_batch_fwd_res and cvae_bn2d_batch_bwd (every one precedes the first
launch, so dummy pointers are never read), the workspace query, the yardstick of tests/test_bn2d_batch_bwd.py held against an fp32 CPU evaluation of the
kernels' formulas in their sum order and against autograd, two wrong kernels it must refuse, the float64 restatement of the whole training-mode decoder
against torch's own, and the keyword plumbing of train_decoder / train_all / train_adapters."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bn2d_batch_reference as br  # noqa: E402
import bn2d_batch_bwd_reference as bb  # noqa: E402

OK, E_BADSHAPE, E_DTYPE, E_UNSUPPORTED, E_WORKSPACE, E_LAUNCH, E_NULLPTR = 0, -1, -2, -3, -4, -5, -6
ONE = C.c_void_p(64)                                                   # non-null, 16-byte aligned, never read: each case ends in a check
NONE, LEAKY02, LEAKY001 = 0, 3, 4


def res(y=ONE, gamma=ONE, beta=ONE, a=ONE, mean=ONE, rstd=ONE, rm=ONE, rv=ONE, P=24, Cc=16, momentum=0.1, eps=1e-5, act=NONE, dtype=0, ws=ONE, nbytes=None,
        resid=ONE):
    from causal_vae_amd import _lib as L
    nbytes = L.lib.cvae_bn2d_batch_workspace_bytes(24, 16) if nbytes is None else nbytes
    return L.lib.cvae_bn2d_batch_fwd_res(y, gamma, beta, a, mean, rstd, rm, rv, P, Cc, momentum, eps, act, dtype, ws, nbytes, None, resid)


def bwd(y=ONE, dy=ONE, a=ONE, gamma=ONE, mean=ONE, rstd=ONE, dx=ONE, dgamma=ONE, dbeta=ONE, P=24, Cc=16, act=LEAKY001, dtype=0, ws=ONE, nbytes=None):
    from causal_vae_amd import _lib as L
    nbytes = L.lib.cvae_bn2d_batch_bwd_workspace_bytes(24, 16) if nbytes is None else nbytes
    return L.lib.cvae_bn2d_batch_bwd(y, dy, a, gamma, mean, rstd, dx, dgamma, dbeta, P, Cc, act, dtype, ws, nbytes, None)


def test_act_codes_are_the_headers():
    from causal_vae_amd import _lib as L
    assert (L.act_code(None), L.act_code("leaky02"), L.act_code("leaky001")) == (NONE, LEAKY02, LEAKY001)


def test_residual_forward_refusals():
    from causal_vae_amd import _lib as L
    assert len(L.SIGNATURES["cvae_bn2d_batch_fwd_res"]) == 18
    for act in (1, 2, LEAKY02, LEAKY001):
        assert res(act=act) == E_UNSUPPORTED, act                      # a residual behind an activation
    for name in ("y", "gamma", "beta", "a", "mean", "rstd", "ws"):
        assert res(**{name: None}) == E_NULLPTR, name
    assert res(rm=None) == E_NULLPTR and res(rv=None) == E_NULLPTR
    for name in ("y", "a", "resid"):
        assert res(**{name: C.c_void_p(72)}) == E_UNSUPPORTED, name
    for name in ("gamma", "beta", "mean", "rstd", "rm", "rv", "ws"):
        assert res(**{name: C.c_void_p(66)}) == E_UNSUPPORTED, name
    assert res(nbytes=L.lib.cvae_bn2d_batch_workspace_bytes(24, 16) - 1) == E_WORKSPACE
    assert res(Cc=12) == E_BADSHAPE and res(Cc=0) == E_BADSHAPE and res(Cc=2056) == E_BADSHAPE and res(P=1) == E_BADSHAPE
    assert res(momentum=1.5) == E_BADSHAPE and res(eps=0.0) == E_BADSHAPE and res(act=5) == E_UNSUPPORTED
    assert res(dtype=2) == E_DTYPE and res(dtype=-1) == E_DTYPE
    if not torch.cuda.is_available():                                  # valid arguments pass every check; without a device the launch itself fails
        assert res() == E_LAUNCH and res(dtype=1) == E_LAUNCH and res(rm=None, rv=None) == E_LAUNCH       # (with one, dummy pointers must never get this far)
        for act in (1, 2, LEAKY02, LEAKY001):
            assert res(act=act, resid=None) == E_LAUNCH                # no residual: the plain entry, every activation legal


def test_backward_refusals():
    from causal_vae_amd import _lib as L
    assert len(L.SIGNATURES["cvae_bn2d_batch_bwd"]) == 16 and L.lib.cvae_bn2d_batch_bwd_workspace_bytes.restype is C.c_size_t
    for name in ("y", "dy", "a", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta", "ws"):
        assert bwd(**{name: None}) == E_NULLPTR, name
    for name in ("y", "dy", "a", "dx"):
        assert bwd(**{name: C.c_void_p(72)}) == E_UNSUPPORTED, name    # 8-byte aligned only
    for name in ("gamma", "mean", "rstd", "dgamma", "dbeta", "ws"):
        assert bwd(**{name: C.c_void_p(66)}) == E_UNSUPPORTED, name    # float arrays: 4 bytes
    assert bwd(nbytes=L.lib.cvae_bn2d_batch_bwd_workspace_bytes(24, 16) - 1) == E_WORKSPACE and bwd(nbytes=0) == E_WORKSPACE
    assert bwd(Cc=12) == E_BADSHAPE and bwd(Cc=0) == E_BADSHAPE and bwd(Cc=4) == E_BADSHAPE and bwd(Cc=2056) == E_BADSHAPE
    assert bwd(P=1) == E_BADSHAPE and bwd(P=0) == E_BADSHAPE and bwd(P=-3) == E_BADSHAPE
    assert bwd(act=5) == E_UNSUPPORTED and bwd(act=-1) == E_UNSUPPORTED
    assert bwd(dtype=2) == E_DTYPE and bwd(dtype=7) == E_DTYPE and bwd(dtype=-1) == E_DTYPE
    assert bwd(act=NONE, a=None, dtype=2) == E_DTYPE                   # without an activation `a` is not asked for: the next failing check answers
    assert bwd(act=NONE, a=C.c_void_p(72), nbytes=0) == E_WORKSPACE    # .. nor is its alignment
    if not torch.cuda.is_available():
        for dtype in (0, 1):
            for act in range(5):
                assert bwd(dtype=dtype, act=act) == E_LAUNCH
            assert bwd(dtype=dtype, act=NONE, a=None) == E_LAUNCH


def test_workspace_bytes_is_monotone_in_P():
    from causal_vae_amd import _lib as L
    q = L.lib.cvae_bn2d_batch_bwd_workspace_bytes
    assert q(1, 16) == 0 and q(24, 12) == 0 and q(24, 4096) == 0       # what the entry refuses
    Ps = (2, 24, 256, 257, 3077, 262144, 262145, 262401, 1966080, 7864320, 1 << 30)
    sizes = [q(P, 16) for P in Ps]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    for P in Ps:                                                       # two fp32 rows (sum g, sum g xh) per chunk
        assert q(P, 16) >= 2 * br.parts(P) * 16 * 4
    assert (br.chunk_rows(262401), br.parts(262401), bb.runs(513)[0], len(bb.runs(513))) == (512, 513, (0, 33), 16)
    assert bb.runs(13) == [(g, g + 1) for g in range(13)] and bb.runs(1) == [(0, 1)] and bb.runs(960)[-1] == (900, 960)


CASES = [(P, Cc, bf, act) for bf in (False, True) for Cc, act in ((8, "leaky001"), (16, None), (16, "leaky001"), (64, "leaky02"), (128, None)) for P in (2, 24, 257, 3077)]


def _case(P, Cc, bf16, act):
    d = br.inputs(P, Cc, 200 + P + Cc, bf16)
    slope = bb.SLOPES[act]
    ref, err = br.forward(d["y"], d["gamma"], d["beta"], None, None, 0.1, 1e-5, slope=1.0 if slope is None else slope, bf16=bf16)
    return d, slope, ref, err


@pytest.mark.parametrize("P,Cc,bf16,act", CASES)
def test_the_bounds_hold_for_an_fp32_evaluation_in_the_kernels_order(P, Cc, bf16, act):
    d, slope, ref, err = _case(P, Cc, bf16, act)
    fw = br.emulate_fp32(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5, slope=1.0 if slope is None else slope)
    mask = None if slope is None else fw["a"].double() > 0             # the masks of the forward that ran
    bref, berr = bb.backward(d["y"], d["dy"], mask, d["gamma"], ref["mean"], ref["rstd"], err["mean"], err["rstd"], slope, bf16)
    auto = bb.autograd_backward(d["y"], d["dy"], mask, d["gamma"], d["beta"], 1e-5, slope)
    for k in auto:                                                     # the restatement that carries the bound IS autograd's function
        assert float((auto[k] - bref[k]).abs().max()) <= 1e-10 * max(float(auto[k].abs().max()), 1e-30), k
        assert bool((berr[k] > 0).all()), k
    got = bb.emulate_bwd_fp32(d["y"], d["dy"], fw["a"], d["gamma"], fw["mean"], fw["rstd"], slope)
    for k in ("dx", "dgamma", "dbeta"):
        assert br.max_ratio(got[k], bref[k], berr[k]) <= 1.0, k
    if not bf16 and P >= 24:                                           # .. and they are no blank cheque: two wrong kernels are outside
        for variant in ("no_dgamma", "p_minus_1"):
            wrong = bb.emulate_bwd_fp32(d["y"], d["dy"], fw["a"], d["gamma"], fw["mean"], fw["rstd"], slope, variant)
            assert br.max_ratio(wrong["dx"], bref["dx"], berr["dx"]) > 1.0, variant


@pytest.mark.parametrize("P,Cc,bf16", [(P, Cc, bf) for bf in (False, True) for Cc in (16, 128) for P in (2, 24, 257, 3077)])
def test_the_residual_forward_bounds_hold_for_an_fp32_evaluation(P, Cc, bf16):
    d = br.inputs(P, Cc, 300 + P + Cc, bf16)
    resid = d["dy"]                                                    # any tensor of y's shape and dtype
    ref, err = bb.forward_res(d["y"], resid, d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5, bf16)
    got = bb.emulate_res_fp32(d["y"], resid, d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5)
    for k in ("mean", "rstd", "a", "running_mean", "running_var"):
        assert br.max_ratio(got[k], ref[k], err[k]) <= 1.0, k
    assert br.max_ratio(got["a"].double() - resid.double(), ref["a"], err["a"]) > 1.0      # the sum without its residual is outside
    bn = torch.nn.BatchNorm2d(Cc, eps=br.f32(1e-5), momentum=br.f32(0.1)).double()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]), bn.bias.copy_(d["beta"]), bn.running_mean.copy_(d["rm"]), bn.running_var.copy_(d["rv"])
    a = (resid.double() + bn.train()(d["y"].double().t().reshape(1, Cc, P, 1)).reshape(Cc, P).t()).detach()
    assert float((ref["a"] - a).abs().max()) <= 1e-12 * max(float(a.abs().max()), 1.0)


def test_keywords_and_guards():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import CausalViTVAE, ViTVAE
    vae = ViTVAE(img_size=(64, 96), depth=1).eval()
    assert vae._decoder_batch_stats is False
    vae.train_decoder(batch_stats=True)
    assert vae._decoder_batch_stats is True and vae._decoder_grads and not vae.training and not any(m.training for m in vae.decoder.modules())
    vae.train_decoder()
    assert vae._decoder_batch_stats is False                             # the default is the running-statistics form
    vae.train_decoder(batch_stats=True)
    vae.freeze_decoder()
    assert vae._decoder_batch_stats is False and not any(p.requires_grad for p in vae.decoder.parameters())
    assert len(vae.train_all(decoder_batch_stats=True)) == len(list(vae.parameters())) and vae._decoder_batch_stats and not vae._stem_batch_stats
    vae.train_all(stem_batch_stats=True)
    assert not vae._decoder_batch_stats and vae._stem_batch_stats
    vae.train_all(stem_batch_stats=True, decoder_batch_stats=True)
    assert vae._decoder_batch_stats and vae._stem_batch_stats
    with pytest.raises(CvaeError, match="training walk"):
        vae._decode_walk(torch.zeros(2, 128), False, batch_stats=True)
    vae.train()
    with pytest.raises(RuntimeError, match="eval mode"):                 # .train() is refused as before, with the text it had
        vae.decode_with_grad(torch.zeros(2, 128))
    with pytest.raises(RuntimeError, match="batch-statistics BatchNorm2d is not implemented"):
        vae.decode(torch.zeros(2, 128))

    model = CausalViTVAE(img_size=(64, 96), depth=1)
    with pytest.raises(CvaeError, match="decoder=True"):
        model.train_adapters(decoder_batch_stats=True)
    with pytest.raises(CvaeError, match="decoder=True"):
        model.train_adapters(transformer=True, decoder_batch_stats=True)
    model.train_adapters(decoder=True, decoder_batch_stats=True)
    assert model.backbone._decoder_batch_stats and not model.backbone.training
    model.train_adapters(decoder=True)
    assert not model.backbone._decoder_batch_stats
    model.train_adapters(decoder=True, decoder_batch_stats=True)
    model.train_adapters()
    assert not model.backbone._decoder_batch_stats


def test_the_batch_statistics_walk_is_the_reference_train_mode_decoder():
    """tests/vit_decoder_bn_reference.py's float64 restatement of the decoder equals torch's own nn decoder under .train() in float64: the image, the 48
    gradients, dz, the 22 running statistics and the 11 counters"""
    import vit_decoder_bn_reference as db
    from causal_vae_amd.vit import ViTVAE
    torch.manual_seed(0)
    vae = ViTVAE(img_size=(64, 96), depth=1)
    db.randomize_decoder_bn(vae, 1)
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    gen = torch.Generator().manual_seed(4)
    z = torch.randn(3, 128, generator=gen)
    g_img = torch.randn(3, 1, 64, 96, generator=gen, dtype=torch.float64)
    auto = db.torch_train_decoder(sd, z, g_img, torch.float64)
    fw = db.decoder_bn_forward(sd, z, (2, 3))
    got = db.decoder_bn_vjp(sd, z, g_img, (2, 3), db.masks_of(fw), forward=fw)
    same = lambda a, b, floor=1e-300: float((a - b).abs().max()) <= 1e-10 * max(float(b.abs().max()), floor)
    assert same(fw["image"], auto["image"]) and same(got["dz"], auto["dz"])
    assert len(db.PARAM_KEYS) == 48 and len(db.CONV_BIAS_KEYS) == 11 and len(db.BUFFER_KEYS) == 33
    for k in db.PARAM_KEYS:
        scale = float(auto[k.replace(".bias", ".weight")].abs().max()) if k in db.CONV_BIAS_KEYS else 1e-300      # zero in exact arithmetic
        assert same(got[k], auto[k], scale), k
    for k in db.BUFFER_KEYS:                                             # the restatement's momentum is the fp32 constant 0.1f = 0.1 (1 + 1.5e-8)
        if k.endswith("num_batches_tracked"):
            assert int(fw["buffers"][k]) == int(auto["buffers"][k]) == int(sd[k]) + 1, k
        else:
            assert float((fw["buffers"][k].double() - auto["buffers"][k].double()).abs().max()) <= 1e-7 * float(auto["buffers"][k].double().abs().max()), k
