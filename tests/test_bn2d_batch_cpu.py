"""The batch-statistics stem without a GPU: cvae_bn2d_batch_fwd's argument checks (every one precedes the first launch, so dummy pointers are
never read), the workspace query, the yardstick of tests/test_bn2d_batch.py held against an fp32 CPU evaluation of the kernel's formulas and against
autograd, and the keyword plumbing of train_stem / train_all / train_adapters."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bn2d_batch_reference as br  # noqa: E402

OK, E_BADSHAPE, E_DTYPE, E_UNSUPPORTED, E_WORKSPACE, E_LAUNCH, E_NULLPTR = 0, -1, -2, -3, -4, -5, -6
ONE = C.c_void_p(64)                                                   # non-null, 16-byte aligned, never read: each case ends in a check


def fwd(y=ONE, gamma=ONE, beta=ONE, a=ONE, mean=ONE, rstd=ONE, rm=ONE, rv=ONE, P=12, Cc=32, momentum=0.1, eps=1e-5, act=4, dtype=0, ws=ONE, nbytes=None):
    from causal_vae_amd import _lib as L
    nbytes = L.lib.cvae_bn2d_batch_workspace_bytes(12, 32) if nbytes is None else nbytes
    return L.lib.cvae_bn2d_batch_fwd(y, gamma, beta, a, mean, rstd, rm, rv, P, Cc, momentum, eps, act, dtype, ws, nbytes, None)


def test_refusals_come_with_the_documented_codes():
    from causal_vae_amd import _lib as L
    assert len(L.SIGNATURES["cvae_bn2d_batch_fwd"]) == 17 and L.lib.cvae_bn2d_batch_workspace_bytes.restype is C.c_size_t
    for name in ("y", "gamma", "beta", "a", "mean", "rstd", "ws"):
        assert fwd(**{name: None}) == E_NULLPTR, name
    assert fwd(rm=None) == E_NULLPTR and fwd(rv=None) == E_NULLPTR     # the running buffers come together
    for name in ("y", "a"):
        assert fwd(**{name: C.c_void_p(72)}) == E_UNSUPPORTED, name    # 8-byte aligned only
    for name in ("gamma", "beta", "mean", "rstd", "rm", "rv", "ws"):
        assert fwd(**{name: C.c_void_p(66)}) == E_UNSUPPORTED, name    # float arrays: 4 bytes
    assert fwd(nbytes=L.lib.cvae_bn2d_batch_workspace_bytes(12, 32) - 1) == E_WORKSPACE and fwd(nbytes=0) == E_WORKSPACE
    assert fwd(Cc=36) == E_BADSHAPE and fwd(Cc=0) == E_BADSHAPE and fwd(Cc=4) == E_BADSHAPE and fwd(Cc=2056) == E_BADSHAPE
    assert fwd(P=1) == E_BADSHAPE and fwd(P=0) == E_BADSHAPE and fwd(P=-3) == E_BADSHAPE      # torch: "Expected more than 1 value per channel"
    assert fwd(dtype=2) == E_DTYPE and fwd(dtype=7) == E_DTYPE and fwd(dtype=-1) == E_DTYPE
    for m in (-0.01, 1.01, float("nan"), float("inf")):
        assert fwd(momentum=m) == E_BADSHAPE, m
    for e in (0.0, -1e-5, float("nan")):
        assert fwd(eps=e) == E_BADSHAPE, e
    assert fwd(act=5) == E_UNSUPPORTED and fwd(act=-1) == E_UNSUPPORTED
    assert fwd(rm=None, rv=None, nbytes=0) == E_WORKSPACE              # untracked statistics are legal: the next check answers
    if not torch.cuda.is_available():                                  # valid arguments pass every check; without a device the launch itself fails
        for dtype in (0, 1):
            for act in range(5):
                assert fwd(dtype=dtype, act=act) == E_LAUNCH
        assert fwd(momentum=0.0) == E_LAUNCH and fwd(momentum=1.0) == E_LAUNCH and fwd(rm=None, rv=None) == E_LAUNCH


def test_workspace_bytes():
    from causal_vae_amd import _lib as L
    q = L.lib.cvae_bn2d_batch_workspace_bytes
    assert q(1, 32) == 0 and q(12, 36) == 0 and q(12, 4096) == 0       # what the entry refuses
    sizes = [q(P, 64) for P in (2, 12, 256, 257, 3077, 7680, 262144, 262145, 1966080, 1 << 30)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    for P in (2, 257, 3077, 262145, 1966080):                          # two fp32 rows (mean, M2) per chunk, at most 1024 chunks, chunks of whole 256-row units
        assert q(P, 64) == 2 * min((P + 255) // 256, 1024) * 64 * 4 >= 2 * br.parts(P) * 64 * 4 and br.parts(P) <= 1024 and br.chunk_rows(P) % 256 == 0
    assert br.parts(262144) == 1024 and br.parts(262145) == 513        # why the query is not the chunk count itself: that one is not monotone
    assert (br.parts(256), br.parts(257), br.parts(3077), br.chunk_rows(1966080), br.parts(1966080)) == (1, 2, 13, 2048, 960)
    assert q(3077, 256) == 4 * q(3077, 64)


CASES = [(P, Cc, bf) for bf in (False, True) for Cc in (32, 256) for P in (2, 12, 257, 3077)]


@pytest.mark.parametrize("P,Cc,bf16", CASES)
def test_the_bounds_hold_for_an_fp32_evaluation(P, Cc, bf16):
    d = br.inputs(P, Cc, 100 + P + Cc, bf16)
    ref, err = br.forward(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5, bf16=bf16)
    got = br.emulate_fp32(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5)
    for k in got:
        assert br.max_ratio(got[k], ref[k], err[k]) <= 1.0, k
    # .. and they are no blank cheque: a variance off by one part in a thousand, or a mean off by a hundredth of a standard deviation, is outside
    if P >= 257:
        assert br.max_ratio(ref["var"] * 1.001, ref["var"], err["var"]) > 1.0
        assert br.max_ratio(ref["mean"] + 0.01 * ref["var"].sqrt(), ref["mean"], err["mean"]) > 1.0
    # torch's own training-mode BatchNorm2d in float64 is the reference
    bn = torch.nn.BatchNorm2d(Cc, eps=br.f32(1e-5), momentum=br.f32(0.1)).double()   # the fp32 constants the C ABI receives
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]), bn.bias.copy_(d["beta"]), bn.running_mean.copy_(d["rm"]), bn.running_var.copy_(d["rv"])
    a = torch.nn.functional.leaky_relu(bn.train()(d["y"].double().t().reshape(1, Cc, P, 1)), br.f32(0.01)).reshape(Cc, P).t()
    same = lambda x, y: float((x - y).abs().max()) <= 1e-12 * max(float(y.abs().max()), 1.0)
    assert same(ref["a"], a.detach()) and same(ref["running_mean"], bn.running_mean) and same(ref["running_var"], bn.running_var)


def test_the_cancellation_input_discriminates():
    """channels 1000 + 0.01 N(0, 1): the shifted sums stay inside the bound, the float32 E[y^2] - E[y]^2 formula misses the variance by thousands of bounds"""
    d = br.inputs(3077, 32, 100 + 3077 + 32, False, cancel=True)
    ref, err = br.forward(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5)
    got = br.emulate_fp32(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], 0.1, 1e-5)
    for k in got:
        assert br.max_ratio(got[k], ref[k], err[k]) <= 1.0, k
    naive = br.naive_var_fp32(d["y"])
    assert float(ref["var"].max()) < 1.3e-4 and float((naive - ref["var"]).abs().max()) > 0.01
    assert br.max_ratio(naive, ref["var"], err["var"]) > 1000.0


@pytest.mark.parametrize("bf16", [False, True])
def test_the_backward_restatement_is_autograds(bf16):
    d = br.inputs(257, 32, 3, bf16)
    ref, err = br.forward(d["y"], d["gamma"], d["beta"], None, None, 0.1, 1e-5, bf16=bf16)
    mask = ref["v"] > 0
    assert bool(mask.any()) and not bool(mask.all())
    bref, berr = br.backward(d["y"], d["dy"], mask, d["gamma"], ref["mean"], ref["rstd"], err["mean"], err["rstd"], bf16=bf16)
    auto = br.autograd_backward(d["y"], d["dy"], mask, d["gamma"], d["beta"], 1e-5)
    for k in auto:
        assert float((auto[k] - bref[k]).abs().max()) <= 1e-12 * float(auto[k].abs().max()), k
        assert bool((berr[k] > 0).all())
    wrong = br.backward(d["y"], d["dy"], mask, d["gamma"], ref["mean"], ref["rstd"], err["mean"], err["rstd"], slope=0.2, bf16=bf16)[0]
    assert br.max_ratio(wrong["dx"], bref["dx"], berr["dx"]) > 1.0      # another slope is outside the bound


def test_keywords_and_guards():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import CausalViTVAE, ViTVAE, ViTVAEEncoder
    enc = ViTVAEEncoder(img_size=(64, 96), depth=1).eval()
    enc.requires_grad_(False)
    assert enc._stem_batch_stats is False
    params = enc.train_stem(batch_stats=True)
    assert enc._stem_batch_stats is True and len(params) == 20 and all(p.requires_grad for p in params)
    assert not enc.training and not any(m.training for m in enc.stem)                        # asked by keyword: the module stays in eval mode
    enc.train_stem()
    assert enc._stem_batch_stats is False                                                     # the default is the running-statistics form
    enc.train_stem(batch_stats=True)
    enc.freeze_stem()
    assert enc._stem_batch_stats is False and not any(p.requires_grad for p in enc.stem.parameters())
    enc.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        enc.train_stem(batch_stats=True)
    assert enc._stem_batch_stats is False
    with pytest.raises(RuntimeError, match="eval mode"):                                      # .train() is refused as before
        enc.cls_features(torch.zeros(2, 1, 64, 96))
    with pytest.raises(CvaeError, match="training walk"):
        enc.eval()._walk(torch.zeros(2, 1, 64, 96), stem_batch_stats=True)

    vae = ViTVAE(img_size=(64, 96), depth=1).eval()
    assert len(vae.train_all(stem_batch_stats=True)) == len(list(vae.parameters())) and vae._stem_batch_stats
    vae.train_all()
    assert not vae._stem_batch_stats

    model = CausalViTVAE(img_size=(64, 96), depth=1)
    with pytest.raises(CvaeError, match="stem=True"):
        model.train_adapters(transformer=True, stem_batch_stats=True)
    with pytest.raises(CvaeError, match="stem=True"):
        model.train_adapters(stem_batch_stats=True)
    model.train_adapters(transformer=True, stem=True, stem_batch_stats=True)
    assert model.backbone._stem_batch_stats and not model.backbone.training
    model.train_adapters(transformer=True, stem=True)
    assert not model.backbone._stem_batch_stats
    model.train_adapters()
    assert not model.backbone._stem_batch_stats


def test_the_batch_statistics_walk_is_the_reference_train_mode_stem():
    """tests/vit_stem_bn_reference.py's float64 restatement of the five layers equals torch's nn.Sequential(...).train() in float64: values, the 20 gradients,
    the image's gradient and the running buffers"""
    import vit_stem_bn_reference as sb
    from causal_vae_amd.vit import ViTVAEEncoder
    import vit_reference as vr
    torch.manual_seed(0)
    enc = ViTVAEEncoder(img_size=(64, 96), depth=1)
    vr.randomize_stem_bn(enc.stem, 1)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    x = vr.vit_inputs(3, 64, 96, seed=5)
    dstem = torch.randn(3, 6, 256, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    auto = sb.torch_train_stem(sd, x, dstem, torch.float64)
    fw = sb.stem_bn_forward(sd, x)
    got = sb.stem_bn_vjp(sd, x, dstem, masks=[a > 0 for a in fw["a"]], want_dx=True)
    same = lambda a, b, floor=1e-300: float((a - b).abs().max()) <= 1e-11 * max(float(b.abs().max()), floor)
    assert same(fw["stem"], auto["stem"])
    for k in sb.STEM_KEYS:
        scale = float(auto[k.replace(".bias", ".weight")].abs().max()) if k in sb.CONV_BIAS_KEYS else 1e-300      # zero in exact arithmetic
        assert same(got[k], auto[k], scale), k
    assert same(got["dx"], auto["dx"])
    for k in sb.BUFFER_KEYS:                                             # the restatement's momentum is the fp32 constant 0.1f = 0.1 (1 + 1.5e-8)
        assert float((fw["buffers"][k].double() - auto["buffers"][k].double()).abs().max()) <= 1e-7 * float(auto["buffers"][k].double().abs().max()), k
