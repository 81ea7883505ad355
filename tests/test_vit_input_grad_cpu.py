"""CPU tests of the encoder's image gradient: the float64 yardstick of tests/vit_input_grad_reference.py against torch.autograd through an
independent restatement, its Grad-CAM against the reference class's arithmetic written out in numpy, its integrated gradients at one step, and the argument
checks of the two C entries, which answer before any device is touched."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_input_grad_reference as ir  # noqa: E402

F64 = torch.float64
IMG, DEPTH, B = (64, 96), 2, 3
_CASE = {}


def case():
    """state_dict, image and cotangents of the one CPU case, and the helper's float64 result: computed once, shared, never modified"""
    if not _CASE:
        from causal_vae_amd.vit.models import ViTVAEEncoder
        torch.manual_seed(0)
        model = ViTVAEEncoder(img_size=IMG, depth=DEPTH, latent_dim=128)
        vr.randomize_stem_bn(model.stem, 1)
        g = torch.Generator().manual_seed(21)
        _CASE.update(sd={k: v.detach().clone() for k, v in model.state_dict().items()}, x=vr.vit_inputs(B, *IMG, seed=5).to(F64),
                     g_mu=torch.randn(B, 128, generator=g).to(F64), g_lv=torch.randn(B, 128, generator=g).to(F64), g_cls=torch.randn(B, 256, generator=g).to(F64))
        c = _CASE
        c["ref"] = ir.image_vjp(c["sd"], c["x"], DEPTH, c["g_mu"], c["g_lv"])
    return _CASE


def test_image_vjp_equals_autograd_in_float64():
    c = case()
    x = c["x"].clone().requires_grad_(True)
    cls, mu, lv = ir.torch_encode(c["sd"], x, DEPTH)
    want, = torch.autograd.grad([mu, lv], [x], [c["g_mu"], c["g_lv"]], retain_graph=True)
    r = ir.rel_l2(c["ref"]["dx"], want)
    print(f"image_vjp (mu, log_var) vs autograd: rel-L2 {r:.3e}; forward mu {ir.rel_l2(c['ref']['mu'], mu):.3e}")
    assert c["ref"]["dx"].shape == (B, 1) + IMG and float(want.abs().max()) > 0 and r <= 1e-10
    for cls_only in (False, True):                                          # the CLS-only last block is the same function
        got = ir.image_vjp(c["sd"], c["x"], DEPTH, g_cls=c["g_cls"], cls_only=cls_only)["dx"]
        want_c, = torch.autograd.grad([cls], [x], [c["g_cls"]], retain_graph=True)
        r = ir.rel_l2(got, want_c)
        print(f"image_vjp (cls, cls_only={cls_only}) vs autograd: rel-L2 {r:.3e}")
        assert r <= 1e-10
    only_mu = ir.image_vjp(c["sd"], c["x"], DEPTH, g_mu=c["g_mu"])["dx"]
    want_m, = torch.autograd.grad([mu], [x], [c["g_mu"]])
    assert ir.rel_l2(only_mu, want_m) <= 1e-10


def numpy_gradcam(activations, gradients, normalize=True):
    """GradCAM.__call__'s arithmetic on one image's (C, H, W) arrays, without the resize: mean over the positions, weighted channel sum in channel order, relu,
    minus the min, over (max + 1e-8)"""
    weights = np.mean(gradients, axis=(1, 2))
    cam = np.zeros(activations.shape[1:], dtype=np.float64)
    for i, w in enumerate(weights):
        cam += w * activations[i]
    cam = np.maximum(cam, 0)
    if normalize:
        cam = cam - np.min(cam)
        cam = cam / (np.max(cam) + 1e-8)
    return cam


def test_gradcam_ref_equals_the_reference_arithmetic():
    rng = np.random.default_rng(3)
    for gh, gw, C in ((2, 3, 256), (4, 5, 256), (3, 3, 7)):
        A, dA = rng.standard_normal((2, C, gh, gw)), rng.standard_normal((2, C, gh, gw))
        cl = lambda a: torch.from_numpy(a).flatten(2).transpose(1, 2)      # `b c h w -> b (h w) c`, as the stem output
        for normalize in (True, False):
            got = ir.gradcam_ref(cl(A), cl(dA), normalize).reshape(2, gh, gw).numpy()
            want = np.stack([numpy_gradcam(A[b], dA[b], normalize) for b in range(2)])
            err = float(np.abs(got - want).max())
            print(f"gradcam_ref {gh}x{gw}x{C} normalize={normalize}: max |diff| {err:.2e}")
            assert err <= 1e-12
    A = np.abs(rng.standard_normal((1, 256, 2, 3)))
    neg = -np.ones((1, 256, 2, 3))                                         # every weight negative, every activation positive: an all-negative map
    cl = lambda a: torch.from_numpy(a).flatten(2).transpose(1, 2)
    assert float(ir.gradcam_ref(cl(A), cl(neg)).abs().max()) == 0.0 and float(np.abs(numpy_gradcam(A[0], neg[0])).max()) == 0.0
    const = np.ones((1, 256, 2, 3))                                        # a constant positive map: zeros by the 1e-8 rule
    got = ir.gradcam_ref(cl(const), cl(const))
    assert float(got.abs().max()) == 0.0 and float(np.abs(numpy_gradcam(const[0], const[0])).max()) == 0.0
    assert float(ir.gradcam_ref(cl(const), cl(const), normalize=False).min()) == 256.0


def test_integrated_gradients_with_one_step_is_the_midpoint_gradient():
    g = torch.Generator().manual_seed(4)
    x, base = torch.randn(2, 1, 4, 6, generator=g).to(F64), torch.randn(2, 1, 4, 6, generator=g).to(F64)
    grad = lambda p: torch.sin(p) + 2.0 * p
    got = ir.integrated_gradients(grad, x, base, 1)
    assert torch.equal(got, (x - base) * grad(base + 0.5 * (x - base)))
    assert float(ir.integrated_gradients(grad, x, x, 4).abs().max()) == 0.0
    # a quadratic's gradient is linear along the path: the midpoint rule is exact, so completeness holds to rounding
    f = lambda p: (p * p).sum()
    got = ir.integrated_gradients(lambda p: 2.0 * p, x, base, 3)
    assert abs(float(got.sum()) - float(f(x) - f(base))) <= 1e-12 * float(f(x) + f(base))


def test_entries_answer_bad_arguments_without_a_device():
    from causal_vae_amd import _lib as L
    lib = L.lib
    OK, BADSHAPE, DTYPE, UNSUPPORTED, NULLPTR = 0, -1, -2, -3, -6
    buf = (ctypes.c_char * (1 << 16))()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    g, w, dx = base, base + 16384, base + 32768                            # g: 2 x 2 x 3 x 32 floats = 1536 bytes; w: 2048 bytes; dx: 2 x 4 x 6 floats

    def image(g=g, w=w, dx=dx, B=2, sh=2, sw=3, Cs=32, lh=4, lw=6, nd=2, dt=L.F32, alpha=1.0, acc=0):
        return lib.cvae_conv_down_image_bwd_data(g, w, dx, B, sh, sw, Cs, lh, lw, nd, dt, alpha, acc, None)

    assert image(B=0) == OK and image(B=0, g=None, w=None, dx=None) == OK
    assert image(B=-1) == BADSHAPE and image(sh=0) == BADSHAPE and image(sw=-3) == BADSHAPE and image(lh=-4) == BADSHAPE and image(Cs=0) == BADSHAPE
    assert image(dt=2) == DTYPE and image(dt=-1) == DTYPE and image(dt=7, B=0) == DTYPE
    assert image(Cs=64) == UNSUPPORTED and image(Cs=16) == UNSUPPORTED and image(nd=3) == UNSUPPORTED
    assert image(lh=5) == UNSUPPORTED and image(lw=7) == UNSUPPORTED and image(B=1 << 31) == UNSUPPORTED and image(sh=1 << 20, sw=1 << 12, lh=1 << 21, lw=1 << 13) == UNSUPPORTED
    assert image(g=None) == NULLPTR and image(w=None) == NULLPTR and image(dx=None) == NULLPTR
    assert image(g=g + 8) == UNSUPPORTED and image(w=w + 2) == UNSUPPORTED and image(dx=dx + 1) == UNSUPPORTED
    for over in (g, g + 1532, w, w + 2044, g - 188, w - 188):             # dx (192 bytes) meets g's or w's first or last bytes
        assert image(dx=over) == UNSUPPORTED, over - base
    for dt, nbytes in ((L.F32, 1536), (L.BF16, 768)):                      # the extent of g follows its dtype
        assert image(dx=g + nbytes - 4, dt=dt) == UNSUPPORTED

    A, dA, cam = base, base + 16384, base + 32768                          # 2 x 6 x 256 floats = 12288 bytes each; cam 48 bytes

    def gradcam(A=A, dA=dA, cam=cam, B=2, n=6, normalize=1, dt=L.F32):
        return lib.cvae_gradcam256(A, dA, cam, B, n, normalize, dt, None)

    assert gradcam(B=0) == OK and gradcam(B=0, A=None, dA=None, cam=None) == OK
    assert gradcam(B=-1) == BADSHAPE and gradcam(n=0) == BADSHAPE and gradcam(n=-6) == BADSHAPE
    assert gradcam(dt=2) == DTYPE and gradcam(dt=-1) == DTYPE
    assert gradcam(n=4097) == UNSUPPORTED and gradcam(B=1 << 31) == UNSUPPORTED
    assert gradcam(A=None) == NULLPTR and gradcam(dA=None) == NULLPTR and gradcam(cam=None) == NULLPTR
    assert gradcam(A=A + 4) == UNSUPPORTED and gradcam(dA=dA + 8) == UNSUPPORTED and gradcam(cam=cam + 2) == UNSUPPORTED
    for over in (A, A + 12284, dA, dA + 12284, A - 44, dA - 44):
        assert gradcam(cam=over) == UNSUPPORTED, over - base
    assert gradcam(cam=A + 6140, dt=L.BF16) == UNSUPPORTED                 # bf16 inputs end at 6144 bytes: their last element is inside
