"""GPU tests of the ViT-VAE stem on batch-statistics BatchNorm2d (train_stem(batch_stats=True)): the stem cut at its boundary against the float64
restatement of tests/vit_stem_bn_reference.py (five Conv2d + training-mode BatchNorm2d + LeakyReLU layers; it takes the HIP forward's LeakyReLU masks), the
running statistics, the entries that must not change (inference and probe entries, the flag clear), the captured step and CausalViTVAE.

The rules.  fp32: a tensor may lie at most 6 x as far from the float64 restatement as torch's own fp32 CPU evaluation of the same nn.Sequential(...).train()
lies from its float64 evaluation (L2 distances per tensor: the rule of tests/test_vit_stem_grad.py::test_stem_gradients_against_the_golden).  bf16 (torch's
fp32 distance says nothing about bf16 storage): at most 2 x the distance of the ROUNDING ORACLE — the float64 restatement rounded to bf16 where the kernels store
bf16 — from float64, §16's rule for bf16 (a tensor the oracle does not move at all keeps the fp32 rule, as there).  The five conv-bias gradients are zero in exact arithmetic (the batch mean is subtracted behind them): they are held
element-wise to the absolute rounding bound vit_stem_bn_reference.conv_bias_bound, as gr.k_bias_bound holds the zero third of in_proj_bias.  The running
statistics are held twice: element-wise, per layer, to the kernel test's bound on float64 statistics of the conv output the kernel READ
(tests/bn2d_batch_reference.py), and to the distance rule against the whole restatement.

Measured on the MI355X (the RATIO lines of the run).  The distance rule, worst tensor per case as ratio / allowed: fp32 0.238 (64 x 96, B = 2), 0.224 (B = 3, with
x.grad), 0.234 (96 x 64) — 1.35 to 1.43 times torch's own fp32 distance where 6 are allowed; bf16 0.501 and 0.509 — every tensor 0.91 to 1.02 times the rounding
oracle's distance where 2 are allowed (the last layer's dbeta, which the oracle does not move, under the fp32 rule).  Conv-bias gradients, max |got| / bound:
fp32 0.0003 - 0.023 (|got| at most 7.7e-6 next to weight gradients of 3 to 7), bf16 0.20 - 0.36.  Running statistics against float64 on the conv output the
kernel read, max over the five layers: running_mean 0.35 (fp32) and running_var 0.42 (fp32) of the bound, bf16 no higher.  The HIP forward's LeakyReLU masks
equal the float64 restatement's own in fp32 (0 of 187392 / 281088 signs differ) and differ in 135 / 223 signs in bf16.  None is above 1."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as vd  # noqa: E402
import bn2d_batch_reference as br  # noqa: E402
import vit_stem_bn_reference as sb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CASES = [((64, 96), 2, F32, False), ((64, 96), 2, BF16, False), ((64, 96), 3, F32, True), ((64, 96), 3, BF16, True), ((96, 64), 2, F32, False)]
IDS = [f"{h}x{w}-B{B}-{'bf16' if dt == BF16 else 'f32'}{'-dx' if wx else ''}" for (h, w), B, dt, wx in CASES]


def encoder(img, dtype=F32, seed=0):
    from causal_vae_amd.vit.models import ViTVAEEncoder
    torch.manual_seed(seed)
    model = ViTVAEEncoder(img_size=img, depth=2, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    model.requires_grad_(False)
    return model.to(DEV).eval().set_compute_dtype(dtype)


def buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked")}


def unchanged(model, was, what):
    now = buffers(model)
    assert now.keys() == was.keys() and all(torch.equal(now[k], was[k]) for k in was), f"{what} changed a BatchNorm buffer"


def nchw(t):
    return t.detach().cpu().squeeze(1).permute(0, 3, 1, 2)


def hip_stem(model, x):
    """the HIP training walk's stem alone, on a copy of the model (its buffers move, the model's do not) -> the kept dict of _stem_cl"""
    kept = {}
    with torch.no_grad():
        copy.deepcopy(model)._stem_cl(x, kept, batch_stats=True)
    return kept


def dist(a, b):
    return float((a.detach().cpu().double().reshape(b.shape) - b.double()).norm())


def hold(label, got, r64, own):
    """got within factor x the yardstick's L2 distance from float64 of r64, per tensor (L2); own[k] = (that distance, factor)"""
    worst = (0.0, None)
    for k, g in got.items():
        mine, (own_k, factor) = dist(g, r64[k]), own[k]
        ratio = mine / own_k if own_k > 0 else (0.0 if mine == 0 else float("inf"))
        print(f"{label} {k}: |HIP - float64| {mine:.3e}, yardstick {own_k:.3e}, ratio {ratio:.3f} (allowed {factor})")
        worst = max(worst, (ratio / factor, k))
    print(f"RATIO {label}: worst ratio / allowed {worst[0]:.4f} ({worst[1]})")
    assert worst[0] <= 1.0, (label, worst)


@pytest.mark.parametrize("img,B,dtype,wants_x", CASES, ids=IDS)
def test_stem_cut_at_its_boundary(img, B, dtype, wants_x):
    bf = dtype == BF16
    model = encoder(img, dtype)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x = vr.vit_inputs(B, *img, seed=5).to(DEV)
    model.train_transformer()
    params = model.train_stem(batch_stats=True)
    assert not model.training and not any(m.training for m in model.stem)
    kept = hip_stem(model, x)
    masks = [nchw(a) > 0 for a in kept["ys"]]
    was = buffers(model)
    if wants_x:
        x.requires_grad_(True)
    col = {}
    c = model.cls_features_with_grad(x, col)
    c.backward(torch.randn(B, 256, generator=torch.Generator().manual_seed(3)).to(DEV))
    dstem = col["dstem"].detach().cpu().double()
    assert len(col["stem_g"]) == 5 and all(g.dtype == dtype for g in col["stem_g"]) and col["stem"].dtype == dtype

    xc = x.detach().cpu()
    fw = sb.stem_bn_forward(sd, xc)
    flips = sum(int((m != (a > 0)).sum()) for m, a in zip(masks, fw["a"]))
    print(f"LeakyReLU masks: {flips} of {sum(m.numel() for m in masks)} signs of the HIP forward differ from the float64 restatement's own")
    r64 = sb.stem_bn_vjp(sd, xc, dstem, masks=masks, want_dx=True, forward=fw)
    r64["stem"] = fw["stem"]
    r64.update(fw["buffers"])
    names = [k for k in sb.STEM_KEYS if k not in sb.CONV_BIAS_KEYS] + ["stem", "dx"] + [k for k in sb.BUFFER_KEYS if "num_batches" not in k]
    t64, t32 = sb.torch_train_stem(sd, xc, dstem, F64), sb.torch_train_stem(sd, xc, dstem, F32)
    for t in (t64, t32):
        t.update(t.pop("buffers"))
    own = {k: (dist(t32[k], t64[k]), 6.0) for k in names}                  # torch's fp32 evaluation's distance from torch's float64 evaluation
    if bf:                                                                 # the rounding oracle's distance from float64
        ofw = sb.stem_bn_forward(sd, xc, rnd=vr.round_bf16)
        yard = sb.stem_bn_vjp(sd, xc, dstem, masks=masks, want_dx=True, rnd=vr.round_bf16, forward=ofw)
        yard["stem"] = ofw["stem"]
        yard.update(ofw["buffers"])
        # a zero gap (the last layer's dbeta: sums of the bf16 cotangent itself, nothing is rounded on the way) leaves the fp32 rule, as §16's check does
        own = {k: (dist(yard[k], r64[k]), 2.0) if dist(yard[k], r64[k]) > 0.0 else own[k] for k in names}
    label = IDS[CASES.index((img, B, dtype, wants_x))]
    got = {k: p.grad for k, p in zip(sb.STEM_KEYS, params) if k not in sb.CONV_BIAS_KEYS}
    got["stem"] = col["stem"].view(B, -1, 256)
    if wants_x:
        assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == F32
        got["dx"] = x.grad
    now = buffers(model)
    got.update({k: now[k] for k in sb.BUFFER_KEYS if "num_batches" not in k})
    hold(label, got, r64, own)
    for j, k in enumerate(sb.CONV_BIAS_KEYS):                              # zero in exact arithmetic: an absolute rounding bound, element-wise
        g = dict(zip(sb.STEM_KEYS, params))[k].grad.detach().cpu().double()
        bound = sb.conv_bias_bound(fw, r64, masks, sd, j, bf)
        r = float((g.abs() / bound).max())
        print(f"{label} {k}: max |got| / bound = {r:.4f} (max |got| {float(g.abs().max()):.3e}, weight gradient's max {float(r64[k.replace('.bias', '.weight')].abs().max()):.3e})")
        assert torch.isfinite(g).all() and r <= 1.0, (k, r)
    # the running statistics, element-wise: float64 statistics of the conv output the kernel read, within the kernel test's bound; the counters
    for j in range(5):
        b = f"stem.{3 * j + 1}"
        y = kept["pre"][j].detach().cpu().reshape(-1, sb.CHANNELS[j])
        ref, err = br.forward(y, sd[f"{b}.weight"], sd[f"{b}.bias"], sd[f"{b}.running_mean"], sd[f"{b}.running_var"], sb.MOMENTUM, sb.EPS, bf16=bf)
        for n in ("running_mean", "running_var"):
            r = br.max_ratio(now[f"{b}.{n}"], ref[n], err[n])
            print(f"RATIO {label} {b}.{n} {r:.4f}")
            assert r <= 1.0, (b, n, r)
        assert int(now[f"{b}.num_batches_tracked"]) == int(was[f"{b}.num_batches_tracked"]) + 1
        assert y.shape[0] == B * (img[0] >> (j + 1)) * (img[1] >> (j + 1))


def test_inference_and_probe_entries_keep_the_fold_and_the_buffers():
    model = encoder((64, 96))
    x = vr.vit_inputs(2, 64, 96, seed=5).to(DEV)
    with torch.no_grad():
        want = {"cls": model.cls_features(x), "enc": model.encode(x), "sal": model.saliency(x), "cam": model.gradcam(x),
                "vjp": model.encode_vjp(x, torch.ones(2, 128, device=DEV)), "att": model.attention_weights(x), "roll": model.attention_rollout(x)}
    model.train_transformer()
    model.train_stem(batch_stats=True)
    was = buffers(model)
    with torch.no_grad():
        got = {"cls": model.cls_features(x), "enc": model.encode(x), "sal": model.saliency(x), "cam": model.gradcam(x),
               "vjp": model.encode_vjp(x, torch.ones(2, 128, device=DEV)), "att": model.attention_weights(x), "roll": model.attention_rollout(x)}
        assert torch.equal(model.cls_features_with_grad(x), want["cls"])       # autograd off: cls_features
    for k in want:
        a, b = (got[k], want[k]) if isinstance(want[k], tuple) else ((got[k],), (want[k],))
        assert all(torch.equal(u, v) for u, v in zip(a, b)), k                  # the parent's bits: the fold on the running statistics
        unchanged(model, was, k)
    xg = x.clone().requires_grad_(True)                                        # only the image asks, through frozen parameters: the fold again
    model.freeze_stem(), model.freeze_transformer()
    model._stem_batch_stats = True                                             # even with the flag left set
    c = model.cls_features_with_grad(xg)
    assert torch.equal(c.detach(), want["cls"])
    c.sum().backward()
    unchanged(model, was, "x.grad through frozen parameters")


def test_flag_clear_is_the_old_behaviour():
    model = encoder((64, 96))
    x = vr.vit_inputs(2, 64, 96, seed=5).to(DEV)
    with torch.no_grad():
        c0 = model.cls_features(x)
    model.train_transformer()
    model.train_stem(batch_stats=True)
    g = torch.randn(2, 256, generator=torch.Generator().manual_seed(3)).to(DEV)
    c = model.cls_features_with_grad(x)
    assert not torch.equal(c.detach(), c0)                                     # batch statistics: other values than the running statistics give
    c.backward(g)
    model.zero_grad(set_to_none=True)
    vr.randomize_stem_bn(model.stem, 1)                                        # the buffers as they were
    for i in range(1, 15, 3):
        model.stem[i].num_batches_tracked.zero_()
    for clear in (lambda: model.train_stem(), lambda: (model.freeze_stem(), model.train_stem())):
        model.train_stem(batch_stats=True)
        clear()
        was = buffers(model)
        col = {}
        c = model.cls_features_with_grad(x, col)
        assert torch.equal(c.detach(), c0)                                     # the forward: cls_features' bits
        c.backward(g)
        unchanged(model, was, "the eval-mode training walk")
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.stem.parameters())
        grads = [p.grad.clone() for p in model.stem.parameters()]
        model.zero_grad(set_to_none=True)
    fresh = encoder((64, 96))                                                  # .. and the gradients are those of a model that never saw the flag
    fresh.train_transformer()
    fresh.train_stem()
    fresh.cls_features_with_grad(x).backward(g)
    assert all(torch.equal(a, p.grad) for a, p in zip(grads, fresh.stem.parameters()))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_captured_step_equals_eager(dtype):
    import test_vit_train_graph as tg
    from causal_vae_amd.vit import vit_vae_train_step
    start = tg.vitvae(False, dtype)
    start.train_all(stem_batch_stats=True)
    batches, noises = tg.vit_batches()
    me = copy.deepcopy(start)
    oe, le = tg.eager_run(me, me.parameters(), vit_vae_train_step, batches, noises, beta=0.7)
    mc = copy.deepcopy(start)
    assert mc._stem_batch_stats
    oc, lc = tg.captured_run(mc, mc.parameters(), batches, noises, beta=0.7)
    for i, (a, b) in enumerate(zip(le, lc)):
        print(f"step {i}: eager loss {float(a[0])!r}, captured loss {float(b[0])!r}")
        assert torch.equal(a[0], b[0]), f"loss of step {i}"
    tg.assert_same_training_state(me, oe, mc, oc, "captured against eager")          # parameters, Adam moments, running statistics, counters
    moved = [k for k, v in buffers(me).items() if k.startswith("stem.") and not torch.equal(v, start.state_dict()[k])]
    assert len(moved) == 15, moved                                              # five layers' running_mean, running_var, num_batches_tracked
    assert all(int(me.stem[i].num_batches_tracked) == 3 == int(mc.stem[i].num_batches_tracked) for i in range(1, 15, 3))
    assert all(torch.equal(v, start.state_dict()[k]) for k, v in buffers(me).items() if k.startswith("decoder."))     # the decoder stays on running statistics


def test_causal_vitvae_takes_a_step_on_batch_statistics():
    import test_vit_train_graph as tg
    from causal_vae_amd import FusedAdam
    from causal_vae_amd.vit import causal_vit_train_step
    from causal_vae_amd.vit.causal import CausalViTVAE
    torch.manual_seed(5)
    model = CausalViTVAE(img_size=tg.IMG, depth=tg.DEPTH)
    vd.randomize_decoder_bn(model.backbone.decoder, 6)
    vr.randomize_stem_bn(model.backbone.stem, 7)
    model = model.to(DEV)
    params = model.train_adapters(decoder=True, transformer=True, stem=True, stem_batch_stats=True)
    assert model.backbone._stem_batch_stats and not model.backbone.training
    was = buffers(model.backbone)
    batches, noises = tg.causal_batches(model, 1)
    opt = FusedAdam(params, lr=1e-3)
    out = causal_vit_train_step(model, opt, *batches[0], eps=noises[0])
    assert all(torch.isfinite(t).all() for t in out)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    now = buffers(model.backbone)
    for i in range(1, 15, 3):
        assert not torch.equal(now[f"stem.{i}.running_mean"], was[f"stem.{i}.running_mean"]) and not torch.equal(now[f"stem.{i}.running_var"], was[f"stem.{i}.running_var"])
        assert int(now[f"stem.{i}.num_batches_tracked"]) == int(was[f"stem.{i}.num_batches_tracked"]) + 1
    assert all(torch.equal(v, was[k]) for k, v in now.items() if k.startswith("decoder."))
