"""GPU tests of the ViT-VAE decoder on batch-statistics BatchNorm2d (train_decoder(batch_stats=True)): the decoder cut at its boundary (inputs z and
the image cotangent) against the float64 restatement of tests/vit_decoder_bn_reference.py (it takes the HIP forward's LeakyReLU masks), the running statistics,
the entries that must not change (inference entries, a frozen decoder, the flag clear), the captured step and CausalViTVAE.

The rules (§23's, as tests/test_vit_stem_batchnorm.py states them).  fp32: a tensor may lie at most 6 x as far from the float64 restatement as torch's own fp32 CPU
evaluation of the same nn decoder under .train() lies from its float64 evaluation (L2 distances per tensor).  bf16: at most 2 x the distance of the ROUNDING
ORACLE — the float64 restatement rounded to bf16 where the kernels store bf16 — from float64 (a tensor the oracle does not move at all keeps the fp32 rule).
The 11 BatchNorm-fronted conv-bias gradients are zero in exact arithmetic: they are held element-wise to the absolute rounding bound
vit_decoder_bn_reference.conv_bias_bound.  The 22 running statistics are held element-wise, per layer, to the kernel test's bound on float64 statistics of the
conv output the kernel READ (tests/bn2d_batch_reference.py); the 11 counters are up by one.

Measured on the MI355X (the RATIO lines of the run).  The distance rule, worst tensor per case: fp32 2.71 x torch's own fp32 distance (64 x 96, B = 2), 2.07 x (B = 3),
1.94 x (96 x 64), 1.89 x (B = 1) where 6 are allowed; bf16 1.35 x and 1.16 x the rounding oracle's distance where 2 are allowed.  Conv-bias gradients, max |got| /
bound: fp32 at most 0.015 (|got| at most 1.5e-4), bf16 0.12 - 0.37.  Running statistics against float64 on the conv output the kernel read, max over the 11 layers:
running_mean 0.30, running_var 0.49 of the bound.  The HIP forward's LeakyReLU masks equal the float64 restatement's own in fp32 and differ in 1081 / 1714 of
331776 / 497664 signs in bf16.  None is above 1."""
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
import vit_decoder_bn_reference as db  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CASES = [((64, 96), 2, F32), ((64, 96), 2, BF16), ((64, 96), 3, F32), ((64, 96), 3, BF16), ((96, 64), 2, F32), ((64, 96), 1, F32)]
IDS = [f"{h}x{w}-B{B}-{'bf16' if dt == BF16 else 'f32'}" for (h, w), B, dt in CASES]
STAT = ("running_mean", "running_var", "num_batches_tracked")


def vitvae(img, dtype=F32, seed=0):
    from causal_vae_amd.vit.models import ViTVAE
    torch.manual_seed(seed)
    model = ViTVAE(img_size=img, depth=1, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    vd.randomize_decoder_bn(model.decoder, seed + 2)
    model.requires_grad_(False)
    return model.to(DEV).eval().set_compute_dtype(dtype)


def buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.split(".")[-1] in STAT}


def unchanged(model, was, what):
    now = buffers(model)
    assert now.keys() == was.keys() and all(torch.equal(now[k], was[k]) for k in was), f"{what} changed a BatchNorm buffer"


def nchw(t):
    return t.detach().cpu().float().permute(0, 3, 1, 2)


def cotangent(B, H, W, seed):
    return torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(seed))


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


@pytest.mark.parametrize("img,B,dtype", CASES, ids=IDS)
def test_decoder_cut_at_its_boundary(img, B, dtype):
    bf = dtype == BF16
    grid = (img[0] // 32, img[1] // 32)
    model = vitvae(img, dtype)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.train_decoder(batch_stats=True)
    assert not model.training and not any(m.training for m in model.decoder.modules())
    zc, gc = vd.dec_inputs(B, 128, 300 + B), cotangent(B, *img, 400 + B)
    with torch.no_grad():                                                  # the walk alone, on a copy (its buffers move, the model's do not): the conv outputs read
        _img, (steps, _out_conv, _last) = copy.deepcopy(model)._decode_walk(zc.to(DEV), True, None, keep_inputs=True, batch_stats=True)
    pre = [y for s in steps for y in s.pre]
    assert len(pre) == 11 and all(y.dtype == dtype for y in pre)
    was = buffers(model)
    z = zc.to(DEV).requires_grad_(True)
    col = {}
    image = model.decode_with_grad(z, col)
    image.backward(gc.to(DEV))
    masks = db.masks_from_collect(col)
    params = dict(zip(db.PARAM_KEYS, model._decoder_params()))
    named = dict(model.named_parameters())
    assert all(params[k] is named[k] for k in db.PARAM_KEYS)               # the helper's names are _decoder_params()' tensors
    assert all(p.grad is not None and p.grad.dtype == F32 and torch.isfinite(p.grad).all() for p in params.values())

    fw = db.decoder_bn_forward(sd, zc, grid)
    flips = sum(int((m != (a > 0)).sum()) for m, a in zip(masks, fw["a"]) if m is not None)
    print(f"LeakyReLU masks: {flips} of {sum(m.numel() for m in masks if m is not None)} signs of the HIP forward differ from the float64 restatement's own")
    r64 = db.decoder_bn_vjp(sd, zc, gc, grid, masks, forward=fw)
    acts = lambda f: {**{f"stage{i}": t for i, t in enumerate(f["stages"])}, **{f"inner{i}": t for i, t in enumerate(f["inner"])}, "image": f["image"]}
    r64.update(acts(fw))
    names = [k for k in db.PARAM_KEYS if k not in db.CONV_BIAS_KEYS] + ["dz", "image"] + [f"stage{i}" for i in range(8)] + [f"inner{i}" for i in range(3)]
    assert len(names) == 37 + 2 + 11
    t64, t32 = db.torch_train_decoder(sd, zc, gc, F64), db.torch_train_decoder(sd, zc, gc, F32)
    own = {k: (dist(t32[k], t64[k]), 6.0) for k in names}                  # torch's fp32 evaluation's distance from torch's float64 evaluation
    if bf:                                                                 # the rounding oracle's distance from float64
        ofw = db.decoder_bn_forward(sd, zc, grid, rnd=vr.round_bf16)
        yard = db.decoder_bn_vjp(sd, zc, gc, grid, masks, rnd=vr.round_bf16, forward=ofw)
        yard.update(acts(ofw))
        own = {k: (dist(yard[k], r64[k]), 2.0) if dist(yard[k], r64[k]) > 0.0 else own[k] for k in names}
    label = IDS[CASES.index((img, B, dtype))]
    got = {k: p.grad for k, p in params.items() if k not in db.CONV_BIAS_KEYS}
    got.update(dz=z.grad, image=image)
    got.update({f"stage{i}": nchw(t) for i, t in enumerate(col["stages"])})
    got.update({f"inner{i}": nchw(t) for i, t in enumerate(col["res_inner"])})
    assert set(got) == set(names) and z.grad.dtype == F32 and image.dtype == F32
    hold(label, got, r64, own)
    for j, k in enumerate(db.CONV_BIAS_KEYS):                              # zero in exact arithmetic: an absolute rounding bound, element-wise
        g = params[k].grad.detach().cpu().double()
        bound = db.conv_bias_bound(fw, r64, masks, sd, j, bf)
        r = float((g.abs() / bound).max())
        print(f"{label} {k}: max |got| / bound = {r:.4f} (max |got| {float(g.abs().max()):.3e}, weight gradient's max {float(r64[k.replace('.bias', '.weight')].abs().max()):.3e})")
        assert torch.isfinite(g).all() and r <= 1.0, (k, r)
    # the running statistics, element-wise: float64 statistics of the conv output the kernel read, within the kernel test's bound; the counters
    now = buffers(model)
    for j, (_i, _kind, _c, b, _slope) in enumerate(db.LAYERS):
        y = pre[j].detach().cpu().reshape(-1, pre[j].shape[-1])
        ref, err = br.forward(y, sd[f"{b}.weight"], sd[f"{b}.bias"], sd[f"{b}.running_mean"], sd[f"{b}.running_var"], db.MOMENTUM, db.EPS, bf16=bf)
        for n in ("running_mean", "running_var"):
            r = br.max_ratio(now[f"{b}.{n}"], ref[n], err[n])
            print(f"RATIO {label} {b}.{n} {r:.4f}")
            assert r <= 1.0, (b, n, r)
        assert int(now[f"{b}.num_batches_tracked"]) == int(was[f"{b}.num_batches_tracked"]) + 1
    assert pre[0].shape[0] * pre[0].shape[1] * pre[0].shape[2] == B * 4 * grid[0] * grid[1]
    assert all(torch.equal(now[k], was[k]) for k in was if k.startswith("stem."))


def _entries(model, z, g, x):
    from causal_vae_amd.vit.models import fit_latent
    with torch.no_grad():
        out = {"decode": model.decode(z), "vjp": model.decode_vjp(z, g), "reconstruct": model.reconstruct(x)}
    out["fit"], _losses = fit_latent(model, x, z, 2, 1e-2)
    return out


def test_inference_entries_and_a_frozen_decoder_keep_the_fold_and_the_buffers():
    model = vitvae((64, 96))
    z, g, x = vd.dec_inputs(2, 128, 7).to(DEV), cotangent(2, 64, 96, 8).to(DEV), vr.vit_inputs(2, 64, 96, seed=5).to(DEV)
    want = _entries(model, z, g, x)
    zg = z.clone().requires_grad_(True)
    img = model.decode_with_grad(zg)
    img.backward(g)
    want["frozen"], want["frozen_dz"] = img.detach(), zg.grad.clone()
    model.train_decoder(batch_stats=True)
    was = buffers(model)
    got = _entries(model, z, g, x)
    assert model._decoder_batch_stats                                          # fit_latent leaves the switch as it found it
    for k in got:
        assert torch.equal(got[k], want[k]), k                                 # the parent path's bits: the fold on the running statistics
    unchanged(model, was, "an inference entry")
    model.zero_grad(set_to_none=True)
    model.freeze_decoder()
    model._decoder_batch_stats = True                                          # even with the flag left set: no live parameter, the fold
    zg = z.clone().requires_grad_(True)
    img = model.decode_with_grad(zg)
    img.backward(g)
    assert torch.equal(img.detach(), want["frozen"]) and torch.equal(zg.grad, want["frozen_dz"])
    unchanged(model, was, "a frozen decoder's decode_with_grad")


def test_flag_clear_is_the_old_behaviour():
    model = vitvae((64, 96))
    z, g = vd.dec_inputs(2, 128, 7).to(DEV), cotangent(2, 64, 96, 8).to(DEV)
    with torch.no_grad():
        img0 = model.decode(z)
    start = copy.deepcopy(model.state_dict())
    model.train_decoder(batch_stats=True)
    img = model.decode_with_grad(z.clone().requires_grad_(True))
    assert not torch.equal(img.detach(), img0)                                 # batch statistics: other values than the running statistics give
    img.backward(g)
    model.zero_grad(set_to_none=True)
    model.load_state_dict(start)                                               # the buffers as they were
    grads = None
    for clear in (lambda: model.train_decoder(), lambda: (model.freeze_decoder(), model.train_decoder())):
        model.train_decoder(batch_stats=True)
        clear()
        was = buffers(model)
        zg = z.clone().requires_grad_(True)
        img = model.decode_with_grad(zg)
        assert torch.equal(img.detach(), img0)                                 # the forward: decode's bits
        img.backward(g)
        unchanged(model, was, "the eval-mode training walk")
        grads = [p.grad.clone() for p in model._decoder_params()] + [zg.grad.clone()]
        model.zero_grad(set_to_none=True)
    fresh = vitvae((64, 96))                                                   # .. and the gradients are those of a model that never saw the flag
    fresh.train_decoder()
    zf = z.clone().requires_grad_(True)
    fresh.decode_with_grad(zf).backward(g)
    assert all(torch.equal(a, b) for a, b in zip(grads, [p.grad for p in fresh._decoder_params()] + [zf.grad]))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_captured_step_equals_eager(dtype):
    import test_vit_train_graph as tg
    from causal_vae_amd.vit import vit_vae_train_step
    start = tg.vitvae(False, dtype)
    start.train_all(stem_batch_stats=True, decoder_batch_stats=True)
    batches, noises = tg.vit_batches()
    me = copy.deepcopy(start)
    oe, le = tg.eager_run(me, me.parameters(), vit_vae_train_step, batches, noises, beta=0.7)
    mc = copy.deepcopy(start)
    assert mc._stem_batch_stats and mc._decoder_batch_stats
    oc, lc = tg.captured_run(mc, mc.parameters(), batches, noises, beta=0.7)
    for i, (a, b) in enumerate(zip(le, lc)):
        print(f"step {i}: eager loss {float(a[0])!r}, captured loss {float(b[0])!r}")
        assert torch.equal(a[0], b[0]), f"loss of step {i}"
    tg.assert_same_training_state(me, oe, mc, oc, "captured against eager")          # parameters, Adam moments, running statistics, counters
    moved = [k for k, v in buffers(me).items() if not torch.equal(v, start.state_dict()[k])]
    assert len([k for k in moved if k.startswith("decoder.")]) == 33 and len([k for k in moved if k.startswith("stem.")]) == 15, moved
    for m in (me, mc):
        assert all(int(bn.num_batches_tracked) == 3 for bn in vd.decoder_batchnorms(m.decoder))


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
    params = model.train_adapters(decoder=True, decoder_batch_stats=True)
    assert model.backbone._decoder_batch_stats and not model.backbone.training
    was = buffers(model.backbone)
    batches, noises = tg.causal_batches(model, 1)
    opt = FusedAdam(params, lr=1e-3)
    out = causal_vit_train_step(model, opt, *batches[0], eps=noises[0])
    assert all(torch.isfinite(t).all() for t in out)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
    now = buffers(model.backbone)
    for bn_key in {k.rsplit(".", 1)[0] for k in was if k.startswith("decoder.")}:
        assert not torch.equal(now[f"{bn_key}.running_mean"], was[f"{bn_key}.running_mean"]) and not torch.equal(now[f"{bn_key}.running_var"], was[f"{bn_key}.running_var"])
        assert int(now[f"{bn_key}.num_batches_tracked"]) == int(was[f"{bn_key}.num_batches_tracked"]) + 1
    assert all(torch.equal(v, was[k]) for k, v in now.items() if k.startswith("stem."))
