"""The 12 morphology features on the device (causal_vae_amd.morphology, ops.morph_features12; csrc/morphology.hip) against
tests/morphology_reference.py: the specification in numpy and scipy, sharing no algorithm with the kernel (tests/test_morphology_cpu.py pins it and shows that
the case list reaches every branch).

Shapes 1x1, 1x9, 5x7, 28x28, 33x64, 64x64; per shape the constructed masks that fit (empty, full, single pixels, every pixel at the threshold and one a step
above, a NaN pixel, checkerboard, isolated pixels, serpentine, spiral, comb, both diagonals, a frame on all four borders, the closed-form shapes, ring,
figure-eight, L, two equal components, a thick square beside a larger thin line) and 64 seeded smooth blobs: one launch per shape.
  raw          the int record equals the reference's EXACTLY
  features     1, 2, 3, 7, 8, 9, 10 within 1 ulp of float32 of the rounded reference; 4, 5, 6, 11, 12 within 2^-24 |f| + C 2^-53 scale of the LONGDOUBLE value
               (C = 8, 8, 8, 1, 1).  The reference function's own np.mean is a float32 pairwise sum and is off the exact mean by more than that: the
               comparison is with the longdouble mean of the same float32 differences
  invariances  two runs, B = 1 against row i of B = 257, bf16 against its upcast, [B, 1, H, W] against [B, H, W], a captured and replayed graph: equal bits
  consumers    measured_sensitivity / measured_pair_contrast on seeded models (8 samples x 10 classes) against the reference module's host loop over the same
               decoded images, within the feature bounds carried through the std / mean; measure_counterfactual's row order; morph_mnist12 on 16 synthetic
               digits; extract_refined_features; every refusal

Measured on the MI355X (the RATIO lines: the largest |got - f| / bound over a shape's cases; the float32 rounding alone can reach 1):
  1x1 0 | 1x9 0.988 | 5x7 0.911 | 28x28 0.926 | 33x64 0.879 | 64x64 0.901; 0 of the 6132 values is not the float32 nearest to the longdouble value, so these are
  the ratios of the rounding itself.  sensitivity 1.7e-10 of its propagated bound, pair contrast 0 (both models): the features equal the host loop's bit for bit."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import morphology_reference as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_GOT = {}


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def device_result(shape):
    """(feats [B, 12], raw [B, 32]) of a shape's cases as numpy, from one launch, once"""
    if shape not in _GOT:
        from causal_vae_amd import ops
        x = torch.as_tensor(mr.reference(shape)["images"]).to(DEV)
        feats, raw = ops.morph_features12(x, return_raw=True)
        _GOT[shape] = (feats.cpu().numpy(), raw.cpu().numpy(), x)
    return _GOT[shape]


@pytest.mark.parametrize("shape", mr.SHAPES, ids=shape_id)
def test_raw_record_is_exact(shape):
    ref = mr.reference(shape)
    _feats, raw, _x = device_result(shape)
    assert raw.dtype == np.int32 and raw.shape == (len(ref["names"]), mr.RAW_WORDS)
    for i, name in enumerate(ref["names"]):
        assert np.array_equal(raw[i], ref["raw"][i]), (shape, name, raw[i].tolist(), ref["raw"][i].tolist())


@pytest.mark.parametrize("shape", mr.SHAPES, ids=shape_id)
def test_features_within_bounds(shape):
    ref = mr.reference(shape)
    feats, _raw, _x = device_result(shape)
    assert feats.dtype == np.float32
    worst, other = 0.0, 0
    for i, name in enumerate(ref["names"]):
        worst = max(worst, mr.check_features(feats[i], ref["f"][i], ref["scale"][i], (shape, name)))
        other += mr.rounded_differently(feats[i], ref["f"][i])
    print(f"RATIO morph {shape_id(shape)} {worst:.3g}; {other} of {feats.size} values are not the float32 nearest to the longdouble value")


def test_other_threshold_and_norms():
    from causal_vae_amd import ops
    imgs = mr.reference((28, 28))["images"][-16:]
    thr, norms = 0.5, (100.0, 7.0, 3.0, 9.0)
    feats, raw = ops.morph_features12(torch.as_tensor(imgs).to(DEV), threshold=thr, norms=norms, return_raw=True)
    for i, im in enumerate(imgs):
        r, f, scale = mr.measure(im, np.float32(thr), norms)
        assert np.array_equal(raw[i].cpu().numpy(), r)
        mr.check_features(feats[i].cpu().numpy(), f, scale, ("threshold 0.5", i))


def test_invariances():
    from causal_vae_amd import ops
    for shape in ((28, 28), (64, 64), (5, 7)):
        feats, raw, x = device_result(shape)
        f2, r2 = ops.morph_features12(x, return_raw=True)
        assert np.array_equal(f2.cpu().numpy().view(np.uint32), feats.view(np.uint32)) and np.array_equal(r2.cpu().numpy(), raw)          # two runs
        idx = torch.arange(257, device=DEV) % x.shape[0]
        idx = idx[torch.randperm(257, generator=torch.Generator().manual_seed(3)).to(DEV)]
        fb, rb = ops.morph_features12(x[idx], return_raw=True)
        fb, rb, idx = fb.cpu().numpy(), rb.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(fb.view(np.uint32), feats[idx].view(np.uint32)) and np.array_equal(rb, raw[idx])          # any position of any batch
        for i in (0, 9, x.shape[0] - 1):          # alone
            f1, r1 = ops.morph_features12(x[i:i + 1], return_raw=True)
            assert np.array_equal(f1.cpu().numpy().view(np.uint32), feats[i:i + 1].view(np.uint32)) and np.array_equal(r1.cpu().numpy(), raw[i:i + 1])
        f4 = ops.morph_features12(x[:, None])
        assert np.array_equal(f4.cpu().numpy().view(np.uint32), feats.view(np.uint32))
        assert np.array_equal(ops.morph_features12(x).cpu().numpy().view(np.uint32), feats.view(np.uint32))          # without the raw record


def test_half_precision_inputs_equal_their_upcast():
    from causal_vae_amd import ops
    x = device_result((28, 28))[2]
    for dt in (torch.bfloat16, torch.float16):
        xl = x.to(dt)
        a, ra = ops.morph_features12(xl, return_raw=True)
        b, rb = ops.morph_features12(xl.float(), return_raw=True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ra, rb)


def test_captured_graph_replays_the_eager_result():
    from causal_vae_amd import ops
    x = device_result((28, 28))[2]
    static = x.clone()
    ops.morph_features12(static, return_raw=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f, r = ops.morph_features12(static, return_raw=True)
    static.copy_(x.flip(0))
    g.replay()
    torch.cuda.synchronize()
    fe, re_ = ops.morph_features12(x.flip(0), return_raw=True)
    assert torch.equal(f.view(torch.int32), fe.view(torch.int32)) and torch.equal(r, re_)


# ---- consumers ----
def spread_decoder(model, probe):
    """an untrained decoder answers ~0.5 everywhere: scale its last layer and move its bias so that the median pixel sits at the threshold"""
    last = model.dec_conv[2]
    with torch.no_grad():
        last.weight.mul_(8.0)
        logit = torch.logit(probe().float().clamp(1e-6, 1 - 1e-6))
        last.bias.add_(math.log(0.25) - float(logit.median()))
    frac = float((probe() > 0.2).float().mean())
    assert 0.1 < frac < 0.9, frac          # the masks are neither empty nor full, so the comparison says something
    return model


def seeded_models():
    from causal_vae_amd.mnist_baseline import CausalMorphVAE12
    from causal_vae_amd.mnist_cvae import ConditionalVAE
    torch.manual_seed(11)
    z = torch.randn(8, 10).to(DEV)
    t3 = torch.zeros(8, 10, device=DEV)
    t3[:, 3] = 1.0
    causal = CausalMorphVAE12().to(DEV).eval()
    cvae = ConditionalVAE().to(DEV).eval()
    with torch.no_grad():
        spread_decoder(causal, lambda: causal.decode(causal.morph_predictor(t3), z))
        spread_decoder(cvae, lambda: cvae.decode(z, t3))
    return causal, cvae, z


def test_measured_sensitivity_matches_the_host_loop():
    from causal_vae_amd import measured_sensitivity, FEATURE_NAMES_12
    causal, _cvae, z = seeded_models()
    out = measured_sensitivity(causal, z, keep_images=True)
    images = out["images"][:, :, 0].permute(1, 0, 2, 3).cpu().numpy()          # [T, N, H, W]
    assert images.shape == (10, 8, 28, 28) and out["measured"].shape == (8, 10, 12)
    std, sens, bound = mr.sensitivity_host(images)
    got_std, got = out["std_per_sample"].cpu().numpy(), out["sensitivity"].cpu().numpy()
    ok = ~np.isnan(sens)
    assert ok.sum() >= 11 and np.array_equal(np.isnan(got), ~ok)
    print("RATIO morph sensitivity", float(np.max(np.abs(got - sens)[ok] / bound[ok])), "sensitivity", np.round(sens, 4).tolist())
    assert (np.abs(got - sens)[ok] <= bound[ok]).all(), (got, sens, bound)
    assert np.nanmax(np.abs(got_std - std)) <= np.nanmax(bound) * 8
    assert sens[ok].max() > 1e-3          # the classes do move the features
    names = [r["feature"] for r in out["ranking"]]
    vals = [r["sensitivity"] for r in out["ranking"]]
    assert sorted(names) == sorted(FEATURE_NAMES_12)
    finite = [v for v in vals if v == v]
    assert finite == sorted(finite, reverse=True) and all(v != v for v in vals[len(finite):])


@pytest.mark.parametrize("which", ["causal", "cvae"])
def test_measured_pair_contrast_matches_the_host_loop(which):
    from causal_vae_amd import measured_pair_contrast
    causal, cvae, z = seeded_models()
    out = measured_pair_contrast(causal if which == "causal" else cvae, z, 3, 8, keep_images=True)
    xa, xb = out["images_a"][:, 0].cpu().numpy(), out["images_b"][:, 0].cpu().numpy()
    assert xa.shape == (8, 28, 28) and not np.array_equal(xa, xb)
    diff, norm, e, e_norm = mr.pair_contrast_host(xa, xb)
    got, got_norm = out["diff"].cpu().numpy(), out["normalized"].cpu().numpy()
    ok = ~np.isnan(diff)
    assert ok.sum() >= 11 and np.array_equal(np.isnan(got), ~ok)
    print(f"RATIO morph pair {which}", float(np.max(np.abs(got - diff)[ok] / e[ok])), float(np.max(np.abs(got_norm - norm)[ok] / e_norm[ok])))
    assert (np.abs(got - diff)[ok] <= e[ok]).all() and (np.abs(got_norm - norm)[ok] <= e_norm[ok]).all()
    assert np.nanmax(diff) > 1e-3 and abs(np.nanmax(got_norm) - 100) < 1e-3


def test_measure_counterfactual_shape_and_row_order():
    from causal_vae_amd import measure_counterfactual, ops
    from causal_vae_amd.counterfactual import batched_counterfactual
    causal, _cvae, z = seeded_models()
    m = torch.rand(2, 12, generator=torch.Generator().manual_seed(5)).to(DEV)
    sweep = batched_counterfactual(causal, z[:2], m, features=[0, 3, 5], values=[0.1, 0.9])
    assert sweep.shape == (2, 3, 2, 1, 28, 28)
    got = measure_counterfactual(sweep)
    assert got.shape == (2, 3, 2, 12)
    for b in range(2):
        for f in range(3):
            for v in range(2):
                assert torch.equal(got[b, f, v].view(torch.int32), ops.morph_features12(sweep[b, f, v])[0].view(torch.int32))
    with pytest.raises(Exception):
        measure_counterfactual(sweep[:, :, :, 0])


def test_morph_mnist12_gives_the_reference_triple():
    from causal_vae_amd import morph_mnist12
    imgs, labels = mr.synthetic_digits(16)
    x, m, t = morph_mnist12(imgs, labels, DEV)
    assert x.shape == (16, 1, 28, 28) and x.dtype == torch.float32 and m.shape == (16, 12) and t.shape == (16, 10)
    x_ref = torch.as_tensor(imgs).float().div(255).numpy()          # ToTensor
    assert np.array_equal(x[:, 0].cpu().numpy(), x_ref)
    assert np.array_equal(t.cpu().numpy(), np.eye(10, dtype=np.float32)[labels])
    areas = set()
    for i in range(16):
        raw, f, scale = mr.measure(x_ref[i])
        areas.add(int(raw[mr.RAW_AREA]))
        mr.check_features(m[i].cpu().numpy(), f, scale, ("digit", i))
    assert len(areas) > 8 and min(areas) > 0
    x5, m5, t5 = morph_mnist12(torch.as_tensor(x_ref), labels, DEV, limit_count=5)          # floats are taken as they are
    assert x5.shape[0] == 5 and torch.equal(m5, m[:5]) and torch.equal(t5, t[:5])


def test_extract_refined_features_signature():
    from causal_vae_amd import extract_refined_features
    img = torch.as_tensor(mr.reference((28, 28))["images"][-1])[None]
    for given in (img, img.to(DEV)):
        f = extract_refined_features(given)
        assert f.dtype == torch.float32 and tuple(f.shape) == (12,) and f.device.type == "cpu"
        assert np.array_equal(f.numpy(), device_result((28, 28))[0][-1])


def test_refusals_precede_any_launch():
    from causal_vae_amd import ops, _lib
    bad = [torch.zeros(4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 65, 4), torch.zeros(1, 4, 65), torch.zeros(1, 4, 4, dtype=torch.int32),
           torch.zeros(1, 4, 4, dtype=torch.float64), torch.zeros(0, 4, 4)]
    for x in bad:
        with pytest.raises(_lib.CvaeError):
            ops.morph_features12(x.to(DEV))
    with pytest.raises(_lib.CvaeError):
        ops.morph_features12(torch.zeros(1, 4, 4))          # a CPU tensor
    for kw in (dict(norms=(1, 2, 3)), dict(norms=(1, 0, 1, 1)), dict(threshold=float("nan"))):
        with pytest.raises(_lib.CvaeError):
            ops.morph_features12(torch.zeros(1, 4, 4, device=DEV), **kw)
    # the C entry's own codes, with nothing to launch on
    assert _lib.lib.cvae_morph12_f32(None, 1, 4, 4, 0.2, 1.0, 1.0, 1.0, 1.0, None, None, None) == -6
    assert _lib.lib.cvae_morph12_f32(None, 1, 65, 4, 0.2, 1.0, 1.0, 1.0, 1.0, None, None, None) == -3
    assert _lib.lib.cvae_morph12_f32(None, 0, 4, 4, 0.2, 1.0, 1.0, 1.0, 1.0, None, None, None) == -1
