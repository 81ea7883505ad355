"""What the morphology tests (causal_vae_amd.morphology) rest on, checked without a GPU on tests/morphology_reference.py: the specification
is pinned without skimage, which is not installed where this runs.
  closed forms   a filled h x w rectangle: perimeter 2 (h - 1) + 2 (w - 1), major axis 4 sqrt((max(h, w)^2 - 1) / 12), extent 1, solidity 1, Euler 1, and
                 orientation feature 1.0 when wide; a single pixel: [1/784, 0, 0.2, 0, 0, 0.75, 1, 1, 1/3, 0.75, ..]; the two-pixel diagonal 0.25 and the
                 anti-diagonal 0.75 for the orientation tie; a ring Euler 0, a figure-eight -1
  cross-checks   Euler by bit-quads = 1 - holes (holes by 4-connected labelling of the padded background); the integer hull count = the count from
                 scipy.spatial.ConvexHull's facet equations with the boundary included, on every component measured in the case list
  coverage       the union of the cases' perimeter histograms holds all ten weighted codes; some case has an area tie, a thickest region outside the largest
                 component, a pixel equal to float32(0.2) and one a step above, no background, no foreground, a - c == 0 with b < 0, b > 0 and b = 0, and pixel
                 centres exactly on a hull edge: the GPU test cannot pass vacuously
  constants      C_MORPH follows the rule from the ratios the same formulas reach in float64 numpy against longdouble with C = 1
  consumers      the propagation forms hold when the features move by their slack
  refusals       every ops.morph_args refusal is a CvaeError raised without a device

Measured here with C = 1 (float64 twin against longdouble, the largest ratio over the case list): MajorAxis 1.91, Eccentricity 1.57, Orientation 1.26,
H_Symmetry 0.20, V_Symmetry 0.16: C = 8, 8, 8, 1, 1.  The float32 np.mean the reference function itself uses is off the exact mean by up to 7.3e-8 on these
cases, against a bound of ~6e-8 |f| that must also hold the rounding of the result: hence the longdouble mean as the value compared with."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.spatial import ConvexHull

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import morphology_reference as mr  # noqa: E402

F = {n: i for i, n in enumerate(mr.FEATURE_NAMES_12)}


def feats_of(mask, shape=(28, 28), at=(3, 4)):
    img = np.zeros(shape, dtype=np.float32)
    m = np.asarray(mask, dtype=bool)
    img[at[0]:at[0] + m.shape[0], at[1]:at[1] + m.shape[1]][m] = 1.0
    raw, f, _s = mr.measure(img)
    return raw, f.astype(np.float64)


def test_feature_names_are_the_reference_order():
    from causal_vae_amd import FEATURE_NAMES_12
    assert tuple(FEATURE_NAMES_12) == mr.FEATURE_NAMES_12 == ("Area", "Perimeter", "Thickness", "MajorAxis", "Eccentricity", "Orientation", "Solidity", "Extent",
                                                              "AspectRatio", "Euler", "H_Symmetry", "V_Symmetry")


@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (5, 3), (1, 6), (7, 1), (4, 9), (10, 10)])
def test_filled_rectangle(h, w):
    raw, f = feats_of(np.ones((h, w)))
    assert raw[mr.RAW_AREA] == h * w and raw[mr.RAW_EULER] == 1 and raw[mr.RAW_CONVEX] == h * w
    # a line one pixel wide has no corners: its two end pixels carry code 3 (weight 0), the others code 5, so its perimeter is its length minus 2
    assert math.isclose(f[F["Perimeter"]] * 100, 2 * (h - 1) + 2 * (w - 1) if min(h, w) > 1 else max(h, w) - 2, rel_tol=1e-15, abs_tol=1e-15)
    assert math.isclose(f[F["MajorAxis"]] * 28, 4 * math.sqrt((max(h, w) ** 2 - 1) / 12), rel_tol=1e-14, abs_tol=1e-15)
    assert f[F["Extent"]] == 1 and f[F["Solidity"]] == 1 and f[F["Euler"]] == 0.75
    assert math.isclose(f[F["AspectRatio"]], w / h / 3, rel_tol=1e-15)
    assert math.isclose(f[F["Thickness"]] * 5, (min(h, w) + 1) // 2, rel_tol=1e-15)
    if w > h:
        assert f[F["Orientation"]] == 1.0          # atan2(+0, negative) = pi: the major axis lies along the columns
    elif h > w:
        assert f[F["Orientation"]] == 0.5
    else:
        assert f[F["Orientation"]] == 0.75 and f[F["Eccentricity"]] == 0          # a == c, b == 0: +pi / 4


def test_single_pixel_and_the_orientation_tie():
    raw, f = feats_of(np.ones((1, 1)))
    want = [1 / 784, 0, 0.2, 0, 0, 0.75, 1, 1, 1 / 3, 0.75]
    assert np.allclose(f[:10], want, rtol=1e-15, atol=0) and raw[mr.RAW_COMPONENTS] == 1
    assert math.isclose(f[10], 1 - 2 / 784, rel_tol=1e-15) and math.isclose(f[11], 1 - 2 / 784, rel_tol=1e-15)
    _r, fd = feats_of(np.eye(2))
    _r, fa = feats_of(np.eye(2)[:, ::-1])
    assert math.isclose(fd[F["Orientation"]], 0.25, rel_tol=1e-15) and math.isclose(fa[F["Orientation"]], 0.75, rel_tol=1e-15)
    assert fd[F["Eccentricity"]] == 1 and fa[F["Eccentricity"]] == 1


def test_ring_and_figure_eight():
    ring = mr.place(5, 5, mr.RING)
    eight = mr.place(7, 4, mr.EIGHT)
    r, f = feats_of(ring)
    assert r[mr.RAW_EULER] == 0 and f[F["Euler"]] == 0.5 and r[mr.RAW_CONVEX] == 25
    r, f = feats_of(eight)
    assert r[mr.RAW_EULER] == -1 and f[F["Euler"]] == 0.25
    img = np.zeros((28, 28), dtype=np.float32)          # the largest of two components is the one measured; ties go to the first in raster order
    img[1:4, 1:4] = 1
    img[10:13, 12:15] = 1
    raw, _f, _s = mr.measure(img)
    assert raw[mr.RAW_COMPONENTS] == 2 and raw[mr.RAW_FIRST] == 1 * 28 + 1
    img[10:14, 12:15] = 1
    raw, _f, _s = mr.measure(img)
    assert raw[mr.RAW_FIRST] == 10 * 28 + 12 and raw[mr.RAW_AREA] == 12


def test_empty_and_background_free():
    raw, f, _s = mr.measure(np.zeros((28, 28), dtype=np.float32))
    assert raw[mr.RAW_STATUS] == mr.STATUS_EMPTY and (f == 0).all()
    raw, f, _s = mr.measure(np.ones((28, 28), dtype=np.float32))
    assert raw[mr.RAW_STATUS] == mr.STATUS_NO_BACKGROUND and np.isnan(f[2]) and not np.isnan(np.delete(f, 2)).any() and raw[mr.RAW_MAXD2] == -1


def measured_components():
    for shape in mr.SHAPES:
        ref = mr.reference(shape)
        for name, raw, ex in zip(ref["names"], ref["raw"], ref["extras"]):
            if "comp" in ex:
                yield shape, name, raw, ex


def test_euler_is_one_minus_holes():
    n = 0
    for shape, name, raw, ex in measured_components():
        bg = np.pad(~ex["comp"], 1, constant_values=True)
        _lab, k = ndimage.label(bg)          # 4-connected background: the outside is one of them
        assert raw[mr.RAW_EULER] == 1 - (k - 1), (shape, name)
        n += 1
    assert n > 400


def test_hull_count_equals_the_facet_equations():
    n = 0
    for shape, name, raw, ex in measured_components():
        rr, cc = np.nonzero(ex["comp"])
        pts = np.concatenate([np.stack([rr - 0.5, cc], 1), np.stack([rr + 0.5, cc], 1), np.stack([rr, cc - 0.5], 1), np.stack([rr, cc + 0.5], 1)])
        eq = ConvexHull(pts).equations
        R, C = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        inside = (eq[:, 0][:, None, None] * R + eq[:, 1][:, None, None] * C + eq[:, 2][:, None, None] <= 1e-9).all(axis=0)
        assert int(inside.sum()) == raw[mr.RAW_CONVEX], (shape, name)
        n += 1
    assert n > 400


def test_case_list_reaches_every_branch():
    codes, seen = set(), dict(tie=0, outside=0, on_edge=0, full=0, empty=0, at_thr=0, above_thr=0, b_neg=0, b_pos=0, b_zero=0, nan=0)
    thr = np.float32(0.2)
    for shape in mr.SHAPES:
        ref = mr.reference(shape)
        for img, raw, ex in zip(ref["images"], ref["raw"], ref["extras"]):
            seen["empty"] += int(raw[mr.RAW_STATUS]) & mr.STATUS_EMPTY != 0
            seen["full"] += int(raw[mr.RAW_STATUS]) & mr.STATUS_NO_BACKGROUND != 0
            seen["at_thr"] += bool((img == thr).any())
            seen["above_thr"] += bool((img == np.nextafter(thr, np.float32(1))).any())
            seen["nan"] += bool(np.isnan(img).any())
            if "comp" not in ex:
                continue
            codes |= ex["codes"]
            seen["tie"] += ex["area_tie"]
            seen["outside"] += ex["thickest_outside"]
            seen["on_edge"] += ex["hull_on_edge"] > 0
            m20, m02, m11 = mr.central(raw)
            if m20 == m02:          # a - c == 0; b = -mu11 / A
                seen["b_neg" if m11 > 0 else ("b_pos" if m11 < 0 else "b_zero")] += 1
    assert codes == set(mr.PERIM_CODES), sorted(set(mr.PERIM_CODES) - codes)
    assert all(v > 0 for v in seen.values()), seen
    big = mr.reference((64, 64))
    assert big["raw"][big["names"].index("serpentine")][mr.RAW_AREA] > 2000 and big["raw"][big["names"].index("spiral")][mr.RAW_AREA] > 2000
    assert big["raw"][big["names"].index("isolated")][mr.RAW_COMPONENTS] == 1024 and big["raw"][big["names"].index("checkerboard")][mr.RAW_EULER] < -900


def test_constants_follow_the_rule():
    worst = {k: 0.0 for k in mr.BOUNDED}
    mean_gap = 0.0
    for shape in mr.SHAPES:
        ref = mr.reference(shape)
        for img, raw, f, scale in zip(ref["images"], ref["raw"], ref["f"], ref["scale"]):
            f64, _s = mr.features(raw, img, dtype=np.float64)
            for k in mr.BOUNDED:
                if np.isnan(float(f[k])) or (f64[k] == f[k]):
                    continue
                worst[k] = max(worst[k], abs(float(np.longdouble(f64[k]) - f[k])) / (mr.U64 * scale[k]))
            if not np.isnan(img).any() and int(raw[mr.RAW_STATUS]) & mr.STATUS_EMPTY == 0:
                mean_gap = max(mean_gap, abs(float(np.longdouble(np.float32(1) - np.mean(np.abs(img - img[:, ::-1]))) - f[10])))
    print("RATIO morph float64 twin", {mr.FEATURE_NAMES_12[k]: round(v, 3) for k, v in worst.items()}, "float32 np.mean off by", mean_gap)
    for k in mr.BOUNDED:
        assert mr.C_MORPH[k] == mr.constant_rule(worst[k]), (k, worst[k])


def test_propagation_forms_hold_under_the_slack():
    rng = np.random.RandomState(0)
    imgs = np.stack([mr.blob(28, 28, 7000 + i) for i in range(20)]).reshape(5, 4, 28, 28)          # [T, N, H, W]
    Fh, E = mr.measure_batch(imgs)
    std, sens, bound = mr.sensitivity_host(imgs)
    moved = Fh.astype(np.float64) + E * rng.choice([-1.0, 1.0], size=E.shape)
    std2 = np.std(moved.transpose(1, 0, 2), axis=1).mean(axis=0)
    ok = ~np.isnan(sens)
    assert (np.abs(std2 - sens)[ok] <= bound[ok]).all()
    diff, norm, e, e_norm = mr.pair_contrast_host(imgs[0], imgs[1])
    Fa, Ea = mr.measure_batch(imgs[0])
    Fb, Eb = mr.measure_batch(imgs[1])
    d2 = np.abs((Fa + Ea * rng.choice([-1.0, 1.0], size=Ea.shape)) - (Fb + Eb * rng.choice([-1.0, 1.0], size=Eb.shape))).mean(axis=0)
    ok = ~np.isnan(diff)
    assert (np.abs(d2 - diff)[ok] <= e[ok]).all()
    n2 = d2 / (np.nanmax(d2) + 1e-9) * 100
    assert (np.abs(n2 - norm)[ok] <= e_norm[ok]).all()


def test_every_refusal_is_raised_without_a_device():
    from causal_vae_amd import ops, _lib, measure_counterfactual
    ok = torch.zeros(2, 28, 28)
    bad = [dict(x=torch.zeros(4, 4)), dict(x=torch.zeros(1, 1, 1, 4, 4)), dict(x=torch.zeros(1, 2, 4, 4)), dict(x=torch.zeros(1, 65, 4)), dict(x=torch.zeros(1, 1, 4, 65)),
           dict(x=torch.zeros(1, 4, 4, dtype=torch.int32)), dict(x=torch.zeros(1, 4, 4, dtype=torch.uint8)), dict(x=torch.zeros(1, 4, 4, dtype=torch.float64)),
           dict(x=torch.zeros(0, 4, 4)), dict(x=np.zeros((1, 4, 4), dtype=np.float32)), dict(x=ok, norms=(1, 2, 3)), dict(x=ok, norms=(1, 1, 0, 1)),
           dict(x=ok, norms=(1, 1, float("inf"), 1)), dict(x=ok, threshold=float("nan"))]
    for kw in bad:
        with pytest.raises(_lib.CvaeError) as e:
            ops.morph_args("morph_features12", **kw)
        assert "MI355X only" not in str(e.value), kw          # refused for its own reason, before the device is asked about
    with pytest.raises(_lib.CvaeError, match="MI355X only"):
        ops.morph_args("morph_features12", ok)          # a CPU tensor: the last refusal
    with pytest.raises(_lib.CvaeError):
        ops.morph_features12(ok)
    with pytest.raises(_lib.CvaeError):
        measure_counterfactual(torch.zeros(2, 3, 2, 28, 28))
    # the C entry refuses by itself too, before anything could be launched
    f = _lib.lib.cvae_morph12_f32
    assert f(None, 1, 4, 4, 0.2, 1.0, 1.0, 1.0, 1.0, None, None, None) == -6 and f(None, 1, 65, 4, 0.2, 1.0, 1.0, 1.0, 1.0, None, None, None) == -3
    assert f(None, 0, 4, 4, 0.2, 1.0, 1.0, 1.0, 1.0, None, None, None) == -1 and f(None, 1, 4, 4, 0.2, 1.0, 0.0, 1.0, 1.0, None, None, None) == -1
    assert all(_lib.lib.cvae_morph12_threads(h, w) in (64, 128, 256, 512) for h, w in mr.SHAPES) and ops.MORPH_RAW_WORDS == mr.RAW_WORDS
