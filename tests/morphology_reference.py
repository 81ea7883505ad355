"""The 12 morphology features of an image (causal_vae_amd.morphology, csrc/morphology.hip) restated in numpy and scipy, as the tests' reference:
the project's specification of mnist_test/01_baseline_causal_vae/dataset.py:11-99 (extract_refined_features), written without skimage at hand.

Nothing here shares an algorithm with the kernel: components by scipy.ndimage.label (3 x 3 structure), the perimeter by binary_erosion and convolve over ALL
pixels (as skimage does; the kernel visits border pixels only), the thickness by distance_transform_edt, the convex area by a monotone chain over all 4 A
points in Python integers with every bounding-box centre tested against every edge, the Euler number by bit-quads on a padded array.  The float formulas run
in numpy.longdouble (64-bit mantissa here), and in float64 for the constants' rule: C = max(1, 2^ceil(log2(4 worst))), `worst` the largest ratio the float64
twin reaches against longdouble with C = 1 over the case list (tests/test_morphology_cpu.py measures it again and holds every constant).

Bounds.  The kernel forms every feature in float64 from exact integers and rounds once to float32, so |got - f| <= 2^-24 |f| + C 2^-53 scale:
  features 1, 2, 3, 7, 8, 9, 10   one or two float64 operations on integers: asked to be within 1 ulp of float32 of the rounded reference
  4 MajorAxis     4 sqrt(lambda1) / norm, lambda1 a sum of non-negative terms of exact integers                     scale = |f|
  5 Eccentricity  sqrt(disc / lambda1), both well-conditioned                                                       scale = |f|
  6 Orientation   (atan2 / 2 + pi / 2) / pi                                                                         scale = 1
  11, 12          1 - S / n, S a sum of n non-negative float32 terms in some fixed order: |fl(S) - S| <= (n-1) u S    scale = 1 + (n - 1) mean
The reference's own np.mean runs in float32 (pairwise) and differs from the exact mean by up to ~1e-7 relative, more than these bounds allow: the comparison
is with the longdouble mean of the same float32 terms."""
import math

import numpy as np
from scipy import ndimage

FEATURE_NAMES_12 = ("Area", "Perimeter", "Thickness", "MajorAxis", "Eccentricity", "Orientation", "Solidity", "Extent", "AspectRatio", "Euler", "H_Symmetry",
                    "V_Symmetry")
THRESHOLD = np.float32(0.2)
NORMS = (784.0, 100.0, 5.0, 28.0)          # area, perimeter, thickness, axis
PERIM_CODES = (5, 7, 15, 17, 25, 27, 21, 33, 13, 23)          # weight 1 (six), sqrt 2 (two), (1 + sqrt 2) / 2 (two)

# the raw record, int32 [RAW_WORDS] per image (include/cvae_hip.h, CVAE_MORPH_RAW_*)
RAW_WORDS = 32
(RAW_STATUS, RAW_COMPONENTS, RAW_FIRST, RAW_AREA, RAW_MINR, RAW_MINC, RAW_MAXR, RAW_MAXC, RAW_SR, RAW_SC, RAW_SRR, RAW_SCC, RAW_SRC) = range(13)
RAW_PERIM = 13          # ten counts, in PERIM_CODES order
RAW_MAXD2, RAW_CONVEX, RAW_Q1, RAW_Q3, RAW_QD, RAW_EULER = 23, 24, 25, 26, 27, 28
STATUS_EMPTY, STATUS_NO_BACKGROUND = 1, 2

EXACT_ULP = (0, 1, 2, 6, 7, 8, 9)          # features asked within 1 ulp of float32
BOUNDED = (3, 4, 5, 10, 11)                # features under a derived bound
C_MORPH = {3: 8.0, 4: 8.0, 5: 8.0, 10: 1.0, 11: 1.0}          # per feature index; float64 numpy reaches 1.91, 1.57, 1.26, 0.20, 0.16 (test_morphology_cpu.py)
U64, U32 = 2.0 ** -53, 2.0 ** -24


def constant_rule(worst):
    return max(1.0, 2.0 ** math.ceil(math.log2(4.0 * worst))) if worst > 0 else 1.0


# ---- the integers ----
def _hull(points):
    """Andrew's monotone chain on integer points [(x, y)], collinear points dropped; counter-clockwise."""
    pts = sorted(set(points))

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lo, up = half(pts), half(reversed(pts))
    return lo[:-1] + up[:-1]


def convex_count(comp):
    """(pixel centres inside or ON the hull of the points (r +- 1/2, c), (r, c +- 1/2) of the component's pixels, how many of them lie exactly on an edge
    without being pixels of the component), in doubled coordinates: all integers."""
    rr, cc = np.nonzero(comp)
    pts = []
    for r, c in zip(rr.tolist(), cc.tolist()):
        pts += [(2 * r - 1, 2 * c), (2 * r + 1, 2 * c), (2 * r, 2 * c - 1), (2 * r, 2 * c + 1)]
    hull = np.array(_hull(pts), dtype=np.int64)
    r0, r1, c0, c1 = rr.min(), rr.max(), cc.min(), cc.max()
    R, C = np.meshgrid(2 * np.arange(r0, r1 + 1), 2 * np.arange(c0, c1 + 1), indexing="ij")
    a, b = hull, np.roll(hull, -1, axis=0)
    cross = (b[:, 0] - a[:, 0])[:, None, None] * (C[None] - a[:, 1][:, None, None]) - (b[:, 1] - a[:, 1])[:, None, None] * (R[None] - a[:, 0][:, None, None])
    inside = (cross >= 0).all(axis=0)
    on_edge = inside & (cross == 0).any(axis=0) & ~comp[r0:r1 + 1, c0:c1 + 1]
    return int(inside.sum()), int(on_edge.sum())


def bit_quads(comp):
    p = np.pad(comp.astype(np.int64), 1)
    q = p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:]
    q1, q3 = int((q == 1).sum()), int((q == 3).sum())
    qd = int(((q == 2) & (p[:-1, :-1] == p[1:, 1:])).sum())
    return q1, q3, qd


def perimeter_histogram(comp):
    """skimage.measure.perimeter(image, 4) up to the weights: the histogram (50 bins) of the convolution of the border image, over all pixels"""
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    border = comp & ~ndimage.binary_erosion(comp, cross, border_value=0)
    codes = ndimage.convolve(border.astype(np.int64), np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
    return np.bincount(codes.ravel(), minlength=50)


def components(mask):
    """[(first raster index, area, boolean image)] of the 8-connected components, ordered by first pixel"""
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))
    out = []
    for k in range(1, n + 1):
        comp = lab == k
        out.append((int(np.argmax(comp.ravel())), int(comp.sum()), comp))
    return sorted(out, key=lambda t: t[0])


def raw_record(img, threshold=THRESHOLD, extras=None):
    """the int record of one image [H, W] (float32).  extras: a dict that receives what the coverage conditions ask about."""
    img = np.asarray(img, dtype=np.float32)
    assert img.ndim == 2
    mask = img > np.float32(threshold)
    raw = np.zeros(RAW_WORDS, dtype=np.int64)
    if not mask.any():
        raw[RAW_STATUS], raw[RAW_FIRST] = STATUS_EMPTY, -1
        return raw
    comps = components(mask)
    areas = [a for _f, a, _c in comps]
    first, area, comp = comps[int(np.argmax(areas))]          # ties: the lowest label
    rr, cc = np.nonzero(comp)
    raw[RAW_COMPONENTS], raw[RAW_FIRST], raw[RAW_AREA] = len(comps), first, area
    raw[RAW_MINR], raw[RAW_MINC], raw[RAW_MAXR], raw[RAW_MAXC] = rr.min(), cc.min(), rr.max() + 1, cc.max() + 1
    raw[RAW_SR], raw[RAW_SC], raw[RAW_SRR], raw[RAW_SCC], raw[RAW_SRC] = rr.sum(), cc.sum(), (rr * rr).sum(), (cc * cc).sum(), (rr * cc).sum()
    hist = perimeter_histogram(comp)
    raw[RAW_PERIM:RAW_PERIM + 10] = hist[list(PERIM_CODES)]
    if mask.all():
        raw[RAW_STATUS] |= STATUS_NO_BACKGROUND
        raw[RAW_MAXD2] = -1
        d2 = None
    else:
        d2 = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)
        raw[RAW_MAXD2] = d2.max()
    raw[RAW_CONVEX], on_edge = convex_count(comp)
    raw[RAW_Q1], raw[RAW_Q3], raw[RAW_QD] = bit_quads(comp)
    e4 = raw[RAW_Q1] - raw[RAW_Q3] - 2 * raw[RAW_QD]
    assert e4 % 4 == 0
    raw[RAW_EULER] = e4 // 4
    if extras is not None:
        extras.update(area_tie=areas.count(area) > 1, thickest_outside=d2 is not None and int(d2[comp].max()) < int(d2.max()), hull_on_edge=on_edge,
                      codes=set(np.nonzero(hist)[0].tolist()) & set(PERIM_CODES), comp=comp)
    return raw


# ---- the floats ----
def central(raw):
    """(M20, M02, M11) = A^2 (mu20, mu02, mu11) / A as exact integers: A sum r^2 - (sum r)^2 and so on"""
    A, sr, sc, srr, scc, src = (int(raw[i]) for i in (RAW_AREA, RAW_SR, RAW_SC, RAW_SRR, RAW_SCC, RAW_SRC))
    return A * srr - sr * sr, A * scc - sc * sc, A * src - sr * sc


def features(raw, img, norms=NORMS, dtype=np.longdouble):
    """(the 12 features [12] in `dtype`, the scale of each derived bound [12]) from the record and the grey image"""
    T = dtype
    f, scale = np.zeros(12, dtype=T), np.ones(12, dtype=np.float64)
    if int(raw[RAW_STATUS]) & STATUS_EMPTY:
        return f, scale
    img = np.asarray(img, dtype=np.float32)
    H, W = img.shape
    an, pn, tn, xn = (T(v) for v in norms)
    A = T(int(raw[RAW_AREA]))
    n = [T(int(v)) for v in raw[RAW_PERIM:RAW_PERIM + 10]]
    s2 = np.sqrt(T(2))
    f[0] = A / an
    f[1] = ((n[0] + n[1] + n[2] + n[3] + n[4] + n[5]) + (n[6] + n[7]) * s2 + (n[8] + n[9]) * ((T(1) + s2) / T(2))) / pn
    f[2] = T(np.nan) if int(raw[RAW_MAXD2]) < 0 else np.sqrt(T(int(raw[RAW_MAXD2]))) / tn
    m20, m02, m11 = central(raw)
    # a = mu02 / A, c = mu20 / A, b = -mu11 / A with mu / A = M / A^2.  Everything below is formed from the exact integers p = M02 + M20 = A^2 (a + c),
    # q = M02 - M20 = A^2 (a - c) and M11 = -A^2 b, so that no difference of rounded quotients appears: hyp = A^2 disc, lambda1 = (p + hyp) / (2 A^2),
    # disc / lambda1 = 2 hyp / (p + hyp), atan2(-2 b, c - a) = atan2(2 M11, -q)
    p, q = T(m02 + m20), T(m02 - m20)
    hyp = np.sqrt(q * q + T(4) * T(m11) * T(m11))
    l1 = max((p + hyp) / (T(2) * A * A), T(0))
    f[3] = T(4) * np.sqrt(l1) / xn
    f[4] = np.sqrt(T(2) * hyp / (p + hyp)) if l1 > 0 else T(0)
    pi = T(4) * np.arctan(T(1))
    if m02 == m20:
        ori = -pi / T(4) if m11 > 0 else pi / T(4)          # b < 0 <=> M11 > 0
    else:
        ori = np.arctan2(T(2 * m11), T(m20 - m02)) / T(2)
    f[5] = (ori + pi / T(2)) / pi
    f[6] = A / T(int(raw[RAW_CONVEX]))
    h, w = T(int(raw[RAW_MAXR] - raw[RAW_MINR])), T(int(raw[RAW_MAXC] - raw[RAW_MINC]))
    f[7] = A / (h * w)
    f[8] = (w / h) / T(3)
    f[9] = (T(int(raw[RAW_EULER])) + T(2)) / T(4)
    npx = H * W
    for k, flipped in ((10, img[:, ::-1]), (11, img[::-1, :])):
        mean = np.abs(img - flipped).astype(T).sum() / T(npx)          # float32 differences, as the reference forms them; the mean exactly
        f[k] = T(1) - mean
        scale[k] = 1.0 + (npx - 1) * float(mean)
    scale[3], scale[4] = abs(float(f[3])), abs(float(f[4]))
    return f, scale


def bounds(f, scale, consts=C_MORPH):
    """the derived bound per feature [12] (inf where a feature is compared in ulps instead)"""
    b = np.full(12, np.inf)
    for k in BOUNDED:
        b[k] = U32 * abs(float(f[k])) + consts[k] * U64 * float(scale[k])
    return b


def ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float32))
    return np.spacing(v).astype(np.float64)


def measure(img, threshold=THRESHOLD, norms=NORMS, extras=None):
    """(raw [RAW_WORDS] int64, features [12] longdouble, scale [12]) of one image"""
    raw = raw_record(img, threshold, extras)
    f, scale = features(raw, img, norms)
    return raw, f, scale


def extract_refined_features(img, threshold=THRESHOLD, norms=NORMS):
    """the reference function's result under this specification: float32 [12]"""
    _raw, f, _s = measure(np.asarray(img, dtype=np.float32).reshape(img.shape[-2:]), threshold, norms)
    return f.astype(np.float32)


def check_features(got, f, scale, what):
    """assert one image's float32 features against the longdouble ones; returns the largest ratio of the bounded features"""
    got = np.asarray(got, dtype=np.float32)
    ref32 = f.astype(np.float32)
    worst = 0.0
    for k in EXACT_ULP:
        if np.isnan(ref32[k]):
            assert np.isnan(got[k]), (what, FEATURE_NAMES_12[k], got[k])
            continue
        assert abs(float(got[k]) - float(ref32[k])) <= ulp32(ref32[k]), (what, FEATURE_NAMES_12[k], got[k], ref32[k])
    b = bounds(f, scale)
    for k in BOUNDED:
        if np.isnan(ref32[k]):          # a NaN pixel reaches the symmetry means, here as in the reference
            assert np.isnan(got[k]), (what, FEATURE_NAMES_12[k], got[k])
            continue
        err = abs(float(np.longdouble(got[k]) - f[k]))
        assert err <= b[k], (what, FEATURE_NAMES_12[k], got[k], f[k], err, b[k])
        worst = max(worst, err / b[k] if b[k] > 0 else 0.0)
    return worst


def rounded_differently(got, f):
    """how many of one image's float32 features are not the float32 nearest to the longdouble value"""
    got, ref32 = np.asarray(got, dtype=np.float32), f.astype(np.float32)
    return int(((got != ref32) & ~(np.isnan(got) & np.isnan(ref32))).sum())


# ---- consumers: the reference's host loops, and how the feature bounds travel through them ----
def feature_slack(f, scale):
    """|device float32 feature - this module's float32 feature| can be at most this, per feature [12]: one ulp, or the derived bound plus the rounding of the
    reference's own float32 (half an ulp); 0 for a NaN (both are NaN)"""
    ref32 = f.astype(np.float32)
    e = np.where(np.isnan(ref32), 0.0, ulp32(np.nan_to_num(ref32)))
    b = bounds(f, scale)
    for k in BOUNDED:
        e[k] = b[k] + 0.5 * ulp32(ref32[k])
    return e


def measure_batch(images):
    """float32 features [..., 12] and slacks [..., 12] of images [..., H, W] by the host loop"""
    images = np.asarray(images, dtype=np.float32)
    lead = images.shape[:-2]
    flat = images.reshape((-1,) + images.shape[-2:])
    F, E = np.zeros((len(flat), 12), dtype=np.float32), np.zeros((len(flat), 12))
    for i, im in enumerate(flat):
        _raw, f, scale = measure(im)
        F[i], E[i] = f.astype(np.float32), feature_slack(f, scale)
    return F.reshape(lead + (12,)), E.reshape(lead + (12,))


def sensitivity_host(images):
    """analyze_counterfactual.py:74-102 on images [T, N, H, W]: all_measured_m [N, T, 12] -> (std over T per sample [N, 12], its mean [12], bound [12]).
    std is a seminorm scaled by 1 / sqrt(T): |std(x) - std(y)| <= std(x - y) <= max |x - y|, so the bound on the mean is the mean over samples of the largest
    slack over T, plus the float64 rounding of the two reductions (8 ulps of float64 of the largest value)."""
    F, E = measure_batch(images)
    F, E = F.transpose(1, 0, 2).astype(np.float64), E.transpose(1, 0, 2)
    std = np.std(F, axis=1)
    return std, std.mean(axis=0), E.max(axis=1).mean(axis=0) + 8 * 2.0 ** -52 * np.nan_to_num(np.abs(F)).max()


def pair_contrast_host(images_a, images_b):
    """analyze_pairwise_importance.py:64-74: mean |feat_a - feat_b| [12], its 0-100 normalisation, and the bound of each.  ||a - b| - |a' - b'|| <= e_a + e_b;
    v / (m + 1e-9): |d(v / m)| <= (dv + (v / m) dm) / m with dm <= max dv."""
    Fa, Ea = measure_batch(images_a)
    Fb, Eb = measure_batch(images_b)
    diff = np.abs(Fa - Fb).astype(np.float64).mean(axis=0)          # float32 subtraction, as torch.abs(feat_a - feat_b) does it
    e = (Ea + Eb).mean(axis=0) + ulp32(np.nan_to_num(np.abs(Fa - Fb))).max(axis=0) + 8 * 2.0 ** -52
    m = np.nanmax(diff) + 1e-9
    norm = diff / m * 100
    e_norm = 100 * (e + (np.nan_to_num(diff) / m) * np.nanmax(e)) / m * (1 + 1e-12) + 1e-12
    return diff, norm, e, e_norm


# ---- the cases ----
SHAPES = ((1, 1), (1, 9), (5, 7), (28, 28), (33, 64), (64, 64))
N_BLOBS = 64


def grey(mask, lo=0.0, hi=1.0):
    return np.where(np.asarray(mask, dtype=bool), np.float32(hi), np.float32(lo)).astype(np.float32)


def serpentine(H, W):
    """a one-pixel corridor that runs every other row and turns at alternate ends: the longest label propagation"""
    m = np.zeros((H, W), dtype=bool)
    m[0::2, :] = True
    for k, r in enumerate(range(1, H, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """a one-pixel corridor wound inwards with one-pixel gaps"""
    m = np.zeros((H, W), dtype=bool)
    top, bottom, left, right = 0, H - 1, 0, W - 1
    r, c, d = 0, 0, 0
    m[0, 0] = True
    while True:
        if d == 0:
            nr, nc, ok = r, right, right > c
            top += 2
        elif d == 1:
            nr, nc, ok = bottom, c, bottom > r
            right -= 2
        elif d == 2:
            nr, nc, ok = r, left, left < c
            bottom -= 2
        else:
            nr, nc, ok = top, c, top < r
            left += 2
        if not ok:
            return m
        m[min(r, nr):max(r, nr) + 1, min(c, nc):max(c, nc) + 1] = True
        r, c, d = nr, nc, (d + 1) % 4


def comb(H, W):
    m = np.zeros((H, W), dtype=bool)
    m[H - 1, :] = True
    m[:, 0::2] = True
    return m


def blob(H, W, seed):
    rng = np.random.RandomState(seed)
    s = ndimage.gaussian_filter(rng.rand(H, W), sigma=max(0.8, min(H, W) / 9.0), mode="constant")
    lo, hi = s.min(), s.max()
    s = (s - lo) / (hi - lo) if hi > lo else np.full_like(s, 0.5)
    level = rng.uniform(0.3, 0.7)
    return np.clip(0.2 + 1.5 * (s - level) + 0.05 * rng.rand(H, W), 0.0, 1.0).astype(np.float32)


def place(H, W, pixels, r0=0, c0=0):
    m = np.zeros((H, W), dtype=bool)
    for r, c in pixels:
        m[r0 + r, c0 + c] = True
    return m


def rect(H, W, r0, c0, h, w):
    m = np.zeros((H, W), dtype=bool)
    m[r0:r0 + h, c0:c0 + w] = True
    return m


RING = [(r, c) for r in range(5) for c in range(5) if not (1 <= r <= 3 and 1 <= c <= 3)]
EIGHT = [(r, c) for r in range(7) for c in range(4) if not (r in (1, 2, 4, 5) and c in (1, 2))]
ELL = [(r, 0) for r in range(6)] + [(5, c) for c in range(1, 4)]
ON_EDGE = [(0, 0), (1, 1), (1, 2)]          # the centre of (0, 1) lies on the hull edge from the top of (0, 0) to the top of (1, 2)

_CASES = {}


def cases(shape):
    """[(name, image [H, W] float32)] of one shape: the constructed masks that fit it, then N_BLOBS seeded blobs"""
    if shape in _CASES:
        return _CASES[shape]
    H, W = shape
    out = [("empty", grey(np.zeros(shape, bool))), ("full", grey(np.ones(shape, bool))), ("single", grey(place(H, W, [(0, 0)]))),
           ("last-pixel", grey(place(H, W, [(H - 1, W - 1)])))]
    thr = np.float32(THRESHOLD)
    at = np.full(shape, thr, dtype=np.float32)          # every pixel equal to the threshold: below it; one a step above
    at[H // 2, W // 2] = np.nextafter(thr, np.float32(1))
    out.append(("at-threshold", at))
    nan = grey(place(H, W, [(0, 0)]), 0.1, 0.9)
    nan[H - 1, W - 1] = np.nan
    out.append(("nan-pixel", nan))
    chk = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
    iso = np.zeros(shape, dtype=bool)
    iso[0::2, 0::2] = True
    out += [("checkerboard", grey(chk, 0.1, 0.7)), ("isolated", grey(iso)), ("serpentine", grey(serpentine(H, W))), ("spiral", grey(spiral(H, W))),
            ("comb", grey(comb(H, W))), ("diagonal", grey(np.eye(H, W, dtype=bool))), ("antidiagonal", grey(np.eye(H, W, dtype=bool)[:, ::-1]))]
    frame = np.zeros(shape, dtype=bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    out.append(("four-borders", grey(frame)))
    if H >= 2 and W >= 2:
        out += [("diag2", grey(place(H, W, [(0, 0), (1, 1)]))), ("anti2", grey(place(H, W, [(0, 1), (1, 0)])))]
    if H >= 2 and W >= 3:
        out.append(("on-edge", grey(place(H, W, ON_EDGE))))
    if H >= 5 and W >= 7:
        out += [("rect-wide", grey(rect(H, W, 1, 1, 3, 5))), ("rect-tall", grey(rect(H, W, 0, 2, 5, 2))), ("square", grey(rect(H, W, 1, 2, 3, 3))),
                ("ring", grey(place(H, W, RING, 0, 1)))]
    if H >= 28 and W >= 28:
        two = rect(H, W, 2, 2, 3, 3) | rect(H, W, 10, 12, 3, 3)
        line_square = rect(H, W, 1, 1, 1, 20) | rect(H, W, 8, 8, 4, 4)          # the line is larger (20 > 16), the square is thicker
        out += [("eight", grey(place(H, W, EIGHT, 3, 5))), ("ell", grey(place(H, W, ELL, 4, 4))), ("two-equal", grey(two)), ("thick-elsewhere", grey(line_square)),
                ("ring-and-eight", grey(place(H, W, RING, 1, 1) | place(H, W, EIGHT, 12, 12)))]
    out += [(f"blob{s}", blob(H, W, 1000 * H + 10 * W + s)) for s in range(N_BLOBS)]
    _CASES[shape] = out
    return out


_REF = {}


def reference(shape):
    """{"names", "images" [B, H, W], "raw" [B, RAW_WORDS], "f" [B, 12] longdouble, "scale" [B, 12], "extras" [dict]} of a shape's cases, computed once"""
    if shape not in _REF:
        cs = cases(shape)
        raws, fs, scales, extras = [], [], [], []
        for _name, img in cs:
            ex = {}
            raw, f, scale = measure(img, extras=ex)
            raws.append(raw); fs.append(f); scales.append(scale); extras.append(ex)
        _REF[shape] = dict(names=[n for n, _ in cs], images=np.stack([im for _, im in cs]), raw=np.stack(raws), f=np.stack(fs), scale=np.stack(scales),
                           extras=extras)
    return _REF[shape]


def synthetic_digits(n, seed=0):
    """(uint8 images [n, 28, 28], labels [n]): strokes of a few pixels' width, for morph_mnist12"""
    rng = np.random.RandomState(seed)
    imgs = np.zeros((n, 28, 28), dtype=np.uint8)
    for i in range(n):
        s = ndimage.gaussian_filter(rng.rand(28, 28), 2.5)
        s = (s - s.min()) / (s.max() - s.min())
        imgs[i] = np.clip(255 * np.clip(3 * (s - 0.55), 0, 1), 0, 255).astype(np.uint8)
    return imgs, rng.randint(0, 10, n)
