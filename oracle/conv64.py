"""Float64 reference of the k4 / s2 / p1 convolution family (include/cvae_hip.h: csrc/conv_mfma.hip, csrc/conv_c1.hip) with derived error bounds.

  down(L, w, bias, act, mask)            S = act(gather(L, w) + bias) [* (mask > 0)]      nn.Conv forward, ConvTranspose backward-data
  up(S, w, bias, act, mask, l_dims)      L = act(scatter(S, w) + bias) [* (mask > 0)]     nn.ConvTranspose forward, Conv backward-data (l = 2 s or 2 s + 1)
  wgrad(S, L, dbias_side)                dW[cs][cl][k] = sum S[b, s, cs] L[b, 2 s - 1 + k, cl], and the bias gradient (0: sum of S, 1: sum of L)

Tensors are channels-last [B, D, H, W, C] (D == 1 for 2D) of any dtype / device, the weight is [Cs][Cl][k..] (4 x 4 or 4 x 4 x 4: its rank gives nd);
all work is float64 on the CPU.  Each function returns `ref` and an elementwise `err`, the bound on how far an fp32 evaluation of the same sum may lie
from it, by the rule of oracle/fused64.py: a product-sum of K terms contributes C sqrt(K) U (|A| . |B| + |bias|) with C = 4, U = 2^-24 and K the real
number of terms of THAT element (taps inside the volume x Cl for `down`; 2^nd taps x Cs for `up`; batch x positions whose tap lies inside L for
`wgrad`).  Split-K, K-split waves, slabs and grouped launches reorder the same sum: they do not change K.  ReLU and LeakyReLU are 1-Lipschitz and sigmoid
1/4-Lipschitz, so the bound passes through the activation (sigmoid adds 4 U for its own expf / divide); a mask multiplies both by 0 / 1.
`out_bound` adds the rounding of the stored result: half a bf16 ulp, or half an e4m3 ulp (with the subnormal step 2^-9 and saturation at 448).

Operands are the caller's business — the reference multiplies exactly what it is given:
  * bf16 launches: pass activations already rounded to bf16 and the weight rounded to bf16 (the pack kernels round the fp32 master weight once);
  * the single-channel layers (Cl == 1) take the fp32 master weight in every form, and what they multiply depends on the compute dtype: the fp32 kernels
    (down_c1_kernel<float>, up_c1_kernel, wgrad_c1_kernel<float>) multiply it as it is; the bf16 kernels (down_c1_kernel<bf16>, down_c1_vec_kernel,
    up_c1_mfma_kernel, up_c1_mfma_walk_kernel) round it to bf16 into MFMA fragments, so their reference takes the bf16-rounded weight; the mixed forms
    (fp32 image, bf16 S: down_c1_vec_kernel<float>, wgrad_c1_kernel<bf16, float>) round the IMAGE to bf16 on its way into LDS, so their reference takes
    the bf16-rounded image;
  * fp8 launches: pass decoded codes times their scales (tensor and weight alike).

fp8 products (f8_mfma=True) carry one more term, from the arithmetic of v_mfma_scale_f32_32x32x64_f8f6f4 itself as measured with uniform operands
(tools/probes/mfma_f8_sum_probe.hip, results in its header): the instruction adds its 64 products in groups of 8, and inside a group every product is
TRUNCATED toward zero to a multiple of 2^(E - 13), E the exponent of the group's largest product (next to 2^16, a product of 4 vanishes and 15 becomes 8);
the group sums and C are then added at about fp32 precision.  So every product may lose up to 2^-13 of the largest product it is grouped with, whatever
fp32 would have kept: C sqrt(K) 2^-13 Pmax by the same independent-errors rule, Pmax = the largest |product| of that element (computed tap by tap; no
product is grouped with a larger one, so the grouping inside the kernel need not be known).  Truncation toward zero is a BIASED error: the sqrt(K) rule
holds here because the weights, hence the products, have both signs; a product-sum of one sign would need K in place of sqrt(K).  The bf16 and fp32
MFMAs show no such term (ratios <= 0.4).

drop= (self-tests only, tests/test_conv_reference_cpu.py) evaluates a deliberately wrong variant of the product; see _MUTATIONS.
"""
import math

import torch
import torch.nn.functional as F

from .fused64 import BF16_HALF_ULP, C, U, _ps, compare  # noqa: F401  (compare is re-exported: one comparison for every reference)

_MUTATIONS = {
    "product": "('product', (c_in, tap)): one (tap, input channel) product missing from every sum  [down, up]",
    "kstep": "('kstep', (c0, tap)): the 16 input channels c0 .. c0 + 15 of one tap missing  [down, up]",
    "replicate_face": "('replicate_face', axis): the zero padding of the low face of one axis (0 = D, 1 = H, 2 = W) replaced by edge replication  [down, up, wgrad]",
    "parity_shift": "('parity_shift', (pd, ph, pw)): the outputs of one parity class moved by one voxel along W within their class  [up]",
    "ragged_last": "('ragged_last',): the last position of the last sample left out of the sums  [wgrad]",
    "slab_bf16": "('slab_bf16', n): the sum cut into n partial slabs (input-channel chunks for down, position slabs for wgrad), each rounded to bf16 before they are added  [down, wgrad]",
    "bias_per_split": "('bias_per_split', n): the bias added once per split, n times in all  [down, up]",
}
F8_GROUP_TRUNC = 2.0 ** -13     # the fp8 MFMA truncates a product to 2^-13 of the largest product of its group of 8 (module docstring)
LIPSCHITZ = {None: 1.0, "relu": 1.0, "leaky02": 1.0, "sigmoid": 0.25}


def _d64(v):
    return None if v is None else v.detach().to("cpu", torch.float64)


def _nc(x):
    """channels-last [B, D, H, W, C] -> [B, C, D, H, W] float64"""
    return _d64(x).permute(0, 4, 1, 2, 3).contiguous()


def _cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _w5(w):
    """weight as float64 [Cs][Cl][kd][4][4] (kd = 1 for 2D) and nd"""
    w = _d64(w)
    return (w.unsqueeze(2), 2) if w.dim() == 4 else (w, 3)


def _geom(nd):
    return ((1, 2, 2), (0, 1, 1)) if nd == 2 else ((2, 2, 2), (1, 1, 1))


def _act(pre, act):
    if act is None:
        return pre
    if act == "relu":
        return F.relu(pre)
    if act == "leaky02":
        return F.leaky_relu(pre, 0.2)
    if act == "sigmoid":
        return torch.sigmoid(pre)
    raise ValueError(act)


def _finish(pre, e_pre, act, mask):
    ref = _act(pre, act)
    err = LIPSCHITZ[act] * e_pre + (4 * U * ref.abs() if act == "sigmoid" else 0.0)
    if mask is not None:
        keep = (_d64(mask) > 0).to(torch.float64)
        ref, err = ref * keep, err * keep
    return ref, err


def _bf16(v):
    return v.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _tap_index(tap, nd):
    """flat tap number (kd, kh, kw order; kh, kw for 2D) -> index into the [kd][4][4] weight"""
    return (0, tap // 4, tap % 4) if nd == 2 else (tap // 16, tap // 4 % 4, tap % 4)


def _drop_weight(w, nd, drop, in_axis):
    """zero the weight entries of a 'product' / 'kstep' mutation; in_axis: the weight axis of the INPUT channel (1 for down, 0 for up)"""
    if not drop or drop[0] not in ("product", "kstep"):
        return w
    c0, tap = drop[1]
    n = 1 if drop[0] == "product" else 16
    w = w.clone()
    kd, kh, kw = _tap_index(tap, nd)
    if in_axis == 1:
        w[:, c0:c0 + n, kd, kh, kw] = 0.0
    else:
        w[c0:c0 + n, :, kd, kh, kw] = 0.0
    return w


def down(L, w, bias=None, act=None, mask=None, drop=None, f8_mfma=False):
    """S = act(conv_k4s2p1(L, w) + bias) [* (mask > 0)].  L [B, ld, lh, lw, Cl], w [Cs][Cl][k..], bias [Cs], mask of S's shape; s = floor(l / 2).
    Returns (ref, err, pre, e_pre): the result and its bound (before the rounding of the stored value: out_bound), and the pre-activation with its bound
    (what decides a ReLU mask bit: relu_bits)."""
    w5, nd = _w5(w)
    stride, pad = _geom(nd)
    x = _nc(L)
    b = _d64(bias)
    Cl = x.shape[1]
    padding = (pad[2], pad[2], pad[1], pad[1], pad[0], pad[0])
    xp, xa = F.pad(x, padding), F.pad(x.abs(), padding)
    if drop and drop[0] == "replicate_face":
        ax = 2 + drop[1]
        idx0, idx1 = [slice(None)] * 5, [slice(None)] * 5
        idx0[ax], idx1[ax] = 0, 1
        xp = xp.clone()
        xp[tuple(idx0)] = xp[tuple(idx1)]
    wm = _drop_weight(w5, nd, drop, 1)
    if drop and drop[0] == "slab_bf16":
        n = drop[1]
        step = Cl // n
        pre = sum(_bf16(F.conv3d(xp[:, i * step:(i + 1) * step], wm[:, i * step:(i + 1) * step], None, stride)) for i in range(n))
    else:
        pre = F.conv3d(xp, wm, None, stride)
    nb = drop[1] if (drop and drop[0] == "bias_per_split") else 1
    if b is not None:
        pre = pre + nb * b.view(1, -1, 1, 1, 1)
    mag = F.conv3d(xa, w5.abs(), None, stride) + (b.abs().view(1, -1, 1, 1, 1) if b is not None else 0.0)
    ones = F.pad(torch.ones(1, 1, *x.shape[2:], dtype=torch.float64), padding)
    K = F.conv3d(ones, torch.ones(1, 1, *w5.shape[2:], dtype=torch.float64), None, stride) * Cl          # taps inside the volume x channels
    e_pre = C * torch.sqrt(K.clamp_min(1.0)) * U * mag
    if f8_mfma:
        pm = torch.zeros_like(mag)                           # the largest |product| of each element
        wa, (sd_, sh_, sw_) = w5.abs(), mag.shape[2:]
        for kd in range(w5.shape[2]):
            for kh in range(4):
                for kw in range(4):
                    xs = xa[:, :, kd:kd + stride[0] * sd_:stride[0], kh:kh + 2 * sh_:2, kw:kw + 2 * sw_:2]
                    pm = torch.maximum(pm, (xs.permute(0, 2, 3, 4, 1).unsqueeze(4) * wa[:, :, kd, kh, kw]).amax(-1).permute(0, 4, 1, 2, 3))
        e_pre = e_pre + C * torch.sqrt(K.clamp_min(1.0)) * F8_GROUP_TRUNC * pm
    pre, e_pre = _cl(pre), _cl(e_pre)
    ref, err = _finish(pre, e_pre, act, mask)
    return ref, err, pre, e_pre


def _crop(full, l_dims, nd, shift=(0, 0, 0)):
    """the padding-1 window of a padding-0 transposed convolution: output index l sits at l + 1 of the full result"""
    d0 = (0 if nd == 2 else 1) + shift[0]
    return full[:, :, d0:d0 + l_dims[0], 1 + shift[1]:1 + shift[1] + l_dims[1], 1 + shift[2]:1 + shift[2] + l_dims[2]]


def up(S, w, bias=None, act=None, mask=None, l_dims=None, drop=None, f8_mfma=False):
    """L = act(conv_transpose_k4s2p1(S, w) + bias) [* (mask > 0)].  S [B, sd, sh, sw, Cs], w [Cs][Cl][k..], bias [Cl], mask of L's shape.
    l_dims (ld, lh, lw): the extent of the result, 2 s (default) or 2 s + 1 per strided axis (the data gradient of a conv over an odd extent).
    Returns (ref, err, pre, e_pre) as `down`."""
    w5, nd = _w5(w)
    stride, _ = _geom(nd)
    x = _nc(S)
    b = _d64(bias)
    Cs = x.shape[1]
    sd, sh, sw = x.shape[2:]
    l_dims = ((1 if nd == 2 else 2 * sd), 2 * sh, 2 * sw) if l_dims is None else tuple(int(v) for v in l_dims)
    for l, s, strided in zip(l_dims, (sd, sh, sw), (nd == 3, True, True)):
        assert (l in (2 * s, 2 * s + 1)) if strided else l == 1, (l_dims, (sd, sh, sw))
    wm = _drop_weight(w5, nd, drop, 0)
    shift = [0, 0, 0]
    xm = x
    if drop and drop[0] == "replicate_face":       # one replicated source plane in front of the low face: the window moves by one source voxel
        ax = drop[1]
        xm = torch.cat([x.narrow(2 + ax, 0, 1), x], 2 + ax)
        shift[ax] = 2
    pre = _crop(F.conv_transpose3d(xm, wm, None, stride), l_dims, nd, shift)
    nb = drop[1] if (drop and drop[0] == "bias_per_split") else 1
    if b is not None:
        pre = pre + nb * b.view(1, -1, 1, 1, 1)
    if drop and drop[0] == "parity_shift":
        pd, ph, pw = drop[1]
        pre = pre.clone()
        sub = pre[:, :, (pd if nd == 3 else 0)::(2 if nd == 3 else 1), ph::2, pw::2]
        pre[:, :, (pd if nd == 3 else 0)::(2 if nd == 3 else 1), ph::2, pw::2] = torch.roll(sub, 1, 4)
    mag = _crop(F.conv_transpose3d(x.abs(), w5.abs(), None, stride), l_dims, nd) + (b.abs().view(1, -1, 1, 1, 1) if b is not None else 0.0)
    e_pre = _ps(2 ** nd * Cs) * mag
    if f8_mfma:
        full = torch.zeros_like(F.conv_transpose3d(x[:, :1], w5[:1].abs(), None, stride))      # the largest |product| of each element, scattered tap by tap
        xl, wa = x.abs().permute(0, 2, 3, 4, 1).unsqueeze(4), w5.abs()
        for kd in range(w5.shape[2]):
            for kh in range(4):
                for kw in range(4):
                    m = (xl * wa[:, :, kd, kh, kw].t()).amax(-1).permute(0, 4, 1, 2, 3)
                    dsl = slice(kd, kd + 2 * sd, 2) if nd == 3 else slice(0, 1)
                    view = full[:, :, dsl, kh:kh + 2 * sh:2, kw:kw + 2 * sw:2]
                    full[:, :, dsl, kh:kh + 2 * sh:2, kw:kw + 2 * sw:2] = torch.maximum(view, m)
        e_pre = e_pre + C * math.sqrt(2 ** nd * Cs) * F8_GROUP_TRUNC * _crop(full, l_dims, nd)
    pre, e_pre = _cl(pre), _cl(e_pre)
    ref, err = _finish(pre, e_pre, act, mask)
    return ref, err, pre, e_pre


def wgrad(S, L, dbias_side=None, nd=3, drop=None):
    """dW [Cs][Cl][k..] = sum over batch and positions of S[b, s, cs] L[b, 2 s - 1 + k, cl] (zero outside L), and with dbias_side 0 / 1 the bias
    gradient: the sum of S over batch and positions [Cs] / of L [Cl].  S [B, sd, sh, sw, Cs], L [B, ld, lh, lw, Cl], l >= 2 s.
    Returns (ref, err): dicts with 'dW' and, when asked for, 'dbias'."""
    s, l = _d64(S), _d64(L)
    B, sd, sh, sw, Cs = s.shape
    _, ld, lh, lw, Cl = l.shape
    if drop and drop[0] == "ragged_last":
        s = s.clone()
        s[-1, -1, -1, -1, :] = 0.0
    pads = (0, 0, 1, 1, 1, 1) + ((1, 1) if nd == 3 else (0, 0))
    lp = F.pad(l, pads)
    if drop and drop[0] == "replicate_face":
        ax = 1 + drop[1]
        i0, i1 = [slice(None)] * 5, [slice(None)] * 5
        i0[ax], i1[ax] = 0, 1
        lp[tuple(i0)] = lp[tuple(i1)]
    kd_n = 4 if nd == 3 else 1
    dW = torch.zeros(Cs, Cl, kd_n, 4, 4, dtype=torch.float64)
    mag = torch.zeros_like(dW)
    K = torch.zeros(kd_n, 4, 4, dtype=torch.float64)
    inside = lambda k, n_s, n_l: sum(1 for i in range(n_s) if 0 <= 2 * i - 1 + k < n_l)
    sf, sa = s.reshape(-1, Cs), s.abs().reshape(-1, Cs)
    nsl = drop[1] if (drop and drop[0] == "slab_bf16") else 0
    for kd in range(kd_n):
        for kh in range(4):
            for kw in range(4):
                dsl = slice(kd, kd + 2 * sd, 2) if nd == 3 else slice(0, 1)
                lk = lp[:, dsl, kh:kh + 2 * sh:2, kw:kw + 2 * sw:2, :].reshape(-1, Cl)
                if nsl:
                    cuts = [round(i * sf.shape[0] / nsl) for i in range(nsl + 1)]
                    dW[:, :, kd, kh, kw] = sum(_bf16(sf[a:b].t() @ lk[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
                else:
                    dW[:, :, kd, kh, kw] = sf.t() @ lk
                mag[:, :, kd, kh, kw] = sa.t() @ lk.abs()
                K[kd, kh, kw] = B * (inside(kd, sd, ld) if nd == 3 else 1) * inside(kh, sh, lh) * inside(kw, sw, lw)
    e = C * torch.sqrt(K.clamp_min(1.0)) * U * mag
    if nd == 2:
        dW, e = dW[:, :, 0], e[:, :, 0]
    ref, err = {"dW": dW}, {"dW": e}
    if dbias_side is not None:
        t = l if dbias_side else s
        n = t.numel() // t.shape[-1]
        ref["dbias"] = t.reshape(n, -1).sum(0)
        err["dbias"] = _ps(n) * t.abs().reshape(n, -1).sum(0)
    return ref, err


# ------------------------------------------------------------------------------------------------ the rounding of the stored result
def e4m3_half_ulp(x):
    """half the spacing of OCP e4m3 at |x| (<= 448): 2^(floor(log2 |x|) - 4), and 2^-10 in the subnormal range |x| < 2^-6 (step 2^-9)"""
    a = x.abs().clamp(2.0 ** -6, 448.0)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 4.0)


def out_bound(ref, err, out, scale=1.0):
    """The reference and the bound of the STORED result.  out: 'f32' (as computed), 'bf16' (plus half a bf16 ulp at |ref| + err), or 'e4m3': codes of
    result / scale, compared as decoded code values times scale — the reference saturates at 448 scale, the bound adds the fp32 rounding of the
    multiplication by 1 / scale and half an e4m3 ulp at |ref| + err."""
    if out == "f32":
        return ref, err
    if out == "bf16":
        return ref, err + BF16_HALF_ULP * (ref.abs() + err)
    if out == "e4m3":
        x, ex = ref / scale, err / scale + 2 * U * (ref / scale).abs()
        return x.clamp(-448.0, 448.0) * scale, (ex + e4m3_half_ulp((x.abs() + ex).clamp_max(448.0))) * scale
    raise ValueError(out)


def relu_bits(bits, pre, e_pre, mask=None):
    """Check a launch's relu_bits_out (int32 words, bit j of word i = element 32 i + j in memory order) against the pre-activation: the bit must equal
    pre > 0 wherever |pre| > e_pre (a masked element is 0: bit clear); elsewhere either value is accepted.  Returns (wrong, undecided, total)."""
    b = bits.detach().cpu().to(torch.int64) & 0xFFFFFFFF
    got = ((b.reshape(-1, 1) >> torch.arange(32, dtype=torch.int64)) & 1).reshape(-1).bool()
    p, e = pre.reshape(-1), e_pre.reshape(-1)
    want = p > 0
    decided = p.abs() > e
    if mask is not None:
        keep = _d64(mask).reshape(-1) > 0
        want = want & keep
        decided = decided | ~keep
    return int(((got != want) & decided).sum()), int((~decided).sum()), p.numel()


def undecided_fraction(pre, e_pre):
    """share of a case's elements whose ReLU bit the bound cannot decide (must stay <= 0.1 %: the inputs, not the kernel, keep it so)"""
    return float((pre.abs() <= e_pre).double().mean())


def max_ratio(got, ref, err):
    """max |got - ref| / err over the elements with err > 0 (an element with err == 0 must match exactly: inf otherwise)"""
    g = got.detach().to("cpu", torch.float64).reshape(ref.shape)
    d = (g - ref).abs()
    r = torch.where(err > 0, d / err.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max()) if r.numel() else 0.0


def structured(shape):
    """value = f(b, z, y, x, c) of small integers, every one exactly representable in bf16 (|v| <= 128) and distinct enough that a swapped index
    shows: v = ((3 b + 5 z + 7 y + 11 x + 13 c) mod 31) - 15"""
    B, D, H, W, Cc = shape
    ar = lambda n, k: torch.arange(n, dtype=torch.float64) * k
    v = ar(B, 3).view(B, 1, 1, 1, 1) + ar(D, 5).view(1, D, 1, 1, 1) + ar(H, 7).view(1, 1, H, 1, 1) + ar(W, 11).view(1, 1, 1, W, 1) + ar(Cc, 13).view(1, 1, 1, 1, Cc)
    return (v % 31 - 15).to(torch.float32)


def one_hot_weight(Cs, Cl, nd, shift=3):
    """w[cs][cl][tap] = 1 for exactly one (cl, tap) per cs — cl = (cs + shift) mod Cl, tap = (5 cs + 1) mod 4^nd — else 0: every output is ONE input element, so a
    wrong coordinate in a kernel shows as a wrong integer at a named place"""
    taps = 4 ** nd
    w = torch.zeros(Cs, Cl, taps)
    cs = torch.arange(Cs)
    w[cs, (cs + shift) % Cl, (5 * cs + 1) % taps] = 1.0
    return w.reshape(Cs, Cl, *([4] * nd))


# ------------------------------------------------------------------------------------------------ seeded cases
def make_case(kind, seed, nd, B, Cl, Cs, size, dtype=torch.float32, bias=True, masked=False, structure=False, odd_l=False, bits=False):
    """Inputs of one launch on the CPU, as fp32 tensors whose values are already rounded to `dtype` where the kernel reads that dtype.
    kind 'down': size = the LARGE extent (ld, lh, lw) / (lh, lw); 'up' and 'wgrad': size = the SMALL extent, L = 2 s (+ 1 per strided axis with odd_l).
    Keys: L or S (the input; both for wgrad), w (fp32 master weight, handed to the kernel), w_ref (what the kernel multiplies: w rounded to bf16 in a
    bf16 case), bias, mask (independent random 0 / 1 tensor of the result's shape, or None), l_dims / s_dims.
    structure: small-integer inputs (structured) and a one-hot weight.  bits: a bias of magnitude 1 .. 3 with mixed signs, which keeps the
    pre-activations of a ReLU-bit case away from zero (undecided_fraction)."""
    g = torch.Generator().manual_seed(seed)
    rd = lambda v: v.to(dtype).to(torch.float32)
    size = tuple(size)
    full = lambda e: ((1,) + e) if nd == 2 else e
    if kind == "down":
        l_dims = full(size)
        s_dims = tuple((v // 2) if (i > 0 or nd == 3) else 1 for i, v in enumerate(l_dims))
    else:
        s_dims = full(size)
        l_dims = tuple((2 * v + (1 if odd_l else 0)) if (i > 0 or nd == 3) else 1 for i, v in enumerate(s_dims))
    c = dict(kind=kind, nd=nd, dtype=dtype, l_dims=l_dims, s_dims=s_dims, B=B, Cl=Cl, Cs=Cs)
    fan = (Cl * 4 ** nd) if kind == "down" else (Cs * 2 ** nd)
    if structure:
        w = one_hot_weight(Cs, Cl, nd)
        mk = lambda shape: structured(shape)
    else:
        w = torch.randn(Cs, Cl, *([4] * nd), generator=g) / math.sqrt(fan)
        mk = lambda shape: rd(torch.randn(*shape, generator=g))
    c["w"], c["w_ref"] = w, rd(w)
    if kind in ("down", "wgrad"):
        c["L"] = mk((B, *l_dims, Cl))
    if kind in ("up", "wgrad"):
        c["S"] = mk((B, *s_dims, Cs))
    cout, odims = (Cs, s_dims) if kind == "down" else (Cl, l_dims)
    if bias and kind != "wgrad":
        b = torch.randn(cout, generator=g)
        if bits:
            b = torch.where(b >= 0, 1.0, -1.0) * (1.0 + 2.0 * torch.rand(cout, generator=g))
        c["bias"] = b
    else:
        c["bias"] = None
    c["mask"] = rd((torch.rand(B, *odims, cout, generator=g) > 0.4).float() * (0.5 + torch.rand(B, *odims, cout, generator=g))) if (masked and kind != "wgrad") else None
    return c


def reference(c, act=None, drop=None, dbias_side=None, f8_mfma=False):
    """the float64 reference of a make_case case: (ref, err, pre, e_pre) for down / up, (ref, err) dicts for wgrad"""
    if c["kind"] == "down":
        return down(c["L"], c["w_ref"], c["bias"], act, c["mask"], drop=drop, f8_mfma=f8_mfma)
    if c["kind"] == "up":
        return up(c["S"], c["w_ref"], c["bias"], act, c["mask"], l_dims=c["l_dims"], drop=drop, f8_mfma=f8_mfma)
    return wgrad(c["S"], c["L"], dbias_side, nd=c["nd"], drop=drop)


# the ReLU-bit cases of tests/test_conv_reference.py (kind, nd, B, Cl, Cs, size, dtype, split-K): the CPU file asserts on these very cases that at most 0.1 % of
# the elements are undecided
BIT_SEED = 600
BIT_CASES = [("down", 3, 2, 32, 64, (8, 8, 18), "bf16", True), ("down", 3, 1, 128, 256, (8, 8, 8), "f32", True), ("down", 3, 1, 128, 256, (8, 8, 8), "bf16", False),
             ("down", 2, 3, 32, 64, (30, 44), "bf16", True), ("up", 3, 2, 64, 128, (3, 4, 4), "bf16", True), ("up", 2, 3, 32, 64, (7, 7), "f32", True),
             ("up", 3, 1, 32, 64, (4, 4, 5), "bf16", True), ("up", 3, 2, 96, 64, (4, 9, 8), "bf16", True)]
