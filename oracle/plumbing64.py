"""Float64 references of csrc/elementwise.hip (cast, the two LDS transposes, concat panels, one-hot, activation forward / backward, channel sum, adaptive
average pool and bare flatten, linear resize) and csrc/vessel2d.hip (k3 <-> k4 weight transform, clamp, channels-last BatchNorm2d forward / backward) with derived
elementwise error bounds, in the style and with the constants of oracle/dense64.py and oracle/loss64.py (U = 2^-24, C = 4; `compare` and `max_ratio` are the same
functions; loss64.ULP for div / sqrtf / rsqrtf, dense64.ULP for __expf, measured over [-8, 8] only: a sigmoid argument beyond that range is refused).

Every function returns (ref, err): dicts of CPU tensors.  The rules:
  pure moves             cast, ncs_to_nsc / nsc_to_ncs, copy_panels, onehot_panel, flatten_fwd / flatten_bwd, clamp_fwd / clamp_bwd: ref is the expected tensor IN THE
                         DESTINATION DTYPE, err is zero: the result must have the same bits (`same_bits`: a NaN must be a NaN, its payload is free).  float -> bf16 is
                         round-to-nearest-even (`bf16_rne`, integer arithmetic, checked against torch's .bfloat16()).  clamp is torch.clamp: a NaN stays a NaN.
  activation             act_fwd: one fp32 operation (the slope product; ReLU and none are exact), the sigmoid is dense64's 1.f / (1.f + __expf(-v)).  act_bwd:
                         g = dy act'(y) with y the saved OUTPUT, an input of the call: dense64._act_grad (0, 1 or 3 roundings), its branch margin asserted.
  channel sum            C sqrt(P) U sum |x| per channel (P the real term count; row blocks, trees and the finish pass reorder the same sum).
  adaptive pool          windows [floor(o I / O), ceil((o + 1) I / O)) per axis, T = the window's real size: C sqrt(T) U sum |x| / T plus the division.
                         Backward: the sum over EVERY window that contains the voxel of dout / T; every quotient carries its division's rounding, the sum of n terms
                         C sqrt(n) U sum |term|; the ReLU mask is the sign of the stored x (an input: exact).
  linear resize          tap position s = scale (o + 0.5) - 0.5, scale the FP32 quotient in / out the kernel forms, evaluated in float64; clamped at 0; i0 = floor(s)
                         (at most in - 1), w1 = s - i0 (exact in fp32: Sterbenz), w0 = 1 - w1 (one rounding).  The nest of three levels costs per level two products,
                         one sum and the weight's rounding: NEST = 12 roundings over sum |w x|.  The kernel's s differs from the float64 one by at most
                         eps_s = U (|scale (o + 0.5)| + |s|): the product and the subtraction round once each ((float) o + 0.5f is exact; contracted into one FMA only
                         the second remains), and the value moves by eps_s |dv/ds| per axis, dv/ds the difference of the two taps' slices.  Near an integer s the
                         kernel's tap INDEX may differ from the reference's, but the value is continuous across it (w1 -> 1 on one side is w1 = 0 on the other):
                         a row whose s lies within 4 eps_s of an integer takes the steeper of the two segments that meet there (3 -> 7 and 300 -> 420 have such
                         rows: s = 1 at o = 3 with an inexact fp32 scale).
                         Backward: the transpose with the same weights; a source voxel's T nonzero terms cost (C sqrt(T) + NEST) U sum |w g| plus the same tap term.
  k3 <-> k4              K4 = A W3 A^T, dW3 = A^T dK4 A, A of 0 / 1: sums of at most four terms, C sqrt(4) U sum |terms|.
  BatchNorm2d            loss64.bn1d's two-pass rule with this kernel's operations: mean = sum * (1.f / P), var = sqdev / P, rstd = 1.f / sqrtf(var + eps); the
                         rounding of x - mean is amplified by rstd; running statistics with the unbiased variance var * (P / (P - 1.f)) and the fp32 momentum; the
                         activation through dense64._act.  Backward: g = dy act'(y) (y an input), dbeta = sum g, dgamma = sum g (x - mean) rstd, and
                         dx = gamma rstd / P (P g - dbeta - xhat dgamma) bounded over the MAGNITUDES P |g| + |dbeta| + |xhat dgamma| of the cancelling inner sum.
  bf16                   the caller passes operands already rounded to bf16 (`bf16`); an output stored in bf16 adds one bf16 rounding (fused64.bf16_out).
dtype = torch.float32 evaluates the same formulas in fp32 on the CPU (the stand-in for a correct kernel of tests/test_plumbing_reference_cpu.py; the bounds returned
with it are meaningless).  drop= (self-tests only) evaluates a deliberately wrong variant, see _MUTATIONS.

The second half replays the launch geometry of both files (grid_1d, channel_sum_geometry, bn2d_blocks) and holds the shape tables both test files walk, the seam
each row crosses named next to it.
"""
import math

import torch

from . import dense64 as d64
from .conv64 import max_ratio  # noqa: F401  (re-exported: the tests take it from here)
from .fused64 import C, U, _ps, bf16_out, compare  # noqa: F401
from .loss64 import ULP as _LOSS_ULP
from .loss64 import f32, gen  # noqa: F401

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NONE, RELU, SIGMOID, LEAKY02, LEAKY001 = d64.ACTS
ACTS = d64.ACTS
SIG_RANGE, BRANCH_MARGIN = d64.SIG_RANGE, d64.BRANCH_MARGIN
ULP = {"__expf": d64.ULP["__expf"], "div": _LOSS_ULP["div"], "sqrtf": _LOSS_ULP["sqrtf"], "rsqrtf": _LOSS_ULP["rsqrtf"]}
NEST = 12.0

_MUTATIONS = {
    "last_row": "('last_row',): the channel sum without its last row  [channel_sum; the bound at small P, the structured case at every P]",
    "unclipped_div": "('unclipped_div',): the pool divisor is the nominal window I / O per axis, not the real window's size  [pool_fwd; bound and structured; equal at 8 -> 4]",
    "pm1": "('pm1',): the pool backward looks for windows only among floor(i O / I) - 1 .. + 1, the rule shipped before this file  [pool_bwd; bound and structured at "
           "1 -> 3, 2 -> 7; identical at O <= I]",
    "align_corners": "('align_corners',): resize taps at s = o (in - 1) / (out - 1)  [resize_fwd / resize_bwd; bound]",
    "swap_taps": "('swap_taps',): the two tap weights of every axis exchanged  [resize_fwd / resize_bwd; bound]",
    "biased_running_var": "('biased_running_var',): running_var updated with the biased variance  [bn2d_fwd; bound on running_var]",
    "one_pass_var": "('one_pass_var',): var = E[x^2] - E[x]^2 in fp32  [bn2d_fwd; bound, in the channel of mean 50 and std 0.1]",
    "dx_no_dgamma": "('dx_no_dgamma',): dx without its xhat dgamma term  [bn2d_bwd; bound]",
    "tile_edge": "('tile_edge',): index 64 of the transposed axes (the second 64-wide tile's first row / column) left unwritten  [ncs_to_nsc / nsc_to_ncs / flatten; bits]",
    "bf16_trunc": "('bf16_trunc',): float -> bf16 by truncation  [every pure move with a bf16 destination; bits, on the ties and on random values]",
}


def _chk(drop):
    if drop and drop[0] not in _MUTATIONS:
        raise ValueError(drop[0])
    return drop[0] if drop else None


def _t(v, dtype):
    return None if v is None else v.detach().to("cpu").to(dtype)


def _out(ref, err):
    return {k: v.detach().to(F64) for k, v in ref.items()}, {k: v.detach().to(F64) for k, v in err.items()}


def _u(name):
    return ULP[name] * 2.0 * U


def bf16(v):
    """v rounded to bf16 (nearest-even), as fp32: what a kernel reading bf16 sees"""
    return None if v is None else v.detach().to(F32).to(BF16).to(F32)


# ------------------------------------------------------------------------------------------------ pure moves
def bf16_rne(x, trunc=False):
    """float32 -> bfloat16 in integer arithmetic: round to nearest, ties to even (NaN -> a quiet NaN); trunc: drop the low 16 bits"""
    b = x.detach().to("cpu", F32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    r = (b >> 16) if trunc else ((b + 0x7FFF + ((b >> 16) & 1)) >> 16)
    r = torch.where(nan, (b >> 16) | 0x40, r) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16).view(BF16)


def move(v, dd=F32, drop=None):
    """v (fp32 or bf16 values) as the destination dtype dd holds it"""
    v = v.detach().to("cpu")
    if dd == F32:
        return v.to(F32)
    return v if v.dtype == BF16 else bf16_rne(v, trunc=_chk(drop) == "bf16_trunc")


def bits(v):
    v = v.detach().to("cpu").contiguous()
    return v.view(torch.int32 if v.dtype == F32 else torch.int16)


def same_bits(got, want):
    """elementwise: the same bits, or both NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return (bits(got) == bits(want)) | (torch.isnan(got.float()) & torch.isnan(want.float()))


def _exact(**ref):
    return ref, {k: torch.zeros(v.shape, dtype=F64) for k, v in ref.items()}


def _edge(v, drop, dims):
    """the 'tile_edge' mutation: index 64 of each of `dims` zeroed"""
    if _chk(drop) == "tile_edge":
        v = v.clone()
        for d in dims:
            if v.shape[d] > 64:
                v.select(d, 64).zero_()
    return v


def cast(x, dd=F32, drop=None):
    return _exact(dst=move(x, dd, drop))


def ncs_to_nsc(x, dd=F32, drop=None):
    """x [B][C][S] -> [B][S][C]"""
    return _exact(dst=_edge(move(x, dd, drop).permute(0, 2, 1).contiguous(), drop, (1, 2)))


def nsc_to_ncs(x, dd=F32, drop=None):
    """x [B][S][C] -> [B][C][S]"""
    return _exact(dst=_edge(move(x, dd, drop).permute(0, 2, 1).contiguous(), drop, (1, 2)))


def copy_panels(panels, wide, col0, gather):
    """panels: list of [B][w_i]; wide [B][ws].  gather == 0: the panels written into wide[:, col0 ..]; else: those column ranges out into the panels"""
    wide = wide.detach().clone()
    off, outs = col0, []
    for pnl in panels:
        w = pnl.shape[1]
        if gather:
            outs.append(wide[:, off:off + w].clone())
        else:
            wide[:, off:off + w] = pnl
        off += w
    return _exact(**({f"p{i}": o for i, o in enumerate(outs)} if gather else dict(wide=wide)))


def onehot_panel(t, nc):
    """t [B] int64 -> [B][nc]; a class outside [0, nc) gives a row of zeros"""
    return _exact(dst=(t.detach().to("cpu")[:, None] == torch.arange(nc)[None, :]).to(F32))


def flatten_fwd(x, drop=None):
    """x [B][V][C] -> out [B][C V] fp32, column c V + p"""
    B, V, Cc = x.shape
    return _exact(out=_edge(x.detach().to("cpu").to(F32).permute(0, 2, 1).contiguous(), drop, (1, 2)).reshape(B, Cc * V))


def flatten_bwd(dout, mask, V, Cc, dd=F32, drop=None):
    """dout [B][C V] fp32, mask [B][V][C] or None -> dx [B][V][C] in dd: dout where the mask is > 0 (-0.0, 0 and negatives: zero), else +0"""
    g = dout.detach().to("cpu", F32).reshape(-1, Cc, V).permute(0, 2, 1).contiguous()
    if mask is not None:
        g = torch.where(mask.detach().to("cpu").float() > 0, g, torch.zeros_like(g))
    return _exact(dx=_edge(move(g, dd, drop), drop, (1, 2)))


def clamp_fwd(x, lo, hi):
    return _exact(y=torch.clamp(x.detach().to("cpu", F32), f32(lo), f32(hi)))


def clamp_bwd(x, g, lo, hi):
    x, g = x.detach().to("cpu", F32), g.detach().to("cpu", F32)
    return _exact(dx=torch.where((x >= f32(lo)) & (x <= f32(hi)), g, torch.zeros_like(g)))


def specials():
    """fp32 values a conversion or a clamp goes wrong on: +-0, +-inf, NaN, denormals, exact bf16 ties (both parities), the largest finite (rounds to inf)"""
    t = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -133 + 2.0 ** -141,
         1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23,
         2.0 - 2.0 ** -8, 2.0 - 2.0 ** -9, 3.3895313892515355e38, 3.4028234663852886e38, -3.4028234663852886e38, 1.0, -1.0, 0.5, -0.25, 0.75]
    return torch.tensor(t, dtype=F64).to(F32)


# ------------------------------------------------------------------------------------------------ activations
def _act(pre, e_pre, act):
    """act(pre) and its bound (dense64._act, with the kernel's v > 0 ? v : 0 for the ReLU: -0.0 becomes +0)"""
    if act == RELU:
        return torch.where(pre > 0, pre, torch.zeros_like(pre)), e_pre
    return d64._act(pre, e_pre, act)


def act_fwd(x, act, out_bf16=False, dtype=F64):
    x = _t(x, dtype)
    y, e = _act(x, torch.zeros_like(x), act)
    return _out(dict(y=y), dict(y=bf16_out(e, y) if out_bf16 else e))


def act_bwd(dy, y, act, out_bf16=False, dtype=F64):
    dy, y = _t(dy, dtype), _t(y, dtype)
    f, r = d64._act_grad(y, act)
    g = dy if f is None else dy * f
    e = r * U * g.abs()
    return _out(dict(dx=g), dict(dx=bf16_out(e, g) if out_bf16 else e))


# ------------------------------------------------------------------------------------------------ channel sum
def channel_sum(x, dtype=F64, drop=None):
    """x [P][C] -> out [C]"""
    x = _t(x, dtype)
    P = x.shape[0]
    s = (x[:-1] if _chk(drop) == "last_row" else x).sum(0)
    return _out(dict(out=s), dict(out=_ps(P) * x.abs().sum(0)))


# ------------------------------------------------------------------------------------------------ adaptive average pool
def windows(I, O):
    """[(lo, hi)] of the O adaptive windows over I inputs"""
    return [((o * I) // O, -((-(o + 1) * I) // O)) for o in range(O)]


def _pool_mat(I, O, dtype, pm1=False):
    """M [O][I] of 0 / 1: window o contains input i (pm1: and o lies within 1 of floor(i O / I)); sizes [O]"""
    M = torch.zeros(O, I, dtype=dtype)
    for o, (lo, hi) in enumerate(windows(I, O)):
        M[o, lo:hi] = 1.0
    size = M.sum(1)
    if pm1:
        for i in range(I):
            c = (i * O) // I
            M[:max(c - 1, 0), i] = 0.0
            M[c + 2:, i] = 0.0
    return M, size


def _apply3(x, Md, Mh, Mw):
    """x [B][D][H][W][C] -> [B][C][OD][OH][OW] through [O][I] matrices, width first"""
    x = torch.einsum("fw,bdhwc->bdhfc", Mw, x)
    x = torch.einsum("eh,bdhfc->bdefc", Mh, x)
    return torch.einsum("ad,bdefc->bcaef", Md, x)


def _apply3_t(g, Md, Mh, Mw):
    """g [B][C][OD][OH][OW] -> [B][D][H][W][C] through the transposes"""
    g = torch.einsum("fw,bcaef->bcaew", Mw, g)
    g = torch.einsum("eh,bcaew->bcahw", Mh, g)
    return torch.einsum("ad,bcahw->bdhwc", Md, g)


def pool_fwd(x, out, dtype=F64, drop=None):
    """x [B][D][H][W][C], out = (OD, OH, OW) -> out [B][C OD OH OW]"""
    x = _t(x, dtype)
    B, D, H, W, Cc = x.shape
    mats = [_pool_mat(I, O, dtype) for I, O in zip((D, H, W), out)]
    T = torch.einsum("a,e,f->aef", *[m[1] for m in mats])
    div = T
    if _chk(drop) == "unclipped_div":
        div = torch.full_like(T, (D / out[0]) * (H / out[1]) * (W / out[2]))
    s = _apply3(x, *[m[0] for m in mats])
    mag = _apply3(x.abs(), *[m[0] for m in mats])
    r = s / div
    e = C * torch.sqrt(T) * U * mag / T + _u("div") * r.abs()
    return _out(dict(out=r.reshape(B, -1)), dict(out=e.reshape(B, -1)))


def pool_bwd(dout, mask, dims, out, out_bf16=False, dtype=F64, drop=None):
    """dout [B][C OV], mask [B][D][H][W][C] or None (the ReLU output x: the gradient passes where x > 0), dims = (D, H, W) -> dx [B][D][H][W][C]"""
    dout = _t(dout, dtype)
    B = dout.shape[0]
    pm1 = _chk(drop) == "pm1"
    full = [_pool_mat(I, O, dtype) for I, O in zip(dims, out)]
    mats = [_pool_mat(I, O, dtype, pm1)[0] for I, O in zip(dims, out)]
    T = torch.einsum("a,e,f->aef", *[m[1] for m in full])
    q = dout.reshape(B, -1, *out) / T
    dx = _apply3_t(q, *mats)
    mag = _apply3_t(q.abs(), *mats)
    n = _apply3_t(torch.ones(1, 1, *out, dtype=dtype), *[m[0] for m in full])        # windows containing the voxel
    e = (C * torch.sqrt(n) * U + _u("div")) * mag
    if mask is not None:
        keep = _t(mask, dtype) > 0
        dx, e = torch.where(keep, dx, torch.zeros_like(dx)), torch.where(keep, e, torch.zeros_like(e))
    return _out(dict(dx=dx), dict(dx=bf16_out(e, dx) if out_bf16 else e))


def pool_bwd_sequential_f32(dout, dims, out):
    """avgpool_bwd_kernel's own arithmetic in fp32, without a mask: every voxel adds dout / T (a correctly rounded fp32 division) over its windows in ascending
    (od, oh, ow) order.  Where every O <= I the candidates floor(i O / I) - 1 .. + 1 the kernel used to try are exactly these windows in this order
    (tests/test_plumbing_reference_cpu.py), so this is what the kernel gave there before its window range was made exact: the bits that must not change."""
    dout = dout.detach().to("cpu", F32)
    B = dout.shape[0]
    g = dout.reshape(B, -1, *out)
    dx = torch.zeros(B, *dims, g.shape[1], dtype=F32)
    wd, wh, ww = (windows(I, O) for I, O in zip(dims, out))
    for a, (d0, d1) in enumerate(wd):
        for e, (h0, h1) in enumerate(wh):
            for f, (w0, w1) in enumerate(ww):
                T = torch.tensor(float((d1 - d0) * (h1 - h0) * (w1 - w0)), dtype=F32)
                dx[:, d0:d1, h0:h1, w0:w1, :] += (g[:, :, a, e, f] / T)[:, None, None, None, :]
    return dx


# ------------------------------------------------------------------------------------------------ linear resize
def taps(n_in, n_out, dtype=F64, drop=None, shift=0.0):
    """A [out][in] the tap weights, dA [out][in] their derivative by the tap position, eps_s [out] how far the kernel's position may lie from the float64 one,
    dA2 [out][in] the derivative on the NEIGHBOURING segment for the rows whose position lies within 4 eps_s of an integer (None: no such row).
    shift (self-tests only): every position moved by shift * eps_s, which is what the bound's tap term has to cover, index flips included."""
    mode = _chk(drop)
    scale = torch.tensor(float(n_in), dtype=F32) / torch.tensor(float(n_out), dtype=F32)           # the kernel's fp32 quotient
    o = torch.arange(n_out, dtype=dtype)
    p = scale.to(dtype) * (o + 0.5)
    s = p - 0.5
    eps_s = (U * (p.abs() + s.abs())).to(dtype)
    if mode == "align_corners":
        s = o * (n_in - 1) / max(n_out - 1, 1)
    s = (s + shift * eps_s).clamp_min(0.0)
    i0 = torch.floor(s).to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    w1 = s - i0.to(dtype)
    w0 = 1.0 - w1
    if mode == "swap_taps":
        w0, w1 = w1, w0
    rows = torch.arange(n_out)
    A, dA = torch.zeros(n_out, n_in, dtype=dtype), torch.zeros(n_out, n_in, dtype=dtype)
    A.index_put_((rows, i0), w0, accumulate=True)
    A.index_put_((rows, i1), w1, accumulate=True)
    one = torch.ones_like(w0)
    dA.index_put_((rows, i0), -one, accumulate=True)
    dA.index_put_((rows, i1), one, accumulate=True)
    # a position within rounding of an integer k: the kernel may sit on the other side of it, on the segment [k - 1, k] (s >= k) or [k, k + 1] (s < k)
    k = torch.round(s).to(torch.int64)
    near = ((s - k.to(dtype)).abs() < 4 * eps_s) & (k >= 1) & (k <= n_in - 1)
    dA2 = None
    if bool(near.any()):
        above = s >= k.to(dtype)
        lo = torch.where(above, k - 1, k).clamp(0, n_in - 1)
        hi = torch.where(above, k, k + 1).clamp(0, n_in - 1)
        dA2 = torch.zeros(n_out, n_in, dtype=dtype)
        dA2.index_put_((rows[near], lo[near]), -one[near], accumulate=True)
        dA2.index_put_((rows[near], hi[near]), one[near], accumulate=True)
    return A, dA, eps_s, dA2


def _bcast(v, axis):
    """v [O] shaped to broadcast over [B][C][OD][OH][OW] along output axis 0 / 1 / 2"""
    return v.reshape([-1 if a == axis else 1 for a in range(3)])


def resize_fwd(src, out, dtype=F64, drop=None, shift=0.0):
    """src [B][d][h][w][C] (fp32 values; bf16-rounded for a bf16 source), out = (D, H, W) -> dst [B][D][H][W][C] fp32"""
    src = _t(src, dtype)
    tp = [taps(i, o, dtype, drop, shift) for i, o in zip(src.shape[1:4], out)]
    A = [t[0] for t in tp]
    v = _apply3(src, *A)
    e = NEST * U * _apply3(src.abs(), *[a.abs() for a in A])
    for ax in range(3):
        slope = _apply3(src, *[tp[k][1] if k == ax else A[k] for k in range(3)]).abs()
        if tp[ax][3] is not None:                                 # the steeper of the two segments that meet at the integer
            slope = torch.maximum(slope, _apply3(src, *[tp[k][3] if k == ax else A[k] for k in range(3)]).abs())
        e = e + _bcast(tp[ax][2], ax) * slope
    return _out(dict(dst=v.permute(0, 2, 3, 4, 1)), dict(dst=e.permute(0, 2, 3, 4, 1)))


def resize_bwd(ddst, dims, out_bf16=False, dtype=F64, drop=None, shift=0.0):
    """ddst [B][D][H][W][C] fp32, dims = (d, h, w) of the source -> dsrc [B][d][h][w][C]"""
    g = _t(ddst, dtype).permute(0, 4, 1, 2, 3)
    out = g.shape[2:]
    tp = [taps(i, o, dtype, drop, shift) for i, o in zip(dims, out)]
    A = [t[0] for t in tp]
    absA = [a.abs() for a in A]
    v = _apply3_t(g, *A)
    mag = _apply3_t(g.abs(), *absA)
    n = _apply3_t(torch.ones(1, 1, *out, dtype=dtype), *[(a != 0).to(dtype) for a in A])
    e = (C * torch.sqrt(n) + NEST) * U * mag
    for ax in range(3):
        dmat = tp[ax][1].abs() + (0.0 if tp[ax][3] is None else tp[ax][3].abs())      # both segments' entries
        mats = [tp[k][2][:, None] * dmat if k == ax else absA[k] for k in range(3)]
        e = e + _apply3_t(g.abs(), *mats)
    return _out(dict(dsrc=v), dict(dsrc=bf16_out(e, v) if out_bf16 else e))


# ------------------------------------------------------------------------------------------------ k3 <-> k4
A43 = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 0.0], [1.0, 0.0, 0.0]], dtype=F64)


def conv3_to_k4(w3, dtype=F64):
    """w3 [Cout][Cin][3][3] -> k4 [Cin][Cout][4][4] = A W3 A^T"""
    w3, A = _t(w3, dtype), A43.to(dtype)
    return _out(dict(k4=torch.einsum("ka,oiab,lb->iokl", A, w3, A)), dict(k4=_ps(4) * torch.einsum("ka,oiab,lb->iokl", A, w3.abs(), A)))


def k4_to_conv3_grad(dk4, dtype=F64):
    """dk4 [Cin][Cout][4][4] -> dw3 [Cout][Cin][3][3] = A^T dK4 A"""
    g, A = _t(dk4, dtype), A43.to(dtype)
    return _out(dict(dw3=torch.einsum("ka,iokl,lb->oiab", A, g, A)), dict(dw3=_ps(4) * torch.einsum("ka,iokl,lb->oiab", A, g.abs(), A)))


# ------------------------------------------------------------------------------------------------ BatchNorm2d, channels-last [P][C]
def bn2d_fwd(x, gamma, beta, rm, rv, momentum, eps, training, act, mean=None, rstd=None, out_bf16=False, dtype=F64, drop=None):
    """training: y, mean, rstd (and running_mean / running_var where rm / rv are given); else mean / rstd are inputs and y the only output"""
    mode = _chk(drop)
    x, gamma, beta, rm, rv, mean, rstd = (_t(v, dtype) for v in (x, gamma, beta, rm, rv, mean, rstd))
    P = x.shape[0]
    mom, eps = f32(momentum), f32(eps)
    ref, err = {}, {}
    if training:
        mean = x.sum(0) / P
        e_mean = _ps(P) * x.abs().sum(0) / P + (_u("div") + U) * mean.abs()          # the sum, 1.f / P, the product
        dev = x - mean
        e_dev = e_mean + U * dev.abs()
        q = (dev * dev).sum(0)
        e_q = (2 * dev.abs() * e_dev + e_dev * e_dev).sum(0) + (_ps(P) + 3 * U) * q
        var = q / P
        if mode == "one_pass_var":
            var = (x * x).sum(0) / P - mean * mean
            q = var * P
        e_var = e_q / P + _u("div") * var.abs()
        rstd = 1.0 / torch.sqrt(var + eps)
        e_rstd = rstd * ((e_var + U * (var + eps)) / (2 * (var + eps)) + _u("sqrtf") + _u("div"))
        ref.update(mean=mean, rstd=rstd)
        err.update(mean=e_mean, rstd=e_rstd)
        if rm is not None:
            uv = var if mode == "biased_running_var" else var * (P / (P - 1.0))
            ref["running_mean"] = (1.0 - mom) * rm + mom * mean
            err["running_mean"] = mom * e_mean + 4 * U * (rm.abs() + mom * mean.abs())
            ref["running_var"] = (1.0 - mom) * rv + mom * uv
            err["running_var"] = mom * (e_var * P / (P - 1.0) + (_u("div") + 2 * U) * uv.abs()) + 4 * U * (rv.abs() + mom * uv.abs())
    else:
        dev = x - mean
        e_dev, e_rstd = U * dev.abs(), torch.zeros_like(rstd)
    xh = dev * rstd
    e_xh = e_dev * rstd + dev.abs() * e_rstd + U * xh.abs()
    pre = xh * gamma + beta
    e_pre = gamma.abs() * e_xh + 2 * U * ((xh * gamma).abs() + beta.abs())
    y, e_y = _act(pre, e_pre, act)
    ref["y"], err["y"] = y, (bf16_out(e_y, y) if out_bf16 else e_y)
    return _out(ref, err)


def bn2d_bwd(x, dy, y, gamma, mean, rstd, act, out_bf16=False, dtype=F64, drop=None):
    """x, dy, y [P][C]; gamma, mean, rstd [C], all inputs of the call -> dx, dgamma, dbeta"""
    mode = _chk(drop)
    x, dy, y, gamma, mean, rstd = (_t(v, dtype) for v in (x, dy, y, gamma, mean, rstd))
    P = x.shape[0]
    f, r = d64._act_grad(y, act)
    g = dy if f is None else dy * f
    e_g = r * U * g.abs()
    xh = (x - mean) * rstd
    e_xh = 2 * U * xh.abs()
    db = g.sum(0)
    e_db = _ps(P) * g.abs().sum(0) + e_g.sum(0)
    t = g * xh
    dg = t.sum(0)
    e_dg = _ps(P) * t.abs().sum(0) + ((3 + r) * U * t.abs()).sum(0)
    xdg = torch.zeros_like(xh) if mode == "dx_no_dgamma" else xh * dg
    inner = P * g - db - xdg
    mag = P * g.abs() + db.abs() + (xh * dg).abs()
    e_inner = P * e_g + e_db + xh.abs() * e_dg + e_xh * dg.abs() + 3 * U * mag
    coef = gamma * rstd / P
    dx = coef * inner
    e_dx = coef.abs() * e_inner + (_u("div") + 2 * U) * dx.abs()
    return _out(dict(dx=dx, dgamma=dg, dbeta=db), dict(dx=bf16_out(e_dx, dx) if out_bf16 else e_dx, dgamma=e_dg, dbeta=e_db))


# ------------------------------------------------------------------------------------------------ operands
def operands(kind, seed, *shape, lo=-2, hi=2):
    """a tensor of `shape`.  'random': standard Gaussian.  'structured': small integers f(seed, flat index) in [lo, hi], distinct enough along every axis that a
    swapped, repeated or dropped index shows, every sum of them exact in fp32 and every one exact in bf16."""
    n = int(math.prod(shape)) if shape else 1
    if kind == "structured":
        i = torch.arange(n, dtype=torch.int64)
        v = (i * (7 + 2 * seed) + (i // 13) * 5 + (i // 64) * 3 + (i // 257) * 11 + (i * i) % 17 + seed) % (hi - lo + 1) + lo
        return v.to(F32).reshape(shape)
    return torch.randn(n, generator=gen(seed * 7919 + n * 31 + len(shape))).reshape(shape)


def act_input(kind, seed, n):
    """act_fwd's x: 'random': Gaussian scaled by 2 (inside the sigmoid's measured range) with 0 and -0.0 among them; 'structured': integers in [-3, 3] and a -0.0"""
    v = operands(kind, seed, n, lo=-3, hi=3) if kind == "structured" else (2.0 * operands(kind, seed, n)).clamp(-SIG_RANGE, SIG_RANGE)
    if n > 2:
        v[n // 2], v[n - 1] = 0.0, -0.0
    else:
        v[0] = -0.0
    return v


def act_output(kind, seed, n, act):
    """a saved activation OUTPUT (dense64.act_output), with an exact 0 and a -0.0 where the activation has a branch"""
    v = d64.act_output(kind, seed, 1, n, act)
    if v is None:
        return None
    v = v.reshape(-1).clone()
    if act != SIGMOID and not (kind == "structured" and act != RELU) and n > 2:
        v[n // 3], v[n - 2] = 0.0, -0.0
    return v


def bn_case(kind, seed, P, Cc, bf=False):
    """x [P][C] with channel 1 of mean 50 and std 0.1 and channel 2 constant (random kind), gamma in +-[0.5, 1.2], beta in [-0.5, 0.5] (a sigmoid argument stays
    inside 8), running statistics, dy, and a saved output y per activation code.  bf: x and dy rounded to bf16."""
    g = gen(seed * 104729 + P * 13 + Cc)
    x = operands(kind, seed, P, Cc)
    if kind == "random":
        x[:, 1] = 50.0 + 0.1 * x[:, 1]
        x[:, 2] = 3.25
    sign = torch.where(torch.rand(Cc, generator=g) < 0.5, -1.0, 1.0)
    c = dict(x=x, dy=operands(kind, seed + 1, P, Cc), gamma=sign * (0.5 + 0.7 * torch.rand(Cc, generator=g)), beta=torch.rand(Cc, generator=g) - 0.5,
             rm=torch.randn(Cc, generator=g), rv=0.5 + torch.rand(Cc, generator=g))
    if bf:
        c["x"], c["dy"] = bf16(c["x"]), bf16(c["dy"])
    return c


# ------------------------------------------------------------------------------------------------ the launch geometry of both files, replayed
def _cdiv(a, b):
    return (a + b - 1) // b


def grid_1d(n, block=256, cap=2048):
    """cvae_grid_1d (common.h)"""
    return max(1, min(_cdiv(n, block), cap))


def channel_sum_geometry(P, Cc, bf=False, aligned=True):
    """channel_sum_gx / channel_sum_launch: dict(path 'vec' | 'scalar', fold, gx (row blocks with scratch), gy, rows, groups, ws_floats (what gx > 1 asks for))"""
    VEC = 8 if bf else 4
    Pv, Cv, fold = P, Cc, 0
    if Cc == 1 and P % VEC == 0 and P >= VEC:
        Pv, Cv, fold = P // VEC, VEC, 1
    if Cv % VEC == 0 and aligned:
        groups = Cv // VEC
        gpb = min(groups, 256)
        rows, gy = 256 // gpb, _cdiv(groups, gpb)
        passes, gx = _cdiv(Pv, rows), 1
        if passes > 64:
            gx = min(_cdiv(passes, 32), _cdiv(1024, gy))
        path = "vec"
    else:
        cl = min(Cc, 256)
        rows, gy, groups = 256 // cl, _cdiv(Cc, cl), 0
        gx = max(1, min(_cdiv(P, rows * 64), _cdiv(2048, gy)))
        path, fold = "scalar", 0
    row = 1 if fold else Cc
    return dict(path=path, fold=fold, gx=gx, gy=gy, rows=rows, groups=groups, ws_floats=gx * row if gx > 1 else 0)


def bn2d_blocks(P, Cc):
    """(row blocks gb, rows per pass R) of bn2d_reduce_kernel"""
    lanes = Cc // 8
    R = 256 // lanes
    return max(1, min(_cdiv(P, R * 16), 1024)), R


def bn2d_workspace_floats(P, Cc, backward):
    return (2 if backward else 1) * bn2d_blocks(P, Cc)[0] * Cc


# ------------------------------------------------------------------------------------------------ the shapes both test files walk
N_ELEMENTWISE = [1, 257, 524288 + 5]                             # one thread; a second block's tail; past the 2048 x 256 grid cap: a second grid-stride trip
TRANSPOSE_C = [1, 2, 63, 64, 65, 130]                            # the cast shortcut; a tile's corner; one below / at / one past the 64 tile; three tiles
TRANSPOSE_S = [1, 63, 64, 65, 200]
TRANSPOSE_B = [1, 3]
FLATTEN_V = [1, 49, 64, 65, 130]
FLATTEN_C = [1, 63, 64, 65, 70]
# (P, C, bf16, offset elements, what it crosses)
CHANNEL_SUM = [
    (340, 12, False, 0, "vec: 3 groups, 85 rows (an idle thread, a non-power-of-two tree); 4-deep loop, remainder 0"),
    (428, 12, False, 0, "vec: remainders 1 and 2"),
    (600, 12, False, 0, "vec: remainders 0 and 3"),
    (7000, 12, False, 0, "vec: 83 passes: gx = 3 row blocks and the finish pass"),
    (204, 40, True, 0, "vec bf16: 5 groups, 51 rows; remainder 0"),
    (260, 40, True, 0, "vec bf16: remainders 1 and 2"),
    (359, 40, True, 0, "vec bf16: remainders 0 and 3"),
    (9, 1024, False, 0, "vec: 256 groups, one row per pass"),
    (70, 1024, False, 0, "vec: 70 passes: gx = 3"),
    (9, 1028, False, 0, "vec: a second blockIdx.y holding one group"),
    (16385, 1028, False, 0, "vec: 257 groups, gx at its 1024 / gy cap (512): 67 MB, the one large buffer of the family"),
    (4096, 1, False, 0, "fold: C = 1, P a multiple of 4"),
    (66560, 1, False, 0, "fold: 65 passes, gx = 3, scratch rows of one float"),
    (16, 1, True, 0, "fold bf16"),
    (1001, 1, False, 0, "scalar, cl = 1: P no multiple of 4"),
    (1, 19, False, 0, "scalar: P = 1"),
    (50, 19, False, 0, "scalar: 13 rows, P below 8 strides (the clamped 8-deep loop)"),
    (2000, 19, False, 0, "scalar: gx = 3"),
    (130, 257, False, 0, "scalar: two column blocks, gx = 3"),
    (300, 64, False, 1, "scalar with C % 4 == 0: x offset by one element (4-byte aligned only)"),
    (300, 64, True, 1, "scalar bf16 with C % 8 == 0: x offset by one element (2-byte aligned only)"),
]
# (B, (D, H, W), C, (OD, OH, OW), what it crosses); 2D cases as D = OD = 1
POOL = [
    (2, (1, 8, 8), 5, (1, 4, 4), "divisible"),
    (2, (5, 6, 9), 3, (4, 4, 4), "overlapping windows, three different ratios"),
    (3, (1, 7, 7), 4, (1, 3, 3), "overlapping windows of 3"),
    (2, (1, 3, 3), 4, (1, 4, 4), "output larger than input"),
    (2, (1, 2, 2), 3, (1, 7, 7), "2 -> 7: up to four windows contain a voxel"),
    (2, (1, 1, 1), 3, (1, 3, 3), "1 -> 3: every window contains the one voxel"),
    (1, (2, 2, 1), 2, (5, 5, 4), "2 -> 5 and 1 -> 4 in 3D"),
    (2, (1, 66, 66), 64, (1, 65, 65), "B OV C = 540 800 > 524 288: the second grid-stride trip of both kernels"),
]
POOL_LEGACY_COMPLETE = [s for s in POOL if all(o <= i for i, o in zip(s[1], s[3]))]       # O <= I: the former candidate rule was complete
# (B, (d, h, w), C, (D, H, W), what it crosses): the generic kernels
RESIZE = [
    (2, (1, 16, 16), 3, (1, 9, 11), "downscale, two ratios"),
    (1, (1, 16, 16), 3, (1, 3, 3), "16 -> 3: taps skip sources"),
    (2, (1, 8, 8), 3, (1, 8, 8), "identity"),
    (2, (1, 1, 1), 3, (1, 5, 5), "1 -> 5: both taps are the one source"),
    (2, (1, 5, 5), 3, (1, 1, 1), "5 -> 1"),
    (1, (3, 5, 4), 3, (8, 6, 9), "3D, three different ratios"),
    (2, (1, 4, 3), 1, (1, 8, 6), "exact 2x with W % 4 != 0: the generic path"),
    (2, (1, 3, 30), 3, (1, 7, 42), "3 -> 7, 30 -> 42: tap positions within rounding of an integer (s = 1 at o = 3, inexact fp32 scale): the tap index may flip"),
    (1, (1, 210, 210), 3, (1, 420, 420), "B D H W C = 529 200 > 524 288: the second grid-stride trip of the forward (2x with C = 3: generic)"),
    (1, (1, 420, 420), 3, (1, 210, 210), "B d h w C = 529 200: the second grid-stride trip of the backward"),
]
# C = 1, the exact-2x kernels
RESIZE_2X = [
    (1, (1, 1, 2), (1, 2, 4), "the smallest: d = 1 -> 1 (2D form), h = 1 -> 2"),
    (2, (1, 1, 2), (2, 2, 4), "d = 1 -> 2, h = 1 -> 2"),
    (2, (1, 5, 6), (1, 10, 12), "2D form D = d = 1"),
    (2, (3, 5, 6), (6, 10, 12), "3D"),
]
RESIZE_2X_BIG_FWD = (1, (64, 128, 130), (128, 256, 260))        # 2 129 920 output quads > 8192 x 256 (34 MB of fp32 out)
RESIZE_2X_BIG_BWD = (1, (64, 128, 258), (128, 256, 516))        # 2 113 536 source voxels > 8192 x 256 (67.6 MB of fp32 gradient)
K34 = [(1, 1), (3, 5), (17, 16), (32, 64)]                       # (Cout, Cin); 17 x 16 = 272 pairs: a block tail
BN_C = [8, 24, 40, 264, 2048]                                    # one lane; an idle tail thread (85 / 51 row groups); C > 256: the per-channel loop's second trip; the limit


def bn_P(Cc):
    """P = 2, 3, one below R, 16 R + 1 (two scratch rows)"""
    R = bn2d_blocks(1, Cc)[1]
    return sorted({2, 3, 16 * R + 1} | ({R - 1} if R - 1 >= 2 else set()))


BN_CAP = (16385, 2048)                                           # bf16: 1025 row blocks wanted, the scratch's 1024-row cap (67 MB)
