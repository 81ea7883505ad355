"""Float64 reference of csrc/bn2d_batch.hip (cvae_bn2d_batch_fwd) and of cvae_bn2d_bwd behind it, with element-wise bounds derived from the sums the kernels
issue — the yardstick of tests/test_bn2d_batch*.py and of the running statistics in tests/test_vit_stem_batchnorm.py.  Own code, plain torch on the CPU.

The rules are oracle/loss64.py's (U = 2^-24, C = 4): a fixed-order fp32 sum of K terms lies within C sqrt(K) U sum |term| of the exact sum, one fp32 operation
within U |result|, an elementary function within its measured ulps (loss64.ULP), and a value stored in bf16 within half a bf16 ulp (2^-8 relative, fused64's
constant) of what was rounded.  All references are float64 functions of the STORED values (bf16 inputs are exact inputs).

forward(y, gamma, beta, rm, rv, momentum, eps, slope, bf16) -> (ref, err) for mean, rstd, var, a, v (the pre-activation), running_mean, running_var.
What the kernel computes (csrc/bn2d_batch.hip): the rows are cut into chunks of chunk_rows(P); per chunk g with shift K_g = its first row and d = y - K_g,
    s1 = sum d, s2 = sum d^2, mean_g = K_g + s1 / n_g, M2_g = s2 - s1 (s1 / n_g);
the chunks are merged pairwise in index order (n = na + nb, dm = mb - ma, f = nb / n, ma += dm f, M2a += M2b + dm^2 na f); var = M2 / P,
rstd = 1 / sqrt(var + eps), a = act((y - mean) (rstd gamma) + beta), running = (1 - m) running + m (mean | var P / (P - 1)).
The bounds, per channel (ps(K) = C sqrt(K) U):
    e(mean_g)  = (ps(n_g) + U) sum |d| / n_g + 2 U |s1 / n_g| + U |mean_g|                        d: one rounding each; the division; the addition
    e(M2_g)    = (ps(n_g) + 3 U) sum d^2 + 2 |s1 / n_g| (ps(n_g) + U) sum |d| + 4 U s1^2 / n_g + U M2_g
    e(mean)    = max_g e(mean_g) + ps(G) (3 D + max_g |mean_g|)                                  D = the spread of the chunk means: |dm| <= D + errors
    e(M2)      = sum_g e(M2_g) + 4 (D + e(mean)) e(mean) P + ps(G) 6 M2                           dm carries both means' errors; five roundings per merge
    e(var)     = e(M2) / P + U var;      e(rstd) = rstd ((e(var) + U (var + eps)) / (2 (var + eps)) + u(sqrtf) + u(div))
    e(v)       = (e(mean) + U |y - mean|) |k| + |y - mean| (|gamma| e(rstd) + U |k|) + U |t| + U |v|,  k = rstd gamma, t = (y - mean) k, v = t + beta
    e(a)       = e(v) + U |a| (+ 2^-8 (|a| + e(v)) stored in bf16): LeakyReLU has Lipschitz constant 1, an undecided sign costs no more than e(v)
    running_*  as loss64.bn1d.
A merge sees at most G = parts(P) values, so ps(G) covers the sequential runs of the finish kernel whichever way they are grouped.

backward(y, dy, mask, gamma, mean, rstd, e_mean, e_rstd, slope, bf16) -> (ref, err) for dx, dgamma, dbeta of cvae_bn2d_bwd given the forward's statistics:
g = dy * (mask ? 1 : slope), dbeta = sum g, dgamma = sum g xh, xh = (y - mean) rstd, dx = gamma rstd / P (P g - dbeta - xh dgamma); the reference is what float64
autograd gives for a = where(mask, v, slope v) (asserted in the CPU test), the bound loss64.bn1d's for its dx / dw / db with the statistics' errors as inputs.

emulate_fp32(y, ...) evaluates the kernel's formulas in fp32 on the CPU (torch's own summation order inside a chunk): the stand-in for a correct kernel with
which the CPU test shows that the bounds hold, and naive_var_fp32 is the E[y^2] - E[y]^2 formula that they must refuse on the cancellation input."""
import math

import torch

from oracle.loss64 import C, U, _ps, _u  # noqa: F401

F64, F32 = torch.float64, torch.float32
BF16_HALF_ULP = 2.0 ** -8
ROWS, MAX_PARTS = 256, 1024                     # BNB_ROWS, BNB_MAX_PARTS of csrc/bn2d_batch.hip


def chunk_rows(P):
    return ROWS * ((P + ROWS * MAX_PARTS - 1) // (ROWS * MAX_PARTS))


def parts(P):
    return (P + chunk_rows(P) - 1) // chunk_rows(P)


def f32(v):
    return float(torch.tensor(float(v), dtype=F32))


def leaky(v, slope, mask=None):
    return torch.where(v > 0 if mask is None else mask, v, slope * v)


def inputs(P, Cc, seed, bf16, cancel=False):
    """y [P, Cc] in its stored dtype with per-channel scales 0.1 .. 3 and offsets of a few standard deviations (cancel: 1000 + 0.01 N(0, 1), fp32), the affine
    pair, running statistics and a cotangent"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    if cancel:
        y = 1000.0 + 0.01 * r(P, Cc)
    else:
        y = r(P, Cc) * (0.1 + 2.9 * torch.rand(Cc, generator=g)) + 2.0 * r(Cc)
    y = y.to(torch.bfloat16 if bf16 else F32)
    dy = r(P, Cc).to(y.dtype)
    return dict(y=y, dy=dy, gamma=0.5 + torch.rand(Cc, generator=g), beta=0.1 * r(Cc), rm=0.1 * r(Cc), rv=0.5 + torch.rand(Cc, generator=g))


def moments(y):
    """float64 (mean, M2, e_mean, e_M2) of the stored y [P, C] with the bounds of the chunked, shifted, merged evaluation"""
    y = y.to(F64)
    P = y.shape[0]
    ch, G = chunk_rows(P), parts(P)
    mean, M2 = y.mean(0), ((y - y.mean(0)) ** 2).sum(0)
    e_mg, e_M2g, mg = [], [], []
    for g in range(G):
        blk = y[g * ch:(g + 1) * ch]
        n = blk.shape[0]
        d = blk - blk[0]
        s1, a1, a2 = d.sum(0), d.abs().sum(0), (d * d).sum(0)
        m1 = s1 / n
        ps = _ps(n)
        mg.append(blk[0] + m1)
        e_mg.append((ps + U) * a1 / n + 2 * U * m1.abs() + U * mg[-1].abs())
        e_M2g.append((ps + 3 * U) * a2 + 2 * m1.abs() * (ps + U) * a1 + 4 * U * s1 * m1 + U * (a2 - s1 * m1).abs())
    mg, e_mg, e_M2g = torch.stack(mg), torch.stack(e_mg), torch.stack(e_M2g)
    D = mg.max(0).values - mg.min(0).values
    e_mean = e_mg.max(0).values + (_ps(G) * (3 * D + mg.abs().max(0).values) if G > 1 else 0.0)
    e_M2 = e_M2g.sum(0) + ((4 * (D + e_mean) * e_mean * P + _ps(G) * 6 * M2) if G > 1 else 0.0)
    return mean, M2, e_mean, e_M2


def forward(y, gamma, beta, rm, rv, momentum, eps, slope=0.01, bf16=False):
    P = y.shape[0]
    yd, gamma, beta = y.to(F64), gamma.to(F64), beta.to(F64)
    mom, eps, slope = f32(momentum), f32(eps), f32(slope)
    mean, M2, e_mean, e_M2 = moments(y)
    var = M2 / P
    e_var = e_M2 / P + U * var
    rstd = 1.0 / torch.sqrt(var + eps)
    e_rstd = rstd * ((e_var + U * (var + eps)) / (2 * (var + eps)) + _u("sqrtf") + _u("div"))
    dev, k = yd - mean, rstd * gamma
    t = dev * k
    v = t + beta
    e_v = (e_mean + U * dev.abs()) * k.abs() + dev.abs() * (gamma.abs() * e_rstd + U * k.abs()) + U * t.abs() + U * v.abs()
    a = leaky(v, slope)
    e_a = e_v + U * a.abs()
    if bf16:
        e_a = e_a + BF16_HALF_ULP * (a.abs() + e_v)
    ref = dict(mean=mean, rstd=rstd, var=var, a=a, v=v)
    err = dict(mean=e_mean, rstd=e_rstd, var=e_var, a=e_a, v=e_v)
    if rm is not None:
        rm, rv = rm.to(F64), rv.to(F64)
        uv = M2 / (P - 1)
        ref["running_mean"] = (1.0 - mom) * rm + mom * mean
        err["running_mean"] = mom * e_mean + 3 * U * (rm.abs() + mom * mean.abs())
        ref["running_var"] = (1.0 - mom) * rv + mom * uv
        err["running_var"] = mom * (e_var * P / (P - 1) + 3 * U * uv) + 4 * U * (rv.abs() + mom * uv)
    return ref, err


def backward(y, dy, mask, gamma, mean, rstd, e_mean, e_rstd, slope=0.01, bf16=False):
    """mean / rstd: the statistics the kernel was GIVEN (float64 copies of the forward's outputs would make e_mean = e_rstd = 0; the tests pass the float64
    reference and its bounds, so the result is comparable with autograd)."""
    P = y.shape[0]
    yd, dyd, gamma = y.to(F64), dy.to(F64), gamma.to(F64)
    slope = f32(slope)
    g = dyd * torch.where(mask, torch.ones_like(dyd), torch.full_like(dyd, slope))
    e_g = U * g.abs()
    dev = yd - mean
    xh = dev * rstd
    e_xh = (e_mean + U * dev.abs()) * rstd + dev.abs() * e_rstd + U * xh.abs()
    mxh = xh.abs() + e_xh
    sp = 4 * U                                                      # per-workgroup partial sums added in index order
    s1, s2 = g.sum(0), (g * xh).sum(0)
    e_s1 = (_ps(P) + sp) * g.abs().sum(0) + e_g.sum(0)
    e_s2 = (_ps(P) + sp) * (g.abs() * mxh).sum(0) + (g.abs() * (e_xh + 2 * U * mxh) + e_g * mxh).sum(0)
    inner = P * g - s1 - xh * s2
    mag = P * g.abs() + s1.abs() + mxh * s2.abs()
    c = gamma * rstd / P
    dx = c * inner
    # what a whole channel shares (the statistics' and the two sums' errors) and what is each element's own (its roundings, the bf16 store)
    e_common = gamma.abs() / P * (e_rstd * inner.abs() + rstd * (e_s1 + e_xh * s2.abs() + mxh * e_s2))
    e_local = gamma.abs() / P * rstd * (P * e_g + 4 * U * mag) + 4 * U * dx.abs()
    if bf16:
        e_local = e_local + BF16_HALF_ULP * (dx.abs() + e_common + e_local)
    return dict(dx=dx, dgamma=s2, dbeta=s1), dict(dx=e_common + e_local, dgamma=e_s2, dbeta=e_s1, dx_common=e_common, dx_local=e_local)


def autograd_backward(y, dy, mask, gamma, beta, eps, slope=0.01):
    """float64 autograd of a = where(mask, v, slope v), v = batch_norm(y; gamma, beta) in training mode, with the cotangent dy"""
    yd = y.to(F64).clone().requires_grad_(True)
    gm, bt = gamma.to(F64).clone().requires_grad_(True), beta.to(F64).clone().requires_grad_(True)
    v = torch.nn.functional.batch_norm(yd, None, None, gm, bt, True, 0.0, f32(eps))
    a = torch.where(mask, v, f32(slope) * v)
    a.backward(dy.to(F64))
    return dict(dx=yd.grad, dgamma=gm.grad, dbeta=bt.grad)


def emulate_fp32(y, gamma, beta, rm, rv, momentum, eps, slope=0.01):
    """the kernel's formulas in fp32 on the CPU -> dict like forward's ref (the stored dtype's rounding of `a` included)"""
    P = y.shape[0]
    x = y.to(F32)
    ch, G = chunk_rows(P), parts(P)
    n = m = M2 = None
    for g in range(G):
        blk = x[g * ch:(g + 1) * ch]
        nb = torch.tensor(float(blk.shape[0]), dtype=F32)
        d = blk - blk[0]
        s1, s2 = d.sum(0), (d * d).sum(0)
        m1 = s1 / nb
        mb, M2b = blk[0] + m1, (s2 - s1 * m1).clamp_min(0)
        if n is None:
            n, m, M2 = nb, mb, M2b
        else:
            tot = n + nb
            dm, f = mb - m, nb / tot
            m, M2, n = m + dm * f, M2 + (M2b + dm * dm * (n * f)), tot
    fP = torch.tensor(float(P), dtype=F32)
    var = M2 / fP
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    v = (x - m) * (rstd * gamma.to(F32)) + beta.to(F32)
    a = leaky(v, torch.tensor(slope, dtype=F32)).to(y.dtype)
    mom = torch.tensor(momentum, dtype=F32)
    return dict(mean=m, rstd=rstd, var=var, a=a, running_mean=(1 - mom) * rm.to(F32) + mom * m, running_var=(1 - mom) * rv.to(F32) + mom * var * (fP / (fP - 1)))


def naive_var_fp32(y):
    """E[y^2] - E[y]^2 with fp32 sums: what the kernel must NOT compute"""
    x = y.to(F32)
    return (x * x).mean(0) - x.mean(0) ** 2


def max_ratio(got, ref, err):
    g = got.detach().to("cpu", F64).reshape(ref.shape)
    d = (g - ref).abs()
    r = torch.where(err > 0, d / err.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return float(r.max())
