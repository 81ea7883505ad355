"""Float64 reference of cvae_bn2d_batch_bwd and of cvae_bn2d_batch_fwd_res (csrc/bn2d_batch.hip) with element-wise bounds derived from the sums
the kernels issue: the yardstick of tests/test_bn2d_batch_bwd*.py and of the running statistics and conv-bias gradients in tests/test_vit_decoder_batchnorm.py.
Own code, plain torch on the CPU; it imports tests/bn2d_batch_reference.py (the forward's reference, the rules, the chunking) and changes nothing there.

The rules are that file's (oracle/loss64.py: U = 2^-24, C = 4, ps(K) = C sqrt(K) U for a fixed-order fp32 sum of K terms, one fp32 operation within U |result|,
half a bf16 ulp = 2^-8 relative per bf16 store).  All references are float64 functions of the STORED values.

What the backward computes.  g = dy act'(a) (one product; exact where the factor is 1), xh = (y - mean) rstd, t = g xh.
  sums     per chunk (chunk_rows(P) rows, one workgroup) the row groups' sequential sums, then the groups in order: ONE fixed-order sum of the chunk's n_g terms,
           e(S_g) = sum e(term) + ps(n_g) sum (|term| + e(term))
  finish   run s of ceil(G / 16) consecutive chunk sums added in index order, then the runs in order:
           e(run) = sum e(S_g) + ps(len) sum (|S_g| + e(S_g)),   e(S) = sum e(run) + ps(runs) sum (|run| + e(run))            (chunked_sum replays this)
  apply    mb = dbeta / P, mg = dgamma / P, k = gamma rstd (one rounding each), dx = k ((g - mb) - xh mg): one rounding per operation, and the errors of mean and
           rstd carried in through xh and k.  dx_common is what a channel's elements share (k, mb, mg, the statistics), dx_local each element's own roundings
           and its bf16 store (the split tests/vit_stem_bn_reference.py's conv_bias_bound uses).
forward_res: a = resid + v with v, e(v) the forward's pre-activation and its bound (bn2d_batch_reference.forward): e(a) = e(v) + U |a| (+ the bf16 store).
emulate_bwd_fp32 evaluates the kernel's formulas in fp32 on the CPU in the kernel's own sum order (row groups, groups, chunks, runs): the stand-in for a correct
kernel with which the CPU test shows that the bounds hold; its `variant` argument builds the wrong kernels the bounds must refuse."""
import torch

import bn2d_batch_reference as br
from bn2d_batch_reference import BF16_HALF_ULP, F32, F64, U, _ps, chunk_rows, f32, max_ratio, parts  # noqa: F401

SEGS = 16                                        # BNB_SEGS of csrc/bn2d_batch.hip
SLOPES = {None: None, "leaky02": 0.2, "leaky001": 0.01}


def runs(G):
    per = (G + SEGS - 1) // SEGS
    return [(s * per, min(G, (s + 1) * per)) for s in range(SEGS) if s * per < G]


def _chain(S, E):
    """exact sum and bound of adding the values S (errors E) in order"""
    tot, err = sum(S), sum(E)
    if len(S) > 1:
        err = err + _ps(len(S)) * sum(s.abs() + e for s, e in zip(S, E))
    return tot, err


def chunked_sum(t, e_t):
    """(the channel sums of t [P, C], their bound) for the kernels' chunk / run order; e_t: each term's own error"""
    P = t.shape[0]
    ch, G = chunk_rows(P), parts(P)
    S, E = [], []
    for g in range(G):
        blk, eb = t[g * ch:(g + 1) * ch], e_t[g * ch:(g + 1) * ch]
        S.append(blk.sum(0))
        E.append(eb.sum(0) + _ps(blk.shape[0]) * (blk.abs() + eb).sum(0))
    RS, RE = zip(*[_chain(S[g0:g1], E[g0:g1]) for g0, g1 in runs(G)])
    return _chain(list(RS), list(RE))


def backward(y, dy, mask, gamma, mean, rstd, e_mean, e_rstd, slope=None, bf16=False):
    """mask / slope None: no activation (g = dy).  mean / rstd: float64 statistics with the bounds of what the kernel was given."""
    P = y.shape[0]
    yd, dyd, gamma = y.to(F64), dy.to(F64), gamma.to(F64)
    if slope is None:
        g, e_g = dyd, torch.zeros_like(dyd)
    else:
        g = dyd * torch.where(mask, torch.ones_like(dyd), torch.full_like(dyd, f32(slope)))
        e_g = U * g.abs()
    dev = yd - mean
    xh = dev * rstd
    e_xh_c = e_mean * rstd + dev.abs() * e_rstd                       # shared by the channel
    e_xh_l = U * dev.abs() * rstd + U * xh.abs()                      # the element's own
    e_xh = e_xh_c + e_xh_l
    mxh, mg_ = xh.abs() + e_xh, g.abs() + e_g
    t = g * xh
    e_t = mg_ * e_xh + e_g * mxh + U * mg_ * mxh
    s1, e_s1 = chunked_sum(g, e_g)
    s2, e_s2 = chunked_sum(t, e_t)
    mb, mg = s1 / P, s2 / P
    e_mb, e_mg = e_s1 / P + U * mb.abs(), e_s2 / P + U * mg.abs()
    k = gamma * rstd
    e_k = gamma.abs() * e_rstd + U * k.abs()
    d1, q = g - mb, xh * mg
    inner = d1 - q
    dx = k * inner
    m_in = g.abs() + mb.abs() + e_mb + mxh * (mg.abs() + e_mg)        # a magnitude that covers every intermediate
    e_common = e_k * m_in + k.abs() * (e_mb + mxh * e_mg + e_xh_c * mg.abs())
    e_local = k.abs() * (e_g + e_xh_l * (mg.abs() + e_mg) + 3 * U * m_in) + U * (k.abs() + e_k) * m_in
    if bf16:
        e_local = e_local + BF16_HALF_ULP * (dx.abs() + e_common + e_local)
    return dict(dx=dx, dgamma=s2, dbeta=s1), dict(dx=e_common + e_local, dgamma=e_s2, dbeta=e_s1, dx_common=e_common, dx_local=e_local)


def autograd_backward(y, dy, mask, gamma, beta, eps, slope=None):
    """float64 autograd of a = where(mask, v, slope v) (slope None: a = v), v = batch_norm(y; gamma, beta) in training mode, with the cotangent dy"""
    yd = y.to(F64).clone().requires_grad_(True)
    gm, bt = gamma.to(F64).clone().requires_grad_(True), beta.to(F64).clone().requires_grad_(True)
    v = torch.nn.functional.batch_norm(yd, None, None, gm, bt, True, 0.0, f32(eps))
    a = v if slope is None else torch.where(mask, v, f32(slope) * v)
    a.backward(dy.to(F64))
    return dict(dx=yd.grad, dgamma=gm.grad, dbeta=bt.grad)


def forward_res(y, resid, gamma, beta, rm, rv, momentum, eps, bf16=False):
    """bn2d_batch_reference.forward without an activation, plus the residual: (ref, err) with `a` = resid + v"""
    ref, err = br.forward(y, gamma, beta, rm, rv, momentum, eps, slope=1.0, bf16=bf16)
    a = resid.to(F64) + ref["v"]
    e_a = err["v"] + U * a.abs()
    if bf16:
        e_a = e_a + BF16_HALF_ULP * (a.abs() + err["v"])
    ref["a"], err["a"] = a, e_a
    return ref, err


def _seq_sum(rows):
    """rows [n, ...] added one after the other in fp32"""
    acc = torch.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def emulate_bwd_fp32(y, dy, a, gamma, mean, rstd, slope=None, variant=None):
    """the backward's formulas in fp32, in the kernel's sum order -> dict(dx (stored dtype), dgamma, dbeta).  variant "no_dgamma": dx without its dgamma term;
    "p_minus_1": dbeta divided by P - 1 in dx (two wrong kernels)."""
    P, Cc = y.shape
    x, d, gamma, mean, rstd = y.to(F32), dy.to(F32), gamma.to(F32), mean.to(F32), rstd.to(F32)
    g = d if slope is None else d * torch.where(a.to(F32) > 0, torch.tensor(1.0), torch.tensor(slope, dtype=F32))
    xh = (x - mean) * rstd
    t = g * xh
    ch, G, R = chunk_rows(P), parts(P), 256 // (Cc // 8)
    parts1, parts2 = [], []
    for c in range(G):
        out = []
        for v in (g[c * ch:(c + 1) * ch], t[c * ch:(c + 1) * ch]):
            n = v.shape[0]
            pad = torch.cat([v, torch.zeros((-n) % R, Cc, dtype=F32)]).view(-1, R, Cc)     # row p0 + rg + i R is pad[i][rg]; adding 0 changes nothing
            out.append(_seq_sum(_seq_sum(pad)))                                           # a group's rows in order, then the groups in order
        parts1.append(out[0]), parts2.append(out[1])
    fin = lambda ps: _seq_sum([_seq_sum(ps[g0:g1]) for g0, g1 in runs(G)])
    dbeta, dgamma = fin(parts1), fin(parts2)
    fP = torch.tensor(float(P), dtype=F32)
    mb = dbeta / (fP - 1 if variant == "p_minus_1" else fP)
    mg = torch.zeros_like(dgamma) if variant == "no_dgamma" else dgamma / fP
    dx = (gamma * rstd) * ((g - mb) - xh * mg)
    return dict(dx=dx.to(y.dtype), dgamma=dgamma, dbeta=dbeta)


def emulate_res_fp32(y, resid, gamma, beta, rm, rv, momentum, eps):
    """the residual forward in fp32: bn2d_batch_reference.emulate_fp32's statistics, a = resid + ((y - mean) (rstd gamma) + beta) rounded once"""
    got = br.emulate_fp32(y, gamma, beta, rm, rv, momentum, eps, slope=1.0)
    v = (y.to(F32) - got["mean"]) * (got["rstd"] * gamma.to(F32)) + beta.to(F32)
    got["a"] = (resid.to(F32) + v).to(y.dtype)
    return got
