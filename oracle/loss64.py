"""Float64 references of csrc/losses.hip (every scalar loss, BatchNorm1d and its rank-spanning split form, fused Adam, gradient clipping) with derived
elementwise error bounds, in the style and with the constants of oracle/fused64.py (U = 2^-24, C = 4; `compare` and `max_ratio` are the same functions).

Every function returns (ref, err): dicts of float64 CPU tensors, err[k] an elementwise bound on how far an fp32 evaluation of the same sums may lie from
ref[k].  The rules:
  a sum of K terms       C sqrt(K) U sum |term| over the MAGNITUDES of the summed terms (KLD's 1 + lv - mu^2 - e^lv cancels: its four addends are the terms),
                         plus the sum of the terms' own errors
  one fp32 operation     U times the magnitude of its result
  an elementary function ULP[name] fp32 ulps of its result (one ulp: relative 2^-23 = 2 U), plus |f'| times the error of its argument
  BatchNorm              two-pass variance; the rounding of x - mean is amplified by 1 / sqrt(var + eps), as fused64.bottleneck does for its BatchNorm
  accumulate (`prefill`) the kernels add their sum to what *out holds: one more rounding of the result
dtype = torch.float32 evaluates the same formulas in fp32 on the CPU (the stand-in for a correct kernel of tests/test_loss_reference_cpu.py; the bounds
returned with it are meaningless).  Constants the kernels hold in fp32 (0.1f, 1e-6f, 1e-12f, the betas, lr, eps, momentum) enter as those fp32 values.

Data-dependent branches (the log clamp at -100, the BCE gradient's 1e-12 floor, x < 0.1, sign(r), the positive-weight clamps, the clip coefficient's min)
are asserted to be decided clear of rounding by the reference itself; the generators below make such inputs.

WHAT THE ADAM REFERENCE IS: torch.optim.Adam's update rule (no weight decay, no amsgrad) in float64, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), bc = 1 - b^t, with b1, b2, lr, eps the FP32 values the C ABI receives (0.9f = 0.9 + 2.4e-8,
0.999f = 0.999 - 1.0e-8).  It is not the recipe with the unrounded betas 0.9 / 0.999: `adam_recipe_distance` gives the distance between the two.
"""
import math

import torch

from .conv64 import max_ratio  # noqa: F401  (re-exported: the tests take it from here)
from .fused64 import C, U, _ps, compare  # noqa: F401

F64, F32 = torch.float64, torch.float32

# Maximum error of the fp32 device functions csrc/losses.hip calls, in ulps of the result.  Nothing in this repository documents them, so every figure
# is MEASURED: tools/probes/math_ulp_probe.hip (compiled with the flags of csrc/Makefile) compares the function on the MI355X with the float64 function of
# the same fp32 argument over 2^26 arguments per range, the ranges covering what tests/test_loss_reference.py feeds them; the entry is the next integer at or
# above twice the largest error seen.  The error is counted in ulps of the exact result's own binade.
ULP = {
    "expf": 2,       # measured 0.862 ulp over [-80, 0], [-10, 10], [-1, 1]
    "logf": 5,       # measured 2.308 ulp over [1e-37, 1], [0.5, 2], [1, 1e6] (more than the 1 ulp tests/test_philox_reference.py takes from HIP's documentation)
    "log1pf": 2,     # measured 0.567 ulp, log1pf(-p) over p in [1e-30, 1 - 2^-24]
    "sqrtf": 1,      # measured 0.500 ulp over [1e-30, 1e12]: correctly rounded
    "rsqrtf": 2,     # measured 0.864 ulp over [1e-12, 1e12]
    "powf": 3,       # measured 0.977 ulp (0.9f) and 1.287 ulp (0.999f), powf(b, t) for t = 1 .. 100000
    "div": 1,        # measured 0.500 ulp, a / b and 1.f / x over [1e-12, 1e12]: correctly rounded
}


def _u(name):
    """relative error of one call of an elementary function"""
    return ULP[name] * 2.0 * U


def f32(v):
    """the fp32 value of a Python float, as a Python float (what a float argument of the C ABI, or an `f` literal of the kernel, holds)"""
    return float(torch.tensor(float(v), dtype=F32))


EPS6, EPS12, TENTH = f32(1e-6), f32(1e-12), f32(0.1)


def _t(v, dtype):
    return None if v is None else (v.detach().to("cpu", dtype) if torch.is_tensor(v) else torch.tensor(float(v), dtype=dtype))


def _d(v):
    return v.detach().to(F64)


def _out(ref, err):
    return {k: _d(v) for k, v in ref.items()}, {k: _d(v) for k, v in err.items()}


def _acc(s, e, prefill):
    """*out += s: the value the output holds afterwards and its bound (one more rounding)"""
    r = s + prefill
    return r, e + (U * r.abs() if prefill != 0.0 else 0.0)


def _sum(t, e_t, K=None, mag=None):
    """sum of the terms t (own errors e_t): (sum, bound).  mag: the magnitudes summed, where a term is itself a cancelling expression."""
    K = t.numel() if K is None else K
    mag = t.abs() if mag is None else mag
    return t.sum(), _ps(K) * mag.sum() + (e_t.sum() if torch.is_tensor(e_t) else 0.0)


TINY = 2.0 ** -126              # the smallest normal fp32: a result below it may be flushed to zero


def _exp(x, e_x=0.0):
    v = torch.exp(x)
    return v, v * (_u("expf") + e_x) + TINY


# ------------------------------------------------------------------------------------------------ two-input reductions and their gradients
def _bce_terms(p, x):
    lp_raw, lq_raw = torch.log(p), torch.log1p(-p)
    for raw in (lp_raw, lq_raw):
        assert not bool(((raw + 100.0).abs() < 1.0).any()), "a log lies at the -100 clamp: the branch is not decided clear of rounding"
    lp, lq = lp_raw.clamp_min(-100.0), lq_raw.clamp_min(-100.0)
    a, b = x * lp, (1.0 - x) * lq
    t = -(a + b)
    return t, a.abs() * (_u("logf") + 2 * U) + b.abs() * (_u("log1pf") + 3 * U) + U * t.abs()


def reduce2(kind, a, b=None, prefill=0.0, dtype=F64):
    """cvae_sse_fwd / cvae_sum_fwd / cvae_sqnorm / cvae_bce_fwd (a = p, b = x): out = prefill + sum"""
    a, b = _t(a, dtype).reshape(-1), _t(b, dtype)
    if kind == "sse":
        d = a - b.reshape(-1)
        t, e = d * d, 3 * U * d * d
    elif kind == "sum":
        t, e = a, 0.0 * a
    elif kind == "sqnorm":
        t, e = a * a, U * a * a
    elif kind == "bce":
        t, e = _bce_terms(a, b.reshape(-1))
    else:
        raise ValueError(kind)
    s, es = _sum(t, e)
    r, er = _acc(s, es, prefill)
    return _out(dict(out=r), dict(out=er))


def sqnorm_multi(tensors, prefill=0.0, dtype=F64):
    """cvae_sqnorm_multi: prefill + the sum of g^2 over a list of tensors"""
    return reduce2("sqnorm", torch.cat([_t(g, dtype).reshape(-1) for g in tensors]), prefill=prefill, dtype=dtype)


def sse_bwd(a, b, gout, scale, dtype=F64):
    """da = 2 (a - b) (*gout) scale (gout None: 1)"""
    a, b = _t(a, dtype), _t(b, dtype)
    g = (1.0 if gout is None else _t(gout, dtype)) * f32(scale)
    da = 2.0 * (a - b) * g
    return _out(dict(da=da), dict(da=4 * U * da.abs()))


def bce_bwd(p, x, gout, dtype=F64):
    """dp = (p - x) / max((1 - p) p, 1e-12f) * (*gout)"""
    p, x = _t(p, dtype), _t(x, dtype)
    prod = (1.0 - p) * p
    assert not bool(((prod - EPS12).abs() < 1e-3 * EPS12).any()), "(1 - p) p lies at the 1e-12 floor"
    g = 1.0 if gout is None else _t(gout, dtype)
    dp = (p - x) / prod.clamp_min(EPS12) * g
    return _out(dict(dp=dp), dict(dp=(5 * U + _u("div")) * dp.abs()))


# ------------------------------------------------------------------------------------------------ vessel recon terms
def pos_weight(sum_x, n_pos, dtype=F64):
    """(pw, bound): clamp((1 - pf) / (pf + 1e-6f), 1, 50), pf = sum_x / (n_pos + 1e-6f).  Asserts that the clamps are decided clear of rounding."""
    sx = _t(sum_x, dtype).reshape(())
    den0 = _t(float(n_pos), dtype) + EPS6
    pf = sx / den0
    e_pf = pf.abs() * (2 * U + _u("div"))                       # (float) n_pos, the sum with 1e-6f, the division
    num, den = 1.0 - pf, pf + EPS6
    e_num, e_den = e_pf + U * num.abs(), e_pf + U * den.abs()
    raw = num / den
    e_raw = (e_num + raw.abs() * e_den) / den.abs() + _u("div") * raw.abs()
    pw = raw.clamp(1.0, 50.0)
    inside = bool((raw > 1.0) & (raw < 50.0))
    for edge in (1.0, 50.0) if dtype == F64 else ():
        assert abs(float(raw) - edge) > 8 * float(e_raw) + 1e-9, f"the positive weight {float(raw)} lies at its clamp {edge}"
    return pw, (e_raw if inside else 0.0 * e_raw), inside


def wmse_sparsity(r, x, sum_x, n_pos, prefill=(0.0, 0.0), g_recon=None, g_sp=None, dtype=F64, pw_cap=None):
    """cvae_wmse_sparsity_fwd (out[0] += sum (r - x)^2 (1 + (pw - 1) x), out[1] += sum |r| [x < 0.1f]) and _bwd (dr; a NULL g_* is 0).
    pw_cap (self-tests only): clamp the positive weight at this value instead of 50."""
    r, x = _t(r, dtype).reshape(-1), _t(x, dtype).reshape(-1)
    assert not bool(((x - TENTH).abs() < 0.01).any()), "an x lies near 0.1: the sparsity mask is not decided"
    assert not bool(((r != 0) & (r.abs() < 1e-3)).any()), "an r lies near 0 without being 0: the sign in the sparsity gradient is not decided"
    pw, e_pw, inside = pos_weight(sum_x, n_pos, dtype)
    if pw_cap is not None:
        pw = pw.clamp_max(pw_cap)
    d = r - x
    w = 1.0 + (pw - 1.0) * x
    t0 = d * d * w
    e0 = 6 * U * t0.abs() + d * d * x.abs() * e_pw
    mask = x < TENTH
    t1 = torch.where(mask, r.abs(), torch.zeros_like(r))
    s0, es0 = _sum(t0, e0)
    s1, es1 = _sum(t1, 0.0)
    r0, er0 = _acc(s0, es0, prefill[0])
    r1, er1 = _acc(s1, es1, prefill[1])
    gr = 0.0 if g_recon is None else _t(g_recon, dtype)
    gs = 0.0 if g_sp is None else _t(g_sp, dtype)
    a = gr * 2.0 * d * w
    dr = a + torch.where(mask, gs * torch.sign(r), torch.zeros_like(r))
    e_dr = 6 * U * a.abs() + (gr * 2.0 * d * x).abs() * e_pw + U * dr.abs()
    return _out(dict(out=torch.stack([r0, r1]), dr=dr, pw=pw), dict(out=torch.stack([er0, er1]), dr=e_dr, pw=e_pw))


# ------------------------------------------------------------------------------------------------ reparameterise + KLD, latent head
def _kld(mu, lv):
    """-0.5 sum(1 + lv - mu^2 - e^lv) and its bound: four addends per element"""
    ev, e_ev = _exp(lv)
    mag = 1.0 + lv.abs() + mu * mu + ev
    t = 1.0 + lv - mu * mu - ev
    s, es = _sum(t, 3 * U * mag + U * mu * mu + e_ev, K=4 * t.numel(), mag=mag)
    return -0.5 * s, 0.5 * es


def _reparam(mu, lv, eps):
    eh, e_eh = _exp(0.5 * lv)
    z = mu + eps * eh
    return z, eps.abs() * (e_eh + U * eh) + U * z.abs()


def _head_bwd(mu, lv, pairs, gk):
    """d mu, d logvar of z_k = mu + eps_k exp(lv / 2) (pairs of (dz_k, eps_k)) and of the KLD under the gradient gk"""
    ev, e_ev = _exp(lv)
    eh, e_eh = _exp(0.5 * lv)
    k = gk * 0.5 * (ev - 1.0)
    e_k = abs(gk) * 0.5 * (e_ev + U * (ev - 1.0).abs()) + 3 * U * k.abs()
    gm, ge = gk * mu, torch.zeros_like(mu)
    e_gm, mag_ge = 2 * U * gm.abs(), torch.zeros_like(mu)
    for dz, eps in pairs:
        gm = gm + dz
        e_gm = e_gm + U * gm.abs()
        ge = ge + dz * eps
        mag_ge = mag_ge + (dz * eps).abs()
    h = ge * 0.5 * eh
    gl = k + h
    e_gl = e_k + 0.5 * (2 * len(pairs) * U * mag_ge * eh + ge.abs() * e_eh) + 2 * U * h.abs() + U * gl.abs()
    return gm, e_gm, gl, e_gl


def reparam_kld(mu, lv, eps, prefill=0.0, dz=None, gkld=None, gk_scale=1.0, dtype=F64):
    """cvae_reparam_kld_fwd (z, kld = prefill + KLD) and _bwd (dmu, dlogvar; gk = *gkld * gk_scale, a NULL gkld / dz is 0)"""
    mu, lv, eps, dz = (_t(v, dtype) for v in (mu, lv, eps, dz))
    z, e_z = _reparam(mu, lv, eps)
    s, es = _kld(mu, lv)
    k, ek = _acc(s, es, prefill)
    gk = 0.0 if gkld is None else float(_t(gkld, dtype) * f32(gk_scale))
    gm, e_gm, gl, e_gl = _head_bwd(mu, lv, [] if dz is None else [(dz, eps)], gk)
    fix = U * abs(gk) * (mu.abs() + 0.5 * (torch.exp(lv) - 1.0).abs())      # the rounding of gk = *gkld * gk_scale itself
    return _out(dict(z=z, kld=k, dmu=gm, dlogvar=gl), dict(z=e_z, kld=ek, dmu=e_gm + fix, dlogvar=e_gl + fix))


def latent_head(h, eps1, eps2=None, dz1=None, dz2=None, gkld=None, dtype=F64):
    """cvae_latent_head_fwd on h = [B][2 Z] rows (mu | logvar): z1, z2, kld (ASSIGNED), and _bwd: dh [B][2 Z]"""
    h, eps1, eps2, dz1, dz2 = (_t(v, dtype) for v in (h, eps1, eps2, dz1, dz2))
    Z = h.shape[1] // 2
    mu, lv = h[:, :Z], h[:, Z:]
    ref, err = {}, {}
    ref["z1"], err["z1"] = _reparam(mu, lv, eps1)
    if eps2 is not None:
        ref["z2"], err["z2"] = _reparam(mu, lv, eps2)
    ref["kld"], err["kld"] = _kld(mu, lv)
    gk = 0.0 if gkld is None else float(_t(gkld, dtype))
    pairs = [(g, e) for g, e in ((dz1, eps1), (dz2, eps2)) if g is not None]
    gm, e_gm, gl, e_gl = _head_bwd(mu, lv, pairs, gk)
    ref["dh"], err["dh"] = torch.cat([gm, gl], 1), torch.cat([e_gm, e_gl], 1)
    return _out(ref, err)


# ------------------------------------------------------------------------------------------------ Gaussian NLL
def gauss_nll(m, mu, lv, prefill=0.0, gout=None, dtype=F64):
    """cvae_gauss_nll_fwd: out = prefill + 0.5 sum(lv + (m - mu)^2 / e^lv); _bwd: dmu, dlogvar (gout None: 1)"""
    m, mu, lv = (_t(v, dtype).reshape(-1) for v in (m, mu, lv))
    d = m - mu
    ev, e_ev = _exp(lv)
    q = d * d / ev
    e_q = q * (3 * U + e_ev / ev + _u("div"))
    t = lv + q
    s, es = _sum(t, e_q + U * t.abs(), K=2 * t.numel(), mag=lv.abs() + q)
    r, er = _acc(0.5 * s, 0.5 * es, prefill)
    g = 1.0 if gout is None else _t(gout, dtype)
    iv = 1.0 / ev
    r_iv = e_ev / ev + _u("div")
    dmu = g * (-d * iv)
    dlv = g * 0.5 * (1.0 - d * d * iv)
    e_dmu = dmu.abs() * (3 * U + r_iv)
    e_dlv = abs(g) * 0.5 * (d * d * iv * (3 * U + r_iv) + U * (1.0 - d * d * iv).abs()) + 2 * U * dlv.abs()
    return _out(dict(out=r, dmu=dmu, dlogvar=dlv), dict(out=er, dmu=e_dmu, dlogvar=e_dlv))


# ------------------------------------------------------------------------------------------------ softmax CE / uniform KL
def _log_softmax(logits):
    Cn = logits.shape[1]
    mx = logits.max(1, keepdim=True).values
    sh = logits - mx
    e, e_e = _exp(sh, U * sh.abs())
    se = e.sum(1, keepdim=True)
    e_se = _ps(Cn) * se + e_e.sum(1, keepdim=True)
    lse = torch.log(se)
    e_lse = e_se / se + _u("logf") * lse.abs()
    logp = sh - lse
    e_logp = U * sh.abs() + e_lse + U * logp.abs()
    sm = e / se
    e_sm = sm * (e_e / e.clamp_min(1e-300) + e_se / se + _u("div"))
    return logp, e_logp, sm, e_sm


def softmax_ce(logits, target, prefill=0.0, gout=None, dtype=F64, no_onehot=False):
    """cvae_softmax_ce_fwd: out = prefill + mean_b CE; _bwd: dlogits = (softmax - onehot) / B * gout (None: 1).
    no_onehot (self-tests only): the gradient without its onehot term."""
    x = _t(logits, dtype)
    B, Cn = x.shape
    tg = target.detach().to("cpu", torch.int64)
    logp, e_logp, sm, e_sm = _log_softmax(x)
    t = -logp.gather(1, tg[:, None])[:, 0] / B
    e_t = e_logp.gather(1, tg[:, None])[:, 0] / B + _u("div") * t.abs()
    s, es = _sum(t, e_t)
    r, er = _acc(s, es, prefill)
    oh = torch.zeros_like(x).scatter_(1, tg[:, None], 0.0 if no_onehot else 1.0)
    g = 1.0 if gout is None else _t(gout, dtype)
    dl = g * (sm - oh) / B
    e_dl = (e_sm + U * (sm - oh).abs()) * abs(g) / B + (U + _u("div")) * dl.abs()
    return _out(dict(out=r, dlogits=dl), dict(out=er, dlogits=e_dl))


def uniform_kl(logits, prefill=0.0, gout=None, dtype=F64):
    """cvae_uniform_kl_fwd: out = prefill + sum u (log u - log_softmax) / B, u = 1 / C; _bwd: dlogits = (softmax - u) / B * gout"""
    x = _t(logits, dtype)
    B, Cn = x.shape
    logp, e_logp, sm, e_sm = _log_softmax(x)
    u = 1.0 / Cn
    e_u = _u("div") * u                                          # the kernel's u is the fp32 quotient
    lu = math.log(u)
    e_lu = e_u / u + _u("logf") * abs(lu)
    diff = lu - logp
    t = u * diff / B
    e_t = (e_u * diff.abs() + u * (e_lu + e_logp + U * diff.abs())) / B + (U + _u("div")) * t.abs()
    s, es = _sum(t, e_t)
    r, er = _acc(s, es, prefill)
    g = 1.0 if gout is None else _t(gout, dtype)
    dl = g * (sm - u) / B
    e_dl = (e_sm + e_u + U * (sm - u).abs()) * abs(g) / B + (U + _u("div")) * dl.abs()
    return _out(dict(out=r, dlogits=dl), dict(out=er, dlogits=e_dl))


# ------------------------------------------------------------------------------------------------ BatchNorm1d
def bn1d(x, w, b, dy, rm, rv, momentum, eps, split=1, dtype=F64, var_div=None, n_stat=None):
    """Train-mode BatchNorm1d of the WHOLE batch x [N][F], forward and backward: y, save_mean, save_rstd, running_mean / running_var (unbiased N - 1),
    dx, dw, db.  w / b / rm / rv may be None.  split: the number of equal "ranks" the split form (cvae_bn1d_stats / _apply_stats / _bwd_sums / _bwd_apply)
    cuts the batch into; it only widens the bounds by the roundings of that form (the rank sums added, inv_n = 1 / N rounded, n = 1 / inv_n).
    Self-tests only: var_div replaces N - 1 in the running variance, n_stat replaces N as the divisor of the statistics."""
    x, w, b, dy, rm, rv = (_t(v, dtype) for v in (x, w, b, dy, rm, rv))
    N, Fn = x.shape
    mom, eps = f32(momentum), f32(eps)
    n = float(N if n_stat is None else n_stat)
    sp = 4 * U if split > 1 else 0.0                              # rank sums added, inv_n rounded, one product
    mean = x.sum(0) / n
    e_mean = _ps(N) * x.abs().sum(0) / n + (_u("div") + sp) * mean.abs()
    dev = x - mean
    e_dev = e_mean + U * dev.abs()
    q = (dev * dev).sum(0)
    e_q = (2 * dev.abs() * e_dev + e_dev * e_dev).sum(0) + (_ps(N) + 3 * U + sp) * q
    var = q / n
    e_var = e_q / n + _u("div") * var
    rstd = 1.0 / torch.sqrt(var + eps)
    e_rstd = rstd * ((e_var + U * (var + eps)) / (2 * (var + eps)) + _u("rsqrtf"))
    xh = dev * rstd
    e_xh = e_dev * rstd + dev.abs() * e_rstd + U * xh.abs()
    ww = torch.ones(Fn, dtype=dtype) if w is None else w
    bb = torch.zeros(Fn, dtype=dtype) if b is None else b
    y = xh * ww + bb
    e_y = ww.abs() * e_xh + 2 * U * ((xh * ww).abs() + bb.abs())
    ref = dict(y=y, save_mean=mean, save_rstd=rstd)
    err = dict(y=e_y, save_mean=e_mean, save_rstd=e_rstd)
    if rm is not None:
        ref["running_mean"] = (1.0 - mom) * rm + mom * mean
        err["running_mean"] = mom * e_mean + 3 * U * (rm.abs() + mom * mean.abs())
    if rv is not None:
        nm1 = float(N - 1 if var_div is None else var_div)
        e_nm1 = (2 * U * N / (N - 1)) if split > 1 else 0.0       # n = 1.f / inv_n, then n - 1.f
        uv = q / nm1
        ref["running_var"] = (1.0 - mom) * rv + mom * uv
        err["running_var"] = mom * (e_q / nm1 + (e_nm1 + sp) * uv) + 4 * U * (rv.abs() + mom * uv)
    if dy is not None:
        mxh = xh.abs() + e_xh
        s1, s2 = dy.sum(0), (dy * xh).sum(0)
        e_s1 = (_ps(N) + sp) * dy.abs().sum(0)
        e_s2 = (_ps(N) + sp) * (dy.abs() * mxh).sum(0) + (dy.abs() * (e_xh + 2 * U * mxh)).sum(0)
        inner = dy - s1 / n - xh * s2 / n
        mag = dy.abs() + s1.abs() / N + mxh * s2.abs() / N
        dx = ww * rstd * inner
        e_inner = e_s1 / N + (e_xh * s2.abs() + mxh * e_s2) / N + (4 * U + 2 * _u("div")) * mag
        e_dx = ww.abs() * (e_rstd * inner.abs() + rstd * e_inner) + 3 * U * dx.abs()
        ref.update(dx=dx, dw=s2, db=s1)
        err.update(dx=e_dx, dw=e_s2, db=e_s1)
    return _out(ref, err)


def bn1d_eval(x, w, b, rm, rv, eps, dtype=F64):
    """cvae_bn1d_eval_fwd: y = (x - rm) / sqrt(rv + eps) * w + b"""
    x, w, b, rm, rv = (_t(v, dtype) for v in (x, w, b, rm, rv))
    eps = f32(eps)
    d = x - rm
    sd = torch.sqrt(rv + eps)
    xh = d / sd
    e_xh = xh.abs() * (U + 0.5 * U + _u("sqrtf") + _u("div"))
    ww = 1.0 if w is None else w
    bb = torch.zeros(x.shape[1], dtype=dtype) if b is None else b
    y = xh * ww + bb
    ww_abs = abs(ww) if not torch.is_tensor(ww) else ww.abs()
    return _out(dict(y=y), dict(y=ww_abs * e_xh + 2 * U * ((xh * ww).abs() + bb.abs())))


# ------------------------------------------------------------------------------------------------ Adam
def adam(p, m, v, grads, lr, b1, b2, eps, t0=1, device_step=False, gscale=None, dtype=F64, bc2_lag=0):
    """len(grads) steps of Adam from the state (p, m, v) at step numbers t0, t0 + 1, ...: see the module docstring for what this reference is.
    device_step: the corrections are 1 - powf(b, t) in the kernel (bound: ULP['powf'] ulps of b^t, relative to 1 - b^t: it grows as b^t -> 1, at small t
    for b2); else the caller rounds the float64 1 - b^t to fp32 (one rounding).  gscale: a scalar multiplied into every gradient first.
    bc2_lag (self-tests only): bc2 of step t - bc2_lag.  Returns (ref, err) with keys p, m, v."""
    p, m, v = (_t(x, dtype).clone().reshape(-1) for x in (p, m, v))
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    e_p, e_m, e_v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    gs = None if gscale is None else float(_t(gscale, dtype))
    for k, g in enumerate(grads):
        t = t0 + k
        g = _t(g, dtype).reshape(-1)
        e_g = 0.0 * g
        if gs is not None:
            g = g * gs
            e_g = U * g.abs()
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** (t - bc2_lag)
        if device_step:
            r_bc1, r_bc2 = (_u("powf") * b1 ** t + U * bc1) / bc1, (_u("powf") * b2 ** t + U * bc2) / bc2
        else:
            r_bc1 = r_bc2 = U
        if dtype == F32:
            bc1, bc2 = f32(bc1), f32(bc2)
        a1, a2 = b1 * m, (1.0 - b1) * g
        e_m = b1 * e_m + (1.0 - b1) * e_g + 3 * U * (a1.abs() + a2.abs())
        m = a1 + a2
        c1, c2 = b2 * v, (1.0 - b2) * g * g
        e_v = b2 * e_v + (1.0 - b2) * 2 * g.abs() * e_g + 4 * U * (c1 + c2)
        v = c1 + c2
        sq = torch.sqrt(v)
        e_sq = torch.where(v > 0, e_v / (2 * sq.clamp_min(1e-300)), torch.sqrt(e_v)) + _u("sqrtf") * sq
        rbc2 = 1.0 / math.sqrt(bc2)
        r_rbc2 = 0.5 * r_bc2 + _u("sqrtf") + _u("div")
        den = sq * rbc2 + eps
        e_den = rbc2 * (e_sq + (r_rbc2 + U) * sq) + U * den
        step = lr / bc1
        upd = step * (m / den)
        e_upd = step / den * e_m + upd.abs() * (r_bc1 + 2 * _u("div") + U + e_den / den)
        p = p - upd
        e_p = e_p + e_upd + U * p.abs()
    return _out(dict(p=p, m=m, v=v), dict(p=e_p, m=e_m, v=e_v))


def adam_recipe_distance(p, grads, lr=1e-3, eps=1e-8):
    """max |p_ref - p_recipe| / max |p_recipe - p0| after len(grads) steps: the reference above (fp32 betas / lr / eps) against torch.optim.Adam in float64
    with the unrounded betas 0.9 / 0.999, the recipe the reference project trains with.  A number to print, not a bound."""
    p0 = _t(p, F64).reshape(-1)
    z = torch.zeros_like(p0)
    ref, _ = adam(p0, z, z, grads, lr, 0.9, 0.999, eps)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(0.9, 0.999), eps=eps)
    for g in grads:
        q.grad = _t(g, F64).reshape(-1).clone()
        opt.step()
    return float((ref["p"] - q.detach()).abs().max() / (q.detach() - p0).abs().max())


# ------------------------------------------------------------------------------------------------ clipping and the scalar combinations
def clip_coef(sq, max_norm, dtype=F64):
    """min(1, max_norm / (sqrt(sq) + 1e-6f)); asserts that the min is decided clear of rounding"""
    sq = _t(sq, dtype).reshape(())
    raw = f32(max_norm) / (torch.sqrt(sq) + EPS6)
    e_raw = raw * (_u("sqrtf") + U + _u("div"))
    assert abs(float(raw) - 1.0) > 8 * float(e_raw), "the clip coefficient lies at 1"
    return _out(dict(scale=raw.clamp_max(1.0)), dict(scale=e_raw if float(raw) < 1.0 else 0.0 * e_raw))


def scale(g, s, dtype=F64):
    r = _t(g, dtype) * _t(s, dtype)
    return _out(dict(g=r), dict(g=U * r.abs()))


def weighted_sum(terms, weights, g=None, dtype=F64):
    """cvae_weighted_sum: fwd [sum_i w_i t_i, w_0 t_0, ...]; bwd [w_i * g] (g None: 1)"""
    tv = torch.stack([_t(t, dtype).reshape(()) for t in terms])
    w = torch.tensor([f32(x) for x in weights], dtype=dtype)
    v = w * tv
    s, es = _sum(v, U * v.abs())
    gv = 1.0 if g is None else _t(g, dtype)
    bw = w * gv
    return _out(dict(fwd=torch.cat([s[None], v]), bwd=bw), dict(fwd=torch.cat([es[None], U * v.abs()]), bwd=U * bw.abs()))


def combine3(out4, wb, wc, dtype=F64):
    """out4[0] = out4[1] + wb out4[2] + wc out4[3]"""
    o = _t(out4, dtype).clone()
    a, b, c = o[1], f32(wb) * o[2], f32(wc) * o[3]
    o[0] = a + b + c
    e = torch.zeros_like(o)
    e[0] = _ps(3) * (a.abs() + b.abs() + c.abs())
    return _out(dict(out4=o), dict(out4=e))


# ------------------------------------------------------------------------------------------------ inputs with every branch decided
def gen(seed):
    return torch.Generator().manual_seed(seed)


def bce_inputs(seed, n):
    """p in (0.02, 0.98) with the edge values p = 0, 1, 1e-30, 1 - 2^-24 planted (as far as n allows; both gradient floors are among them), x binary there"""
    g = gen(seed)
    p = 0.02 + 0.96 * torch.rand(n, generator=g)
    x = torch.rand(n, generator=g)
    edge_p = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24, 0.0, 1.0]
    edge_x = [0.0, 1.0, 0.0, 1.0, 1.0, 0.0]                       # the last two: the log clamp at -100 enters the sum
    for i in range(min(n, len(edge_p)) if n >= 4 else 0):
        p[n - 1 - i], x[n - 1 - i] = edge_p[i], edge_x[i]
    return p.float(), x.float()


def vessel_inputs(seed, n, kind="general"):
    """(r, x): x binary with ~10 % ones and, in `general`, a tenth of the zeros replaced by values in [0.15, 0.9] (at least 0.05 away from 0.1); r away from
    zero (|r| >= 0.01) with every 7th value exactly zero.  kind 'zeros' / 'ones': x all 0 / all 1 (the positive weight sits on its clamp 50 / 1);
    'sparse': one x in 512 is 1 (the weight is clamped at 50 and multiplies those terms)."""
    g = gen(seed)
    if kind == "zeros":
        x = torch.zeros(n)
    elif kind == "ones":
        x = torch.ones(n)
    elif kind == "sparse":                                       # one voxel in 512 set: the raw weight is ~511, clamped at 50, and weighs real terms
        x = torch.zeros(n)
        x[::512] = 1.0
    else:
        x = (torch.rand(n, generator=g) < 0.1).float()
        soft = (torch.rand(n, generator=g) < 0.1) & (x == 0)
        x = torch.where(soft, 0.15 + 0.75 * torch.rand(n, generator=g), x)
    r = torch.randn(n, generator=g)
    r = torch.where(r.abs() < 0.01, torch.full_like(r, 0.01), r)
    r[::7] = 0.0
    return r.float(), x.float()
