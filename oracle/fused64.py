"""Float64 references of the two fused kernel families on the training step's hot path, with derived error bounds.

  bottleneck(...)   the dense middle of CausalBioVAE (csrc/bottleneck.hip, ops.BioBottleneck): pool, cat, enc_fc, fc_mu / fc_logvar,
                    reparameterize, mechanism_net with BatchNorm1d, dec_input, and the backward from given upstream gradients.
  elbo_up2x(...)    the ELBO with the exact-2x linear resize folded in (csrc/recon_loss.hip, ops.ElboUp2x).

Each returns the reference values (`ref`) and, for every compared tensor, an elementwise bound (`err`) on how far an fp32 evaluation of the same
sums may lie from it.  The bound is carried through the graph in first order: a product-sum of K terms contributes C * sqrt(K) * U * (|A| . |B|)
(the float64 |A| and |B|, U = 2^-24), and the error already in an operand travels on through the same sum in quadrature, sqrt(A^2 . err(B)^2)
(independent roundings; the linear |A| . err(B) would add a factor of up to sqrt(K) per layer and let few-percent errors pass at the model shapes).  BatchNorm and exp have their own
terms (the rounding in h - mean is amplified by 1 / sqrt(var + eps), which is 1 / sqrt(bn_eps) for a zero-variance column).  `compare` checks
a kernel's outputs against them; tests/test_fused_reference_cpu.py checks that a plain fp32 run passes and that dropping one term fails.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24                  # unit roundoff of fp32
C = 4.0                         # the one constant of every product-sum bound
BF16_HALF_ULP = 2.0 ** -8       # relative: half a bf16 ulp of x is at most |x| 2^-8

PARAMS = ("W1", "b1", "W2", "b2", "Wmu", "bmu", "Wlv", "blv", "Wm0", "bm0", "gamma", "beta", "Wm3", "bm3", "Wm5", "bm5", "Wd", "bd")
RELU_PRE = ("p1", "p2", "bn_y", "p3")     # internal ReLU pre-activations: their masks must agree exactly


def _ps(K):
    return C * math.sqrt(max(K, 1)) * U


def _rss(e, W):
    """an operand's error carried through a product-sum: sqrt(err^2 . W^2).  The rounding errors of different terms are independent, so they
    add in quadrature (the same model as the sqrt(K) of the product-sum rule); |err| . |W| would assume every sign aligned."""
    return torch.sqrt((e * e) @ (W * W))


def _lin(x, ex, W, b):
    """y = x W^T + b with its bound: C sqrt(K) U (|x| |W|^T + |b|) + sqrt(err(x)^2 (W^2)^T) (W, b exact fp32 values)."""
    y = x @ W.t() + (b if b is not None else 0.0)
    mag = x.abs() @ W.abs().t() + (b.abs() if b is not None else 0.0)
    return y, _ps(W.shape[1] + 1) * mag + _rss(ex, W.t())


def _pool(y_cl, out_size):
    """y_cl [M, D, H, W, C] -> NC(D)HW average over the non-overlapping windows, flattened C-major (nn.Flatten on NC(D)HW)."""
    M, D, H, W, Cc = y_cl.shape
    OD, OH, OW = out_size
    y = y_cl.permute(0, 4, 1, 2, 3).reshape(M, Cc, OD, D // OD, OH, H // OH, OW, W // OW)
    return y.mean(dim=(3, 5, 7)).reshape(M, Cc * OD * OH * OW), (D // OD) * (H // OH) * (W // OW)


def bottleneck(y_cl, m, t_onehot, eps, params, running_mean, running_var, momentum, bn_eps, out_size, g_dec_cl, g_mu, g_logvar, g_mhat,
               training=True, drop=None, dtype=torch.float64):
    """Float64 forward + backward of the fused bottleneck.  Tensors may be of any dtype / device; all work is float64 on the CPU.
    A SyncBatchNorm run over ranks is compared with this whole-batch computation.  g_* may be None (zero).  drop (self-tests only): remove one term from the computation,
    ('k1_col', k) / ('pool_voxel', (b, d, h, w)) / ('wgrad_row', m) / ('hm_unit', j) / ('dy_slab', (n0, n1)).
    dtype=torch.float32 evaluates the same graph in fp32 (the self-tests' stand-in for a correct kernel; its bounds are then meaningless).
    Returns (ref, err, pre): ref / err dicts of the compared tensors, pre = the ReLU pre-activations with their bounds."""
    d64 = lambda v: None if v is None else v.detach().to("cpu", dtype)
    P = {k: d64(v) for k, v in zip(PARAMS, params)}
    y = d64(y_cl).clone()
    m, t, eps = d64(m), d64(t_onehot), d64(eps)
    M, Dv, Hv, Wv, Cc = y.shape
    OD, OH, OW = out_size
    if drop and drop[0] == "k1_col":
        P["W1"] = P["W1"].clone()
        P["W1"][:, drop[1]] = 0.0
    if drop and drop[0] == "pool_voxel":
        b, dd, hh, ww = drop[1]
        y[b, dd, hh, ww, :] = 0.0
    if drop and drop[0] == "hm_unit":
        P["Wm3"] = P["Wm3"].clone()
        P["Wm3"][:, drop[1]] = 0.0
    leaves = {k: P[k].clone().requires_grad_(True) for k in PARAMS}
    yl = y.clone().requires_grad_(True)

    # ---- forward (autograd, float64) and its bounds
    feat, nvox = _pool(yl, out_size)
    xcat = torch.cat([feat, m, t], 1)
    e_xcat = torch.cat([_ps(nvox) * _pool(y.abs(), out_size)[0], torch.zeros_like(m), torch.zeros_like(t)], 1)
    p1, e_p1 = _lin(xcat, e_xcat, leaves["W1"], leaves["b1"])
    h1 = F.relu(p1)
    e_h1 = e_p1 * (p1 > 0)
    p2, e_p2 = _lin(h1, e_h1, leaves["W2"], leaves["b2"])
    h2 = F.relu(p2)
    e_h2 = e_p2 * (p2 > 0)
    mu, e_mu = _lin(h2, e_h2, leaves["Wmu"], leaves["bmu"])
    lv, e_lv = _lin(h2, e_h2, leaves["Wlv"], leaves["blv"])
    ex = torch.exp(0.5 * lv)
    z = mu + eps * ex
    e_ex = ex * (0.5 * e_lv + 4 * U * (1.0 + lv.abs()))             # exp: argument rounding (~|x| U) + a few ulp of the exp itself
    e_z = e_mu + eps.abs() * e_ex + 2 * U * (mu.abs() + (eps * ex).abs())
    a, e_a = _lin(t, torch.zeros_like(t), leaves["Wm0"], leaves["bm0"])
    nb = M
    if training:
        mean = a.mean(0)
        e_mean = e_a.mean(0) + _ps(nb) * a.abs().mean(0)
        dev = a - mean
        var = (dev * dev).mean(0)
        e_dev = e_a + e_mean + U * dev.abs()
        e_var = (2 * dev.abs() * e_dev).mean(0) + _ps(nb) * var + e_dev.pow(2).mean(0)
    else:
        mean, var = d64(running_mean), d64(running_var)
        dev = a - mean
        e_dev = e_a + U * (a.abs() + mean.abs())
        e_var = U * var
    invstd = 1.0 / torch.sqrt(var + bn_eps)
    xhat = dev * invstd
    e_invstd = invstd * (e_var / (2 * (var + bn_eps)) + 3 * U)
    e_xhat = e_dev * invstd + dev.abs() * e_invstd + U * xhat.abs()
    mag_xhat = xhat.abs() + e_xhat                                  # what the kernel's xhat can be as large as (BN backward operands)
    bn_y = leaves["gamma"] * xhat + leaves["beta"]
    e_bn_y = leaves["gamma"].abs() * e_xhat + 2 * U * ((leaves["gamma"] * xhat).abs() + leaves["beta"].abs())
    r1 = F.relu(bn_y)
    e_r1 = e_bn_y * (bn_y > 0)
    p3, e_p3 = _lin(r1, e_r1, leaves["Wm3"], leaves["bm3"])
    a2 = F.relu(p3)
    e_a2 = e_p3 * (p3 > 0)
    mh, e_mh = _lin(a2, e_a2, leaves["Wm5"], leaves["bm5"])
    zm = torch.cat([z, mh], 1)
    e_zm = torch.cat([e_z, e_mh], 1)
    dec, e_dec = _lin(zm, e_zm, leaves["Wd"], leaves["bd"])
    cl = lambda v: v.reshape(M, Cc, OD, OH, OW).permute(0, 2, 3, 4, 1)
    dec_cl, e_dec_cl = cl(dec), cl(e_dec)

    # ---- backward: autograd from the given upstream gradients
    g_dec = d64(g_dec_cl)
    zeros = lambda v: torch.zeros_like(v)
    g_mu, g_lv, g_mh = (zeros(mu) if g_mu is None else d64(g_mu)), (zeros(lv) if g_logvar is None else d64(g_logvar)), (zeros(mh) if g_mhat is None else d64(g_mhat))
    obj = (dec_cl * g_dec).sum() + (mu * g_mu).sum() + (lv * g_lv).sum() + (mh * g_mh).sum()
    names = list(PARAMS)
    gr = torch.autograd.grad(obj, [leaves[k] for k in names] + [yl], allow_unused=True)
    grads = {"d" + k: (v if v is not None else zeros(P[k])) for k, v in zip(names, gr[:-1])}
    dy_cl = gr[-1] * (y > 0)

    # bounds of the backward (the same first-order rule, written out)
    with torch.no_grad():
        ag = g_dec.permute(0, 4, 1, 2, 3).reshape(M, -1).abs()
        Fn = Cc * OD * OH * OW
        e = {}
        e["dWd"] = _ps(M) * ag.t() @ zm.abs() + _rss(ag.t(), e_zm)
        e["dbd"] = _ps(M) * ag.sum(0)
        dzm = (g_dec.permute(0, 4, 1, 2, 3).reshape(M, -1)) @ P["Wd"]
        e_dzm = _ps(Fn) * ag @ P["Wd"].abs()
        Z = mu.shape[1]
        dz, e_dz = dzm[:, :Z], e_dzm[:, :Z]
        dmh = dzm[:, Z:] + g_mh
        e_dmh = e_dzm[:, Z:] + U * dmh.abs()
        dmu = dz + g_mu
        e_dmu = e_dz + U * dmu.abs()
        dlv = dz * eps * 0.5 * ex + g_lv
        e_dlv = e_dz * (eps * 0.5 * ex).abs() + (dz * eps * 0.5).abs() * e_ex + 4 * U * ((dz * eps * 0.5 * ex).abs() + g_lv.abs())

        def wgrad(g, eg, x, ex_):        # dW = g^T x over the batch, db = sum g
            return _ps(M) * g.abs().t() @ x.abs() + _rss(eg.t(), x) + _rss(g.t(), ex_), _ps(M) * g.abs().sum(0) + eg.pow(2).sum(0).sqrt()

        def dgrad(g, eg, W, mask):       # dx = (g W) * mask
            return (_ps(W.shape[0]) * g.abs() @ W.abs() + _rss(eg, W)) * mask

        e["dWmu"], e["dbmu"] = wgrad(dmu, e_dmu, h2, e_h2)
        e["dWlv"], e["dblv"] = wgrad(dlv, e_dlv, h2, e_h2)
        dh2 = (dmu @ P["Wmu"] + dlv @ P["Wlv"]) * (p2 > 0)
        e_dh2 = (_ps(2 * Z) * (dmu.abs() @ P["Wmu"].abs() + dlv.abs() @ P["Wlv"].abs()) + _rss(e_dmu, P["Wmu"]) + _rss(e_dlv, P["Wlv"])) * (p2 > 0)
        e["dW2"], e["db2"] = wgrad(dh2, e_dh2, h1, e_h1)
        g1 = (dh2 @ P["W2"]) * (p1 > 0)
        e_g1 = dgrad(dh2, e_dh2, P["W2"], p1 > 0)
        e["dW1"], e["db1"] = wgrad(g1, e_g1, xcat.detach(), e_xcat)
        dx = g1 @ P["W1"]
        e_dx = _ps(P["W1"].shape[0]) * g1.abs() @ P["W1"].abs() + _rss(e_g1, P["W1"])
        e_dy = e_dx[:, :Fn] / nvox + U * (dx[:, :Fn].abs() / nvox)
        e_dy = e_dy.reshape(M, Cc, OD, 1, OH, 1, OW, 1).expand(M, Cc, OD, Dv // OD, OH, Hv // OH, OW, Wv // OW).reshape(M, Cc, Dv, Hv, Wv)
        e["dy_cl"] = e_dy.permute(0, 2, 3, 4, 1) * (y > 0)
        # mechanism_net
        e["dWm5"], e["dbm5"] = wgrad(dmh, e_dmh, a2, e_a2)
        da2 = (dmh @ P["Wm5"]) * (p3 > 0)
        e_da2 = dgrad(dmh, e_dmh, P["Wm5"], p3 > 0)
        e["dWm3"], e["dbm3"] = wgrad(da2, e_da2, r1.detach(), e_r1)
        dyb = (da2 @ P["Wm3"]) * (bn_y > 0)
        e_dyb = dgrad(da2, e_da2, P["Wm3"], bn_y > 0)
        xh = xhat.detach()
        e["dgamma"] = _ps(nb) * (dyb.abs() * mag_xhat).sum(0) + (e_dyb * xh.abs() + dyb.abs() * e_xhat).sum(0)
        e["dbeta"] = _ps(nb) * dyb.abs().sum(0) + e_dyb.sum(0)
        k = (P["gamma"] * invstd.detach() / nb).abs()
        sdy = dyb.abs().sum(0)
        sdx = (dyb.abs() * mag_xhat).sum(0)
        # dx = k (n dy - sum dy - xhat sum dy xhat): rounding of the three terms, the errors of dy / xhat / the two sums, and of k (invstd)
        mag_dxb = k * (nb * dyb.abs() + sdy + mag_xhat * sdx)
        e_dxb = (3 * U + _ps(nb) + e_invstd / invstd) * mag_dxb + k * (nb * e_dyb + e["dbeta"] + e_xhat * sdx + mag_xhat * e["dgamma"])
        # dWm0 = dx^T t, dbm0 = sum dx: the rounding of the sums is bounded through the magnitude of dx's terms (dbm0 is 0 in exact arithmetic)
        e["dWm0"] = _ps(nb) * mag_dxb.t() @ t.abs() + e_dxb.t() @ t.abs()
        e["dbm0"] = _ps(nb) * mag_dxb.sum(0) + e_dxb.sum(0)

    ref = dict(mu=mu.detach(), logvar=lv.detach(), m_hat=mh.detach(), dec_cl=dec_cl.detach(), dy_cl=dy_cl, **{k: v.detach() for k, v in grads.items()})
    err = dict(mu=e_mu, logvar=e_lv, m_hat=e_mh, dec_cl=e_dec_cl, **e)
    if drop and drop[0] == "wgrad_row":      # one batch row missing from a weight-gradient sum: dW1 -= g1[m]^T xcat[m]
        r = drop[1]
        ref["dW1"] = ref["dW1"] - g1[r:r + 1].t() @ xcat.detach()[r:r + 1]
    if drop and drop[0] == "dy_slab":        # one slab of enc_fc.0 rows (the backward's NS split) missing from d(xcat), hence from dy_cl
        n0, n1 = drop[1]
        part = (g1[:, n0:n1] @ P["W1"][n0:n1, :Fn]) / nvox
        part = part.reshape(M, Cc, OD, 1, OH, 1, OW, 1).expand(M, Cc, OD, Dv // OD, OH, Hv // OH, OW, Wv // OW).reshape(M, Cc, Dv, Hv, Wv)
        ref["dy_cl"] = ref["dy_cl"] - part.permute(0, 2, 3, 4, 1) * (y > 0)
    if training:
        rm, rv = d64(running_mean), d64(running_var)
        ref["running_mean"] = (1 - momentum) * rm + momentum * mean.detach()
        ref["running_var"] = (1 - momentum) * rv + momentum * var.detach() * nb / (nb - 1)
        err["running_mean"] = momentum * e_mean + 3 * U * (rm.abs() + momentum * mean.detach().abs())
        err["running_var"] = momentum * e_var * nb / (nb - 1) + 4 * U * (rv.abs() + momentum * var.detach() * nb / (nb - 1))
    err = {k: v.detach() for k, v in err.items()}
    pre = {k: (v.detach(), ev.detach()) for k, (v, ev) in dict(p1=(p1, e_p1), p2=(p2, e_p2), bn_y=(bn_y, e_bn_y), p3=(p3, e_p3)).items()}
    return ref, err, pre


def bf16_out(err, ref):
    """The bound of an output stored in bf16: the fp32 bound plus half a bf16 ulp of the value."""
    return err + BF16_HALF_ULP * (ref.abs() + err)


def mask_margin(pre):
    """The ReLU pre-activations that lie within their bound of zero (must be none: then the kernel's masks equal the reference's exactly).
    Returns {name: count}."""
    return {k: int(((v.abs() <= ev) & (ev > 0)).sum()) + int(((v == 0) & (ev > 0)).sum()) for k, (v, ev) in pre.items()}


def compare(got, ref, err, names=None):
    """Every |got - ref| <= err, elementwise.  Returns a list of failure messages (empty: all within their bounds)."""
    bad = []
    for k in (names or ref.keys()):
        g = got[k].detach().to("cpu", torch.float64).reshape(ref[k].shape)
        r, e = ref[k], err[k]
        d = (g - r).abs()
        over = ~(d <= e)                        # NaN counts as over
        if bool(over.any()):
            i = int(torch.nonzero(over.reshape(-1))[0])
            bad.append(f"{k}: {int(over.sum())}/{over.numel()} outside the bound; first at flat {i}: got {float(g.reshape(-1)[i]):.9g} "
                       f"ref {float(r.reshape(-1)[i]):.9g} |diff| {float(d.reshape(-1)[i]):.3g} > bound {float(e.reshape(-1)[i]):.3g}")
    return bad


def nudge_biases(case, out_size, bn_eps, training=True, rounds=8):
    """Move the bias of every unit whose ReLU pre-activation lies within 8x its bound of zero (b1, b2, beta, bm3), so that the masks of an fp32
    evaluation cannot differ from the reference's.  Works in place on case['params'] (fp32 tensors); returns the number of units moved."""
    idx = {"p1": 1, "p2": 3, "bn_y": 11, "p3": 13}
    moved = 0
    for _ in range(rounds):
        _, _, pre = bottleneck(case["y_cl"], case["m"], case["t"], case["eps"], case["params"], case["rm"], case["rv"], 0.1, bn_eps, out_size,
                               case["g_dec"], None, None, None, training=training)
        changed = False
        for k, (v, ev) in pre.items():
            near = ((v.abs() <= 8 * ev) | (v == 0)).any(0)
            if bool(near.any()):
                b = case["params"][idx[k]]
                shift = (16 * ev.max(0).values + 1e-3 * (b.double().cpu().abs() + 1e-2)).to(b.dtype).to(b.device)
                sign = torch.where(v.mean(0) >= 0, 1.0, -1.0).to(b.dtype).to(b.device)
                b[near.to(b.device)] += (sign * shift)[near.to(b.device)]
                moved += int(near.sum())
                changed = True
                break                                       # downstream pre-activations depend on this layer: recompute first
        if not changed:
            return moved
    return moved


def make_case(seed, M, spatial, Cc, out_size, m_dim, t_dim, N1, N2, Z, HM, y_dtype=torch.float32, labels=None, bn_eps=1e-5, training=True):
    """Random inputs, parameters (fan-in scaled, non-zero BatchNorm beta) and upstream gradients of one bottleneck case, on the CPU, with the
    biases nudged (nudge_biases) so that no ReLU pre-activation lies near zero.  labels: int64 [M] class indices (default: random)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    uni = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    OD, OH, OW = out_size
    S = OD * OH * OW
    K1, K4 = Cc * S + m_dim + t_dim, Z + m_dim
    y = F.relu(rnd(M, *spatial, Cc)).to(y_dtype)
    lin = lambda n, k, s=1.0: [uni(n, k) * s / math.sqrt(k), uni(n) / math.sqrt(k)]
    params = lin(N1, K1, 2.0) + lin(N2, N1, 2.0) + lin(Z, N2) + lin(Z, N2, 0.5) + lin(HM, t_dim, 2.0)
    params += [1.0 + 0.5 * uni(HM), 0.5 * uni(HM)] + lin(HM, HM, 2.0) + lin(m_dim, HM) + lin(Cc * S, K4)
    labels = torch.randint(0, t_dim, (M,), generator=g) if labels is None else torch.as_tensor(labels, dtype=torch.int64)
    case = dict(y_cl=y, m=torch.rand(M, m_dim, generator=g), labels=labels, t=F.one_hot(labels, t_dim).float(), eps=rnd(M, Z),
                params=[p.float().contiguous() for p in params], rm=0.1 * rnd(HM), rv=1.0 + torch.rand(HM, generator=g),
                g_dec=rnd(M, OD, OH, OW, Cc).to(y_dtype), g_mu=rnd(M, Z), g_logvar=rnd(M, Z), g_mhat=rnd(M, m_dim))
    nudge_biases(case, out_size, bn_eps, training=training)
    return case


# ------------------------------------------------------------------------------------------------ ELBO with the exact-2x resize
def elbo_up2x(src_cl, x, m_hat, m, mu, logvar, gamma, g_loss):
    """oracle.functional.cascade_loss(F.interpolate(src, size(x), trilinear | bilinear, align_corners=False), x, m_hat, m, mu, logvar, gamma)
    in float64 and its gradients (w.r.t. src, m_hat, mu, logvar) under the incoming gradient g_loss.  src_cl: [B, d, h, w, 1] channels-last;
    x: [B, 1, D, H, W] or [B, 1, H, W].  Returns (ref, err) with ref keys loss, recon, m_loss, kld, up, dsrc, d_mhat, dmu, dlv."""
    from .functional import cascade_loss
    d64 = lambda v: v.detach().to("cpu", torch.float64)
    nd = x.dim() - 2
    src = d64(src_cl)
    B, d, h, w, _ = src.shape
    src_n = (src.permute(0, 4, 1, 2, 3) if nd == 3 else src[:, 0].permute(0, 3, 1, 2)).clone().requires_grad_(True)
    x, m_hat, m, mu, logvar = d64(x), d64(m_hat).requires_grad_(True), d64(m), d64(mu).requires_grad_(True), d64(logvar).requires_grad_(True)
    mode = "trilinear" if nd == 3 else "bilinear"
    up = F.interpolate(src_n, size=tuple(x.shape[2:]), mode=mode, align_corners=False)
    loss, recon, m_loss, kld = cascade_loss(up, x, m_hat, m, mu, logvar, gamma)
    gs, gmh, gmu, glv = torch.autograd.grad(loss * g_loss, [src_n, m_hat, mu, logvar])
    with torch.no_grad():
        taps = 2 ** nd                                            # source values behind one output of a linear resize
        up_abs = F.interpolate(src_n.detach().abs(), size=tuple(x.shape[2:]), mode=mode, align_corners=False)
        e_up = _ps(taps) * up_abs
        res = (up - x).detach()
        N = x.numel()
        e_recon = _ps(N) * (res * res).sum() + (2 * res.abs() * e_up).sum()
        dm = (m_hat - m).detach()
        e_mloss = _ps(m.numel()) * (dm * dm).sum()
        e_kld = 0.5 * (_ps(mu.numel()) * (1 + logvar.abs() + mu * mu + torch.exp(logvar)).detach().sum()
                       + (4 * U * (1 + logvar.abs()) * torch.exp(logvar)).detach().sum())
        e_loss = e_recon + abs(gamma) * e_mloss + e_kld + 2 * U * (recon.abs() + abs(gamma) * m_loss.abs() + kld.abs()).detach()
        # dsrc = 2 g U^T (up - x): sums of (2^nd taps of the transpose) x (2 outputs per axis of t1), and the error of up itself
        ag = abs(float(g_loss))
        srcg = src_n.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            u2 = F.interpolate(srcg, size=tuple(x.shape[2:]), mode=mode, align_corners=False)
            (ut,) = torch.autograd.grad(u2, srcg, grad_outputs=(res.abs() + e_up + U * (up_abs + x.abs())))
        e_ds = 2 * ag * _ps(4 ** nd) * ut + 2 * U * gs.abs()
        to_cl = (lambda v: v.permute(0, 2, 3, 4, 1)) if nd == 3 else (lambda v: v.permute(0, 2, 3, 1).unsqueeze(1))
        ref = dict(loss=loss.detach(), recon=recon.detach(), m_loss=m_loss.detach(), kld=kld.detach(), dsrc=to_cl(gs).reshape(src.shape), d_mhat=gmh, dmu=gmu, dlv=glv,
                   up=up.detach().reshape(B, -1))
        err = dict(loss=e_loss, recon=e_recon + 2 * U * recon.abs().detach(), m_loss=e_mloss + U * m_loss.abs().detach(), kld=e_kld + U * kld.abs().detach(),
                   dsrc=to_cl(e_ds).reshape(src.shape), d_mhat=4 * U * gmh.abs(), dmu=2 * U * gmu.abs(),
                   dlv=0.5 * ag * (4 * U * (1 + logvar.abs().detach()) * torch.exp(logvar.detach())) + 3 * U * glv.abs(),
                   up=(e_up + U * up_abs).reshape(B, -1))
    return ref, err
