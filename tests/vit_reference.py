"""A restatement of the reference's ViTVAE.encode (vessel_analysis/00_core/vit_backbone.py:158-179, eval mode) in plain torch ops, with attention written
out as softmax(Q K^T / sqrt(d)) V — the yardstick of tests/test_vit_*.py, in the style of oracle/conv64.py.  Own code; it reads a state_dict with the
reference's keys and nothing else.

encode_ref(sd, x, depth)                     float64 values of every stage
composed_bound(sd, x, depth)                 the per-layer fp32 bounds composed over depth: a bound on ||fp32 evaluation - float64 value|| per stage
encode_ref(..., rnd=round_bf16)              the ROUNDING ORACLE: float64 arithmetic with operands rounded to bf16 exactly where the bf16 kernels round
                                             (folded stem weights and stem activations, LayerNorm output, GEMM weights, QKV, P, attention output, MLP hidden)
encode_ref(..., dtype=torch.float32 / torch.bfloat16)   the same ops run eagerly in that dtype on x's device (the timing baseline of tools/vit_encode_probe.py)

How the fp32 bound is derived (u = 2^-24; nothing here is fitted to a kernel's output).  A value v carries e >= |computed - v|.
  dot product of K terms + bias, any summation order:   e_y = sum |w| e_x + (K + 2) u (sum |w x| + |b|)            (gamma_K of Higham, first order)
  stem conv: the same with K = 16 Cin (the k4 form issues 16 taps) + 3 more for the fp32 BatchNorm fold of the weight and bias; LeakyReLU is 1-Lipschitz
  LayerNorm(256), y = g xhat + b, xhat = (x - mean) rstd:  a perturbation dx moves xhat by rstd (dx - mean(dx) - xhat mean(xhat dx)), so
        e_xhat = rstd (e_x + mean e_x + |xhat| mean(|xhat| e_x)) + rstd (258 u mean|x| + u |x - mean|) + 140 u |xhat|   (mean: 256-term sum; var: 256 + 3
        roundings, halved by the square root), e_y = |g| e_xhat + 3 u (|g xhat| + |b|)
  attention: scores s = q.k / sqrt(32): bilinear, e_s = (e_q|k| + |q|e_k + e_q e_k + 35 u |q||k|) / sqrt(32) + 4 u (|s| + |max s|) (the exp2 argument);
        p = softmax(s): dp/p = ds_j - sum_k p_k ds_k, so e_p = p (e_s + sum p e_s + (N + N/32 + 12) u) (row sum of N terms, one rescale per 32-key tile,
        exp2 and the division a few ulp); o = p v: e_o = e_p |v| + p e_v + (N + N/32 + 8) u p|v|
  GELU (erf): |gelu'| <= 1.13: e_y = 1.13 e_x + 8 u (|y| + |x|) (erff is a few ulp of a value <= 1, multiplied by x / 2)
  residual add: e = e_a + e_b + u |a + b|
These element-wise propagations serve a kernel tested alone.  Over the whole model the composition is composed_bound's (its docstring): element-wise
worst cases multiply by sum |w| at every layer and are useless after two blocks.  For a kernel tested alone the inputs are exact (e = 0) and only the local term remains: c u sum|terms| with c the accumulation length.
bf16 kernels against float64 ON ROUNDED OPERANDS: products of bf16 values are exact in fp32 and accumulation is fp32, so the same local terms hold;
a bf16 result adds its own rounding 2^-8 |y|; attention adds 2 x 2^-8 p|v| for P (kernel and reference both round P once, at different scales)."""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
UBF = 2.0 ** -8           # bf16: 8 significant bits, round to nearest
F64 = torch.float64
STEM_CIN = (1, 32, 64, 128, 256)


def round_bf16(t):
    return t.float().bfloat16().to(t.dtype)


def vit_inputs(B, H, W, seed):
    """binary sparse vessel-like images, as the other vessel fixtures use"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, H, W, generator=g) < 0.08).float()


def randomize_stem_bn(stem, seed):
    """non-trivial eval statistics and affine parameters for the five stem BatchNorm2d layers (a fresh module would fold to the identity): gamma in
    [0.5, 1.5], beta ~ 0.1 N(0, 1), running_mean ~ 0.1 N(0, 1), running_var in [0.5, 1.5] (far above eps)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i in range(1, 15, 3):
            bn = stem[i]
            n = bn.num_features
            bn.weight.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.copy_(0.1 * torch.randn(n, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(n, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))


# ---- stage functions: (value, bound) -> (value, bound); bound tensors are None when not asked for ---------------------------------------
def linear_b(x, ex, W, b, out_u=0.0):
    y = x @ W.T + b
    if ex is None:
        return y, None
    K = W.shape[1]
    e = ex @ W.abs().T + (K + 2) * U32 * (x.abs() @ W.abs().T + b.abs())
    return y, e + out_u * (y.abs() + e)


def layernorm_b(x, ex, g, b, eps, out_u=0.0):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xhat = d * rstd
    y = xhat * g + b
    if ex is None:
        return y, None
    exh = rstd * (ex + ex.mean(-1, keepdim=True) + xhat.abs() * (xhat.abs() * ex).mean(-1, keepdim=True))
    exh = exh + rstd * (258 * U32 * x.abs().mean(-1, keepdim=True) + U32 * d.abs()) + 140 * U32 * xhat.abs()
    e = g.abs() * exh + 3 * U32 * ((xhat * g).abs() + b.abs())
    return y, e + out_u * (y.abs() + e)


def gelu_b(x, ex, out_u=0.0):
    y = 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    if ex is None:
        return y, None
    e = 1.13 * ex + 8 * U32 * (y.abs() + x.abs())
    return y, e + out_u * (y.abs() + e)


def attention_b(q, eq, k, ek, v, ev, n_query_rows=None, rnd=None, p_u=0.0, out_u=0.0, heads=8):
    """q, k, v [B, N, 256] -> [B, nq, 256].  rnd: P (the unnormalised exp(s - max)) is rounded for the P V product, its row sum is not — as the kernel."""
    B, N, D = k.shape
    nq = N if n_query_rows is None else n_query_rows
    hd = D // heads
    sp = lambda t, n: t[:, :n].reshape(B, n, heads, hd).transpose(1, 2)
    qh, kh, vh = sp(q, nq), sp(k, N), sp(v, N)
    scale = 1.0 / math.sqrt(hd)
    s = (qh @ kh.transpose(-1, -2)) * scale
    mx = s.amax(-1, keepdim=True)
    pu = torch.exp(s - mx)
    l = pu.sum(-1, keepdim=True)
    o = ((rnd(pu) if rnd is not None else pu) @ vh) / l
    merge = lambda t: t.transpose(1, 2).reshape(B, nq, D)
    if eq is None:
        return merge(o), None
    eqh, ekh, evh = sp(eq, nq), sp(ek, N), sp(ev, N)
    es = (eqh @ kh.abs().transpose(-1, -2) + qh.abs() @ ekh.transpose(-1, -2) + eqh @ ekh.transpose(-1, -2)
          + (hd + 3) * U32 * (qh.abs() @ kh.abs().transpose(-1, -2))) * scale + 4 * U32 * (s.abs() + mx.abs())
    p = pu / l
    ep = p * (es + (p * es).sum(-1, keepdim=True) + (N + N / 32 + 12) * U32)
    pav = p @ vh.abs()
    eo = ep @ vh.abs() + p @ evh + (N + N / 32 + 8) * U32 * pav + 2 * p_u * pav
    eo = eo + out_u * (o.abs() + eo)
    return merge(o), merge(eo)


def stem_layer_b(h, eh, sd, i, get, rnd=None, out_u=0.0, pre_act=False):
    """Conv2d(k3, s2, p1) + eval BatchNorm2d + LeakyReLU(0.01) of stem layer i on NCHW.  rnd: the folded form the kernels run, operands rounded."""
    c, b = 3 * i, 3 * i + 1
    w, bias = get(f"stem.{c}.weight"), get(f"stem.{c}.bias")
    gam, bet, mean, var = (get(f"stem.{b}.{n}") for n in ("weight", "bias", "running_mean", "running_var"))
    if rnd is None and eh is None:
        y = F.conv2d(h, w, bias, stride=2, padding=1)
        y = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-5) * gam[None, :, None, None] + bet[None, :, None, None]
        return F.leaky_relu(y, 0.01), None
    s = gam / torch.sqrt(var + 1e-5)
    wf, bf = w * s[:, None, None, None], (bias - mean) * s + bet
    r = rnd if rnd is not None else (lambda t: t)
    y = F.conv2d(r(h), r(wf), bf, stride=2, padding=1)
    e = None
    if eh is not None:
        K = 16 * w.shape[1] + 5
        e = F.conv2d(eh, wf.abs(), None, stride=2, padding=1) + K * U32 * (F.conv2d(h.abs(), wf.abs(), bf.abs(), stride=2, padding=1))
        e = e + out_u * (y.abs() + e)
    if pre_act:
        return y, e
    return r(F.leaky_relu(y, 0.01)), e


class _Probe:
    """One draw of the rounding-error model of composed_bound: `at(v, e)` returns v + e * sigma with independent random signs sigma."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def at(self, v, e):
        sign = torch.randint(0, 2, v.shape, generator=self.g, dtype=torch.int8).to(v.dtype) * 2 - 1
        return v + e * sign


def encode_ref(sd, x, depth, dtype=F64, rnd=None, cls_only_last=False, probe=None):
    """Returns a dict: stem [B, 256, h, w], tokens (list: the stream after every block), cls_rows (list: its CLS row), cls_out, mu, log_var.
    probe (a _Probe, float64 without rounding only): every stage's result is displaced by its LOCAL fp32 bound (the element-wise terms of the module
    docstring with exact inputs) times a random sign before the next stage reads it — see composed_bound."""
    get = lambda k: sd[k].to(device=x.device, dtype=dtype)
    r = rnd if rnd is not None else (lambda t: t)
    zero = lambda v: torch.zeros_like(v) if probe is not None else None
    hit = lambda v, e: probe.at(v, e) if probe is not None else v
    h = x.to(dtype)
    B = h.shape[0]
    for i in range(5):
        if probe is None:
            h, _ = stem_layer_b(h, None, sd, i, get, rnd)
        else:
            y, e = stem_layer_b(h, zero(h), sd, i, get, pre_act=True)
            h = F.leaky_relu(probe.at(y, e), 0.01)
    out = {"stem": h, "tokens": [], "cls_rows": []}
    t = h.flatten(2).transpose(1, 2)
    t = torch.cat([get("cls_token").expand(B, -1, -1), t], dim=1) + get("pos_embedding")[:, :t.shape[1] + 1]
    t = hit(t, U32 * t.abs())

    def lin(v, W, b):
        y, e = linear_b(v, zero(v), W, b)
        return hit(y, e)

    def ln(v, g, b):
        y, e = layernorm_b(v, zero(v), g, b, 1e-5)
        return hit(y, e)

    for i in range(depth):
        p = f"transformer.{i}."
        nq = 1 if (cls_only_last and i == depth - 1) else None
        y = r(ln(t, get(p + "norm1.weight"), get(p + "norm1.bias")))
        qkv = r(lin(y, r(get(p + "attn.in_proj_weight")), get(p + "attn.in_proj_bias")))
        q, k, v = qkv.split(256, dim=-1)
        a, e = attention_b(q, zero(q), k, zero(k), v, zero(v), n_query_rows=nq, rnd=rnd)
        a = r(hit(a, e))
        o = lin(a, r(get(p + "attn.out_proj.weight")), get(p + "attn.out_proj.bias"))
        if nq is not None:
            t = t[:, :1]
        t = t + o
        t = hit(t, U32 * t.abs())
        y = ln(t, get(p + "norm2.weight"), get(p + "norm2.bias"))
        pre = lin(r(y), r(get(p + "mlp.0.weight")), get(p + "mlp.0.bias"))
        hdn, e = gelu_b(pre, zero(pre))
        o = lin(r(hit(hdn, e)), r(get(p + "mlp.3.weight")), get(p + "mlp.3.bias"))
        t = t + o
        t = hit(t, U32 * t.abs())
        out["tokens"].append(t)
        out["cls_rows"].append(t[:, 0])
    c = ln(t[:, 0], get("to_latent.weight"), get("to_latent.bias"))
    out["cls_out"] = c
    out["mu"] = lin(c, get("fc_mu.weight"), get("fc_mu.bias"))
    out["log_var"] = lin(c, get("fc_var.weight"), get("fc_var.bias"))
    return out


def flat(out, depth):
    """the stages of an encode_ref result by the names the goldens use"""
    d = {"stem": out["stem"], "cls_out": out["cls_out"], "mu": out["mu"], "log_var": out["log_var"]}
    for i in range(depth):
        d[f"tokens{i}"], d[f"cls_row{i}"] = out["tokens"][i], out["cls_rows"][i]
    return d


PROBES, SIGMAS = 4, 3.0
_BOUNDS = {}


def composed_bound(sd, x, depth, key=None):
    """The per-layer fp32 bounds composed over depth: name -> a bound on the Frobenius norm ||fp32 evaluation - float64 value|| of that stage.

    Composition.  To first order the error of a stage's fp32 result is  sum over the stages s up to it of  J_s eps_s,  with eps_s the rounding error
    stage s commits on exact inputs, |eps_s| <= e_s element-wise (e_s = the local bound c u sum|terms| of the module docstring), and J_s the Jacobian of
    the rest of the network at the float64 point.  The worst case over the signs of eps_s needs |J_s| and multiplies by sum |w| at every layer (it
    reaches 1e14 after two blocks, overflow after six): it guards nothing.  Rounding errors are not adversarial; the model used is the one behind
    probabilistic error analysis (Higham & Mary 2019): independent signs — but with every magnitude AT its worst-case local bound e_s, which alone
    over-states a K-term sum's typical error by about sqrt(K).  One draw of that model is one float64 forward pass in which every stage's result is
    displaced by e_s sigma_s, sigma_s = +-1 at random (encode_ref(probe=...)): its distance from the plain pass is sum_s J_s (e_s sigma_s) — the actual
    Jacobian action, up to second order (relative 1e-6 here).  The bound is SIGMAS = 3 times the root mean square of that distance over PROBES = 4
    draws.  Nothing in it comes from a kernel's output.  key: cache the result under this name (one goldens case)."""
    if key is not None and key in _BOUNDS:
        return _BOUNDS[key]
    plain = flat(encode_ref(sd, x, depth), depth)
    sq = {k: 0.0 for k in plain}
    for s in range(PROBES):
        got = flat(encode_ref(sd, x, depth, probe=_Probe(9000 + s)), depth)
        for k in plain:
            sq[k] += float((got[k] - plain[k]).norm()) ** 2
    res = ({k: SIGMAS * math.sqrt(v / PROBES) for k, v in sq.items()}, plain)
    if key is not None:
        _BOUNDS[key] = res
    return res


def fro_ratio(got, ref, bound):
    return float((got.detach().cpu().double() - ref).norm()) / bound


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm())
