"""A restatement of the reference's CausalViTVAE (vessel_analysis/00_core/models.py:181-307, eval mode) in plain torch ops — the yardstick of
tests/test_causal_vit*.py.  Own code; it reads a state_dict with the reference's keys.  The backbone is tests/vit_reference.py (steps A-D: encode_ref's
`cls_out`) and tests/vit_decoder_reference.py (backbone.decode); what is stated here is the part that is not backbone: the three dense heads, the two
clamps, the reparameterisation, and the composition.

head_b(x, ex, layers, ...)            (value, element-wise bound) of one head on inputs carrying the bound ex (zeros: the local bound of a head tested alone)
forward_ref(sd, x, m, t, eps, depth)  float64 values: cls_out, mu, logvar, z, m_mu, m_logvar, z_vit, recon_x
forward_ref(..., rnd=round_bf16)      the ROUNDING ORACLE of the bf16 backbone (the heads are fp32 in both modes: nothing is rounded in them)
forward_ref(..., probe=_Probe)        one draw of the error model of composed_bound
composed_bound(sd, x, m, t, eps, depth)   name -> bound on ||fp32 evaluation - float64 value||_F, composed as vit_reference.composed_bound composes it

Local fp32 bounds of a head (u = 2^-24; counted from the operations csrc/heads.hip issues, nothing fitted to its output).  A value v carries e >= |computed - v|.
  Linear, K inputs: one fmaf chain of K (rounded up to a multiple of 4: the padding terms are exact zeros) products from 0, then + bias:
        e_y = sum |w| e_x + (K + 2) u (sum |w x| + |b|)                                               (vit_reference.linear_b)
  eval BatchNorm1d, y = fma(v - mean, s, beta), s = gamma * (1 / sqrt(var + eps)): v - mean one rounding, s four (add, sqrt, divide, multiply), the fma one:
        e_y = |s| e_v + 6 u (|v - mean| |s| + |beta|)
  LeakyReLU(slope <= 1): 1-Lipschitz, one rounding of slope * v:   e_y = e_v + u |y|
  clamp: exact and 1-Lipschitz:  e unchanged
  z = fma(eps, exp(0.5 lv), mu): 0.5 lv exact; expf counted as a relative error of 3 u, in the unit of every other line here (an ulp of a value is at most
        2 u of it, so 3 u is 1.5 ulp; the HIP math API documents 1 ulp = 2 u for expf, one u is kept over that figure); the argument's error e_lv / 2
        scales the result by exp(+-e_lv / 2); the fma rounds once:
        e_z = e_mu + |eps| std (expm1(e_lv / 2) + 3 u) + u |z|
"""
import math

import torch
import torch.nn.functional as F

from vit_reference import U32, F64, round_bf16, _Probe, linear_b, encode_ref, fro_ratio, rel_l2, PROBES, SIGMAS, vit_inputs   # noqa: F401
from vit_decoder_reference import decode_ref

Z_DIM, M_DIM, T_DIM = 128, 12, 19
BN_EPS = 1e-5
HEAD_NAMES = ("mu", "logvar", "z", "m_mu", "m_logvar", "z_vit")


def randomize_head_bn(model, seed):
    """non-trivial eval statistics and affine parameters for the two adapters' BatchNorm1d layers, drawn like vit_reference.randomize_stem_bn: gamma in
    [0.5, 1.5], beta ~ 0.1 N(0, 1), running_mean ~ 0.1 N(0, 1), running_var in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in (model.enc_adapter[1], model.dec_adapter[1]):
            n = bn.num_features
            bn.weight.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.copy_(0.1 * torch.randn(n, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(n, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))


def causal_inputs(B, H, W, seed):
    """x as the ViT fixtures draw it; standardised m, one-hot t and the injected eps from a generator of their own"""
    g = torch.Generator().manual_seed(seed + 1)
    m = torch.randn(B, M_DIM, generator=g)
    t = F.one_hot(torch.randint(0, T_DIM, (B,), generator=g), T_DIM).float()
    eps = torch.randn(B, Z_DIM, generator=g)
    return vit_inputs(B, H, W, seed), m, t, eps


def head_b(x, ex, layers, probe=None):
    """layers: [(W, b, bn, slope)], bn = (gamma, beta, mean, var, eps) or None, slope or None.  ex None: values only.  probe: every layer's result is
    displaced by its LOCAL bound times a random sign before the next layer reads it (ex must then be zeros)."""
    e = ex
    for W, b, bn, slope in layers:
        y, e = linear_b(x, e, W, b)
        if bn is not None:
            gam, bet, mean, var, eps = bn
            s = gam / torch.sqrt(var + eps)
            d = y - mean
            y = d * s + bet
            if e is not None:
                e = s.abs() * e + 6 * U32 * (d.abs() * s.abs() + bet.abs())
        if slope is not None:
            y = torch.where(y > 0, y, slope * y)
            if e is not None:
                e = e + U32 * y.abs()
        if probe is not None:
            y, e = probe.at(y, e), torch.zeros_like(y)
        x = y
    return x, e


def clamp_b(y, e, lo, hi):
    return y.clamp(lo, hi), e


def reparam_b(mu, emu, lv, elv, eps):
    std = torch.exp(0.5 * lv)
    z = mu + eps * std
    if emu is None:
        return z, None
    return z, emu + eps.abs() * std * (torch.expm1(0.5 * elv) + 3 * U32) + U32 * z.abs()


def adapter_layers(get, prefix):
    bn = tuple(get(f"{prefix}.1.{n}") for n in ("weight", "bias", "running_mean", "running_var")) + (BN_EPS,)
    return [(get(prefix + ".0.weight"), get(prefix + ".0.bias"), bn, 0.2), (get(prefix + ".3.weight"), get(prefix + ".3.bias"), None, None)]


def morph_layers(get):
    """the last layer as the stacked [mu | logvar] weight: the same sums, column by column"""
    W = torch.cat([get("morph_predictor_mu.weight"), get("morph_predictor_logvar.weight")], 0)
    b = torch.cat([get("morph_predictor_mu.bias"), get("morph_predictor_logvar.bias")], 0)
    return [(get("morph_predictor_shared.0.weight"), get("morph_predictor_shared.0.bias"), None, 0.2),
            (get("morph_predictor_shared.2.weight"), get("morph_predictor_shared.2.bias"), None, 0.2), (W, b, None, None)]


def backbone_sd(sd):
    return {k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}


def heads_ref(sd, cls_out, m, t, eps, dtype=F64, probe=None, want_bound=False):
    """Everything between backbone.cls_features and backbone.decode.  Returns (values, bounds): dicts over HEAD_NAMES; bounds (want_bound, no probe) are the
    element-wise bounds of each head run on EXACT inputs (z_vit's: dec_adapter on the exact z — an element-wise worst case multiplies by sum |w| at
    every layer, so across chained heads only composed_bound's model says anything)."""
    get = lambda k: sd[k].to(device=cls_out.device, dtype=dtype)
    zero = lambda v: torch.zeros_like(v) if (want_bound or probe is not None) else None
    hit = lambda v, e: probe.at(v, e) if probe is not None else v
    m, t, eps = m.to(cls_out), t.to(cls_out), eps.to(cls_out)
    xin = torch.cat([cls_out, m, t], 1)
    h, e = head_b(xin, zero(xin), adapter_layers(get, "enc_adapter"), probe)
    mu, emu = clamp_b(h[:, :Z_DIM], None if e is None else e[:, :Z_DIM], -100.0, 100.0)
    lv, elv = clamp_b(h[:, Z_DIM:], None if e is None else e[:, Z_DIM:], -10.0, 10.0)
    z, ez = reparam_b(mu, emu, lv, elv, eps)
    z = hit(z, ez)
    hm, em = head_b(t, zero(t), morph_layers(get), probe)
    m_mu, m_lv = hm[:, :M_DIM], hm[:, M_DIM:].clamp(-10.0, 10.0)
    din = torch.cat([m, z], 1)
    z_vit, ev = head_b(din, zero(din), adapter_layers(get, "dec_adapter"), probe)
    vals = dict(mu=mu, logvar=lv, z=z, m_mu=m_mu, m_logvar=m_lv, z_vit=z_vit)
    bounds = None
    if want_bound and probe is None:
        bounds = dict(mu=emu, logvar=elv, z=ez, m_mu=em[:, :M_DIM], m_logvar=em[:, M_DIM:], z_vit=ev)
    return vals, bounds


def forward_ref(sd, x, m, t, eps, depth, dtype=F64, rnd=None, probe=None, decode=True, crop=None):
    """The whole model.  crop (y0, y1, x0, x1): also `recon_crop` = recon_x[:, :, y0:y1, x0:x1] (the part of the image a fixture keeps whole).  rnd: bf16 rounding where the bf16 backbone rounds (its last block then runs for the CLS row alone, as the kernels do); the heads
    round nothing."""
    bsd = backbone_sd(sd)
    enc = encode_ref(bsd, x, depth, dtype=dtype, rnd=rnd, cls_only_last=rnd is not None, probe=probe)
    out = {"cls_out": enc["cls_out"]}
    vals, _ = heads_ref(sd, enc["cls_out"], m, t, eps, dtype=dtype, probe=probe)
    out.update(vals)
    if decode:
        grid = (x.shape[2] // 32, x.shape[3] // 32)
        out["recon_x"] = decode_ref(bsd, out["z_vit"], grid, dtype=dtype, rnd=rnd, probe=probe)["image"]
        if crop is not None:
            out["recon_crop"] = out["recon_x"][:, :, crop[0]:crop[1], crop[2]:crop[3]]
    return out


_BOUNDS = {}


def composed_bound(sd, x, m, t, eps, depth, key=None, decode=True, crop=None):
    """name -> a bound on the Frobenius norm ||fp32 evaluation - float64 value|| of cls_out, the six head outputs and recon_x: the encoder's composed bound
    carried through the adapters, and the decoder's composed bound with the z_vit error as its input error — one error model for the whole chain, the one of
    vit_reference.composed_bound (its docstring): a float64 pass in which every stage (every backbone stage, every head layer, z) is displaced by its LOCAL
    worst-case bound times a random sign, SIGMAS = 3 times the root mean square distance from the plain pass over PROBES = 4 draws.  Returns (bounds, plain)."""
    if key is not None and key in _BOUNDS:
        return _BOUNDS[key]
    plain = forward_ref(sd, x, m, t, eps, depth, decode=decode, crop=crop)
    sq = {k: 0.0 for k in plain}
    for s in range(PROBES):
        got = forward_ref(sd, x, m, t, eps, depth, probe=_Probe(9200 + s), decode=decode, crop=crop)
        for k in plain:
            sq[k] += float((got[k] - plain[k]).norm()) ** 2
    res = ({k: SIGMAS * math.sqrt(v / PROBES) for k, v in sq.items()}, plain)
    if key is not None:
        _BOUNDS[key] = res
    return res
