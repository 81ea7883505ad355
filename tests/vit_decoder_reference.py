"""A restatement of the reference's ViTVAE.decode (vessel_analysis/00_core/vit_backbone.py:7-19, 115-156, 186-193, eval mode) in plain torch ops — the
yardstick of tests/test_vit_decoder*.py, in the style of tests/vit_reference.py.  Own code; it reads a state_dict with the reference's keys.

decode_ref(sd, z, grid)                      float64 values: `grid` (decoder_input viewed [B, 256, gh, gw]), `stage0..7` (NCHW, after each of the 5 transposed
                                             convs and 3 ResBlocks in execution order), `image`
decode_ref(..., rnd=round_bf16)              the ROUNDING ORACLE: float64 with bf16 rounding where the bf16 kernels round: decoder_input's output, every folded
                                             conv weight (the output conv's plain weight), every activation between layers (a ResBlock's inner one included);
                                             z, decoder_input's weight, every bias, the residual sum before its rounding and the image stay unrounded
decode_ref(..., probe=_Probe)                one draw of the error model of composed_bound
decode_ref(..., mutate=...)                  deliberately wrong decoders for the bound-sanity test
decode_ref(..., dtype=torch.float32 / torch.bfloat16)   the same ops run eagerly in that dtype on z's device (the timing baseline of tools/vit_decode_probe.py)

Local fp32 bounds (u = 2^-24; nothing fitted to a kernel's output; a kernel tested alone has exact inputs, so only these remain):
  decoder_input   K = latent_dim products + bias:                                    (K + 2) u (sum |w z| + |b|)
  folded conv     c = accumulation length + 5 (fold of weight and bias: 3, bias add, activation), times u sum |w x| + |b|, with the accumulation length
                  the number of products the KERNEL issues per output: 16 Cin for the zero-embedded k4 form (as the stem), 9 Cin (rounded up to the next
                  multiple of 64) for the 3 x 3 window, 4 Cin (the same) for the sub-pixel form, 144 for the output conv
  residual add    one more rounding: u |x + y|
LeakyReLU is 1-Lipschitz and exact up to one rounding of slope * v (inside the + 5).
bf16 kernels against float64 ON ROUNDED OPERANDS: products of bf16 values are exact in fp32 and accumulation is fp32, so the same local terms hold; a
bf16 result adds its own rounding 2^-8 |y|."""
import math

import torch
import torch.nn.functional as F

from vit_reference import U32, UBF, F64, round_bf16, _Probe, fro_ratio, rel_l2, PROBES, SIGMAS   # noqa: F401

DEC_CHANNELS = (128, 64, 32, 16, 16)
# (kind, decoder index): execution order of the 8 stages
STAGES = (("up", 0), ("res", 3), ("up", 4), ("res", 7), ("up", 8), ("res", 11), ("up", 12), ("up", 15))
OUT_CONV = 18
BN_EPS = 1e-5


def decoder_batchnorms(decoder):
    """every BatchNorm2d of the decoder in module order, the ones nested in the ResBlocks included"""
    return [m for m in decoder.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def randomize_decoder_bn(decoder, seed):
    """non-trivial eval statistics and affine parameters for ALL decoder BatchNorm2d layers (11: 5 after the transposed convs, 2 in each ResBlock), drawn
    like vit_reference.randomize_stem_bn: gamma in [0.5, 1.5], beta ~ 0.1 N(0, 1), running_mean ~ 0.1 N(0, 1), running_var in [0.5, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in decoder_batchnorms(decoder):
            n = bn.num_features
            bn.weight.copy_(0.5 + torch.rand(n, generator=g))
            bn.bias.copy_(0.1 * torch.randn(n, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(n, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(n, generator=g))


def dec_inputs(B, latent_dim, seed):
    return torch.randn(B, latent_dim, generator=torch.Generator().manual_seed(seed))


def fold(sd_get, conv_key, bn_key, transposed, mutate=None):
    """(folded weight, folded bias) of a conv + eval BatchNorm2d pair, in the conv's own layout"""
    w, b = sd_get(conv_key + ".weight"), sd_get(conv_key + ".bias")
    gam, bet, mean, var = (sd_get(f"{bn_key}.{n}") for n in ("weight", "bias", "running_mean", "running_var"))
    s = gam / torch.sqrt(var + BN_EPS)
    if mutate == "bn_mean" :
        mean = torch.zeros_like(mean)
    wf = w * (s[None, :, None, None] if transposed else s[:, None, None, None])
    return wf, (b - mean) * s + bet


def kernel_terms(kind, cin):
    """products the kernel issues per output element (the accumulation length of the local bound)"""
    pad = lambda k: (k + 63) // 64 * 64
    return {"up": 16 * cin if cin >= 64 else pad(4 * cin), "res": pad(9 * cin), "out": 144}[kind]


def conv_b(x, w, b, transposed, c_len, want_bound):
    """(y, local bound or None) of one folded conv on exact inputs"""
    if transposed:
        op = lambda t, ww, bb: F.conv_transpose2d(t, ww, bb, stride=2, padding=1, output_padding=1)
    else:
        op = lambda t, ww, bb: F.conv2d(t, ww, bb, stride=1, padding=1)
    y = op(x, w, b)
    e = (c_len + 5) * U32 * op(x.abs(), w.abs(), b.abs()) if want_bound else None
    return y, e


def decode_ref(sd, z, grid, dtype=F64, rnd=None, probe=None, mutate=None):
    """mutate: None | "no_residual" | "slope" (0.01 where the ResBlocks' 0.2 belongs) | "shift" (output_padding applied at the top / left: the transposed
    convs' result moved by one pixel) | "bn_mean" (running means not folded)."""
    gh, gw = grid
    get = lambda k: sd[k].to(device=z.device, dtype=dtype)
    r = rnd if rnd is not None else (lambda t: t)
    hit = lambda v, e: probe.at(v, e) if probe is not None else v
    want = probe is not None
    zz = z.to(dtype)
    W, b = get("decoder_input.weight"), get("decoder_input.bias")
    h = zz @ W.T + b
    if want:
        h = probe.at(h, (W.shape[1] + 2) * U32 * (zz.abs() @ W.abs().T + b.abs()))
    h = r(h).view(-1, 256, gh, gw)
    out = {"grid": h}
    for i, (kind, idx) in enumerate(STAGES):
        if kind == "up":
            wf, bf = fold(get, f"decoder.{idx}", f"decoder.{idx + 1}", True, mutate)
            y, e = conv_b(h, r(wf), bf, True, kernel_terms("up", wf.shape[0]), want)
            if mutate == "shift":
                y = torch.roll(y, shifts=(1, 1), dims=(2, 3))
            h = r(F.leaky_relu(hit(y, e), 0.01))
        else:
            p = f"decoder.{idx}.conv"
            w1, b1 = fold(get, p + ".0", p + ".1", False, mutate)
            w2, b2 = fold(get, p + ".3", p + ".4", False, mutate)
            c = kernel_terms("res", w1.shape[1])
            y, e = conv_b(h, r(w1), b1, False, c, want)
            y = r(F.leaky_relu(hit(y, e), 0.01 if mutate == "slope" else 0.2))
            y2, e2 = conv_b(y, r(w2), b2, False, c, want)
            s = y2 if mutate == "no_residual" else h + y2
            h = r(hit(s, (e2 + U32 * s.abs()) if want else None))
        out[f"stage{i}"] = h
    w, b = get(f"decoder.{OUT_CONV}.weight"), get(f"decoder.{OUT_CONV}.bias")
    y, e = conv_b(h, r(w), b, False, kernel_terms("out", 16), want)
    out["image"] = hit(y, e)
    return out


_BOUNDS = {}


def composed_bound(sd, z, grid, key=None):
    """name -> a bound on the Frobenius norm ||fp32 evaluation - float64 value|| of every stage and the image, composed exactly as
    vit_reference.composed_bound composes the encoder's (its docstring): every stage displaced by its LOCAL worst-case bound times a random sign in a
    float64 pass (the actual Jacobian action of the rest of the decoder), independent signs, SIGMAS = 3 times the root mean square over PROBES = 4 draws.
    A worst case over signs would multiply by sum |w| (about 30 x the signal gain at default init) at each of the 12 layers."""
    if key is not None and key in _BOUNDS:
        return _BOUNDS[key]
    plain = decode_ref(sd, z, grid)
    sq = {k: 0.0 for k in plain}
    for s in range(PROBES):
        got = decode_ref(sd, z, grid, probe=_Probe(9100 + s))
        for k in plain:
            sq[k] += float((got[k] - plain[k]).norm()) ** 2
    res = ({k: SIGMAS * math.sqrt(v / PROBES) for k, v in sq.items()}, plain)
    if key is not None:
        _BOUNDS[key] = res
    return res
