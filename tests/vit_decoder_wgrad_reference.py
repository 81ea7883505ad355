"""The vector-Jacobian product of the eval-mode ViT-VAE decoder with respect to its PARAMETERS, restated in plain torch ops on vit_decoder_reference's
folding — the yardstick of tests/test_vit_decoder_wgrad*.py.  Own code.

Regime: BatchNorm2d on its running statistics (constants); its weight and bias, and every conv weight and bias, are the variables.  The LeakyReLU masks
are ARGUMENTS, for the reason tests/vit_decoder_grad_reference.py gives: with the masks fixed the decoder is the product of linear maps
y -> y * where(mask, 1, slope), and it is that map's weight VJP the kernels are held to (with float64's own masks it IS the decoder: leaky(y) = y * factor).

decoder_wgrad_ref(sd, z, g_img, grid, masks)         name -> float64 gradient of sum(image * g_img), for all 48 decoder parameters (state_dict names)
decoder_wgrad_ref(..., dtype=torch.float32)          the same ops in fp32 on the CPU: an independent fp32 evaluation, the fp32 yardstick
decoder_wgrad_ref(..., rnd=round_bf16)               the ROUNDING ORACLE: bf16 rounding where the bf16 kernels round: decoder_input's output, every folded weight the
                                                     data path multiplies with (the output conv's plain weight), every activation and every gradient a kernel writes
                                                     between layers; z, the cotangent, every bias and every weight GRADIENT stay unrounded (they are fp32 on the
                                                     device), and the fold's way back reads the unrounded fp32 parameters
decoder_wgrad_ref(..., mutate="no_swap" | "no_bias_term")   deliberately wrong restatements for the bound-sanity test: the gradient of the 16 -> 16 transposed conv
                                                     left in [Cout][Cin] order; dgamma without the dbf (b - running_mean) term

fold_backward_ref(w, b, gamma, mean, var, dwf, dbf, transposed)   the way back through the fold alone: (dw, db, dgamma, dbeta)

Element-wise fp32 bounds of the kernels tested alone (u = 2^-24, counted from the kernels' operations, nothing fitted; inputs exact, bf16 operands bf16-exact so
their products are exact in fp32 and only the sums round):
  conv_s1_wgrad        an element is the sum of n = B H W products (fp32: each fused into the sum by the MFMA) in some fixed order — tile by tile inside a
                       workgroup, then over the slabs: any order of n terms errs by at most (n - 1) u sum|terms|, the fp32 products add one rounding each:
                       (n + 1) u sum |g x|; dbias: n u sum |g|
  conv_s1_c1_wgrad     the same with fmaf chains, the workgroup tree and the workgroup sum: (n + 1) u sum |g x|; dbias n u sum |g|
  latent_to_grid_wgrad B fmaf steps in row order: (B + 1) u sum_b |g z|; dbias B u sum |g|
Whole decoder: per parameter tensor, rel-L2 against float64 at most 4 x that of the fp32 CPU evaluation (fp32), at most 2 x the rounding-oracle gap (bf16): the
project's rules for dz (tests/test_vit_decoder_grad.py)."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import vit_decoder_reference as dr
from vit_decoder_reference import F64, STAGES, OUT_CONV, BN_EPS
from vit_decoder_grad_reference import GATES, factor

BN_NAMES = ("weight", "bias", "running_mean", "running_var")


def fold_backward_ref(w, b, gamma, mean, var, dwf, dbf, transposed, mutate=None):
    """(dw, db, dgamma, dbeta) from the gradient of the folded weight (in w's layout) and bias; s = gamma rstd per BatchNorm channel (dimension 1 of a
    transposed conv's weight, else dimension 0)"""
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    s = gamma * rstd
    shape = (1, -1, 1, 1) if transposed else (-1, 1, 1, 1)
    other = (0, 2, 3) if transposed else (1, 2, 3)
    inner = (dwf * w).sum(other)
    if mutate != "no_bias_term":
        inner = inner + dbf * (b - mean)
    return dwf * s.view(shape), dbf * s, rstd * inner, dbf


def decoder_wgrad_ref(sd, z, g_img, grid, masks, dtype=F64, rnd=None, mutate=None):
    gh, gw = grid
    get = lambda k: sd[k].detach().to(dtype)
    r = rnd if rnd is not None else (lambda t: t)
    fac = lambda name, slope: factor(masks[name], slope, dtype)
    zz = z.detach().to(dtype)
    W, b = get("decoder_input.weight"), get("decoder_input.bias")
    h = r(zz @ W.T + b).view(-1, 256, gh, gw)
    tape, n_res = [], 0
    for i, (kind, idx) in enumerate(STAGES):                            # the fixed-mask forward, keeping every layer's input
        if kind == "up":
            wf, bf = dr.fold(get, f"decoder.{idx}", f"decoder.{idx + 1}", True)
            tape.append((h, None, wf))
            h = r(F.conv_transpose2d(h, r(wf), bf, stride=2, padding=1, output_padding=1) * fac(f"stage{i}", 0.01))
        else:
            p = f"decoder.{idx}.conv"
            w1, b1 = dr.fold(get, p + ".0", p + ".1", False)
            w2, b2 = dr.fold(get, p + ".3", p + ".4", False)
            y = r(F.conv2d(h, r(w1), b1, padding=1) * fac(f"inner{n_res}", 0.2))
            tape.append((h, y, (w1, w2)))
            h = r(h + F.conv2d(y, r(w2), b2, padding=1))
            n_res += 1
    out = {}

    def unfold(conv_key, bn_key, transposed, dwf, dbf):
        gam, _bet, mean, var = (get(f"{bn_key}.{n}") for n in BN_NAMES)
        dw, db, dgam, dbet = fold_backward_ref(get(conv_key + ".weight"), get(conv_key + ".bias"), gam, mean, var, dwf, dbf, transposed, mutate)
        out[conv_key + ".weight"], out[conv_key + ".bias"], out[bn_key + ".weight"], out[bn_key + ".bias"] = dw, db, dgam, dbet

    g = g_img.to(dtype)
    wo = get(f"decoder.{OUT_CONV}.weight")
    out[f"decoder.{OUT_CONV}.weight"] = conv2d_weight(h, wo.shape, g, padding=1)
    out[f"decoder.{OUT_CONV}.bias"] = g.sum().view(1)
    g = r(F.conv_transpose2d(g, r(wo), padding=1) * fac("stage7", 0.01))
    for i in range(len(STAGES) - 1, -1, -1):
        kind, idx = STAGES[i]
        gate = fac(f"stage{i - 1}", 0.01) if (i - 1) in GATES else None
        x, y, ws = tape[i]
        if kind == "up":
            # convT(x, w) is the adjoint of conv2d(., w, stride 2): <convT(x, w), g> = <x, conv2d(g, w)>, so d/dw is conv2d's weight gradient with g as the input
            dwf = conv2d_weight(g, ws.shape, x, stride=2, padding=1)
            if mutate == "no_swap" and ws.shape[0] == ws.shape[1]:
                dwf = dwf.transpose(0, 1).contiguous()
            unfold(f"decoder.{idx}", f"decoder.{idx + 1}", True, dwf, g.sum((0, 2, 3)))
            g = F.conv2d(g, r(ws), stride=2, padding=1)
        else:
            n_res -= 1
            p = f"decoder.{idx}.conv"
            w1, w2 = ws
            unfold(p + ".3", p + ".4", False, conv2d_weight(y, w2.shape, g, padding=1), g.sum((0, 2, 3)))
            t = r(F.conv_transpose2d(g, r(w2), padding=1) * fac(f"inner{n_res}", 0.2))
            unfold(p + ".0", p + ".1", False, conv2d_weight(x, w1.shape, t, padding=1), t.sum((0, 2, 3)))
            g = F.conv_transpose2d(t, r(w1), padding=1) + g
        if gate is not None:
            g = g * gate
        g = r(g)
    G = g.reshape(g.shape[0], -1)
    out["decoder_input.weight"] = G.T @ zz
    out["decoder_input.bias"] = G.sum(0)
    return out


def decoder_param_names(sd):
    """the 48 decoder parameters (no running statistics, no counters) in state_dict order"""
    return [k for k in sd if k.startswith(("decoder_input.", "decoder.")) and not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
