"""The vector-Jacobian product of the eval-mode ViT-VAE decoder with respect to its latent, restated in plain torch ops on vit_decoder_reference's folding —
the yardstick of tests/test_vit_decoder_grad*.py.  Own code.

The LeakyReLU masks are ARGUMENTS.  With the masks fixed the map cotangent -> dz is linear, and it is that linear map the kernels are held to: an fp32
and a float64 forward disagree on the sign of a pre-activation that lies within rounding of zero, one such flip changes that element's factor from 1 to
0.01 (99 %), and over the 15.7 M elements of the last stage those flips outweigh rounding error by orders of magnitude.  The GPU tests therefore pass the
masks of the HIP forward's own activations (which tests/test_vit_decoder.py pins to float64) and, separately, check where those masks may differ from
float64's (test_hip_masks_differ_from_float64_only_within_the_bound).

masks: {"stage0", "stage2", "stage4", "stage6", "stage7", "inner0", "inner1", "inner2"} -> bool NCHW tensors (activation output > 0: LeakyReLU keeps the
sign, and torch's rule is x > 0 ? 1 : slope).  Every LeakyReLU derivative is a multiply by where(mask, 1, slope).

decode_vjp_ref(sd, g_img, grid, masks)                 float64 dz [B, latent]
decode_vjp_ref(..., dtype=torch.float32)               the same ops in fp32 on the CPU: an independent fp32 evaluation, the fp32 yardstick
decode_vjp_ref(..., rnd=round_bf16)                    the ROUNDING ORACLE: bf16 rounding where the bf16 kernels round: every folded weight (the output conv's
                                                       plain weight), every gradient a kernel writes (the ResBlock's inner one included, after its gate; a
                                                       residual sum before its rounding stays unrounded); the cotangent, decoder_input's weight and dz are fp32
decode_vjp_ref(..., mutate="slope" | "no_residual" | "shift")   deliberately wrong chains for the bound-sanity test"""
import torch
import torch.nn.functional as F

import vit_decoder_reference as dr
from vit_decoder_reference import F64, STAGES, OUT_CONV

GATES = (0, 2, 4, 6, 7)            # stages whose output went through LeakyReLU(0.01): the five transposed convs


def factor(mask, slope, dtype):
    return torch.where(mask, torch.ones((), dtype=dtype), torch.full((), slope, dtype=dtype))


def res_inner_ref(sd, stages, dtype=F64, rnd=None):
    """the three ResBlock inner activations leaky02(conv1(h)) from a decode_ref result (decode_ref does not return them)"""
    get = lambda k: sd[k].to(dtype)
    r = rnd if rnd is not None else (lambda t: t)
    out = []
    for i, (kind, idx) in enumerate(STAGES):
        if kind == "res":
            w1, b1 = dr.fold(get, f"decoder.{idx}.conv.0", f"decoder.{idx}.conv.1", False)
            out.append(r(F.leaky_relu(F.conv2d(stages[f"stage{i - 1}"], r(w1), b1, padding=1), 0.2)))
    return out


def masks_of(stages, inner):
    """stages: name -> NCHW activation (a decode_ref result, or the HIP forward's collect brought to NCHW); inner: the three inner activations"""
    m = {f"stage{i}": stages[f"stage{i}"] > 0 for i in GATES}
    m.update({f"inner{j}": y > 0 for j, y in enumerate(inner)})
    return m


def decode_vjp_ref(sd, g_img, grid, masks, dtype=F64, rnd=None, mutate=None):
    get = lambda k: sd[k].to(dtype)
    r = rnd if rnd is not None else (lambda t: t)
    fac = lambda name, slope: factor(masks[name].to(g_img.device), slope, dtype)
    g = F.conv_transpose2d(g_img.to(dtype), r(get(f"decoder.{OUT_CONV}.weight")), padding=1)
    g = r(g * fac("stage7", 0.01))
    n_res = sum(kind == "res" for kind, _ in STAGES)
    for i in range(len(STAGES) - 1, -1, -1):
        kind, idx = STAGES[i]
        gate = fac(f"stage{i - 1}", 0.01) if (i - 1) in GATES else None
        if kind == "up":
            wf, _b = dr.fold(get, f"decoder.{idx}", f"decoder.{idx + 1}", True)
            g = F.conv2d(g, r(wf), stride=2, padding=1)            # the input gradient of ConvTranspose2d(k3, s2, p1, output_padding 1)
            if mutate == "shift":
                g = torch.roll(g, shifts=(1, 1), dims=(2, 3))
        else:
            n_res -= 1
            p = f"decoder.{idx}.conv"
            w1, _b1 = dr.fold(get, p + ".0", p + ".1", False)
            w2, _b2 = dr.fold(get, p + ".3", p + ".4", False)
            t = F.conv_transpose2d(g, r(w2), padding=1) * fac(f"inner{n_res}", 0.01 if mutate == "slope" else 0.2)
            back = F.conv_transpose2d(r(t), r(w1), padding=1)
            g = back if mutate == "no_residual" else back + g
        if gate is not None:
            g = g * gate
        g = r(g)
    return g.reshape(g.shape[0], -1) @ get("decoder_input.weight")
