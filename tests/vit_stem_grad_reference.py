"""The vector-Jacobian product of the ViT-VAE encoder's conv stem (five Conv2d(k3, s2, p1) + eval-mode BatchNorm2d + LeakyReLU(0.01) layers), written out
stage by stage in plain torch ops in the FOLDED form the kernels run: the yardstick of tests/test_vit_stem_grad*.py, beside
tests/vit_encoder_grad_reference.py's transformer.  Own code; it reads a state_dict with the reference's keys, the image and the cotangent of the stem's
output, nothing else.  The forward is vit_reference.stem_layer_b's.

stem_vjp(sd, x, dstem)                          float64 gradients of the 20 stem tensors
stem_vjp(..., dtype=torch.float32)              the same restatement evaluated in fp32 on the CPU (the "4 x" rule's denominator)
stem_vjp(..., rnd=round_bf16)                   the ROUNDING ORACLE: float64 arithmetic, rounded to bf16 exactly where the bf16 kernels round: the folded weights
                                                and the activations (as vit_reference.encode_ref), and every g_j, the gradient of layer j's pre-activation (the gate
                                                is multiplied onto the fp32 sum, then ONE rounding).  The folded weight's and bias's gradients, the way back through
                                                the fold and all 20 results stay unrounded (fp32 in the kernels).
stem_vjp(..., wrong="gate_from_output" / "dgamma_no_bias")   two deliberately wrong restatements (what the yardstick must refuse)
stem_vjp(..., masks=[m_0 .. m_4])               the LeakyReLU masks (activation > 0, NCHW bool) as ARGUMENTS instead of the restatement's own, for the reason
                                                tests/vit_decoder_grad_reference.py gives: a pre-activation that float64 puts at 1.7e-8 is an exact 0.0 in an fp32
                                                evaluation (met at 64 x 96), the two then differentiate DIFFERENT piecewise-linear maps and one element moves a gradient
                                                by 1e-3.  With the masks fixed the stem is a product of linear maps, and it is that map's VJP the kernels are held to;
                                                the GPU tests take the masks of the HIP forward's own activations and check them against float64 wherever the
                                                pre-activation's rounding bound decides the sign (decided_masks).

The chain.  y_j = leaky001(p_j), p_j = conv(y_{j-1}, wf_j) + bf_j with the folded wf = w s, bf = (bias - mean) s + beta, s = gamma rstd, rstd = 1 / sqrt(var + eps),
y_{-1} = the image.  g_4 = dstem * leaky001'(y_4); per layer, last to first: dwf_j = sum g_j (x) y_{j-1}, dbf_j = sum g_j, g_{j-1} = scatter(g_j, wf_j) *
leaky001'(y_{j-1}) with leaky001'(y) = y > 0 ? 1 : 0.01 read off the activation's OUTPUT (LeakyReLU keeps the sign).  Back through the fold, per BatchNorm
channel: dw = s dwf, db = s dbf, dgamma = rstd (sum dwf w + dbf (bias - mean)), dbeta = dbf.
"gate_from_output": the derivative in layer j's data gradient is read off the layer's OWN output y_j (applied to g_j in front of the scatter) instead of
its input's producer y_{j-1} (applied behind it): every g below the last lacks its own gate and carries the gate above it twice.
"dgamma_no_bias": dgamma without the dbf (bias - mean) term."""
import torch
import torch.nn.functional as F

from vit_reference import F64, U32, UBF, round_bf16, stem_layer_b  # noqa: F401

SLOPE = 0.01
EPS = 1e-5


def act_grad(y, mask=None):
    """leaky001' read off the activation's output (or off a given mask = activation > 0)"""
    return torch.where(y > 0 if mask is None else mask, torch.ones_like(y), torch.full_like(y, SLOPE))


def decided_masks(sd, x, ys, bf16):
    """The masks (y > 0, NCHW bool) of a kernel forward's five activations ys (NCHW), each checked against float64: wherever the pre-activation lies farther
    from zero than the bound on its computed value (vit_reference.stem_layer_b's element-wise bound, carried from layer to layer; bf16: on the rounding
    oracle's operands, every stored activation within one bf16 rounding), the kernel's sign must be float64's.  Returns (masks, undecided elements)."""
    get = lambda k: sd[k].detach().to(F64)
    h = x.to(F64)
    eh = torch.zeros_like(h)
    masks, undecided = [], 0
    for j, y in enumerate(ys):
        pre, e = stem_layer_b(h, eh, sd, j, get, rnd=round_bf16 if bf16 else None, out_u=UBF if bf16 else 0.0, pre_act=True)
        mask = y.to(F64) > 0
        loose = pre.abs() <= e
        assert bool(((mask == (pre > 0)) | loose).all()), f"stem layer {j}: a LeakyReLU sign differs from float64's where the rounding bound decides it"
        undecided += int(loose.sum())
        masks.append(mask)
        h = F.leaky_relu(pre, SLOPE)
        h, eh = (round_bf16(h) if bf16 else h), e
    return masks, undecided


def stem_vjp(sd, x, dstem, dtype=F64, rnd=None, wrong=None, want_parts=False, masks=None):
    """x [B, 1, H, W]; dstem [B, Np, 256] (`b (h w) c`, the cotangent of the stem's output).  Returns {state_dict key: gradient} for the 20 stem tensors
    (plus "g": [g_0 .. g_4], NCHW, with want_parts).  masks: see the module docstring."""
    get = lambda k: sd[k].detach().to(dtype=dtype, device=x.device)
    r = rnd if rnd is not None else (lambda t: t)
    h = x.to(dtype)
    B = h.shape[0]
    ins, outs = [], []
    for j in range(5):
        ins.append(h)
        h, _e = stem_layer_b(h, None, sd, j, get, rnd=r)                # the folded form, operands and the activation rounded by r
        outs.append(h)
    _B, C, gh, gw = h.shape
    g = dstem.to(dtype).transpose(1, 2).reshape(B, C, gh, gw)
    m = masks if masks is not None else [None] * 5
    g = r(g * act_grad(outs[4], m[4]))
    grads, gs = {}, [None] * 5
    for j in reversed(range(5)):
        c, b = 3 * j, 3 * j + 1
        w, bias = get(f"stem.{c}.weight"), get(f"stem.{c}.bias")
        gam, mean, var = (get(f"stem.{b}.{n}") for n in ("weight", "running_mean", "running_var"))
        rstd = 1.0 / torch.sqrt(var + EPS)
        s = gam * rstd
        wf = w * s[:, None, None, None]
        gs[j] = g
        dwf = torch.nn.grad.conv2d_weight(r(ins[j]), wf.shape, g, stride=2, padding=1)
        dbf = g.sum(dim=(0, 2, 3))
        grads[f"stem.{c}.weight"] = dwf * s[:, None, None, None]
        grads[f"stem.{c}.bias"] = dbf * s
        tot = (dwf * w).sum(dim=(1, 2, 3))
        grads[f"stem.{b}.weight"] = rstd * (tot if wrong == "dgamma_no_bias" else tot + dbf * (bias - mean))
        grads[f"stem.{b}.bias"] = dbf
        if j:
            if wrong == "gate_from_output":
                g = r(F.conv_transpose2d(g * act_grad(outs[j], m[j]), r(wf), stride=2, padding=1, output_padding=1))
            else:
                g = r(F.conv_transpose2d(g, r(wf), stride=2, padding=1, output_padding=1) * act_grad(outs[j - 1], m[j - 1]))
    if want_parts:
        grads["g"] = gs
    return grads


STEM_KEYS = tuple(f"stem.{i}.{n}" for j in range(5) for i, n in ((3 * j, "weight"), (3 * j, "bias"), (3 * j + 1, "weight"), (3 * j + 1, "bias")))


def rel_l2(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float((a - b).norm() / b.norm())
