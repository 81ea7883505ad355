"""The ViT-VAE stem in TRAINING-mode BatchNorm2d (batch statistics; train_stem(batch_stats=True)), written out stage by stage in plain torch
ops: the yardstick of tests/test_vit_stem_batchnorm.py, beside tests/vit_stem_grad_reference.py's eval-mode (folded) form, which it imports and does not change.
Own code; it reads a state_dict with the reference's keys, the image and the cotangent of the stem's output.

stem_bn_forward(sd, x)                     float64: per layer y_j = conv(a_{j-1}, w_j) + bias_j (a_{-1} = the image), mean_j / var_j over (B, H, W) (biased),
                                           a_j = leaky001((y_j - mean_j) rstd_j gamma_j + beta_j), rstd = 1 / sqrt(var + eps); `stem` = a_4 as [B, Np, 256];
                                           `buffers` = the running statistics after ONE training forward (momentum of 0.1, unbiased variance) and
                                           num_batches_tracked + 1
stem_bn_vjp(sd, x, dstem, masks=...)       float64 gradients of the 20 stem tensors (+ `dx`, `g` = the five g_y) for the cotangent dstem of `stem`:
                                           per layer, last to first, with g the gradient of a_j:  gv = g * (mask_j ? 1 : 0.01);  dbeta = sum gv;
                                           dgamma = sum gv xh;  g_y = gamma rstd (gv - dbeta / P - xh dgamma / P);  dW = g_y (x) a_{j-1};  dbias = sum g_y
                                           (zero in exact arithmetic);  g <- scatter(g_y, w_j)  (no gate: the LeakyReLU derivative belongs to the layer below)
  masks=[m_0 .. m_4]                       the LeakyReLU masks (a_j > 0, NCHW bool) as ARGUMENTS, for the reason tests/vit_stem_grad_reference.py gives; the GPU
                                           tests take the HIP forward's own
  rnd=round_bf16                           the ROUNDING ORACLE: float64 arithmetic, rounded to bf16 exactly where the bf16 kernels store bf16: the conv weights as
                                           operands, every y_j, a_j, g_y and the gradient handed down; statistics, dgamma, dbeta, dW and dbias stay unrounded
                                           (fp32 in the kernels)
  dtype=torch.float32                      the same restatement evaluated in fp32
torch_train_stem(sd, x, dstem, dtype)      torch's own evaluation: the reference's nn.Sequential of Conv2d / BatchNorm2d / LeakyReLU in .train() mode on the CPU in
                                           `dtype`, its autograd, its buffers (the "6 x" rule's yardstick in fp32; equal to the restatement in float64)
conv_bias_bound(..)                        the absolute bound on a conv bias's gradient (see there)"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import bn2d_batch_reference as br
from vit_reference import F64, round_bf16  # noqa: F401
from vit_stem_grad_reference import STEM_KEYS, rel_l2  # noqa: F401

SLOPE, EPS, MOMENTUM = 0.01, 1e-5, 0.1
CHANNELS = (32, 64, 128, 256, 256)
CONV_BIAS_KEYS = tuple(f"stem.{3 * j}.bias" for j in range(5))
BUFFER_KEYS = tuple(f"stem.{3 * j + 1}.{n}" for j in range(5) for n in ("running_mean", "running_var", "num_batches_tracked"))


def _c(v):
    return v[None, :, None, None]


def stem_bn_forward(sd, x, dtype=F64, rnd=None):
    get = lambda k: sd[k].detach().to(dtype=dtype, device="cpu")
    r = rnd if rnd is not None else (lambda t: t)
    h = x.to(dtype)
    out = dict(ins=[], y=[], a=[], mean=[], var=[], rstd=[], buffers={})
    for j in range(5):
        c, b = 3 * j, 3 * j + 1
        y = r(F.conv2d(h, r(get(f"stem.{c}.weight")), get(f"stem.{c}.bias"), stride=2, padding=1))
        n = y.numel() // y.shape[1]
        mean = y.mean(dim=(0, 2, 3))
        var = ((y - _c(mean)) ** 2).mean(dim=(0, 2, 3))
        rstd = 1.0 / torch.sqrt(var + EPS)
        a = r(F.leaky_relu((y - _c(mean)) * _c(rstd * get(f"stem.{b}.weight")) + _c(get(f"stem.{b}.bias")), SLOPE))
        out["ins"].append(h), out["y"].append(y), out["a"].append(a), out["mean"].append(mean), out["var"].append(var), out["rstd"].append(rstd)
        m = br.f32(MOMENTUM)
        out["buffers"][f"stem.{b}.running_mean"] = (1.0 - m) * get(f"stem.{b}.running_mean") + m * mean
        out["buffers"][f"stem.{b}.running_var"] = (1.0 - m) * get(f"stem.{b}.running_var") + m * var * (n / (n - 1))
        out["buffers"][f"stem.{b}.num_batches_tracked"] = sd[f"stem.{b}.num_batches_tracked"].detach().cpu() + 1
        h = a
    out["stem"] = h.flatten(2).transpose(1, 2)
    return out


def stem_bn_vjp(sd, x, dstem, masks=None, dtype=F64, rnd=None, want_dx=False, forward=None):
    get = lambda k: sd[k].detach().to(dtype=dtype, device="cpu")
    r = rnd if rnd is not None else (lambda t: t)
    fw = forward if forward is not None else stem_bn_forward(sd, x, dtype, rnd)
    B, C, gh, gw = fw["a"][4].shape
    g = r(dstem.to(dtype).transpose(1, 2).reshape(B, C, gh, gw))
    grads, gs, gins = {}, [None] * 5, [None] * 5
    for j in reversed(range(5)):
        c, b = 3 * j, 3 * j + 1
        w, gam = get(f"stem.{c}.weight"), get(f"stem.{b}.weight")
        y, a, mean, rstd = fw["y"][j], fw["a"][j], fw["mean"][j], fw["rstd"][j]
        n = y.numel() // y.shape[1]
        mask = (a > 0) if masks is None else masks[j]
        gins[j] = g
        gv = g * torch.where(mask, torch.ones_like(g), torch.full_like(g, SLOPE))
        xh = (y - _c(mean)) * _c(rstd)
        dbeta, dgamma = gv.sum(dim=(0, 2, 3)), (gv * xh).sum(dim=(0, 2, 3))
        gy = r(_c(gam * rstd) * (gv - _c(dbeta) / n - xh * _c(dgamma) / n))
        gs[j] = gy
        grads[f"stem.{c}.weight"] = torch.nn.grad.conv2d_weight(fw["ins"][j], w.shape, gy, stride=2, padding=1)
        grads[f"stem.{c}.bias"] = gy.sum(dim=(0, 2, 3))
        grads[f"stem.{b}.weight"], grads[f"stem.{b}.bias"] = dgamma, dbeta
        if j:
            g = r(F.conv_transpose2d(gy, r(w), stride=2, padding=1, output_padding=1))
        elif want_dx:
            grads["dx"] = F.conv_transpose2d(gy, w, stride=2, padding=1, output_padding=1)
    grads["g"], grads["g_in"] = gs, gins                                 # the five g_y, and the gradient of a_j each was made from
    return grads


def torch_train_stem(sd, x, dstem, dtype):
    """the reference's stem as torch runs it under .train(): {the 20 gradients, dx, stem, buffers}"""
    layers, cin = [], 1
    for cout in CHANNELS:
        layers += [nn.Conv2d(cin, cout, kernel_size=3, stride=2, padding=1), nn.BatchNorm2d(cout), nn.LeakyReLU()]
        cin = cout
    seq = nn.Sequential(*layers)
    seq.load_state_dict({k[len("stem."):]: v.detach().cpu() for k, v in sd.items() if k.startswith("stem.")})
    seq = seq.to(dtype).train()
    xi = x.detach().to(dtype).clone().requires_grad_(True)
    out = seq(xi)
    out.backward(dstem.to(dtype).transpose(1, 2).reshape(out.shape))
    res = {f"stem.{k}": p.grad.detach() for k, p in seq.named_parameters()}
    res["dx"], res["stem"] = xi.grad.detach(), out.detach().flatten(2).transpose(1, 2)
    res["buffers"] = {f"stem.{k}": v.detach().clone() for k, v in seq.named_buffers()}
    return res


def rows(t):
    """NCHW -> the kernels' [P, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_bias_bound(fw, vjp, masks, sd, j, bf16):
    """|dbias_j| <= this, per channel [C]: the channel sum of g_y is zero in exact arithmetic WHATEVER the incoming gradient and y_j are (the batch mean is
    subtracted), so what the kernels return is rounding alone: every stored g_y element within its bound of tests/bn2d_batch_reference.py's backward (the two
    channel sums' and the statistics' errors, shared by the channel's elements and therefore added as they are; the element's own operations and its bf16
    store, independent roundings, added in quadrature with the constant C of every sum rule here), plus the fp32 sum of P of them, C sqrt(P) U sum |g_y|."""
    c, b = 3 * j, 3 * j + 1
    y = rows(fw["y"][j])
    P = y.shape[0]
    gam = sd[f"stem.{b}.weight"].detach().cpu().to(F64)
    gin = vjp["g_in"][j]
    mean, M2, e_mean, e_M2 = br.moments(y)
    var = M2 / P
    e_var = e_M2 / P + br.U * var
    rstd = 1.0 / torch.sqrt(var + EPS)
    e_rstd = rstd * ((e_var + br.U * (var + EPS)) / (2 * (var + EPS)) + br._u("sqrtf") + br._u("div"))
    ref, err = br.backward(y, rows(gin), rows(masks[j]), gam, mean, rstd, e_mean, e_rstd, SLOPE, bf16)
    return err["dx_common"].sum(0) + br.C * torch.sqrt((err["dx_local"] ** 2).sum(0)) + br._ps(P) * ref["dx"].abs().sum(0)
