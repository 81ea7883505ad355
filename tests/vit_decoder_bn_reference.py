"""The ViT-VAE decoder in TRAINING-mode BatchNorm2d (batch statistics; train_decoder(batch_stats=True)), written out stage by stage in plain torch
ops: the yardstick of tests/test_vit_decoder_batchnorm.py and of the float64 comparison in tests/test_bn2d_batch_bwd_cpu.py, built like
tests/vit_stem_bn_reference.py, beside tests/vit_decoder_wgrad_reference.py's eval-mode (folded) form, which it does not change.  Own code; it reads a state_dict
with the reference's keys, the latent z [B, latent_dim] and the cotangent of the image [B, 1, H, W].

LAYERS                                     the 11 (conv, BatchNorm2d) pairs in execution order = ViTVAE._decoder_params()' order: (stage, kind, conv key, bn key,
                                           slope): kind "up" (ConvTranspose2d k3 s2 p1 op1, LeakyReLU(0.01) behind the BatchNorm), "res0" (a ResBlock's first
                                           Conv2d k3, LeakyReLU(0.2)), "res1" (its second, no activation: the block's input is added)
decoder_bn_forward(sd, z, grid)            float64: grid = decoder_input(z) as [B, 256, gh, gw]; per layer y = conv(input) + bias, mean / var over (B, H, W)
                                           (biased), v = (y - mean) rstd gamma + beta, a = leaky(v) ("res1": a = block input + v); `stages` (the 8 stage outputs),
                                           `inner` (the 3 ResBlock inner activations), `image`; `buffers` = the 33 BatchNorm buffers after ONE training forward
decoder_bn_vjp(sd, z, g_img, grid, masks)  float64 gradients of the 48 decoder parameters and `dz`: the output conv, then per layer, last to first, with g the
                                           gradient of the layer's output: gv = g * (mask ? 1 : slope) (no activation: gv = g); dbeta = sum gv; dgamma = sum gv xh;
                                           g_y = gamma rstd (gv - dbeta / P - xh dgamma / P); dW = g_y (x) input; dbias = sum g_y (zero in exact arithmetic);
                                           g <- the conv's input gradient of g_y (+ the block's skip gradient below a ResBlock's first conv); then decoder_input
  masks=[m_0 .. m_10]                      the LeakyReLU masks (a > 0, NCHW bool; None for the "res1" layers) as ARGUMENTS, for the reason
                                           tests/vit_decoder_grad_reference.py gives; the GPU tests take the HIP forward's own
  rnd=round_bf16                           the ROUNDING ORACLE: float64 arithmetic, rounded to bf16 exactly where the bf16 kernels store bf16: the grid, the conv
                                           weights as operands, every y, a (the residual sum rounded once), g_y and every gradient handed down; statistics, dgamma,
                                           dbeta, dW, dbias, the image and dz stay unrounded (fp32 in the kernels)
  dtype=torch.float32                      the same restatement evaluated in fp32
torch_train_decoder(sd, z, g_img, dtype)   torch's own evaluation: the reference's nn decoder in .train() mode on the CPU in `dtype`, its autograd, its buffers
                                           (the "6 x" rule's yardstick in fp32; equal to the restatement in float64)
conv_bias_bound(..)                        the absolute bound on a BatchNorm-fronted conv bias's gradient (see there)"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import bn2d_batch_reference as br
import bn2d_batch_bwd_reference as bb
import vit_decoder_reference as vd
from vit_reference import F64, round_bf16  # noqa: F401

EPS, MOMENTUM = 1e-5, 0.1
OUT = f"decoder.{vd.OUT_CONV}"


def _layers():
    out = []
    for i, (kind, idx) in enumerate(vd.STAGES):
        if kind == "up":
            out.append((i, "up", f"decoder.{idx}", f"decoder.{idx + 1}", 0.01))
        else:
            out += [(i, "res0", f"decoder.{idx}.conv.0", f"decoder.{idx}.conv.1", 0.2), (i, "res1", f"decoder.{idx}.conv.3", f"decoder.{idx}.conv.4", None)]
    return tuple(out)


LAYERS = _layers()
PARAM_KEYS = (("decoder_input.weight", "decoder_input.bias") + tuple(f"{k}.{n}" for _i, _kind, c, b, _s in LAYERS for k, n in ((c, "weight"), (c, "bias"), (b, "weight"), (b, "bias")))
              + (OUT + ".weight", OUT + ".bias"))
CONV_BIAS_KEYS = tuple(c + ".bias" for _i, _kind, c, _b, _s in LAYERS)
BUFFER_KEYS = tuple(f"{b}.{n}" for _i, _kind, _c, b, _s in LAYERS for n in ("running_mean", "running_var", "num_batches_tracked"))


def randomize_decoder_bn(vae, seed):
    vd.randomize_decoder_bn(vae.decoder, seed)


def _c(v):
    return v[None, :, None, None]


def _conv(kind, x, w, b):
    return F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1) if kind == "up" else F.conv2d(x, w, b, padding=1)


def decoder_bn_forward(sd, z, grid, dtype=F64, rnd=None):
    """grid: the patch grid (gh, gw) = (H / 32, W / 32)"""
    gh, gw = grid
    get = lambda k: sd[k].detach().to(dtype=dtype, device="cpu")
    r = rnd if rnd is not None else (lambda t: t)
    zz = z.detach().cpu().to(dtype)
    out = dict(ins=[], y=[], a=[], mean=[], var=[], rstd=[], stages=[], inner=[], buffers={})
    h = r(zz @ get("decoder_input.weight").T + get("decoder_input.bias")).view(zz.shape[0], 256, gh, gw)
    out["grid"] = h
    m = br.f32(MOMENTUM)
    skip = None
    for _i, kind, c, b, slope in LAYERS:
        out["ins"].append(h)
        if kind == "res0":
            skip = h
        y = r(_conv(kind, h, r(get(c + ".weight")), get(c + ".bias")))
        n = y.numel() // y.shape[1]
        mean = y.mean(dim=(0, 2, 3))
        var = ((y - _c(mean)) ** 2).mean(dim=(0, 2, 3))
        rstd = 1.0 / torch.sqrt(var + EPS)
        v = (y - _c(mean)) * _c(rstd * get(b + ".weight")) + _c(get(b + ".bias"))
        a = r(skip + v) if kind == "res1" else r(F.leaky_relu(v, slope))
        for k_, t in (("y", y), ("a", a), ("mean", mean), ("var", var), ("rstd", rstd)):
            out[k_].append(t)
        out["buffers"][b + ".running_mean"] = (1.0 - m) * get(b + ".running_mean") + m * mean
        out["buffers"][b + ".running_var"] = (1.0 - m) * get(b + ".running_var") + m * var * (n / (n - 1))
        out["buffers"][b + ".num_batches_tracked"] = sd[b + ".num_batches_tracked"].detach().cpu() + 1
        (out["inner"] if kind == "res0" else out["stages"]).append(a)
        h = a
    out["image"] = F.conv2d(h, r(get(OUT + ".weight")), get(OUT + ".bias"), padding=1)
    return out


def masks_of(fw):
    """the restatement's own LeakyReLU masks, one per layer (None where no activation follows)"""
    return [None if slope is None else a > 0 for (_i, _kind, _c2, _b, slope), a in zip(LAYERS, fw["a"])]


def masks_from_collect(collect):
    """the HIP forward's masks from decode_with_grad's `collect` (channels-last `stages` and `res_inner`), in LAYERS order, NCHW bool on the CPU"""
    nchw = lambda t: t.detach().cpu().float().permute(0, 3, 1, 2)
    res, out = 0, []
    for i, kind, _c2, _b, _slope in LAYERS:
        if kind == "up":
            out.append(nchw(collect["stages"][i]) > 0)
        elif kind == "res0":
            out.append(nchw(collect["res_inner"][res]) > 0)
            res += 1
        else:
            out.append(None)
    return out


def decoder_bn_vjp(sd, z, g_img, grid, masks, dtype=F64, rnd=None, forward=None):
    get = lambda k: sd[k].detach().to(dtype=dtype, device="cpu")
    r = rnd if rnd is not None else (lambda t: t)
    fw = forward if forward is not None else decoder_bn_forward(sd, z, grid, dtype, rnd)
    zz = z.detach().cpu().to(dtype)
    grads, gys, gins = {}, [None] * len(LAYERS), [None] * len(LAYERS)
    g = g_img.detach().cpu().to(dtype)
    wo = get(OUT + ".weight")
    grads[OUT + ".weight"] = conv2d_weight(fw["stages"][-1], wo.shape, g, padding=1)
    grads[OUT + ".bias"] = g.sum().view(1)
    g = r(F.conv_transpose2d(g, r(wo), padding=1))
    skip_g = None
    for j in reversed(range(len(LAYERS))):
        _i, kind, c, b, slope = LAYERS[j]
        w, gam = get(c + ".weight"), get(b + ".weight")
        y, mean, rstd, x = fw["y"][j], fw["mean"][j], fw["rstd"][j], fw["ins"][j]
        n = y.numel() // y.shape[1]
        gins[j] = g
        if kind == "res1":
            skip_g = g                                                   # the block's input receives the output's gradient as it is
        gv = g if slope is None else g * torch.where(masks[j], torch.ones_like(g), torch.full_like(g, slope))
        xh = (y - _c(mean)) * _c(rstd)
        dbeta, dgamma = gv.sum(dim=(0, 2, 3)), (gv * xh).sum(dim=(0, 2, 3))
        gy = r(_c(gam * rstd) * (gv - _c(dbeta) / n - xh * _c(dgamma) / n))
        gys[j] = gy
        if kind == "up":                                                 # convT(x, w) is the adjoint of conv2d(., w, stride 2): the weight gradient with g_y as the input
            grads[c + ".weight"] = conv2d_weight(gy, w.shape, x, stride=2, padding=1)
            g = r(F.conv2d(gy, r(w), stride=2, padding=1))
        else:
            grads[c + ".weight"] = conv2d_weight(x, w.shape, gy, padding=1)
            g = F.conv_transpose2d(gy, r(w), padding=1)
            g = r(g + skip_g) if kind == "res0" else r(g)
        grads[c + ".bias"] = gy.sum(dim=(0, 2, 3))
        grads[b + ".weight"], grads[b + ".bias"] = dgamma, dbeta
    G = g.reshape(g.shape[0], 256, -1)                                   # nn.Linear's rows are (channel, position)
    grads["decoder_input.weight"] = G.reshape(G.shape[0], -1).T @ zz
    grads["decoder_input.bias"] = G.reshape(G.shape[0], -1).sum(0)
    grads["dz"] = G.reshape(G.shape[0], -1) @ get("decoder_input.weight")
    grads["g"], grads["g_in"] = gys, gins                                # the eleven g_y, and the gradient each was made from
    return grads


class _ResBlock(nn.Module):
    """the reference's ResBlock: x + conv(x)"""

    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(ch, ch, 3, 1, 1), nn.BatchNorm2d(ch), nn.LeakyReLU(0.2, inplace=True), nn.Conv2d(ch, ch, 3, 1, 1), nn.BatchNorm2d(ch))

    def forward(self, x):
        return x + self.conv(x)


def torch_train_decoder(sd, z, g_img, dtype):
    """the reference's decoder as torch runs it under .train(): {the 48 gradients, dz, image, buffers}"""
    gh, gw = g_img.shape[2] // 32, g_img.shape[3] // 32
    dec, cin = [], 256
    for i, cout in enumerate(vd.DEC_CHANNELS):
        dec += [nn.ConvTranspose2d(cin, cout, kernel_size=3, stride=2, padding=1, output_padding=1), nn.BatchNorm2d(cout), nn.LeakyReLU()]
        if i < 3:
            dec.append(_ResBlock(cout))
        cin = cout
    dec.append(nn.Conv2d(cin, 1, kernel_size=3, padding=1))
    lin, seq = nn.Linear(sd["decoder_input.weight"].shape[1], 256 * gh * gw), nn.Sequential(*dec)
    lin.load_state_dict({k[len("decoder_input."):]: v.detach().cpu() for k, v in sd.items() if k.startswith("decoder_input.")})
    seq.load_state_dict({k[len("decoder."):]: v.detach().cpu() for k, v in sd.items() if k.startswith("decoder.")})
    lin, seq = lin.to(dtype).train(), seq.to(dtype).train()
    zi = z.detach().cpu().to(dtype).clone().requires_grad_(True)
    stages, inner = [], []                                               # the 8 stage outputs and the 3 inner activations, as the modules produce them
    for kind, idx in vd.STAGES:
        if kind == "up":
            seq[idx + 2].register_forward_hook(lambda _m, _i, o: stages.append(o.detach().clone()))
        else:
            seq[idx].conv[2].register_forward_hook(lambda _m, _i, o: inner.append(o.detach().clone()))
            seq[idx].register_forward_hook(lambda _m, _i, o: stages.append(o.detach().clone()))
    image = seq(lin(zi).view(-1, 256, gh, gw))
    image.backward(g_img.detach().cpu().to(dtype))
    res = {f"stage{i}": t for i, t in enumerate(stages)}
    res.update({f"inner{i}": t for i, t in enumerate(inner)})
    res.update({f"decoder_input.{k}": p.grad.detach() for k, p in lin.named_parameters()})
    res.update({f"decoder.{k}": p.grad.detach() for k, p in seq.named_parameters()})
    res["dz"], res["image"] = zi.grad.detach(), image.detach()
    res["buffers"] = {f"decoder.{k}": v.detach().clone() for k, v in seq.named_buffers()}
    return res


def rows(t):
    """NCHW -> the kernels' [P, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_bias_bound(fw, vjp, masks, sd, j, bf16):
    """|dbias_j| <= this, per channel [C], for layer j of LAYERS: built like vit_stem_bn_reference.conv_bias_bound on cvae_bn2d_batch_bwd's bounds.  The channel
    sum of g_y is zero in exact arithmetic WHATEVER the incoming gradient and y_j are (the batch mean is subtracted), so what the kernels return is rounding
    alone: every stored g_y element within its bound of tests/bn2d_batch_bwd_reference.py's backward (what the channel's elements share added as it is; the
    element's own operations and its bf16 store, independent roundings, in quadrature with the constant C of every sum rule here), plus the fp32 sum of P of
    them, C sqrt(P) U sum |g_y|."""
    _i, _kind, _c2, b, slope = LAYERS[j]
    y = rows(fw["y"][j])
    P = y.shape[0]
    gam = sd[b + ".weight"].detach().cpu().to(F64)
    mean, M2, e_mean, e_M2 = br.moments(y)
    var = M2 / P
    e_var = e_M2 / P + br.U * var
    rstd = 1.0 / torch.sqrt(var + EPS)
    e_rstd = rstd * ((e_var + br.U * (var + EPS)) / (2 * (var + EPS)) + br._u("sqrtf") + br._u("div"))
    ref, err = bb.backward(y, rows(vjp["g_in"][j]), None if slope is None else rows(masks[j]), gam, mean, rstd, e_mean, e_rstd, slope, bf16)
    return err["dx_common"].sum(0) + br.C * torch.sqrt((err["dx_local"] ** 2).sum(0)) + br._ps(P) * ref["dx"].abs().sum(0)
