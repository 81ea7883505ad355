"""The gradient of the ViT-VAE encoder with respect to the IMAGE, Grad-CAM and integrated gradients in float64: the yardstick of
tests/test_vit_input_grad*.py.  Own code on top of tests/vit_encoder_grad_reference.py (the transformer's VJP down to `dstem`) and
tests/vit_stem_grad_reference.py (the stem's, down to g_0, the gradient of the first layer's pre-activation); this file adds the last hop, 32 channels to the
one-channel image, and the two maps built on it.

image_vjp(sd, x, depth, g_mu, g_lv)             float64: {"dx" [B, 1, H, W], "dstem", "g0" (NCHW), "stem" [B, Np, 256] (the stem's output), "cls_out", "mu", "log_var"}
image_vjp(..., g_cls=...)                       the cotangent of the cls features themselves instead of (g_mu, g_lv)
image_vjp(..., dtype=torch.float32)             the same restatement evaluated in fp32 on the CPU (the "4 x" rule's denominator)
image_vjp(..., rnd=round_bf16)                  the ROUNDING ORACLE of the two reference files, continued: g_0 is rounded to bf16 (the kernels store it so), the
                                                first folded weight is NOT (cvae_conv_down_image_bwd_data keeps it fp32 in both modes), dx is not (fp32 result)
image_vjp(..., masks=[m_0 .. m_4])              the stem's LeakyReLU masks as arguments (vit_stem_grad_reference says why)
torch_encode(sd, x, depth)                      an independent float64 forward in plain differentiable torch ops, the stem in its UNFOLDED form (conv, BatchNorm
                                                formula, LeakyReLU): torch.autograd.grad through it is what image_vjp is checked against on the CPU
gradcam_ref(A, dA, normalize)                   float64 Grad-CAM of [B, n, C] arrays: w = mean_i dA, m = relu(sum_c w A), (m - min) / (max - min + 1e-8)
integrated_gradients(grad, x, baseline, steps)  (x - baseline) / steps * sum_k grad(baseline + ((k - 1/2) / steps)(x - baseline)), k = 1 .. steps

BOUNDS, all from u = 2^-24 (fp32 unit roundoff); nothing is fitted.  Operands are the kernel's own inputs, exact in float64; a bf16 operand is widened exactly.

image_bound(g, w, alpha): cvae_conv_down_image_bwd_data.  An output element is alpha times a sum of K <= 2 x 2 x 32 = 128 products.  The kernel adds them in
  fma chains of 16 (the product is not rounded), then the partials: every term passes through at most 16 + 4 + 1 = 21 additions, each (1 + d), |d| <= u.  Any
  summation order of K terms is covered by gamma_(K-1) <= K u, so with the multiplication by alpha (1 rounding; alpha itself is a float, exact) and headroom
  for second-order terms:  |dx - alpha s| <= (K + 2) u |alpha| sum |g w|, K = 128, the sum over the terms of THAT element (scatter of |g| through |w|).  The
  accumulate form computes fma(alpha, s, dx0): one rounding of the exact alpha s_hat + dx0, so the same bound plus u |result|.
gradcam_bound(A, dA, normalize): cvae_gradcam256.
  w_c:  an n-term chain ((n - 1) u sum_i |dA_ic|), then the product with fl(1 / n) (rounded division, rounded product: 2 u):  e_w[c] = (n + 1) u mean_i |dA_ic|.
  m_i:  64 fma chains of 4 terms (<= 4 roundings a term) and a 6-level pairwise sum (6 more): 10 u sum_c |w_c A_ic|, plus the error of w carried through:
        e_m[i] = sum_c e_w[c] |A_ic| + 11 u sum_c |w_c| |A_ic|  (11: one unit of headroom for second-order terms); max(0, .) is 1-Lipschitz.
  normalised: lo = min m, hi = max m are off by at most E = max_i e_m[i] each.  d = fl(fl(hi - lo) + fl(1e-8)): e_d = 2 E + 3 u d.  The numerator fl(m_i - lo)
        is off by e_m[i] + E + u |m_i - lo|, and the correctly rounded quotient q = num / d <= 1 adds u q:
        e_cam[i] = (e_m[i] + E + u |m_i - lo| + q_i e_d) / (d - e_d) + 2 u q_i.  A map with d <= 2 e_d (constant up to rounding) has no such bound: the caller
        must not ask for one (the tests' constant and all-negative maps are exact zeros on both sides instead).
propagated_gradcam_bound(A, dA, eA, edA): how far the un-normalised map moves when its inputs move by at most eA, edA element-wise (the model-level test: the
  HIP walk's own stem output and dstem against float64's): |delta w_c| <= mean_i edA_ic =: ew[c], and
  |delta m_i| <= sum_c (ew[c] (|A_ic| + eA_ic) + |w_c| eA_ic), exact interval arithmetic of the bilinear form; relu is 1-Lipschitz."""
import torch
import torch.nn.functional as F

import vit_encoder_grad_reference as gr
import vit_stem_grad_reference as sr
from vit_reference import F64, U32, UBF, round_bf16, stem_layer_b  # noqa: F401

K_IMAGE = 128


def stem_forward(sd, x, dtype=F64, rnd=None):
    """the stem's output [B, Np, 256] of the restatement in its folded form (operands and activations rounded by rnd)"""
    get = lambda k: sd[k].detach().to(dtype)
    h = x.to(dtype)
    for j in range(5):
        h, _e = stem_layer_b(h, None, sd, j, get, rnd=rnd if rnd is not None else (lambda t: t))
    return h.flatten(2).transpose(1, 2)


def first_folded_weight(sd, dtype=F64):
    """wf_0 = w s, s = gamma / sqrt(var + eps): the k3 weight [32, 1, 3, 3] of the first stem layer with its BatchNorm folded in"""
    get = lambda k: sd[k].detach().to(dtype)
    s = get("stem.1.weight") / torch.sqrt(get("stem.1.running_var") + sr.EPS)
    return get("stem.0.weight") * s[:, None, None, None]


def last_hop(g0, wf0):
    """dx [B, 1, 2 sh, 2 sw] = the input gradient of Conv2d(1, 32, k3, s2, p1) from the gradient g0 [B, 32, sh, sw] of its output"""
    return F.conv_transpose2d(g0, wf0, stride=2, padding=1, output_padding=1)


def image_vjp(sd, x, depth, g_mu=None, g_lv=None, g_cls=None, dtype=F64, rnd=None, cls_only=False, masks=None):
    stem = stem_forward(sd, x, dtype, rnd)
    if g_cls is None:
        ref = g_mu if g_mu is not None else g_lv
        g_mu = torch.zeros_like(ref) if g_mu is None else g_mu
        g_lv = torch.zeros_like(ref) if g_lv is None else g_lv
    tg, out = gr.transformer_vjp(sd, stem, depth, g_mu, g_lv, dtype=dtype, rnd=rnd, cls_only_last=cls_only, g_cls=g_cls)
    g0 = sr.stem_vjp(sd, x, tg["dstem"], dtype=dtype, rnd=rnd, want_parts=True, masks=masks)["g"][0]
    return dict(out, dx=last_hop(g0, first_folded_weight(sd, dtype)), dstem=tg["dstem"], g0=g0, stem=stem.to(dtype))


def torch_encode(sd, x, depth):
    """(cls features, mu, log_var) in float64, differentiable with respect to x: the unfolded stem, then the transformer in the order the reference class
    runs it (LayerNorm, packed in-projection, softmax attention, out-projection + skip, LayerNorm, MLP with exact GELU + skip)."""
    get = lambda k: sd[k].detach().to(F64)
    h = x.to(F64)
    for j in range(5):
        h, _e = stem_layer_b(h, None, sd, j, get)                       # rnd None, no bound: conv, the BatchNorm formula, LeakyReLU
    B = h.shape[0]
    t = torch.cat([get("cls_token").expand(B, -1, -1), h.flatten(2).transpose(1, 2)], dim=1) + get("pos_embedding")
    for i in range(depth):
        p = f"transformer.{i}."
        y = F.layer_norm(t, (256,), get(p + "norm1.weight"), get(p + "norm1.bias"), 1e-5)
        q, k, v = (y @ get(p + "attn.in_proj_weight").T + get(p + "attn.in_proj_bias")).split(256, dim=-1)
        sh = lambda a: a.reshape(B, -1, 8, 32).transpose(1, 2)
        att = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / 32 ** 0.5, dim=-1) @ sh(v)
        t = t + att.transpose(1, 2).reshape(B, -1, 256) @ get(p + "attn.out_proj.weight").T + get(p + "attn.out_proj.bias")
        y = F.layer_norm(t, (256,), get(p + "norm2.weight"), get(p + "norm2.bias"), 1e-5)
        t = t + F.gelu(y @ get(p + "mlp.0.weight").T + get(p + "mlp.0.bias")) @ get(p + "mlp.3.weight").T + get(p + "mlp.3.bias")
    c = F.layer_norm(t[:, 0], (256,), get("to_latent.weight"), get("to_latent.bias"), 1e-5)
    return c, c @ get("fc_mu.weight").T + get("fc_mu.bias"), c @ get("fc_var.weight").T + get("fc_var.bias")


def image_bound(g, w, alpha=1.0, result=None):
    """element-wise bound [B, 1, 2 sh, 2 sw] of cvae_conv_down_image_bwd_data on exact operands g [B, 32, sh, sw] (NCHW) and the k4 weight w [32, 1, 4, 4];
    result: the (float64) value of the accumulate form's output, which adds its one rounding"""
    e = (K_IMAGE + 2) * U32 * abs(alpha) * F.conv_transpose2d(g.to(F64).abs(), w.to(F64).abs(), stride=2, padding=1)
    return e if result is None else e + U32 * result.to(F64).abs()


def gradcam_ref(A, dA, normalize=True):
    A, dA = A.to(F64), dA.to(F64)
    w = dA.mean(dim=1, keepdim=True)
    m = (A * w).sum(-1).clamp_min(0.0)
    if not normalize:
        return m
    lo, hi = m.amin(1, keepdim=True), m.amax(1, keepdim=True)
    return (m - lo) / (hi - lo + 1e-8)


def gradcam_bound(A, dA, normalize=True):
    A, dA = A.to(F64), dA.to(F64)
    n = A.shape[1]
    w = dA.mean(dim=1, keepdim=True)
    e_w = (n + 1) * U32 * dA.abs().mean(dim=1, keepdim=True)
    e_m = (e_w * A.abs()).sum(-1) + 11 * U32 * (w.abs() * A.abs()).sum(-1)
    if not normalize:
        return e_m
    m = (A * w).sum(-1).clamp_min(0.0)
    lo, hi = m.amin(1, keepdim=True), m.amax(1, keepdim=True)
    E = e_m.amax(1, keepdim=True)
    d = hi - lo + 1e-8
    e_d = 2 * E + 3 * U32 * d
    assert bool((d > 2 * e_d).all()), "gradcam_bound: a map that is constant up to rounding has no normalised bound"
    q = (m - lo) / d
    return (e_m + E + U32 * (m - lo).abs() + q * e_d) / (d - e_d) + 2 * U32 * q


def propagated_gradcam_bound(A, dA, eA, edA):
    A, dA, eA, edA = (t.to(F64) for t in (A, dA, eA, edA))
    w, ew = dA.mean(dim=1, keepdim=True), edA.mean(dim=1, keepdim=True)
    return (ew * (A.abs() + eA) + w.abs() * eA).sum(-1)


def integrated_gradients(grad, x, baseline, steps):
    """grad: a callable, point [B, 1, H, W] -> gradient [B, 1, H, W]; the midpoint rule on the straight path from baseline to x"""
    diff = x - baseline
    total = None
    for k in range(1, steps + 1):
        g = grad(baseline + ((k - 0.5) / steps) * diff)
        total = g if total is None else total + g
    return diff * total / steps


def rel_l2(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float((a - b).norm() / b.norm())
