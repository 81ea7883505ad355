"""A restatement of one dense head of CausalViTVAE in TRAINING mode (batch-statistics BatchNorm1d, running-statistics update, clamps, z) and of its
vector-Jacobian product, in plain torch ops, parametrised by dtype (float64: the yardstick; float32: the CPU evaluation whose distance from float64 the HIP
gradients are measured against) — the yardstick of tests/test_heads_grad*.py.  Own code.

head_forward(x, layers, split, clamp0, clamp1, noise, dtype, want_bound)   values + element-wise bounds of everything cvae_mlp_heads_train_fwd writes
head_vjp(fw, layers, cot, masks, ...)                                       every parameter gradient and dx, with the LeakyReLU and clamp masks as ARGUMENTS
own_masks(fw)                                                               the masks of that forward itself

layers: [(W [N, K], b [N], bn, slope)], bn = dict(gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked) or None; the last layer's W
is the stacked weight of a pair.  The masks are arguments because an fp32 and a float64 forward can disagree on a sign (or on which side of a clamp bound a
value falls) within rounding of zero, and one flip outweighs all rounding: the GPU tests pass the HIP forward's own masks.

Local fp32 bounds (u = 2^-24; counted from the operations csrc/heads.hip issues in training mode; a value v carries e >= |computed - v|; B rows):
  Linear                       e_v = sum |w| e_x + (K + 2) u (sum |w x| + |b|)                                           (vit_reference.linear_b)
  mean = (add chain over rows) / B: B - 1 adds and a divide:      e_m = mean_r e_v + (B + 1) u mean_r |v|
  d = v - mean, one rounding:                                      e_d = e_v + e_m + u |d|
  q = fmaf chain of d d over the rows:                             e_q = sum_r (2 |d| e_d + e_d^2) + (B + 1) u q
  var = q / B:                                                     e_var = e_q / B + u var
  rstd = 1 / sqrtf(var + eps): add, sqrt, divide; 1 / sqrt is convex and decreasing, so the slope at the low end bounds the change:
                                                                   e_rstd = 0.5 e_var (var + eps - e_var)^-1.5 + 3 u rstd
  x^ = d rstd, one rounding:                                       e_x = e_d rstd + |d| e_rstd + e_d e_rstd + u |x^|
  pre = fma(x^, gamma, beta):                                      e_p = |gamma| e_x + u |pre|
  LeakyReLU(slope <= 1):                                           e_y = e_p + u |y|
  running_mean = fma(momentum, mean, (1 - momentum) running_mean): the float momentum, 1 - momentum, the product and the fma round:
                                                                   e = momentum e_m + 4 u (|momentum mean| + |(1 - momentum) running_mean|)
  running_var  the same with the UNBIASED variance q / (B - 1):   e_unb = e_q / (B - 1) + u unb
  clamp exact; z as tests/causal_vit_reference.py (reparam_b).
  db of the Linear in front of a BatchNorm layer: zero in exact arithmetic (sum_r dv = gamma rstd (sum dy - dbeta - dgamma sum_r x^ / B), sum_r x^ = 0), so
  no relative measure exists; what is computed is rounding: per dv about 4 roundings on terms of size T_r = |gamma rstd| (|dy| + |dbeta| / B + |x^ dgamma| / B),
  the B - 1 adds of the row chain, the chains behind dbeta and dgamma (B u each, entering every row with weight 1 / B), and sum_r x^ = rstd B (mean - computed
  mean), |.| <= rstd (B + 1) u mean_r |v| with mean_r |v| <= |mean| + mean_r |x^| / rstd:
        |db| <= (2 B + 16) u db_scale,   db_scale = sum_r T_r + |gamma rstd dgamma| (rstd |mean| + mean_r |x^|)            (head_vjp's `db_scale{l}`)
"""
import torch

from vit_reference import U32, F64, linear_b, rel_l2   # noqa: F401
from causal_vit_reference import reparam_b


def head_forward(x, layers, split, clamp0=None, clamp1=None, noise=None, dtype=F64, want_bound=False, biased_running=False):
    x = x.to(dtype)
    B = x.shape[0]
    e = torch.zeros_like(x) if want_bound else None
    fw = dict(inputs=[], xhat={}, rstd={}, mean={}, pre={}, act={}, running_mean={}, running_var={}, nbt={}, bound={})
    for l, (W, b, bn, slope) in enumerate(layers):
        W, b = W.to(dtype), b.to(dtype)
        fw["inputs"].append(x)
        v, e = linear_b(x, e, W, b)
        if l == len(layers) - 1:
            fw["preclamp"] = v
            break
        if bn is not None:
            gam, bet, mom = bn["gamma"].to(dtype), bn["beta"].to(dtype), bn["momentum"]
            m = v.mean(0)
            d = v - m
            q = (d * d).sum(0)
            var = q / B
            rstd = 1.0 / torch.sqrt(var + bn["eps"])
            xh = d * rstd
            p = xh * gam + bet
            unb = var if biased_running else q / (B - 1)
            rm, rv = bn["running_mean"].to(dtype), bn["running_var"].to(dtype)
            fw["mean"][l], fw["rstd"][l], fw["xhat"][l] = m, rstd, xh
            fw["running_mean"][l], fw["running_var"][l], fw["nbt"][l] = (1 - mom) * rm + mom * m, (1 - mom) * rv + mom * unb, int(bn["num_batches_tracked"]) + 1
            if e is not None:
                e_m = e.mean(0) + (B + 1) * U32 * v.abs().mean(0)
                e_d = e + e_m + U32 * d.abs()
                e_q = (2 * d.abs() * e_d + e_d * e_d).sum(0) + (B + 1) * U32 * q
                e_var = e_q / B + U32 * var
                e_rstd = 0.5 * e_var * (var + bn["eps"] - e_var).clamp_min(1e-300) ** -1.5 + 3 * U32 * rstd
                e_x = e_d * rstd + d.abs() * e_rstd + e_d * e_rstd + U32 * xh.abs()
                e = gam.abs() * e_x + U32 * p.abs()
                e_unb = e_q / (B - 1) + U32 * unb
                fw["bound"].update({f"mean{l}": e_m, f"rstd{l}": e_rstd, f"xhat{l}": e_x,
                                    f"running_mean{l}": mom * e_m + 4 * U32 * ((mom * m).abs() + ((1 - mom) * rm).abs()),
                                    f"running_var{l}": mom * e_unb + 4 * U32 * ((mom * unb).abs() + ((1 - mom) * rv).abs())})
        else:
            p = v
        y = p if slope is None else torch.where(p > 0, p, slope * p)
        if e is not None:
            fw["bound"][f"pre{l}"] = e
            if slope is not None:
                e = e + U32 * y.abs()
        fw["pre"][l], fw["act"][l] = p, y
        x = y
    pc = fw["preclamp"]
    N = pc.shape[1]
    S = N if split is None else split
    first = pc[:, :S] if clamp0 is None else pc[:, :S].clamp(*clamp0)
    second = None if S == N else (pc[:, S:] if clamp1 is None else pc[:, S:].clamp(*clamp1))
    fw.update(first=first, second=second, split=S, clamp0=clamp0, clamp1=clamp1, noise=None if noise is None else noise.to(dtype), z=None)
    if e is not None:
        fw["bound"].update(preclamp=e, first=e[:, :S], second=e[:, S:])
    if noise is not None:
        ef, es = (e[:, :S], e[:, S:]) if e is not None else (None, None)
        fw["z"], ez = reparam_b(first, ef, second, es, fw["noise"])
        if e is not None:
            fw["bound"]["z"] = ez
    return fw


def own_masks(fw):
    """leaky[l]: pre-LeakyReLU value > 0; clamp: lo <= pre-clamp <= hi (torch's rule, bounds inclusive), True where no clamp applies"""
    pc, S = fw["preclamp"], fw["split"]
    cm = torch.ones_like(pc, dtype=torch.bool)
    if fw["clamp0"] is not None:
        cm[:, :S] = (pc[:, :S] >= fw["clamp0"][0]) & (pc[:, :S] <= fw["clamp0"][1])
    if fw["clamp1"] is not None:
        cm[:, S:] = (pc[:, S:] >= fw["clamp1"][0]) & (pc[:, S:] <= fw["clamp1"][1])
    return dict(leaky={l: p > 0 for l, p in fw["pre"].items()}, clamp=cm)


def head_vjp(fw, layers, cot, masks, slope_override=None, use_clamp_mask=True):
    """cot = (g_first, g_second, g_z), each a tensor or None.  Returns dict: dW{l}, db{l}, dgamma{l}, dbeta{l}, dx (the gradient of the concatenated input).
    The forward values come from `fw` (its dtype), the masks from `masks`."""
    pc, S = fw["preclamp"], fw["split"]
    dtype, B = pc.dtype, pc.shape[0]
    g = torch.zeros_like(pc)
    g0, g1, gz = (None if c is None else c.to(dtype) for c in cot)
    if g0 is not None:
        g[:, :S] += g0
    if g1 is not None:
        g[:, S:] += g1
    if gz is not None:
        g[:, :S] += gz
        g[:, S:] += gz * fw["noise"] * 0.5 * torch.exp(0.5 * fw["second"])
    if use_clamp_mask:
        g = g * masks["clamp"].to(dtype)
    out = {}
    for l in range(len(layers) - 1, -1, -1):
        W, _b, bn, slope = layers[l]
        W = W.to(dtype)
        if l < len(layers) - 1:                    # g is the gradient of the layer's activation: LeakyReLU, then BatchNorm
            if slope is not None:
                s = slope if slope_override is None else slope_override
                g = torch.where(masks["leaky"][l], g, s * g)
            if bn is not None:
                xh, rstd, gam = fw["xhat"][l], fw["rstd"][l], bn["gamma"].to(dtype)
                dbeta, dgamma = g.sum(0), (g * xh).sum(0)
                out[f"dbeta{l}"], out[f"dgamma{l}"] = dbeta, dgamma
                out[f"db_scale{l}"] = (gam * rstd).abs() * ((g.abs() + dbeta.abs() / B + xh.abs() * dgamma.abs() / B).sum(0)
                                                            + dgamma.abs() * (rstd * fw["mean"][l].abs() + xh.abs().mean(0)))
                g = gam * rstd * (g - dbeta / B - xh * dgamma / B)
        a = fw["inputs"][l]
        out[f"dW{l}"], out[f"db{l}"] = g.T @ a, g.sum(0)
        g = g @ W
    out["dx"] = g
    return out


def head_grads(x, layers, split, clamp0, clamp1, noise, cot, masks, dtype, **kw):
    """forward in `dtype`, then the VJP in `dtype` with the given masks"""
    return head_vjp(head_forward(x, layers, split, clamp0, clamp1, noise, dtype), layers, cot, masks, **kw)


def sequential_of(layers, dtype=F64):
    """the equivalent nn.Sequential (Linear, BatchNorm1d, LeakyReLU, ..) in .train() mode, for torch.autograd"""
    import torch.nn as nn
    mods = []
    for l, (W, b, bn, slope) in enumerate(layers):
        lin = nn.Linear(W.shape[1], W.shape[0])
        lin.weight.data, lin.bias.data = W.clone().to(dtype), b.clone().to(dtype)
        mods.append(lin)
        if bn is not None:
            m = nn.BatchNorm1d(W.shape[0], eps=bn["eps"], momentum=bn["momentum"])
            m.weight.data, m.bias.data = bn["gamma"].clone().to(dtype), bn["beta"].clone().to(dtype)
            m.running_mean, m.running_var = bn["running_mean"].clone().to(dtype), bn["running_var"].clone().to(dtype)
            m.num_batches_tracked = torch.tensor(int(bn["num_batches_tracked"]))
            mods.append(m)
        if slope is not None:
            mods.append(nn.LeakyReLU(slope))
    return nn.Sequential(*mods).train()


def layers_of(layers):
    """ops.mlp_heads_train's layer list [(linear or pair, bn, slope)] on any device -> this file's [(W, b, bn dict, slope)] on the CPU, float64"""
    d = lambda t: t.detach().cpu().double().clone()
    out = []
    for lin, bn, slope in layers:
        pair = lin if isinstance(lin, (tuple, list)) else (lin,)
        W, b = torch.cat([d(p.weight) for p in pair], 0), torch.cat([d(p.bias) for p in pair], 0)
        bd = None if bn is None else dict(gamma=d(bn.weight), beta=d(bn.bias), eps=bn.eps, momentum=bn.momentum, running_mean=d(bn.running_mean),
                                          running_var=d(bn.running_var), num_batches_tracked=int(bn.num_batches_tracked))
        out.append((W, b, bd, slope))
    return out
