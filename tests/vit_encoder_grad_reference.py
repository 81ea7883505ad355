"""The vector-Jacobian product of the ViT-VAE encoder's transformer (tokens -> six blocks -> to_latent -> fc_mu / fc_var, eval mode), written out stage by
stage in plain torch ops beside tests/vit_reference.py's forward: the yardstick of tests/test_vit_encoder_grad*.py.  Own code; it reads a state_dict with the
reference's keys and the stem's output, nothing else.  The stem is a frozen feature extractor here: the gradient stops at `dstem`.

transformer_vjp(sd, stem, depth, g_mu, g_lv)                       float64 gradients of every transformer-side parameter, and dstem
transformer_vjp(..., dtype=torch.float32)                         the same restatement evaluated in fp32 on the CPU (the "4 x" rule's denominator)
transformer_vjp(..., rnd=round_bf16)                              the ROUNDING ORACLE: float64 arithmetic, rounded to bf16 exactly where the bf16 kernels round:
        forward as vit_reference.encode_ref (LayerNorm output, GEMM weights, QKV, attention output, MLP hidden), the saved GELU pre-activation; backward:
        every cotangent of a tensor the forward stores in bf16 (d hidden, d y2, d attention output, dq / dk / dv, d y), the fp32 stream gradient where it
        enters a GEMM as an operand, P and dS for their products.  The stream gradient itself, every LayerNorm backward and every parameter gradient stay
        unrounded (fp32 in the kernels).
transformer_vjp(..., wrong="dk_from_p" / "dgamma_no_xhat")        two deliberately wrong restatements (what the yardstick must refuse)

Per-kernel constants c of the element-wise bounds c u sum|terms| (u = 2^-24), counted from the kernels' own operations on exact operands:
  token_gemm_bwd_data   N-term dot product in fp32, any order: c = N + 2; the GELU gate multiplies by g' with |g'| <= 1.13 computed to 8 u (erff, expf, two
                        products): e = 1.13 (N + 2) u sum|g W| + 8 u |dx|; the residual add: + u |dx|.  bf16 result: + 2^-8 |dx|.
  token_gemm_wgrad      M-term dot product: 64-token chunks inside a slab, slabs in order: c = M + 2.  Bias: compensated inside a thread and across
                        threads and slabs: c = 4 (2 u of Kahan's first-order term, twice) + M u^2 terms, written c = 4 + M 2^-20.
  layernorm256_bwd      xhat as the forward (vit_reference.layernorm_b on exact input: e_xhat); a = gamma g: 1 u; two 256-term means: 258 u each;
                        dx = rstd (a - m1 - xhat m2): e = rstd (|a| (u + 258 u) + 258 u mean|a| + |xhat| 258 u mean|a xhat| + e_xhat |m2| + mean(|a| e_xhat) |xhat|)
                        + 6 u |dx| + e_rstd |dx|, with e_rstd = 140 u.  dgamma / dbeta: R-term sums (32-row slabs, compensated finish): c = 40 + R / 32 is
                        generous; the tests use c = R + 2 (a plain chain's).
  mhsa_bwd              P = exp(s - lse): e_P = P (35 u |q|.|k| / sqrt(32) + 8 u (|s| + |lse|) + 4 u); dP, delta: 32-term dots, c = 34;
                        dS = P (dP - delta) / sqrt(32): e_dS = (P (e_dP + e_delta) + e_P |dP - delta|) / sqrt(32) + 3 u |dS|;
                        dq = dS K (N terms), dk = dS^T Q, dv = P^T dO (Nq terms): e = e_dS |K| + (N + 2) u |dS||K| and alike.
                        bf16: P and dS are rounded for their products (+ 2^-8 |dS||K| etc.), results are bf16 (+ 2^-8 |.|).
  vit_tokens_bwd        B-term sums: c = B.

The k-bias exception.  in_proj_bias[256:512] (the k bias) has the gradient sum_{b, key} dk[b, key, n] = sum_q Q[q, n] sum_key dS[q, key] = 0 in exact
arithmetic, whatever q, k, v and dO are (softmax is shift-invariant along the keys).  What a kernel returns there is rounding noise, and a ratio of two noises
proves nothing, so it is held to the element-wise bound k_bias_bound(): |db_k[n]| <= sum_{b, q, key} e_dS[q, key] |Q[q, n]| + (Nq + 2) u sum |dS||Q| +
4 u sum_m |dk[m, n]|; bf16 adds 2^-8 (2 sum |dS||Q| + sum_m |dk[m, n]|) (dS rounded for the product, on both sides; dk stored in bf16) and, in e_dS, the saved attention
output's rounding 2^-8 P rowsum|dO O| / sqrt(32).  The bound uses the float64 stage values (the difference to the computed ones is second order)."""
import math

import torch

from vit_reference import F64, U32, UBF, round_bf16  # noqa: F401

HEADS, HD = 8, 32
SCALE = 1.0 / math.sqrt(HD)


def ln_fwd(x, g, b, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd * g + b, (d * rstd, rstd)


def ln_bwd(gy, saved, g, wrong=None):
    xhat, rstd = saved
    a = gy * g
    dx = rstd * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
    flat = lambda t: t.reshape(-1, t.shape[-1])
    dgamma = flat(gy).sum(0) if wrong == "dgamma_no_xhat" else flat(gy * xhat).sum(0)
    return dx, dgamma, flat(gy).sum(0)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def split_heads(t):
    B, n, _ = t.shape
    return t.reshape(B, n, HEADS, HD).transpose(1, 2)


def merge_heads(t):
    B, _h, n, _d = t.shape
    return t.transpose(1, 2).reshape(B, n, HEADS * HD)


def attn_fwd(q, k, v, nq=None, rnd=None):
    """as vit_reference.attention_b (P rounded unnormalised, its row sum not) -> (out [B, nq, 256], lse [B, 8, nq] natural log)"""
    nq = k.shape[1] if nq is None else nq
    qh, kh, vh = split_heads(q[:, :nq]), split_heads(k), split_heads(v)
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    mx = s.amax(-1, keepdim=True)
    pu = torch.exp(s - mx)
    l = pu.sum(-1, keepdim=True)
    o = ((rnd(pu) if rnd is not None else pu) @ vh) / l
    return merge_heads(o), (mx + torch.log(l)).squeeze(-1)


def attn_bwd(q, k, v, out, lse, dout, rnd=None, wrong=None, parts=False):
    """(dq [B, nq, 256], dk, dv [B, N, 256]) from the saved out and lse: P = exp(s - lse), delta = rowsum(dout * out), dS = P (dP - delta) / sqrt(32)."""
    r = rnd if rnd is not None else (lambda t: t)
    nq = out.shape[1]
    qh, kh, vh, oh, gh = split_heads(q[:, :nq]), split_heads(k), split_heads(v), split_heads(out), split_heads(dout)
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = gh @ vh.transpose(-1, -2)
    delta = (gh * oh).sum(-1, keepdim=True)
    ds = p * (dp - delta) * SCALE
    dq = r(ds) @ kh
    dk = (r(p) if wrong == "dk_from_p" else r(ds)).transpose(-1, -2) @ qh
    dv = r(p).transpose(-1, -2) @ gh
    if parts:
        return dict(qh=qh, kh=kh, vh=vh, oh=oh, gh=gh, s=s, p=p, dp=dp, delta=delta, ds=ds, dk=dk, lse=lse)
    return merge_heads(dq), merge_heads(dk), merge_heads(dv)


def k_bias_bound(parts, bf16):
    """the element-wise bound on the k-bias gradient (module docstring) -> [256] float64"""
    P = parts
    nq = P["s"].shape[-2]
    _e_p, e_ds = _e_ds(P, bf16)
    qa = P["qh"].abs()
    dsq = P["ds"].abs().transpose(-1, -2) @ qa                              # [B, 8, N, 32]: sum_q |dS||Q|
    b = e_ds.transpose(-1, -2) @ qa + (nq + 2) * U32 * dsq + 4 * U32 * P["dk"].abs()
    if bf16:
        b = b + 2 * UBF * dsq + UBF * P["dk"].abs()
    return b.sum(dim=(0, 2)).reshape(HEADS * HD)


def _e_ds(P, bf16):
    qa, ka = P["qh"].abs(), P["kh"].abs()
    e_p = P["p"] * (35 * U32 * SCALE * (qa @ ka.transpose(-1, -2)) + 8 * U32 * (P["s"].abs() + P["lse"].abs().unsqueeze(-1)) + 4 * U32)
    e_dp = 34 * U32 * (P["gh"].abs() @ P["vh"].abs().transpose(-1, -2))
    e_delta = (34 * U32 + (UBF if bf16 else 0.0)) * (P["gh"] * P["oh"]).abs().sum(-1, keepdim=True)
    return e_p, (P["p"] * (e_dp + e_delta) + e_p * (P["dp"] - P["delta"]).abs()) * SCALE + 3 * U32 * P["ds"].abs()


def attn_bwd_bounds(parts, bf16, exact_out=True):
    """element-wise bounds (e_dq, e_dk, e_dv), merged to [B, n, 256], of mhsa_bwd on exact operands (module docstring).  exact_out: `out` is an operand
    as given (a kernel tested alone), so delta carries no rounding of a saved output.  bf16: the kernel and the reference each round P and dS once, at
    values that differ by their fp32 error: up to one bf16 step, 2 x 2^-8, on each product term; the results are bf16."""
    P = parts
    nq, N = P["s"].shape[-2:]
    e_p, e_ds = _e_ds(P, bf16 and not exact_out)
    ds, p, ob = P["ds"].abs(), P["p"], (2 * UBF if bf16 else 0.0)
    qa, ka, ga = P["qh"].abs(), P["kh"].abs(), P["gh"].abs()
    e_dq = e_ds @ ka + ((N + 2) * U32 + ob) * (ds @ ka)
    e_dk = e_ds.transpose(-1, -2) @ qa + ((nq + 2) * U32 + ob) * (ds.transpose(-1, -2) @ qa)
    e_dv = e_p.transpose(-1, -2) @ ga + ((nq + 2) * U32 + ob) * (p.transpose(-1, -2) @ ga)
    if bf16:
        e_dq = e_dq + UBF * ((P["ds"] @ P["kh"]).abs() + e_dq)
        e_dk = e_dk + UBF * ((P["ds"].transpose(-1, -2) @ P["qh"]).abs() + e_dk)
        e_dv = e_dv + UBF * ((p.transpose(-1, -2) @ P["gh"]).abs() + e_dv)
    return merge_heads(e_dq), merge_heads(e_dk), merge_heads(e_dv)


def ln_bwd_bounds(x, gy, g, eps=1e-5):
    """element-wise bounds (e_dx [R, 256], e_dgamma [256], e_dbeta [256]) of layernorm256_bwd on exact operands (module docstring)."""
    from vit_reference import layernorm_b
    R = x.shape[0]
    _y, (xhat, rstd) = ln_fwd(x, g, torch.zeros_like(g), eps)
    _v, e_xh = layernorm_b(x, torch.zeros_like(x), torch.ones_like(g), torch.zeros_like(g), eps)
    a = gy * g
    mean = lambda t: t.mean(-1, keepdim=True)
    m2 = mean(a * xhat)
    dx = rstd * (a - mean(a) - xhat * m2)
    e_dx = rstd * (259 * U32 * a.abs() + 258 * U32 * mean(a.abs()) + xhat.abs() * 258 * U32 * mean((a * xhat).abs()) + e_xh * m2.abs()
                   + mean(a.abs() * e_xh) * xhat.abs()) + 146 * U32 * dx.abs()
    e_dg = (R + 2) * U32 * (gy * xhat).abs().sum(0) + (gy.abs() * e_xh).sum(0)
    return e_dx, e_dg, (R + 2) * U32 * gy.abs().sum(0)


def transformer_vjp(sd, stem, depth, g_mu, g_lv, dtype=F64, rnd=None, cls_only_last=False, wrong=None, want_parts=False, g_cls=None):
    """stem [B, Np, 256] (the stem's output, `b (h w) c`); g_mu, g_lv [B, latent] the cotangents of (mu, log_var).
    Returns (grads, out): grads = {state_dict key: gradient} for pos_embedding, cls_token, transformer.*, to_latent.*, fc_mu.*, fc_var.* plus "dstem"
    [B, Np, 256] (and "k_bias_parts": attn_bwd's parts per block, with want_parts); out = {"cls_out", "mu", "log_var"}.
    g_cls [B, 256] (with g_mu = g_lv = None): the cotangent of the cls features themselves, for a consumer that reads them and not (mu, log_var); the
    fc_mu / fc_var entries are then absent."""
    get = lambda k: sd[k].detach().to(dtype=dtype, device=stem.device)
    r = rnd if rnd is not None else (lambda t: t)
    stem = stem.to(dtype)
    B, Np, D = stem.shape
    t = torch.cat([get("cls_token").expand(B, -1, -1), stem], dim=1) + get("pos_embedding")[:, :Np + 1]
    saved = []
    for i in range(depth):
        p = f"transformer.{i}."
        W = {n: get(p + n) for n in ("norm1.weight", "norm1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                                     "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")}
        nq = 1 if (cls_only_last and i == depth - 1) else None
        y, ln1 = ln_fwd(t, W["norm1.weight"], W["norm1.bias"])
        y = r(y)
        qkv = r(y @ r(W["attn.in_proj_weight"]).T + W["attn.in_proj_bias"])
        q, k, v = qkv.split(D, dim=-1)
        att, lse = attn_fwd(q, k, v, nq, rnd)
        att = r(att)
        x1 = (t[:, :1] if nq else t) + att @ r(W["attn.out_proj.weight"]).T + W["attn.out_proj.bias"]
        y2, ln2 = ln_fwd(x1, W["norm2.weight"], W["norm2.bias"])
        y2 = r(y2)
        pre = y2 @ r(W["mlp.0.weight"]).T + W["mlp.0.bias"]
        hid = r(gelu(pre))
        x2 = x1 + hid @ r(W["mlp.3.weight"]).T + W["mlp.3.bias"]
        saved.append(dict(W=W, nq=nq, ln1=ln1, y=y, q=q, k=k, v=v, att=att, lse=lse, ln2=ln2, y2=y2, pre=r(pre), hid=hid, n_in=t.shape[1]))
        t = x2
    c, lnl = ln_fwd(t[:, 0], get("to_latent.weight"), get("to_latent.bias"))
    out = {"cls_out": c, "mu": c @ get("fc_mu.weight").T + get("fc_mu.bias"), "log_var": c @ get("fc_var.weight").T + get("fc_var.bias")}

    if g_cls is None:
        g_mu, g_lv = g_mu.to(dtype), g_lv.to(dtype)
        grads = {"fc_mu.weight": g_mu.T @ c, "fc_mu.bias": g_mu.sum(0), "fc_var.weight": g_lv.T @ c, "fc_var.bias": g_lv.sum(0)}
        gc = g_mu @ get("fc_mu.weight") + g_lv @ get("fc_var.weight")
    else:
        grads, gc = {}, g_cls.to(dtype)
    gcls, grads["to_latent.weight"], grads["to_latent.bias"] = ln_bwd(gc, lnl, get("to_latent.weight"), wrong)
    G = torch.zeros_like(t)
    G[:, 0] = gcls
    flat = lambda a: a.reshape(-1, a.shape[-1])
    parts = []
    for i in reversed(range(depth)):
        s, p = saved[i], f"transformer.{i}."
        W = s["W"]
        Gr = r(G)                                                        # the stream gradient as a GEMM operand
        dpre = r((Gr @ r(W["mlp.3.weight"])) * gelu_grad(s["pre"]))     # one rounding: the gate is applied in the GEMM's epilogue
        grads[p + "mlp.3.weight"], grads[p + "mlp.3.bias"] = flat(Gr).T @ flat(s["hid"]), flat(G).sum(0)
        dy2 = r(dpre @ r(W["mlp.0.weight"]))
        grads[p + "mlp.0.weight"], grads[p + "mlp.0.bias"] = flat(dpre).T @ flat(s["y2"]), flat(dpre).sum(0)
        d, grads[p + "norm2.weight"], grads[p + "norm2.bias"] = ln_bwd(dy2, s["ln2"], W["norm2.weight"], wrong)
        G = G + d
        Gr = r(G)
        datt = r(Gr @ r(W["attn.out_proj.weight"]))
        grads[p + "attn.out_proj.weight"], grads[p + "attn.out_proj.bias"] = flat(Gr).T @ flat(s["att"]), flat(G).sum(0)
        if want_parts:
            parts.append(attn_bwd(s["q"], s["k"], s["v"], s["att"], s["lse"], datt, rnd, parts=True))
        dq, dk, dv = (r(a) for a in attn_bwd(s["q"], s["k"], s["v"], s["att"], s["lse"], datt, rnd, wrong))
        Win = r(W["attn.in_proj_weight"])
        if s["nq"]:
            dkv = torch.cat([dk, dv], dim=-1)
            dy = dkv @ Win[D:]
            dy[:, 0] = dy[:, 0] + dq[:, 0] @ Win[:D]
            dWq, dbq = dq[:, 0].T @ s["y"][:, 0], dq[:, 0].sum(0)
            grads[p + "attn.in_proj_weight"] = torch.cat([dWq, flat(dkv).T @ flat(s["y"])], dim=0)
            grads[p + "attn.in_proj_bias"] = torch.cat([dbq, flat(dkv).sum(0)], dim=0)
            d, grads[p + "norm1.weight"], grads[p + "norm1.bias"] = ln_bwd(dy, s["ln1"], W["norm1.weight"], wrong)
            G, g0 = d, G
            G[:, 0] = G[:, 0] + g0[:, 0]
        else:
            dqkv = torch.cat([dq, dk, dv], dim=-1)
            dy = r(dqkv @ Win)
            grads[p + "attn.in_proj_weight"], grads[p + "attn.in_proj_bias"] = flat(dqkv).T @ flat(s["y"]), flat(dqkv).sum(0)
            d, grads[p + "norm1.weight"], grads[p + "norm1.bias"] = ln_bwd(dy, s["ln1"], W["norm1.weight"], wrong)
            G = G + d
    grads["pos_embedding"] = G.sum(0, keepdim=True)
    grads["cls_token"] = G[:, :1].sum(0, keepdim=True)
    grads["dstem"] = r(G[:, 1:])
    if want_parts:
        grads["k_bias_parts"] = parts[::-1]
    return grads, out


def rel_l2(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float((a - b).norm() / b.norm())
