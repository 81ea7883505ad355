"""The dropout of the ViT-VAE encoder's training path, restated: the mask of include/cvae_hip.h in numpy, and the float64 forward and
backward of the three dropout sites with those masks, beside tests/vit_encoder_grad_reference.py (imported, not edited).  The yardstick of
tests/test_vit_dropout*.py.  Own code.

philox4x32_10(c0, c1, c2, c3, key)      Philox4x32-10 on numpy uint32 arrays -> the four output words
threshold(p), scale(p)                  T = (uint32)((double)(float)p * 2^24) and the fp32 constant s = 1.0f / (1.0f - p)
keep_rows(M, N, p, key, row0, step)     bool [M, N]: row site, element (r, c): counter (c >> 2, lo(R), hi(R), 0), word c & 3, R = row0 + r step
keep_attn(B, N, p, key, nq)             bool [B, 8, nq, N]: attention site, element (b, h, i, j): counter (j >> 2, i, 8 b + h, 0), word j & 3
attn_fwd / attn_bwd / mlp_fwd / mlp_bwd float64 (or any dtype) with masks; transformer_vjp: the whole transformer with masks at every site

Bounds.  They have tests/vit_encoder_grad_reference.py's form, c u sum|terms| (u = 2^-24), over the MASKED terms: a dropped term is an exact zero in the
kernel and in the reference and contributes nothing.  What a dropout adds on a path: the kernel multiplies a kept value x (itself carrying an error e_x) by
the fp32 constant s.  The reference multiplies by the same fp32 s (scale(p) is that constant, exactly), so the constant itself contributes no rounding here;
counting it as one rounding all the same covers a kernel that would form s in another way, and the product x s is one more rounding.  Hence per dropout on a path
    e(x keep s) = keep s e_x + 2 u |x keep s|,
i.e. c grows by 2 on the terms that pass the mask and the operand error is scaled by s where kept, zero where dropped.  Used below:
  attention forward   out = s sum_j keep_ij P_ij v_j: vit_reference.attention_b's terms on exact operands with P replaced by P keep in the P V sum, times s,
                      + 2 u |out|.  The row statistics are the undropped row's: e_P is attention_b's.
  attention backward  dP_m = (dO V^T) keep s: e_dPm = keep s 34 u |dO||V|^T + 2 u |dP_m|;  dS = P (dP_m - delta) / sqrt(32) with gr's e_P, e_delta;
                      Pd = P keep s: e_Pd = keep s e_P + 2 u Pd;  dq, dk, dv as gr.attn_bwd_bounds with these.
  GELU epilogue       y = gelu(pre) keep s: e = keep s e_gelu + 2 u |y| (e_gelu: vit_reference.gelu_b on linear_b's bound)
  residual epilogue   y = resid + (x W^T + b) keep s: e = keep s e_lin + 2 u |(x W^T + b) keep s| + u |y|
  bwd_data            dx = (g W) keep s gelu'(pre): e = keep s (1.13 (N + 2) u |g||W| + 8 u |g W|) + (8 + 2) u |dx|
  dropout_rows        one product: exact to one rounding, u |y| (the tests compare it exactly on ones)."""
import math

import numpy as np
import torch

import vit_encoder_grad_reference as gr
import vit_reference as vr
from vit_reference import F64, U32

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, key):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    return int(np.float64(np.float32(p)) * 16777216.0)


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def _keep(words, p):
    """words: 4 arrays [..., n4] -> bool [..., 4 n4]"""
    w = np.stack(words, axis=-1)
    return ((w >> np.uint32(8)) >= np.uint32(threshold(p))).reshape(*w.shape[:-2], -1)


def keep_rows(M, N, p, key, row0=0, step=1):
    assert N % 4 == 0
    R = (row0 + np.arange(M, dtype=np.uint64) * np.uint64(step))[:, None]
    c = np.arange(N // 4, dtype=np.uint64)[None, :]
    return _keep(philox4x32_10(c, R & MASK32, R >> np.uint64(32), 0, key), p)


def keep_attn(B, N, p, key, nq=None):
    nq = N if nq is None else nq
    n4 = (N + 3) // 4
    bh = np.arange(B * 8, dtype=np.uint64).reshape(B, 8, 1, 1)
    i = np.arange(nq, dtype=np.uint64).reshape(1, 1, nq, 1)
    j4 = np.arange(n4, dtype=np.uint64).reshape(1, 1, 1, n4)
    return _keep(philox4x32_10(j4, i, bh, 0, key), p)[..., :N]


def tmask(keep, p, dtype=F64):
    """keep (numpy bool) -> the multiplier keep * s as a torch tensor"""
    return torch.from_numpy(np.ascontiguousarray(keep)).to(dtype) * float(scale(p))


# ---- attention -----------------------------------------------------------------------------------------------------------------------------------
def attn_fwd(q, k, v, m, nq=None):
    """m [B, 8, nq, N] = keep * s -> (out [B, nq, 256], lse [B, 8, nq] natural log, of the undropped rows)"""
    nq = k.shape[1] if nq is None else nq
    qh, kh, vh = gr.split_heads(q[:, :nq]), gr.split_heads(k), gr.split_heads(v)
    s = (qh @ kh.transpose(-1, -2)) * gr.SCALE
    mx = s.amax(-1, keepdim=True)
    pu = torch.exp(s - mx)
    l = pu.sum(-1, keepdim=True)
    return gr.merge_heads(((pu / l) * m) @ vh), (mx + torch.log(l)).squeeze(-1)


def attn_fwd_bound(q, k, v, m, nq=None):
    """element-wise bound [B, nq, 256] of mhsa_train(dropout) on exact operands (module docstring)"""
    N = k.shape[1]
    nq = N if nq is None else nq
    qh, kh, vh = gr.split_heads(q[:, :nq]), gr.split_heads(k), gr.split_heads(v)
    s = (qh @ kh.transpose(-1, -2)) * gr.SCALE
    mx = s.amax(-1, keepdim=True)
    p = torch.softmax(s, -1)
    es = 35 * U32 * (qh.abs() @ kh.abs().transpose(-1, -2)) * gr.SCALE + 4 * U32 * (s.abs() + mx.abs())
    ep = p * (es + (p * es).sum(-1, keepdim=True) + (N + N / 32 + 12) * U32)
    pm = p * m
    eo = (ep * m) @ vh.abs() + (N + N / 32 + 8) * U32 * (pm @ vh.abs()) + 2 * U32 * (pm @ vh).abs()
    return gr.merge_heads(eo)


def attn_bwd(q, k, v, out, lse, dout, m, parts=False):
    nq = out.shape[1]
    qh, kh, vh, oh, gh = gr.split_heads(q[:, :nq]), gr.split_heads(k), gr.split_heads(v), gr.split_heads(out), gr.split_heads(dout)
    s = (qh @ kh.transpose(-1, -2)) * gr.SCALE
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = (gh @ vh.transpose(-1, -2)) * m
    delta = (gh * oh).sum(-1, keepdim=True)
    ds = p * (dp - delta) * gr.SCALE
    dq, dk, dv = ds @ kh, ds.transpose(-1, -2) @ qh, (p * m).transpose(-1, -2) @ gh
    if parts:
        return dict(qh=qh, kh=kh, vh=vh, oh=oh, gh=gh, s=s, p=p, dp=dp, delta=delta, ds=ds, dk=dk, lse=lse, m=m)
    return gr.merge_heads(dq), gr.merge_heads(dk), gr.merge_heads(dv)


def _e_ds(P):
    qa, ka, m = P["qh"].abs(), P["kh"].abs(), P["m"]
    e_p = P["p"] * (35 * U32 * gr.SCALE * (qa @ ka.transpose(-1, -2)) + 8 * U32 * (P["s"].abs() + P["lse"].abs().unsqueeze(-1)) + 4 * U32)
    e_dp = m * 34 * U32 * (P["gh"].abs() @ P["vh"].abs().transpose(-1, -2)) + 2 * U32 * P["dp"].abs()
    e_delta = 34 * U32 * (P["gh"] * P["oh"]).abs().sum(-1, keepdim=True)
    return e_p, (P["p"] * (e_dp + e_delta) + e_p * (P["dp"] - P["delta"]).abs()) * gr.SCALE + 3 * U32 * P["ds"].abs()


def attn_bwd_bounds(P):
    """(e_dq, e_dk, e_dv) merged to [B, n, 256], of mhsa_bwd(dropout) on exact fp32 operands (module docstring)"""
    nq, N = P["s"].shape[-2:]
    e_p, e_ds = _e_ds(P)
    ds, pd = P["ds"].abs(), P["p"] * P["m"]
    qa, ka, ga = P["qh"].abs(), P["kh"].abs(), P["gh"].abs()
    e_pd = P["m"] * e_p + 2 * U32 * pd
    e_dq = e_ds @ ka + (N + 2) * U32 * (ds @ ka)
    e_dk = e_ds.transpose(-1, -2) @ qa + (nq + 2) * U32 * (ds.transpose(-1, -2) @ qa)
    e_dv = e_pd.transpose(-1, -2) @ ga + (nq + 2) * U32 * (pd.transpose(-1, -2) @ ga)
    return gr.merge_heads(e_dq), gr.merge_heads(e_dk), gr.merge_heads(e_dv)


def k_bias_bound(P):
    """gr.k_bias_bound with the masked e_dS (the k bias's gradient is zero in exact arithmetic with dropout too: sum_j P_ij dPm_ij = dO_i . out_i)"""
    nq = P["s"].shape[-2]
    _e_p, e_ds = _e_ds(P)
    qa = P["qh"].abs()
    dsq = P["ds"].abs().transpose(-1, -2) @ qa
    b = e_ds.transpose(-1, -2) @ qa + (nq + 2) * U32 * dsq + 4 * U32 * P["dk"].abs()
    return b.sum(dim=(0, 2)).reshape(gr.HEADS * gr.HD)


# ---- MLP sites -----------------------------------------------------------------------------------------------------------------------------------
def gelu_dropout(x, W, b, m):
    """-> (gelu(pre) m, pre, bound of the first, bound of pre)"""
    pre, e_pre = vr.linear_b(x, torch.zeros_like(x), W, b)
    y, e = vr.gelu_b(pre, e_pre)
    return y * m, pre, m * e + 2 * U32 * (y * m).abs(), e_pre


def resid_dropout(x, W, b, resid, m):
    lin, e = vr.linear_b(x, torch.zeros_like(x), W, b)
    y = resid + lin * m
    return y, m * e + 2 * U32 * (lin * m).abs() + U32 * y.abs()


def bwd_data_dropout(g, W, pre, m):
    N = g.shape[1]
    gw = g @ W
    dx = gw * m * gr.gelu_grad(pre)
    return dx, m * (1.13 * (N + 2) * U32 * (g.abs() @ W.abs()) + 8 * U32 * gw.abs()) + 10 * U32 * dx.abs()


# ---- the whole transformer with masks ----------------------------------------------------------------------------------------------------------
def block_masks(B, N, rates, keys, dtype=F64, cls_only=False):
    """the three multipliers keep * s of one block: att [B, 8, nq, N], act [B, n, 512], out [B, n, 256] (n = nq = 1 in a CLS-only block: the rows b N)"""
    (pa, pg, po), (ka, kg, ko) = rates, keys
    rows = lambda cols, p, key: tmask(keep_rows(B * N, cols, p, key), p, dtype).view(B, N, cols)[:, :1 if cls_only else N]
    return dict(att=tmask(keep_attn(B, N, pa, ka, 1 if cls_only else N), pa, dtype), act=rows(512, pg, kg), out=rows(256, po, ko))


def transformer_vjp(sd, stem, depth, g_mu, g_lv, masks, dtype=F64, cls_only_last=False, want_parts=False):
    """gr.transformer_vjp (no rounding oracle, no wrong variants) with dropout at the three sites of every block: masks[i] = block_masks(...) of block i.
    -> (grads, out) as there."""
    get = lambda k: sd[k].detach().to(dtype=dtype, device=stem.device)
    stem = stem.to(dtype)
    B, Np, D = stem.shape
    t = torch.cat([get("cls_token").expand(B, -1, -1), stem], dim=1) + get("pos_embedding")[:, :Np + 1]
    saved = []
    for i in range(depth):
        p = f"transformer.{i}."
        W = {n: get(p + n) for n in ("norm1.weight", "norm1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
                                     "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")}
        m = {k: v.to(dtype) for k, v in masks[i].items()}
        nq = 1 if (cls_only_last and i == depth - 1) else None
        y, ln1 = gr.ln_fwd(t, W["norm1.weight"], W["norm1.bias"])
        qkv = y @ W["attn.in_proj_weight"].T + W["attn.in_proj_bias"]
        q, k, v = qkv.split(D, dim=-1)
        att, lse = attn_fwd(q, k, v, m["att"], nq)
        x1 = (t[:, :1] if nq else t) + att @ W["attn.out_proj.weight"].T + W["attn.out_proj.bias"]
        y2, ln2 = gr.ln_fwd(x1, W["norm2.weight"], W["norm2.bias"])
        pre = y2 @ W["mlp.0.weight"].T + W["mlp.0.bias"]
        hid = gr.gelu(pre) * m["act"]
        x2 = x1 + (hid @ W["mlp.3.weight"].T + W["mlp.3.bias"]) * m["out"]
        saved.append(dict(W=W, m=m, nq=nq, ln1=ln1, y=y, q=q, k=k, v=v, att=att, lse=lse, ln2=ln2, y2=y2, pre=pre, hid=hid))
        t = x2
    c, lnl = gr.ln_fwd(t[:, 0], get("to_latent.weight"), get("to_latent.bias"))
    out = {"cls_out": c, "mu": c @ get("fc_mu.weight").T + get("fc_mu.bias"), "log_var": c @ get("fc_var.weight").T + get("fc_var.bias")}
    g_mu, g_lv = g_mu.to(dtype), g_lv.to(dtype)
    grads = {"fc_mu.weight": g_mu.T @ c, "fc_mu.bias": g_mu.sum(0), "fc_var.weight": g_lv.T @ c, "fc_var.bias": g_lv.sum(0)}
    gc = g_mu @ get("fc_mu.weight") + g_lv @ get("fc_var.weight")
    gcls, grads["to_latent.weight"], grads["to_latent.bias"] = gr.ln_bwd(gc, lnl, get("to_latent.weight"))
    G = torch.zeros_like(t)
    G[:, 0] = gcls
    flat = lambda a: a.reshape(-1, a.shape[-1])
    parts = []
    for i in reversed(range(depth)):
        s, p = saved[i], f"transformer.{i}."
        W, m = s["W"], s["m"]
        Gm = G * m["out"]                                                  # the MLP branch's cotangent; the skip carries G
        dpre = (Gm @ W["mlp.3.weight"]) * m["act"] * gr.gelu_grad(s["pre"])
        grads[p + "mlp.3.weight"], grads[p + "mlp.3.bias"] = flat(Gm).T @ flat(s["hid"]), flat(Gm).sum(0)
        dy2 = dpre @ W["mlp.0.weight"]
        grads[p + "mlp.0.weight"], grads[p + "mlp.0.bias"] = flat(dpre).T @ flat(s["y2"]), flat(dpre).sum(0)
        d, grads[p + "norm2.weight"], grads[p + "norm2.bias"] = gr.ln_bwd(dy2, s["ln2"], W["norm2.weight"])
        G = G + d
        datt = G @ W["attn.out_proj.weight"]
        grads[p + "attn.out_proj.weight"], grads[p + "attn.out_proj.bias"] = flat(G).T @ flat(s["att"]), flat(G).sum(0)
        if want_parts:
            parts.append(attn_bwd(s["q"], s["k"], s["v"], s["att"], s["lse"], datt, m["att"], parts=True))
        dq, dk, dv = attn_bwd(s["q"], s["k"], s["v"], s["att"], s["lse"], datt, m["att"])
        Win = W["attn.in_proj_weight"]
        if s["nq"]:
            dkv = torch.cat([dk, dv], dim=-1)
            dy = dkv @ Win[D:]
            dy[:, 0] = dy[:, 0] + dq[:, 0] @ Win[:D]
            grads[p + "attn.in_proj_weight"] = torch.cat([dq[:, 0].T @ s["y"][:, 0], flat(dkv).T @ flat(s["y"])], dim=0)
            grads[p + "attn.in_proj_bias"] = torch.cat([dq[:, 0].sum(0), flat(dkv).sum(0)], dim=0)
            d, grads[p + "norm1.weight"], grads[p + "norm1.bias"] = gr.ln_bwd(dy, s["ln1"], W["norm1.weight"])
            G, g0 = d, G
            G[:, 0] = G[:, 0] + g0[:, 0]
        else:
            dqkv = torch.cat([dq, dk, dv], dim=-1)
            dy = dqkv @ Win
            grads[p + "attn.in_proj_weight"], grads[p + "attn.in_proj_bias"] = flat(dqkv).T @ flat(s["y"]), flat(dqkv).sum(0)
            d, grads[p + "norm1.weight"], grads[p + "norm1.bias"] = gr.ln_bwd(dy, s["ln1"], W["norm1.weight"])
            G = G + d
    grads["pos_embedding"] = G.sum(0, keepdim=True)
    grads["cls_token"] = G[:, :1].sum(0, keepdim=True)
    grads["dstem"] = G[:, 1:]
    if want_parts:
        grads["k_bias_parts"] = parts[::-1]
    return grads, out
