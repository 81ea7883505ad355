"""Float64 restatement of what ViTVAEEncoder.attention_gradients / attention_relevance and ops.mhsa_weight_grads / mhsa_relevance_step compute,
with the fp32 bounds their tests assert.  Own code on top of tests/vit_attention_reference.py and tests/vit_reference.py (imported, not edited); nothing here is
fitted to a kernel's output.

Definitions, per block, batch row b and head h of 8 (head h reads feature columns 32 h .. 32 h + 31):
    P[b, h, i, j]  = softmax_j(q_i . k_j / sqrt(32))                                   vit_attention_reference.weights_from_lse on the kernel's inputs
    gA[b, h, i, j] = sum_{d < 32} dO[b, i, 32 h + d] V[b, j, 32 h + d]                 weight_grads_ref
        the gradient with respect to P taken as a free variable (out = P V): what retain_grad() on the softmax output leaves.  dO is the cotangent of the
        attention output before out_proj.
    Abar[b, i, j]  = 1/8 sum_h max(0, gA P)                                            relevance_matrix_ref
    relevance (Chefer, Gur & Wolf 2021, the self-attention rule): R = I, then R <- R + Abar_l R for l = first .. last; the map is R's CLS row
                                                                                       relevance_matrix(mats)[:, 0]
    as a row vector: r = e_cls; for l = last .. first: r <- r + r Abar_l               relevance_vector(mats)
In the last block only the CLS output reaches a target, so dO, gA and Abar have only row 0: a matrix with fewer rows stands for one padded with zero rows.

Bounds (u = 2^-24; a value v carries e >= |computed - v|).  The references take the kernel's own inputs (q, k, v, lse, dO, r), so the inputs are exact.
    gA:  a 32-term fp32 dot product in any order (gamma_K of Higham, first order, as vit_reference.linear_b without a bias):
             e_g = 34 u sum_d |dO_d V_d|
         bf16 operands: products of bf16 values are exact in fp32 and the accumulation is fp32, so the same term holds on the bf16-exact inputs.
    t_h = max(0, gA P):  the product of two computed values and one rounding; |relu(a) - relu(b)| <= |a - b|, so the max brings in no discontinuity:
             e_t = e_g p + |gA| e_p + e_g e_p + u |gA p|          e_p: vit_attention_reference.weights_from_lse's bound
    Abar: seven fp32 adds of non-negative terms in head order and an exact scaling by 1/8 (vit_attention_reference.averaged):
             e_Abar = 1/8 sum_h e_t + 8 u Abar
    relevance step, out_j = r_j + sum_{i < nq} r_i Abar_ij:  nq products (one rounding each, or none when fused) and a sum of nq + 1 terms in an order that
    depends on the shapes alone — lane chains, their join, the chunks in index order, then r_j; any order of n + 1 terms is within (n + 1) u sum |terms|:
             e_out = sum_i |r_i| e_Abar_ij + (nq + 3) u (|r_j| + sum_i |r_i| Abar_ij)
Each bound is asserted to lie below a sanity ceiling, relative to the sum of the magnitudes it scales with, before it is used: a bound that passed everything
would test nothing.  The ceilings: e_g <= 1e-5 sum|dO V|; e_Abar <= 1e-3 mean_h(sum|dO V| p) (e_p is at most 2e-4 of p at the operand scales of the tests);
e_out <= 1e-3 (|r_j| + sum_i |r_i| mean_h(sum|dO V| p)) for nq <= 1024.

Model level: encoder_probs is the float64 (or, for the 4 x rule's yardstick, fp32 CPU) restatement of the encoder with every block's softmax output and
attention output kept in the autograd graph (retain_grad), so torch's own backward gives gA; target_sum selects what attention_gradients differentiates."""
import math

import torch

import vit_attention_reference as ar
import vit_reference as vr

U32, F64 = vr.U32, vr.F64
HEADS, HD = ar.HEADS, ar.HD


def weight_grads_ref(dout, v):
    """(gA [B, 8, nq, N], its bound e_g, sum_d |dO V|) in float64 from dout [B, nq, 256] and v [B, N, 256] (any dtype, exact values)."""
    nq, N = dout.shape[1], v.shape[1]
    gh, vh = ar.split_heads(dout.double(), nq), ar.split_heads(v.double(), N)
    g = gh @ vh.transpose(-1, -2)
    mag = gh.abs() @ vh.abs().transpose(-1, -2)
    e = 34 * U32 * mag
    assert bool((e <= 1e-5 * mag).all())
    return g, e, mag


def relevance_matrix_ref(p, e_p, g, e_g, mag):
    """(Abar [B, nq, N], e_Abar, mean_h(sum|dO V| p): the magnitudes the bound scales with) from per-head P and gA with their bounds (weights_from_lse,
    weight_grads_ref)."""
    t = torch.relu(g * p)
    e_t = e_g * p + g.abs() * e_p + e_g * e_p + U32 * (g * p).abs()
    abar = t.mean(1)
    e = e_t.mean(1) + 8 * U32 * abar
    magp = (mag * p).mean(1)
    assert bool((e <= 1e-3 * magp + 1e-300).all())
    return abar, e, magp


def relevance_step_ref(abar, e_abar, magp, r):
    """(out, bound) of one relevance step on a row vector: abar, e_abar, magp [B, nq, N] (relevance_matrix_ref), r [B, N] exact; float64."""
    nq, r = abar.shape[1], r.double()
    assert nq <= 1024
    rq = r[:, None, :nq]
    out = r + (rq @ abar)[:, 0]
    mags = r.abs() + (rq.abs() @ abar)[:, 0]
    e = (rq.abs() @ e_abar)[:, 0] + (nq + 3) * U32 * mags
    assert bool((e <= 1e-3 * (r.abs() + (rq.abs() @ magp)[:, 0]) + 1e-300).all())
    return out, e


def _square(A):
    """A block's matrix with all N rows: rows it does not hold are zero (the CLS-only last block)."""
    B, nq, N = A.shape
    return A if nq == N else torch.cat([A, torch.zeros(B, N - nq, N, dtype=A.dtype, device=A.device)], dim=1)


def relevance_matrix(mats):
    """R = I, then R <- R + Abar_l R over mats = [Abar_0 .. Abar_{L-1}], first block first: [B, N, N]."""
    B, N = mats[0].shape[0], mats[0].shape[-1]
    R = torch.eye(N, dtype=mats[0].dtype, device=mats[0].device).expand(B, N, N).clone()
    for A in mats:
        R = R + _square(A) @ R
    return R


def relevance_vector(mats, bounds=None):
    """The CLS row of relevance_matrix as the model computes it: r = e_cls, then r <- r + r Abar_l from the last block to the first: [B, N].  bounds (a list
    like mats: e_Abar): also returns the bound composed per step, e' = e + e Abar + |r| e_Abar + (nq + 3) u (|r| + |r| Abar)."""
    B, N = mats[0].shape[0], mats[0].shape[-1]
    r = torch.zeros(B, N, dtype=mats[0].dtype, device=mats[0].device)
    r[:, 0] = 1.0
    e = torch.zeros_like(r)
    for l in reversed(range(len(mats))):
        A = mats[l]
        nq = A.shape[1]
        rq, eq = r[:, None, :nq], e[:, None, :nq]
        out = r + (rq @ A)[:, 0]
        if bounds is not None:
            e = e + (eq @ A)[:, 0] + (rq.abs() @ bounds[l])[:, 0] + (nq + 3) * U32 * (r.abs() + (rq.abs() @ A)[:, 0])
        r = out
    return (r, e) if bounds is not None else r


# ---- the encoder with its attention inside the autograd graph -------------------------------------------------------------------------------------
def encoder_probs(sd, x, depth, dtype=F64):
    """vit_reference.encode_ref's arithmetic (eval mode, every block for all tokens) in `dtype` on the CPU, attention written out so that its probabilities are
    tensors of the graph.  Returns a dict: mu, log_var, cls_out, and per block the lists P ([B, 8, N, N], retain_grad), att ([B, N, 256], the attention output
    before out_proj, retain_grad) and v ([B, N, 256])."""
    get = lambda k: sd[k].to(dtype=dtype)
    h = x.to(dtype)
    B = h.shape[0]
    for i in range(5):
        h, _ = vr.stem_layer_b(h, None, sd, i, get)
    t = h.flatten(2).transpose(1, 2)
    t = (torch.cat([get("cls_token").expand(B, -1, -1), t], dim=1) + get("pos_embedding")[:, :t.shape[1] + 1]).requires_grad_(True)
    N = t.shape[1]
    ln = lambda v, g, b: vr.layernorm_b(v, None, g, b, 1e-5)[0]
    out = {"P": [], "att": [], "v": []}
    for i in range(depth):
        p = f"transformer.{i}."
        y = ln(t, get(p + "norm1.weight"), get(p + "norm1.bias"))
        q, k, v = (y @ get(p + "attn.in_proj_weight").T + get(p + "attn.in_proj_bias")).split(256, dim=-1)
        P = torch.softmax(ar.split_heads(q, N) @ ar.split_heads(k, N).transpose(-1, -2) / math.sqrt(HD), dim=-1)
        P.retain_grad()
        att = (P @ ar.split_heads(v, N)).transpose(1, 2).reshape(B, N, 256)
        att.retain_grad()
        out["P"].append(P), out["att"].append(att), out["v"].append(v)
        t = t + att @ get(p + "attn.out_proj.weight").T + get(p + "attn.out_proj.bias")
        y = ln(t, get(p + "norm2.weight"), get(p + "norm2.bias"))
        hdn = vr.gelu_b(y @ get(p + "mlp.0.weight").T + get(p + "mlp.0.bias"), None)[0]
        t = t + hdn @ get(p + "mlp.3.weight").T + get(p + "mlp.3.bias")
    c = ln(t[:, 0], get("to_latent.weight"), get("to_latent.bias"))
    out["cls_out"] = c
    out["mu"] = c @ get("fc_mu.weight").T + get("fc_mu.bias")
    out["log_var"] = c @ get("fc_var.weight").T + get("fc_var.bias")
    return out


def target_sum(out, target, index):
    """sum_{k in index} target[:, k] summed over the batch (the rows do not interact in eval mode): what attention_gradients differentiates."""
    y = out["cls_out"] if target == "cls" else out[target]
    cols = slice(None) if index is None else ([index] if isinstance(index, int) else list(index))
    return y[:, cols].sum()


def encoder_attention_grads(sd, x, depth, target="mu", index=None, dtype=F64):
    """torch autograd on encoder_probs -> dict of per-block lists: P, gA (= P.grad), datt (= att.grad), v; all detached, in `dtype`."""
    out = encoder_probs(sd, x, depth, dtype)
    target_sum(out, target, index).backward()
    return {"P": [p.detach() for p in out["P"]], "gA": [p.grad for p in out["P"]], "datt": [a.grad for a in out["att"]], "v": [v.detach() for v in out["v"]]}


def relevance_from_grads(res):
    """The relevance row [B, N] and the per-block matrices Abar_l from encoder_attention_grads' result, in its dtype."""
    mats = [torch.relu(g * p).mean(1) for g, p in zip(res["gA"], res["P"])]
    return relevance_vector(mats), mats
