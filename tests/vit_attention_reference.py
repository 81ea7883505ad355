"""Float64 restatement of what ViTVAEEncoder.attention_weights / attention_rollout and ops.mhsa_weights / mhsa_rollout_step compute, with the
fp32 bounds their tests assert.  Own code, in the style of tests/vit_reference.py (which it imports and does not edit); nothing here is fitted to a
kernel's output.

Definitions.  For one nn.MultiheadAttention(256, 8) in eval mode with queries q [B, nq, 256] and keys k [B, N, 256] (the in-projection's outputs), head h
reads columns 32 h .. 32 h + 31 and
    P[b, h, i, j] = softmax_j(q_i . k_j / sqrt(32))                        head_weights(q, k)            (need_weights=True, average_attn_weights=False)
    Abar[b, i, j] = mean_h P[b, h, i, j]                                    head_weights(q, k).mean(1)    (average_attn_weights=True)
Attention rollout (Abnar & Zuidema 2020) from the CLS token over blocks 0 .. L-1 with residual weight a:
    R = prod_l (a I + (1 - a) Abar_l), the LAST block leftmost;  rollout = R[cls, :]                      rollout_matrix(...)[:, 0]
    as a row vector: r = e_cls; for l = L-1 .. 0: r <- a r + (1 - a) r Abar_l                              rollout_vector(...)
A block whose matrix has only its first nq rows (the CLS-only last block) contributes those rows and the residual term for all N entries; with r = e_cls
that is the full matrix's result.

What the kernels compute, and their bounds (u = 2^-24; a value v carries e >= |computed - v|).  The kernels never normalise: they recompute
    P = 2^(s - lse),  s = (q . k) c,  c = log2(e) / sqrt(32)
from q, k and the fp32 row statistic lse the attention forward left.  weights_from_lse is that expression in float64 ON THE KERNEL'S OWN INPUTS (lse
included), so the inputs are exact and only the local terms remain:
    s:  a 32-term fp32 dot product in any order, then the product with the fp32 constant c (one rounding each for c and the product):
        e_dot = 35 u c sum_d |q_d k_d|;  the exp2 argument s - lse is one fma or two roundings of values |s|, |lse|:  e_s = e_dot + 4 u (|s| + |lse|)
    p = 2^x:  dp = ln 2 p dx, exp2f itself a few ulp:   e_p = p (ln 2 e_s + 4 u)
    averaged over heads: seven fp32 adds of non-negative terms and an exact scaling by 1/8: + 8 u Abar
bf16 operands: products of bf16 values are exact in fp32 and everything after them is fp32, so the same terms hold on the bf16-exact inputs.
Rows sum to one only as far as the forward's lse is the row's log-sum: the forward adds N terms of 2^(s - m) with one rescale per 32-key tile, takes
log2 and adds the maximum m, on scores that carry e_dot + 4 u (|s| + |m|) themselves:
    |sum_j p_j - 1| <= sum_j e_p_j + (N + N / 32 + 12) u + sum_j p_j ln 2 (e_dot_j + 4 u (|s_j| + |m|)) + 4 ln 2 u (|lse| + |m|)          rowsum_bound
    (attention_b's (N + N/32 + 12) u, the p-weighted mean of the forward's score error, and the rounding of log2 l and of m + log2 l)
mhsa_rollout_step sums 8 nq products r_i p per key (two fp32 chains of half of them, joined), scales twice and adds the residual term:
    e_out = (1 - a) / 8 sum_h sum_i |r_i| e_p + (8 nq + 4) u (a |r_j| + (1 - a) / 8 sum_h sum_i |r_i| p)                                  rollout_step_ref
Compared with r @ Abar formed in float64 from mhsa_weights' OWN averaged output, 2 e_p (+ 8 u Abar) takes e_p's place: two kernels round independently."""
import math

import torch

import vit_reference as vr

U32, F64 = vr.U32, vr.F64
HEADS, HD = 8, 32
C_LOG2 = math.log2(math.e) / math.sqrt(HD)
LN2 = math.log(2.0)


def split_heads(t, n):
    """[B, >= n, 256] -> [B, 8, n, 32]"""
    return t[:, :n].reshape(t.shape[0], n, HEADS, HD).transpose(1, 2)


def head_weights(q, k, n_query_rows=None):
    """softmax(q k^T / sqrt(32)) per head: [B, 8, nq, N] in the operands' dtype (float64 for a reference)."""
    N = k.shape[1]
    nq = N if n_query_rows is None else n_query_rows
    s = split_heads(q, nq) @ split_heads(k, N).transpose(-1, -2) / math.sqrt(HD)
    return torch.softmax(s, dim=-1)


def in_projection(x, in_proj_weight, in_proj_bias):
    """(q, k) of nn.MultiheadAttention's packed in-projection for self-attention on x [B, N, 256]."""
    qkv = x @ in_proj_weight.T + in_proj_bias
    return qkv[..., :256], qkv[..., 256:512]


def weights_from_lse(q, k, lse, n_query_rows=None):
    """The kernels' expression in float64 on their own inputs: (P [B, 8, nq, N], its bound e_p) from q, k (any dtype, exact values) and lse fp32 [B, 8, nq]."""
    N = k.shape[1]
    nq = N if n_query_rows is None else n_query_rows
    qh, kh = split_heads(q.double(), nq), split_heads(k.double(), N)
    s = (qh @ kh.transpose(-1, -2)) * C_LOG2
    l = lse.double()[..., None]
    p = torch.exp2(s - l)
    e_s = 35 * U32 * C_LOG2 * (qh.abs() @ kh.abs().transpose(-1, -2)) + 4 * U32 * (s.abs() + l.abs())
    return p, p * (LN2 * e_s + 4 * U32)


def averaged(p, e_p):
    """Head average of (P, e_p) as the kernel forms it: seven fp32 adds and an exact scaling."""
    a = p.mean(1)
    return a, e_p.mean(1) + 8 * U32 * a


def rowsum_bound(q, k, lse, n_query_rows=None):
    """Bound on |sum_j P[b, h, i, j] - 1| for the kernel's P, [B, 8, nq]: see the module docstring."""
    N = k.shape[1]
    nq = N if n_query_rows is None else n_query_rows
    qh, kh = split_heads(q.double(), nq), split_heads(k.double(), N)
    s = (qh @ kh.transpose(-1, -2)) * C_LOG2
    m = s.amax(-1, keepdim=True)
    p, e_p = weights_from_lse(q, k, lse, n_query_rows)
    e_fwd = 35 * U32 * C_LOG2 * (qh.abs() @ kh.abs().transpose(-1, -2)) + 4 * U32 * (s.abs() + m.abs())
    l = lse.double()
    return e_p.sum(-1) + (N + N / 32 + 12) * U32 + (p * LN2 * e_fwd).sum(-1) + 4 * LN2 * U32 * (l.abs() + m[..., 0].abs())


def rollout_step_ref(p, e_p, r, residual):
    """(out, bound) of one rollout factor on a row vector: p, e_p [B, 8, nq, N] (weights_from_lse), r [B, N] exact; float64."""
    nq, r = p.shape[2], r.double()
    rq = r[:, None, :nq, None]
    mix = (rq * p).sum((1, 2)) / HEADS
    mix_abs = (rq.abs() * p).sum((1, 2)) / HEADS
    out = residual * r + (1 - residual) * mix
    e = (1 - residual) * (rq.abs() * e_p).sum((1, 2)) / HEADS + (8 * nq + 4) * U32 * (residual * r.abs() + (1 - residual) * mix_abs)
    return out, e


def rollout_matrix(mats, residual):
    """prod_l (a I + (1 - a) Abar_l) over mats = [Abar_0 .. Abar_{L-1}] ([B, N, N] each), the last block leftmost: [B, N, N]."""
    N = mats[0].shape[-1]
    eye = torch.eye(N, dtype=mats[0].dtype, device=mats[0].device)
    R = None
    for A in reversed(mats):
        F = residual * eye + (1 - residual) * A
        R = F if R is None else R @ F
    return R


def rollout_vector(mats, residual, bounds=None):
    """The CLS row of rollout_matrix as the model computes it: r = e_cls, then r <- a r + (1 - a) r Abar_l from the last block to the first: [B, N].
    A block's matrix may hold only its first rows ([B, nq, N]).  bounds (a list like mats: e_Abar, the element-wise bound of one kernel's averaged weights
    against float64 on its inputs; `mats` came from one kernel and the rollout step recomputes them in another, hence the 2): also returns the bound
    composed per step,  e' = a e + (1 - a) (e Abar + 2 |r| e_Abar + (8 N + 4) u |r| Abar) + u |out|."""
    B, N = mats[0].shape[0], mats[0].shape[-1]
    r = torch.zeros(B, N, dtype=mats[0].dtype, device=mats[0].device)
    r[:, 0] = 1.0
    e = torch.zeros_like(r)
    for l in reversed(range(len(mats))):
        A = mats[l]
        nq = A.shape[1]
        rq, eq = r[:, None, :nq], e[:, None, :nq]
        out = residual * r + (1 - residual) * (rq @ A)[:, 0]
        if bounds is not None:
            e = (residual * e + (1 - residual) * ((eq @ A)[:, 0] + 2 * (rq.abs() @ bounds[l])[:, 0] + (8 * N + 4) * U32 * (rq.abs() @ A)[:, 0]) + U32 * out.abs())
        r = out
    return (r, e) if bounds is not None else r


def block_weights_b(X, blk, eps=1e-5):
    """Block-level float64 reference with its composed fp32 bound: from the block's input stream X [B, N, 256] (exact values) through LayerNorm, the in-projection
    and the softmax.  blk: dict with norm1.weight / norm1.bias / in_proj_weight / in_proj_bias (float64).  Returns (P [B, 8, N, N], e_p): the bounds of
    vit_reference's layernorm_b and linear_b give e_q, e_k; the score term is attention_b's with them; e_p = p (e_s + sum_j p e_s + (N + N/32 + 12) u), the
    lse the kernel reads being the forward's row sum of the same perturbed scores."""
    X = X.double()
    N = X.shape[1]
    y, ey = vr.layernorm_b(X, torch.zeros_like(X), blk["norm1.weight"], blk["norm1.bias"], eps)
    qk, eqk = vr.linear_b(y, ey, blk["in_proj_weight"][:512], blk["in_proj_bias"][:512])
    qh, kh, eq, ek = (split_heads(t, N) for t in (qk[..., :256], qk[..., 256:], eqk[..., :256], eqk[..., 256:]))
    scale = 1.0 / math.sqrt(HD)
    s = (qh @ kh.transpose(-1, -2)) * scale
    mx = s.amax(-1, keepdim=True)
    es = (eq @ kh.abs().transpose(-1, -2) + qh.abs() @ ek.transpose(-1, -2) + eq @ ek.transpose(-1, -2)
          + (HD + 3) * U32 * (qh.abs() @ kh.abs().transpose(-1, -2))) * scale + 4 * U32 * (s.abs() + mx.abs())
    p = torch.softmax(s, dim=-1)
    return p, p * (es + (p * es).sum(-1, keepdim=True) + (N + N / 32 + 12) * U32)
