"""GPU tests of the attention weights and the attention rollout (csrc/vit_attention_probe.inc, ops.mhsa_weights / mhsa_rollout_step,
ViTVAEEncoder.attention_weights / attention_rollout).  Every comparison is against float64 with the bounds derived in tests/vit_attention_reference.py's
docstring (u = 2^-24; nothing is fitted), or is exact (torch.equal).

Shapes: the attention tests' edge cases at their smallest — N = 7 (one ragged tile; a 64 x 96 image), 65 (a full 64-row tile plus one), 130 (two key
workgroups and a ragged third query tile), n_query_rows = N and 1, B = 3, fp32 and bf16 operands (bf16-exact values, float64 on the same values), q and k
as panels of a packed [B, N, 768] buffer and, for one query row, q as its own [B, 1, 256] tensor; operand scales 1 and 3 (flat and peaked rows)."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_attention_reference as ar  # noqa: E402
import vit_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
B = 3
SHAPES = [(7, 7), (7, 1), (65, 65), (65, 1), (130, 130), (130, 1)]


def ops():
    from causal_vae_amd import ops as o
    return o


def within(got, ref, err, what):
    ratio = float(((got.detach().cpu().double() - ref).abs() / err).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


@functools.lru_cache(maxsize=None)
def case(dtype, N, nq, scale):
    """One set of operands, computed once and left unchanged: the packed buffer on the device, mhsa_train's lse for these queries, and the float64 values of
    the kernels' expression on exactly these inputs (P per head with its bound)."""
    g = torch.Generator().manual_seed(1000 * N + int(10 * scale))
    qkv = (scale * torch.randn(B, N, 768, generator=g)).to(dtype)
    d = qkv.to(DEV)
    q, k, v = d[:, :, :256], d[:, :, 256:512], d[:, :, 512:]
    _out, lse = ops().mhsa_train(q, k, v, n_query_rows=nq)
    p, e_p = ar.weights_from_lse(qkv[:, :, :256], qkv[:, :, 256:512], lse.cpu(), nq)
    return {"qkv": qkv, "q": q, "k": k, "v": v, "lse": lse, "p": p, "e_p": e_p}


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("N,nq", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_weights_against_float64(dtype, N, nq, scale):
    c = case(dtype, N, nq, scale)
    heads = ops().mhsa_weights(c["q"], c["k"], c["lse"], nq, average_heads=False)
    mean = ops().mhsa_weights(c["q"], c["k"], c["lse"], nq)
    assert heads.shape == (B, 8, nq, N) and mean.shape == (B, nq, N) and heads.dtype == mean.dtype == F32
    rel = c["e_p"] / c["p"]
    print(f"local bound: {float(rel.min()):.2e} .. {float(rel.max()):.2e} of p")
    within(heads, c["p"], c["e_p"], f"weights per head {dtype} N{N} nq{nq} scale{scale}")
    within(mean, *ar.averaged(c["p"], c["e_p"]), f"weights averaged {dtype} N{N} nq{nq} scale{scale}")
    assert bool((heads >= 0).all()) and bool((mean >= 0).all())
    # rows sum to one as far as the forward's lse is the row's log-sum.  The bound (vit_attention_reference.rowsum_bound) is the forward's part,
    # (N + N/32 + 12) u (row sum of N terms, one rescale per 32-key tile, exp2 and log2) + sum_j p_j ln 2 e_s_j (the p-weighted mean of the forward's score
    # error), and two terms that the comparison itself brings in: sum_j e_p_j, because the sum is taken over THIS kernel's p, each within e_p of
    # float64, and 4 ln 2 u (|lse| + |m|), the rounding of log2 l and of m + log2 l when the forward stores lse in fp32
    dev = (heads.cpu().double().sum(-1) - 1).abs()
    bound = ar.rowsum_bound(c["qkv"][:, :, :256], c["qkv"][:, :, 256:512], c["lse"].cpu(), nq)
    print(f"row sums: max |sum - 1| = {float(dev.max()):.3e}, max ratio to bound = {float((dev / bound).max()):.4f}")
    assert bool((dev <= bound).all())
    # exact: the averaged form is the head-order fp32 sum times 1/8
    s = heads[:, 0]
    for h in range(1, 8):
        s = s + heads[:, h]
    assert torch.equal(mean, s * 0.125)


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("N,nq", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rollout_step_against_float64(dtype, N, nq, scale):
    c = case(dtype, N, nq, scale)
    g = torch.Generator().manual_seed(N + nq)
    r_rand = torch.randn(B, N, generator=g) * torch.exp(2 * torch.randn(B, N, generator=g))       # random signs and magnitudes
    e_cls = torch.zeros(B, N)
    e_cls[:, 0] = 1.0
    mean = ops().mhsa_weights(c["q"], c["k"], c["lse"], nq).cpu().double()
    a_mean, e_mean = ar.averaged(c["p"], c["e_p"])
    for name, r in (("random", r_rand), ("e_cls", e_cls)):
        for residual in (0.5, 0.0):
            got = ops().mhsa_rollout_step(c["q"], c["k"], c["lse"], r.to(DEV), nq, residual)
            assert got.shape == (B, N) and got.dtype == F32
            ref, err = ar.rollout_step_ref(c["p"], c["e_p"], r, residual)
            within(got, ref, err, f"rollout_step {name} a={residual} {dtype} N{N} nq{nq} scale{scale}")
            # against r @ Abar with Abar mhsa_weights' own output: the two kernels round independently (2 e_p, and the average's 8 u Abar)
            rq = r.double()[:, None, :nq]
            ref2 = residual * r.double() + (1 - residual) * (rq @ mean)[:, 0]
            terms = residual * r.double().abs() + (1 - residual) * (rq.abs() @ a_mean)[:, 0]
            err2 = (1 - residual) * (rq.abs() @ (2 * e_mean))[:, 0] + (8 * nq + 4) * vr.U32 * terms
            within(got, ref2, err2, f"rollout_step vs r @ mhsa_weights {name} a={residual} {dtype} N{N} nq{nq} scale{scale}")


@pytest.mark.parametrize("N", [7, 65, 130])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_properties(dtype, N):
    o = ops()
    full, one = case(dtype, N, N, 3.0), case(dtype, N, 1, 3.0)
    q, k, lse = full["q"], full["k"], full["lse"]
    r = torch.randn(B, N, generator=torch.Generator().manual_seed(N)).to(DEV)
    for avg in (True, False):
        w = o.mhsa_weights(q, k, lse, average_heads=avg)
        assert torch.equal(w, o.mhsa_weights(q, k, lse, average_heads=avg))                                  # two runs
        assert torch.equal(w[:1], o.mhsa_weights(q[:1], k[:1], lse[:1].contiguous(), average_heads=avg))    # batch row 0 alone
        # one query row equals row 0 of all rows: q as a panel of the packed buffer, and as its own [B, 1, 256] tensor (the CLS-only block's)
        row0 = w[..., :1, :]
        assert torch.equal(one["lse"], lse[:, :, :1])
        assert torch.equal(o.mhsa_weights(q, k, one["lse"], 1, average_heads=avg), row0)
        assert torch.equal(o.mhsa_weights(q[:, :1].contiguous(), k, one["lse"], 1, average_heads=avg), row0)
        # `out`: a strided batch of a larger buffer
        big = torch.full((B, 2) + tuple(w.shape[1:]), -1.0, device=DEV)
        assert o.mhsa_weights(q, k, lse, average_heads=avg, out=big[:, 0]) is not None and torch.equal(big[:, 0], w) and bool((big[:, 1] == -1).all())
    for nq, c in ((N, full), (1, one)):
        s = o.mhsa_rollout_step(c["q"], k, c["lse"], r, nq, 0.5)
        assert torch.equal(s, o.mhsa_rollout_step(c["q"], k, c["lse"], r, nq, 0.5))
        assert torch.equal(s[:1], o.mhsa_rollout_step(c["q"][:1], k[:1], c["lse"][:1].contiguous(), r[:1].contiguous(), nq, 0.5))
        assert torch.equal(o.mhsa_rollout_step(c["q"], k, c["lse"], r, nq, 1.0), r)                        # residual = 1 returns r
        out = torch.empty_like(r)
        assert o.mhsa_rollout_step(c["q"], k, c["lse"], r, nq, 0.5, out=out) is out and torch.equal(out, s)
    # r = e_cls: only the first row of the matrix matters, so one query row gives the bits of all rows
    e = torch.zeros(B, N, device=DEV)
    e[:, 0] = 1
    assert torch.equal(o.mhsa_rollout_step(q, k, lse, e, N, 0.5), o.mhsa_rollout_step(q[:, :1].contiguous(), k, one["lse"], e, 1, 0.5))


def test_refusals():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAEEncoder
    o = ops()
    c = case(F32, 7, 7, 1.0)
    q, k, lse = c["q"], c["k"], c["lse"]
    r = torch.zeros(B, 7, device=DEV)
    bad = [lambda: o.mhsa_weights(q, k, lse[:, :, :6].contiguous()),                       # lse of the wrong shape
           lambda: o.mhsa_weights(q, k, lse.double()),                                      # ... dtype
           lambda: o.mhsa_weights(q, k, lse.transpose(1, 2).contiguous().transpose(1, 2)),  # ... layout
           lambda: o.mhsa_rollout_step(q, k, lse[:, :4].contiguous(), r),
           lambda: o.mhsa_rollout_step(q, k, lse.half(), r),
           lambda: o.mhsa_weights(q, k.bfloat16(), lse),                                    # mixed dtypes
           lambda: o.mhsa_rollout_step(q.bfloat16(), k, lse, r),
           lambda: o.mhsa_rollout_step(q, k, lse, r, out=r),                                # out is r
           lambda: o.mhsa_rollout_step(q, k, lse, r, residual=-0.1),
           lambda: o.mhsa_rollout_step(q, k, lse, r, residual=1.01),
           lambda: o.mhsa_rollout_step(q, k, lse, r.double()),
           lambda: o.mhsa_rollout_step(q, k, lse, r[:, :6]),
           lambda: o.mhsa_weights(q, k, lse, 0), lambda: o.mhsa_weights(q, k, lse, 8),     # n_query_rows outside 1 .. N
           lambda: o.mhsa_rollout_step(q, k, lse, r, 0), lambda: o.mhsa_rollout_step(q, k, lse, r, 8),
           lambda: o.mhsa_weights(q, k, lse, out=torch.empty(B, 7, 8, device=DEV)),
           lambda: o.mhsa_weights(q.cpu(), k.cpu(), lse.cpu())]
    for f in bad:
        with pytest.raises(CvaeError):
            f()
    m = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=8).to(DEV).eval()
    x = vr.vit_inputs(1, 64, 96, 0).to(DEV)
    for f in (lambda: m.attention_weights(x, query="patches"), lambda: m.attention_weights(x, blocks=[1]), lambda: m.attention_weights(x, blocks=[]),
              lambda: m.attention_rollout(x, residual=2.0)):
        with pytest.raises(CvaeError):
            f()
    with pytest.raises(RuntimeError):
        m.train().attention_rollout(x)                                                      # eval mode only, as every inference entry
    qg = q.clone().requires_grad_(True)
    with pytest.raises(CvaeError):
        o.mhsa_weights(qg, k, lse)                                                          # forward-only


# ---- model level ----------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 96), (128, 160)]            # N = 7 and 21
DEPTH, MB = 2, 2


@functools.lru_cache(maxsize=None)
def built(H, W, dtype):
    from causal_vae_amd.vit import ViTVAEEncoder
    torch.manual_seed(H + W)
    m = ViTVAEEncoder(img_size=(H, W), depth=DEPTH, latent_dim=16)
    vr.randomize_stem_bn(m.stem, H)
    return m.requires_grad_(False).to(DEV).eval().set_compute_dtype(dtype), vr.vit_inputs(MB, H, W, W).to(DEV)


def saved_walk(m, x, cls_only_last):
    """The saving walk's per-block records with the last block in the asked form (the private flag, restored)."""
    flag = m._cls_only_last_block
    try:
        m._cls_only_last_block = cls_only_last
        return m._walk(x, save=True)[1].steps
    finally:
        m._cls_only_last_block = flag


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_model_weights_are_the_ops_on_the_walks_tensors(H, W, dtype):
    m, x = built(H, W, dtype)
    N = m.num_patches + 1
    for query in ("cls", "all"):
        steps = saved_walk(m, x, query == "cls")
        nq = N if query == "all" else 1
        for avg in (True, False):
            got = m.attention_weights(x, query=query, average_heads=avg)
            assert got.shape == ((MB, DEPTH, nq, N) if avg else (MB, DEPTH, 8, nq, N)) and got.dtype == F32
            for i, s in enumerate(steps):
                q, k = (s.q, s.qkv[:, :, :256]) if s.cls_only else (s.qkv[:, :, :256], s.qkv[:, :, 256:512])
                assert q.dtype == dtype
                ref = ops().mhsa_weights(q, k, s.lse[:, :, :nq].contiguous(), nq, average_heads=avg)
                assert torch.equal(got[:, i], ref), (query, avg, i)
            assert torch.equal(m.attention_weights(x, query=query, average_heads=avg, blocks=[1]), got[:, 1:2])
            assert torch.equal(m.attention_weights(x, query=query, average_heads=avg, blocks=(1, 0)), got[:, [1, 0]])
    # row 0 of the "all" form is the "cls" form, in every block
    assert torch.equal(m.attention_weights(x, query="all")[:, :, :1], m.attention_weights(x, query="cls"))


@pytest.mark.parametrize("H,W", SIZES)
def test_model_weights_against_float64_from_the_block_input(H, W):
    """fp32: for each block, float64 from the block's input stream as the GPU produced it, through LayerNorm, the in-projection and the softmax, with the bound
    composed from layernorm_b, linear_b and the score term (vit_attention_reference.block_weights_b).  Measured on the MI355X: see the printed ratios."""
    m, x = built(H, W, F32)
    N = m.num_patches + 1
    steps = saved_walk(m, x, False)
    got = m.attention_weights(x, query="all", average_heads=False)
    sd = {k_: v.detach().cpu().double() for k_, v in m.state_dict().items()}
    for i, s in enumerate(steps):
        pre = f"transformer.{i}."
        blk = {"norm1.weight": sd[pre + "norm1.weight"], "norm1.bias": sd[pre + "norm1.bias"], "in_proj_weight": sd[pre + "attn.in_proj_weight"],
               "in_proj_bias": sd[pre + "attn.in_proj_bias"]}
        p, e_p = ar.block_weights_b(s.X.view(MB, N, 256).cpu(), blk, m.transformer[i].norm1.eps)
        rel = e_p / p
        print(f"block {i}: bound {float(rel.min()):.2e} .. {float(rel.max()):.2e} of p")
        assert float(rel.max()) < 1e-2                                        # the premise: a bound this tight cannot pass vacuously
        within(got[:, i], p, e_p, f"attention_weights {H}x{W} block {i}")


@pytest.mark.parametrize("H,W", SIZES)
def test_no_side_effects(H, W):
    m, x = built(H, W, F32)

    def state():
        return (m.cls_features(x), m.dropout_keys.step, m._cls_only_last_block, "_cls_only_last_block" in vars(m) and vars(m)["_cls_only_last_block"],
                {k_: v.clone() for k_, v in m.state_dict().items()}, m.training, [p.requires_grad for p in m.parameters()])

    def same(a, b):
        assert torch.equal(a[0], b[0]) and a[1:4] == b[1:4] and a[5:] == b[5:]
        assert a[4].keys() == b[4].keys() and all(torch.equal(a[4][k_], b[4][k_]) for k_ in a[4])

    def calls():
        m.attention_weights(x)
        m.attention_weights(x, query="all", average_heads=False)
        m.attention_rollout(x)
        m.attention_rollout(x, residual=0.2, as_grid=False)

    before = state()
    calls()
    same(before, state())
    ref = m.attention_rollout(x)
    try:
        m.train_transformer(dropout=True)                                     # the training forward would drop; these never do, and take no key
        before = state()
        calls()
        same(before, state())
        assert torch.equal(m.attention_rollout(x), ref)
    finally:
        m.freeze_transformer()


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_attention_rollout(H, W, dtype):
    m, x = built(H, W, dtype)
    N = m.num_patches + 1
    row = m.attention_rollout(x, as_grid=False)
    assert row.shape == (MB, N) and row.dtype == F32
    grid = m.attention_rollout(x)
    assert grid.shape == (MB, m.grid_h, m.grid_w) and torch.equal(grid, row[:, 1:].reshape(MB, m.grid_h, m.grid_w))
    # the float64 product of the matrices attention_weights returns, with the bound composed per step
    A = m.attention_weights(x, query="all").cpu().double()
    steps = saved_walk(m, x, False)
    e_A = []
    for s in steps:
        q, k = s.qkv[:, :, :256].cpu(), s.qkv[:, :, 256:512].cpu()
        e_A.append(ar.averaged(*ar.weights_from_lse(q, k, s.lse.cpu()))[1])
    mats = [A[:, i] for i in range(DEPTH)]
    ref, err = ar.rollout_vector(mats, 0.5, bounds=e_A)
    assert float((ar.rollout_matrix(mats, 0.5)[:, 0] - ref).abs().max()) <= 1e-14
    within(row, ref, err, f"attention_rollout {H}x{W} {dtype}")
    # the whole row sums to one: within the bound above, and as far as the matrices' own rows do.  A factor a I + (1 - a) Abar whose rows sum to 1 +- d
    # takes a non-negative row vector of sum S to one of sum S' with |S' - S| <= (1 - a) d S, so from S = 1 over the blocks |S - 1| <= prod_l (1 + (1 - a) d_l) - 1,
    # to every order (d_l: block l's largest rowsum_bound, head-averaged, + 8 u for the average's roundings)
    dev = (row.cpu().double().sum(-1) - 1).abs()
    grow = torch.ones(MB, dtype=torch.float64)
    for s in steps:
        grow = grow * (1 + 0.5 * (ar.rowsum_bound(s.qkv[:, :, :256].cpu(), s.qkv[:, :, 256:512].cpu(), s.lse.cpu()).mean(1) + 8 * vr.U32).amax(-1))
    tol = err.sum(-1) + (grow - 1)
    print(f"row sum: max |sum - 1| = {float(dev.max()):.3e}, bound {float(tol.min()):.3e}")
    assert bool((dev <= tol).all()) and bool((row >= 0).all())
    # the CLS-only and the full last block give the same maps, bit for bit
    try:
        m._cls_only_last_block = False
        assert torch.equal(m.attention_rollout(x, as_grid=False), row)
    finally:
        del m._cls_only_last_block                                           # back to the class's default
    e = torch.zeros(MB, N, device=DEV)
    e[:, 0] = 1
    assert torch.equal(m.attention_rollout(x, residual=1.0, as_grid=False), e)
    assert torch.equal(m.attention_rollout(x, as_grid=False), row)                                        # two runs


def test_delegates():
    from causal_vae_amd.vit import CausalViTVAE, ViTVAE, extract_vit_attention
    torch.manual_seed(2)
    c = CausalViTVAE(img_size=(64, 96), depth=2).to(DEV).eval()
    vr.randomize_stem_bn(c.backbone.stem, 3)
    xs = [vr.vit_inputs(2, 64, 96, 5), vr.vit_inputs(1, 64, 96, 6)]
    maps = [c.backbone.attention_rollout(x.to(DEV)) for x in xs]
    assert torch.equal(c.attention_rollout(xs[0].to(DEV)), maps[0])
    assert torch.equal(c.attention_rollout(xs[0].to(DEV), residual=0.3, as_grid=False), c.backbone.attention_rollout(xs[0].to(DEV), residual=0.3, as_grid=False))
    loader = [{"x": x} for x in xs]
    want = torch.cat(maps).cpu().numpy()
    for model in (c, c.backbone):
        got = extract_vit_attention(model, loader, DEV)
        assert got.shape == (3, 2, 3) and got.dtype == want.dtype and (got == want).all()
    assert isinstance(c.backbone, ViTVAE) and extract_vit_attention(c, [], DEV).shape == (0, 2, 3)
    got = extract_vit_attention(c, loader, DEV, residual=0.3)
    assert (got == torch.cat([c.attention_rollout(x.to(DEV), residual=0.3) for x in xs]).cpu().numpy()).all()
