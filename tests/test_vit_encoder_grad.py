"""GPU tests of the ViT-VAE encoder's transformer gradients (csrc/vit.hip's backward entries, ViTVAEEncoder.train_transformer / cls_features_with_grad /
encode_with_grad, CausalViTVAE.train_adapters(transformer=True)).

Every new kernel alone against float64 on identical, bf16-exact operands, element-wise within c u sum|terms| with the c of
tests/vit_encoder_grad_reference.py's docstring, in both dtypes; with one-hot cotangents where a result is a single product; two runs give the same bits.
The whole transformer against the float64 restatement per parameter tensor and for dstem: fp32 rel-L2 at most 4 x that of the fp32 CPU evaluation of the same
restatement, bf16 at most 2 x the rounding-oracle gap (the rules of DESIGN §14 / §15); the k bias, whose gradient is zero in exact arithmetic, within its
element-wise rounding bound.  Every ratio is printed before it is asserted."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_encoder_grad_reference as gr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
LN2 = 0.6931471805599453
SHAPES = [(256, 768, None), (256, 256, None), (256, 512, None), (512, 256, None), (256, 256, "q"), (256, 512, "kv")]     # (K, N, in_proj row slice)


def ops():
    from causal_vae_amd import ops as o
    return o


def rand(dtype, *shape, seed=0, scale=1.0):
    """bf16-exact values in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).bfloat16().to(dtype)


def within(got, ref, err, what):
    diff = (got.detach().cpu().double() - ref).abs()
    ratio = float((diff / err.clamp_min(1e-300)).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0, (what, ratio)


def weight_slice(K, N, sl, seed):
    """the fp32 nn.Linear weight [N, K] on the device (a row slice of a [768, 256] in-projection for sl = "q" / "kv") and its float64 copy"""
    if sl is None:
        W = rand(F32, N, K, seed=seed, scale=0.2).to(DEV)
        return W, W
    full = rand(F32, 768, 256, seed=seed, scale=0.2).to(DEV)
    return full, (full[:256] if sl == "q" else full[256:])


# ---- attention -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("N", [7, 64, 65, 200])
def test_mhsa_bwd_against_float64(dtype, N, one):
    o, B, nq, bf = ops(), 2, (1 if one else N), dtype == BF16
    qkv = rand(dtype, B, N, 768, seed=N).to(DEV)
    q, k, v = qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:]
    out, lse = o.mhsa_train(q, k, v, n_query_rows=nq)
    assert torch.equal(out, o.mhsa(q, k, v, n_query_rows=nq))              # the training forward: the same bits
    dout = rand(dtype, B, nq, 256, seed=N + 1).to(DEV)
    run = lambda: (lambda d: o.mhsa_bwd(q, k, v, out, lse, dout, d[:, :nq, :256], d[:, :, 256:512], d[:, :, 512:]))(torch.full_like(qkv, 7.0))
    dq, dk, dv = run()
    c = lambda t: t.detach().cpu().double()
    rnd = vr.round_bf16 if bf else None
    parts = gr.attn_bwd(c(q), c(k), c(v), c(out), c(lse) * LN2, c(dout), rnd, parts=True)
    ref = gr.attn_bwd(c(q), c(k), c(v), c(out), c(lse) * LN2, c(dout), rnd)
    _o64, lse64 = gr.attn_fwd(c(q), c(k), c(v), nq)
    within(lse * LN2, lse64, 40 * vr.U32 * (1 + lse64.abs()) + 35 * vr.U32 * (gr.split_heads(c(q)[:, :nq]).abs() @ gr.split_heads(c(k)).abs().transpose(-1, -2)).amax(-1) * gr.SCALE, "lse")
    for name, got, want, err in zip(("dq", "dk", "dv"), (dq, dk, dv), ref, gr.attn_bwd_bounds(parts, bf)):
        assert got.shape == want.shape
        within(got, want, err, f"mhsa_bwd {name} {dtype} N{N} nq{nq}")
    for a, b in zip((dq, dk, dv), run()):
        assert torch.equal(a, b)                                            # fixed-order sums: the same bits


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_mhsa_bwd_one_hot_cotangent(dtype):
    """dOut = 2 at one (row, column of one head): dv is that column, 2 P[row, key] over the keys, and exact zeros elsewhere"""
    o, B, N, b0, q0, col = ops(), 2, 65, 1, 37, 3 * 32 + 5
    qkv = rand(dtype, B, N, 768, seed=3).to(DEV)
    q, k, v = qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:]
    out, lse = o.mhsa_train(q, k, v)
    dout = torch.zeros_like(out)
    dout[b0, q0, col] = 2.0
    d = torch.empty_like(qkv)
    _dq, _dk, dv = o.mhsa_bwd(q, k, v, out, lse, dout, d[:, :, :256], d[:, :, 256:512], d[:, :, 512:])
    c = lambda t: t.detach().cpu().double()
    s = (c(q)[b0, q0, 96:128] @ c(k)[b0, :, 96:128].T) * gr.SCALE
    p = torch.softmax(s, -1)
    got = c(dv)[b0, :, col]
    qk = (c(q)[b0, q0, 96:128].abs() @ c(k)[b0, :, 96:128].abs().T) * gr.SCALE
    rel = 35 * vr.U32 * qk + 8 * vr.U32 * (s.abs() + float(c(lse).abs().max()) * LN2) + 4 * vr.U32 + (2 * vr.UBF if dtype == BF16 else 0)      # e_P / P, + P and dv in bf16
    ratio = float(((got - 2 * p).abs() / (2 * p * rel)).max())
    print(f"one-hot dv {dtype}: {ratio:.4f}")
    assert ratio <= 1.0
    rest = c(dv).clone()
    rest[b0, :, col] = 0
    assert float(rest.abs().max()) == 0.0


# ---- token GEMM ------------------------------------------------------------------------------------------------------------------------------------
def slab_rows():
    """a row count at which a wgrad workgroup walks more than one 64-row chunk and more than one slab exists: from the kernel's own workspace rule"""
    lib = ops().lib
    one = lib.cvae_token_gemm_wgrad_workspace_bytes(1, 256, 256)
    M = next(m for m in range(2, 10000) if lib.cvae_token_gemm_wgrad_workspace_bytes(m, 256, 256) > one)      # first row of the second slab
    return 2 * (M - 1) + 76                                                 # two full slabs and a ragged third


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M", [2, 128, 129, "slabs"])
@pytest.mark.parametrize("K,N,sl", SHAPES)
def test_token_gemm_backward_against_float64(dtype, K, N, sl, M):
    o, bf = ops(), dtype == BF16
    M = slab_rows() if M == "slabs" else M
    assert M < 10000
    g, x = rand(dtype, M, N, seed=K + N + M).to(DEV), rand(dtype, M, K, seed=M).to(DEV)
    _full, W = weight_slice(K, N, sl, 11)
    c = lambda t: t.detach().cpu().double()
    Wd = c(vr.round_bf16(W) if bf else W)
    dx = o.token_gemm_bwd_data(g, W, dtype)
    ref = c(g) @ Wd
    within(dx, ref, (N + 2) * vr.U32 * (c(g).abs() @ Wd.abs()) + (vr.UBF * ref.abs() if bf else 0), f"bwd_data {dtype} K{K} N{N} {sl} M{M}")
    assert torch.equal(dx, o.token_gemm_bwd_data(g, W, dtype))
    dWfull = torch.full((768, 256), 7.0, device=DEV) if sl else None
    dbfull = torch.full((768,), 7.0, device=DEV) if sl else None
    rows = slice(0, 256) if sl == "q" else slice(256, 768)
    run = lambda: o.token_gemm_wgrad(g, x, *((dWfull[rows], dbfull[rows]) if sl else ()))
    dW, db = run()
    within(dW, c(g).T @ c(x), (M + 2) * vr.U32 * (c(g).abs().T @ c(x).abs()), f"wgrad dW {dtype} K{K} N{N} {sl} M{M}")
    within(db, c(g).sum(0), (4 + M * 2.0 ** -20) * vr.U32 * c(g).abs().sum(0), f"wgrad db {dtype} K{K} N{N} {sl} M{M}")
    if sl:                                                                   # written into the row slice of the packed gradient, nothing else touched
        keep = torch.ones(768, dtype=torch.bool)
        keep[rows] = False
        assert float((dWfull[keep.to(DEV)] - 7.0).abs().max()) == 0.0 and float((dbfull[keep.to(DEV)] - 7.0).abs().max()) == 0.0
    dW1, db1 = dW.clone(), db.clone()
    dW2, db2 = run()
    assert torch.equal(dW1, dW2) and torch.equal(db1, db2)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_token_gemm_wgrad_one_row_cotangent(dtype):
    """a cotangent that is zero outside one row: every element of dW is ONE product, exact in fp32 (bf16 operands: 16 significant bits)"""
    o, M, m0 = ops(), slab_rows(), 601
    for K, N, _sl in SHAPES[:4]:
        g, x = torch.zeros(M, N, dtype=dtype, device=DEV), rand(dtype, M, K, seed=5).to(DEV)
        g[m0] = rand(dtype, N, seed=6).to(DEV)
        dW, db = o.token_gemm_wgrad(g, x)
        assert torch.equal(dW.cpu().double(), torch.outer(g[m0].cpu().double(), x[m0].cpu().double()).float().double())
        assert torch.equal(db.cpu(), g[m0].float().cpu())


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_token_gemm_backward_epilogues(dtype):
    """the GELU gate from the training forward's saved pre-activation (fp32 stream gradient as the operand), and the fp32 residual in place on strided rows"""
    o, bf, M = ops(), dtype == BF16, 129
    c = lambda t: t.detach().cpu().double()
    y2 = rand(dtype, M, 256, seed=1).to(DEV)
    W1, b1 = rand(F32, 512, 256, seed=2, scale=0.1).to(DEV), rand(F32, 512, seed=3).to(DEV)
    hid, pre = o.token_gemm_gelu_train(y2, W1, b1)
    assert torch.equal(hid, o.token_gemm(y2, W1, b1, "gelu"))              # the training GELU forward: the eval epilogue's bits
    W1d = c(vr.round_bf16(W1) if bf else W1)
    p64, e = vr.linear_b(c(y2), torch.zeros(M, 256, dtype=F64), W1d, c(b1))
    within(pre, p64, e + (vr.UBF * (p64.abs() + e) if bf else 0), f"gelu_train pre {dtype}")
    G = rand(F32, M, 256, seed=4).to(DEV)                                   # the stream gradient: fp32 in both modes
    W2 = rand(F32, 256, 512, seed=5, scale=0.1).to(DEV)
    W2d = c(vr.round_bf16(W2) if bf else W2)
    dpre = o.token_gemm_bwd_data(G, W2, dtype, gate_pre=pre)
    gate = gr.gelu_grad(c(pre))
    ref = (c(G) @ W2d) * gate
    err = 1.13 * 258 * vr.U32 * (c(G).abs() @ W2d.abs()) + 8 * vr.U32 * ref.abs() + 8 * vr.U32 * (c(G) @ W2d).abs()
    within(dpre, ref, err + (vr.UBF * (ref.abs() + err) if bf else 0), f"bwd_data gelu gate {dtype}")
    big = rand(F32, M, 3, 256, seed=6).to(DEV)                              # the residual: rows with stride 768, updated in place
    before = big.clone()
    Wq = rand(F32, 768, 256, seed=7, scale=0.2).to(DEV)
    dq = rand(dtype, M, 256, seed=8).to(DEV)
    o.token_gemm_bwd_data(dq, Wq[:256], dtype, resid=big[:, 0])
    Wqd = c(vr.round_bf16(Wq[:256]) if bf else Wq[:256])
    ref = c(before[:, 0]) + c(dq) @ Wqd
    within(big[:, 0], ref, 258 * vr.U32 * (c(dq).abs() @ Wqd.abs()) + vr.U32 * ref.abs(), f"bwd_data residual {dtype}")
    assert torch.equal(big[:, 1:], before[:, 1:])
    out32 = o.token_gemm_bwd_data(dq, Wq[:256], dtype, out_dtype=F32)       # fp32 result without a residual (the CLS-only block's kv rows)
    within(out32, c(dq) @ Wqd, 258 * vr.U32 * (c(dq).abs() @ Wqd.abs()), f"bwd_data fp32 result {dtype}")


# ---- LayerNorm, tokens -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdtype", [F32, BF16])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_layernorm_bwd_against_float64(gdtype, rows, accumulate):
    o = ops()
    gen = torch.Generator().manual_seed(rows)
    big = (torch.randn(rows, 2, 256, generator=gen) * 3 + 0.7).to(DEV)
    big[0, 0] = 1.25                                                        # a row of equal values: variance 0, xhat 0, rstd = 1 / sqrt(eps)
    x = big[:, 0]                                                           # strided rows
    gy, gam = rand(gdtype, rows, 256, seed=rows + 1).to(DEV), rand(F32, 256, seed=2).to(DEV)
    old = rand(F32, rows, 3, 256, seed=3).to(DEV)
    c = lambda t: t.detach().cpu().double()
    _y, saved = gr.ln_fwd(c(x), c(gam), torch.zeros(256, dtype=F64))
    ref = gr.ln_bwd(c(gy), saved, c(gam))
    e_dx, e_dg, e_db = gr.ln_bwd_bounds(c(x), c(gy), c(gam))
    if accumulate:
        dst = old.clone()
        run = lambda: (lambda d: o.layernorm256_bwd(gy, x, gam, 1e-5, dx=d[:, 1], accumulate=True))(old.clone())
        dx, dg, db = o.layernorm256_bwd(gy, x, gam, 1e-5, dx=dst[:, 1], accumulate=True)
        assert torch.equal(dst[:, 0], old[:, 0]) and torch.equal(dst[:, 2], old[:, 2])
        want = c(old[:, 1]) + ref[0]
        within(dx, want, e_dx + vr.U32 * want.abs(), f"layernorm_bwd dx += {gdtype} rows{rows}")
    else:
        run = lambda: o.layernorm256_bwd(gy, x, gam, 1e-5)
        dx, dg, db = run()
        within(dx, ref[0], e_dx, f"layernorm_bwd dx {gdtype} rows{rows}")
    within(dg, ref[1], e_dg, f"layernorm_bwd dgamma {gdtype} rows{rows}")
    within(db, ref[2], e_db, f"layernorm_bwd dbeta {gdtype} rows{rows}")
    for a, b in zip((dx, dg, db), run()):
        assert torch.equal(a, b)


@pytest.mark.parametrize("stem_dtype", [F32, BF16])
@pytest.mark.parametrize("B", [1, 3])
def test_vit_tokens_bwd(stem_dtype, B):
    o = ops()
    dtok = rand(F32, B, 7, 256, seed=B).to(DEV) * 1.0009765625             # not bf16-exact: dstem is rounded
    dpos, dcls, dstem = o.vit_tokens_bwd(dtok, stem_dtype)
    c = lambda t: t.detach().cpu().double()
    within(dpos, c(dtok).sum(0), B * vr.U32 * c(dtok).abs().sum(0), f"dpos B{B}")
    assert torch.equal(dcls, dpos[0]) and torch.equal(dstem, dtok[:, 1:].to(stem_dtype))
    for a, b in zip((dpos, dcls, dstem), o.vit_tokens_bwd(dtok, stem_dtype)):
        assert torch.equal(a, b)


# ---- the whole transformer -------------------------------------------------------------------------------------------------------------------------
CASES = [((64, 96), 2), ((256, 320), 3), ((64, 96), 1)]          # B = 1: one CLS row, where a strided [1, 256] view reports itself contiguous
_REF = {}


def encoder(img, seed=0):
    from causal_vae_amd.vit.models import ViTVAEEncoder
    torch.manual_seed(seed)
    model = ViTVAEEncoder(img_size=img, depth=2, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    model.requires_grad_(False)
    return model.to(DEV).eval()


def cotangents(B, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g)


def references(img, B, dtype, cls_only, model, stem):
    """float64, its fp32 CPU evaluation and (bf16) the rounding oracle of one case, computed once and shared"""
    key = (img, B, dtype, cls_only)
    if key not in _REF:
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        st, (gm, gl) = stem.detach().cpu().double().view(B, -1, 256), cotangents(B)
        kw = dict(cls_only_last=cls_only)
        bf = dtype == BF16
        r64 = gr.transformer_vjp(sd, st, 2, gm, gl, want_parts=not bf, **kw)[0]
        r32 = gr.transformer_vjp(sd, st, 2, gm, gl, dtype=F32, **kw)[0]
        oracle = gr.transformer_vjp(sd, st, 2, gm, gl, rnd=vr.round_bf16, want_parts=True, **kw)[0] if bf else None
        _REF[key] = (r64, r32, oracle)
    return _REF[key]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cls_only", [True, False])
@pytest.mark.parametrize("img,B", CASES)
def test_transformer_gradients_against_float64(img, B, dtype, cls_only):
    model = encoder(img).set_compute_dtype(dtype)
    model._cls_only_last_block = cls_only
    x = vr.vit_inputs(B, *img, seed=5).to(DEV)
    with torch.no_grad():
        stem = model._stem_cl(x)
        mu0, lv0 = model.encode(x)
    params = model.train_transformer()
    names = [k for k, _p in model._transformer_named()]
    collect = {}
    mu, lv = model.encode_with_grad(x, collect)
    assert torch.equal(mu, mu0) and torch.equal(lv, lv0)                    # the training forward: the inference path's bits
    gm, gl = cotangents(B)
    torch.autograd.backward([mu, lv], [gm.to(DEV), gl.to(DEV)])
    r64, r32, oracle = references(img, B, dtype, cls_only, model, stem)
    bf = dtype == BF16
    other = oracle if bf else r32
    got = {k: p.grad for k, p in zip(names, params)}
    got["dstem"] = collect["dstem"]
    worst = []
    for k, g in got.items():
        assert g is not None and torch.isfinite(g.float()).all(), k
        a, ref, oth = g.detach().cpu().double().reshape(r64[k].shape), r64[k], other[k].double()
        if k.endswith("attn.in_proj_bias"):                                 # the k bias: zero in exact arithmetic, held to its rounding bound
            i = int(k.split(".")[1])
            bound = gr.k_bias_bound((other if bf else r64)["k_bias_parts"][i], bf)
            kr = float((a[256:512].abs() / bound).max())
            print(f"{k}[256:512] {dtype}: max |got| / bound = {kr:.4f} (max |got| {float(a[256:512].abs().max()):.3e})")
            assert kr <= 1.0, (k, kr)
            keep = torch.ones(768, dtype=torch.bool)
            keep[256:512] = False
            a, ref, oth = a[keep], ref[keep], oth[keep]
        mine, yard, factor, rule = gr.rel_l2(a, ref), gr.rel_l2(oth, ref), (2.0 if bf else 4.0), ("rounding-oracle gap" if bf else "fp32 CPU evaluation")
        if bf and k in ("to_latent.bias", "fc_mu.bias", "fc_var.bias"):
            assert yard == 0.0, (k, yard)
            # to_latent.bias, fc_mu.bias, fc_var.bias: sums of the cotangents alone, with no bf16 rounding anywhere upstream, so the oracle IS float64 and its
            # gap is exactly zero; their kernels are the fp32 ones in both modes and are held to the fp32 rule
            yard, factor, rule = gr.rel_l2(r32[k].double(), ref), 4.0, "fp32 CPU evaluation (no bf16 rounding upstream: oracle gap 0)"
        # a yardstick of exactly zero (B = 1: fc_mu.bias' gradient IS the cotangent, a one-term sum) admits only an exact result
        ratio = mine / yard if yard > 0.0 else (0.0 if mine == 0.0 else float("inf"))
        print(f"{k} {dtype} cls_only={cls_only} {img} B{B}: rel-L2 {mine:.3e}, {rule} {yard:.3e}, ratio {ratio:.3f} (allowed {factor})")
        worst.append((ratio / factor, k))
    print("worst ratio / allowed", max(worst))
    assert max(worst)[0] <= 1.0, max(worst)


def test_absent_cotangent_and_accumulation():
    model = encoder((64, 96))
    x = vr.vit_inputs(2, 64, 96, seed=5).to(DEV)
    params = model.train_transformer()
    gm, _gl = cotangents(2)
    mu, lv = model.encode_with_grad(x)
    torch.autograd.backward([mu, lv], [gm.to(DEV), torch.zeros_like(lv)])
    zero_cot = [p.grad.clone() for p in params]
    model.zero_grad(set_to_none=True)
    mu, lv = model.encode_with_grad(x)
    mu.backward(gm.to(DEV))                                                 # log_var's cotangent is absent
    for (k, p), z in zip(model._transformer_named(), zero_cot):
        if k.startswith("fc_var."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
        else:
            assert torch.equal(p.grad, z), k
    once = [p.grad.clone() for p in params if p.grad is not None]
    mu, lv = model.encode_with_grad(x)
    mu.backward(gm.to(DEV))                                                 # .grad accumulates
    for p, g in zip([p for p in params if p.grad is not None], once):
        assert torch.equal(p.grad, g + g)
    with torch.no_grad():
        assert torch.equal(model.cls_features_with_grad(x), model.cls_features(x))
    model.freeze_transformer()
    assert not model.cls_features_with_grad(x).requires_grad


FULL_BLOCK = ["layernorm256", "token_gemm", "mhsa", "token_gemm", "layernorm256", "token_gemm", "token_gemm"]                     # the module docstring's 7
CLS_BLOCK = ["layernorm256", "token_gemm", "token_gemm", "mhsa", "token_gemm", "layernorm256", "token_gemm", "token_gemm"]       # K and V, then the CLS query: 8


def walk_calls(run):
    """[(ops name, shape of the (first) result, epilogue, whether `out` was left at its default)] of the token-side ops calls `run` makes"""
    o, log = ops(), []
    originals = {n: getattr(o, n) for n in ("vit_tokens", "layernorm256", "token_gemm", "mhsa", "mhsa_train", "token_gemm_gelu_train")}

    def wrap(name, fn):
        def call(*a, **k):
            out = fn(*a, **k)
            epilogue, dest = (a[3] if len(a) > 3 else k.get("epilogue")), (a[5] if len(a) > 5 else k.get("out"))
            log.append((name, tuple((out[0] if isinstance(out, tuple) else out).shape), epilogue if name == "token_gemm" else None, dest is None))
            return out
        return call

    try:
        for n, fn in originals.items():
            setattr(o, n, wrap(n, fn))
        result = run()
    finally:
        for n, fn in originals.items():
            setattr(o, n, fn)
    return result, log


@pytest.mark.parametrize("cls_only", [True, False])
def test_one_walk_two_modes(cls_only):
    """the saving walk issues the inference walk's ops calls (attention and the GELU GEMM in their training forms), block by block the docstring's 7 / 8; only
    the inference walk writes a full block's residual GEMMs in place on the stream"""
    model = encoder((64, 96))
    model._cls_only_last_block = cls_only
    x = vr.vit_inputs(2, 64, 96, seed=5).to(DEV)
    c0, infer = walk_calls(lambda: model.cls_features(x))
    model.train_transformer()
    c1, saving = walk_calls(lambda: model.cls_features_with_grad(x))
    assert c1.requires_grad and torch.equal(c0, c1)
    alias = {"mhsa_train": "mhsa", "token_gemm_gelu_train": "token_gemm"}
    plain = lambda log: [(alias.get(n, n), shape) for n, shape, _e, _d in log]
    assert plain(infer) == plain(saving)
    assert [n for n, _s in plain(infer)] == ["vit_tokens"] + FULL_BLOCK + (CLS_BLOCK if cls_only else FULL_BLOCK) + ["layernorm256"]
    assert {n for n, *_r in infer} == {"vit_tokens", "layernorm256", "token_gemm", "mhsa"}
    assert {n for n, *_r in saving} == {"vit_tokens", "layernorm256", "token_gemm", "mhsa_train", "token_gemm_gelu_train"}
    full = slice(1, 1 + len(FULL_BLOCK) * (1 if cls_only else 2))           # the calls of the full block(s)
    in_place = lambda log: [d for _n, _s, e, d in log[full] if e == "residual"]
    assert in_place(infer) == [True] * len(in_place(infer)) and in_place(saving) == [False] * len(in_place(saving))
    assert len(in_place(infer)) == len(in_place(saving)) == (2 if cls_only else 4)


def test_causal_vitvae_trains_everything_but_the_stem():
    from causal_vae_amd.vessel.train import loss_function, total_loss
    from causal_vae_amd.vit.causal import CausalViTVAE
    import vit_decoder_reference as dr
    torch.manual_seed(5)
    model = CausalViTVAE(img_size=(64, 96), depth=2)
    dr.randomize_decoder_bn(model.backbone.decoder, 6)
    vr.randomize_stem_bn(model.backbone.stem, 7)
    model = model.to(DEV)
    gen = torch.Generator().manual_seed(8)
    B = 3
    x = torch.rand(B, 1, 64, 96, generator=gen).to(DEV)
    m, t = torch.randn(B, model.m_dim, generator=gen).to(DEV), torch.randn(B, model.t_dim, generator=gen).to(DEV)
    eps = torch.randn(B, model.my_z_dim, generator=gen).to(DEV)

    seen = {}

    def step(**kw):
        state = {k: v.clone() for k, v in model.state_dict().items()}
        params = model.train_adapters(**kw)
        model.zero_grad(set_to_none=True)
        if kw.get("transformer"):                                           # the cotangent of the cls features, for the restatement
            inner = model.backbone.cls_features_with_grad
            model.backbone.cls_features_with_grad = lambda xx: (lambda c: (c.register_hook(lambda g: seen.setdefault("g_cls", g.clone())), c)[1])(inner(xx))
        out = model.forward_train(x, m, t, eps=eps)
        model.backbone.__dict__.pop("cls_features_with_grad", None)
        total_loss(*loss_function(out[0], x, out[1], m, *out[2:])).backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        model.load_state_dict(state)                                        # the heads' running statistics moved: both runs start alike
        return params, grads

    base_params, base = step(decoder=True)
    params, grads = step(decoder=True, transformer=True)
    assert len(params) == len(base_params) + len(model.backbone._transformer_named(heads=False)) and len({id(p) for p in params}) == len(params)
    by_id = {id(p): k for k, p in model.named_parameters()}
    with torch.no_grad():
        stem = model.backbone._stem_cl(x).detach().cpu().double().view(B, -1, 256)
    sd = {k: v.detach().cpu() for k, v in model.backbone.state_dict().items()}
    r64 = gr.transformer_vjp(sd, stem, 2, None, None, cls_only_last=True, want_parts=True, g_cls=seen["g_cls"].detach().cpu().double())[0]
    for p in params:
        k = by_id[id(p)]
        g = grads[k]
        assert torch.isfinite(g).all(), k
        if k.endswith("attn.in_proj_bias"):                                 # the k bias: zero in exact arithmetic, held to its element-wise rounding bound
            keep = torch.ones(768, dtype=torch.bool, device=DEV)
            keep[256:512] = False
            assert float(g[keep].abs().max()) > 0.0, k
            bound = gr.k_bias_bound(r64["k_bias_parts"][int(k.split(".")[2])], False)
            kr = float((g[256:512].detach().cpu().double().abs() / bound).max())
            print(f"{k}[256:512]: max |grad| / bound = {kr:.4f} (max |grad| {float(g[256:512].abs().max()):.3e})")
            assert kr <= 1.0, (k, kr)
        else:
            assert float(g.abs().max()) > 0.0, k
    for k, g in base.items():                                               # the heads and the decoder: the same bits as without the transformer
        assert torch.equal(grads[k], g), k
    assert not any(k.startswith("backbone.stem.") for k in grads)
