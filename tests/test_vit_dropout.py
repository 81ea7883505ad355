"""GPU tests of the transformer's dropout (csrc/vit.hip's *_dropout entries, ops.mhsa_train / mhsa_bwd / token_gemm_dropout /
token_gemm_bwd_data / dropout_rows, ViTVAEEncoder.train_transformer(dropout=True) and the pass-through keywords).

p = 0 gives the bits of the entries without dropout.  The mask a kernel applies is revealed exactly (ones through dropout_rows; attention on q = k = 0 and
one-hot values) and equals tests/vit_dropout_reference.py's numpy restatement of include/cvae_hip.h's rule.  Every kernel against float64 with the same
masks on bf16-exact operands, element-wise within the bounds derived in that file's docstring; the whole walk by the 4 x rule of DESIGN §14 / §15 against
the masked float64 restatement, the k bias by its element-wise bound.  Every ratio is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_encoder_grad_reference as gr  # noqa: E402
import vit_dropout_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
LN2 = 0.6931471805599453
KEY_A, KEY_B = 0x1234567890ABCDEF, 0x0FEDCBA987654321
c = lambda t: t.detach().cpu().double()


def ops():
    from causal_vae_amd import ops as o
    return o


def rand(*shape, seed=0, scale=1.0):
    """bf16-exact fp32 values"""
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).bfloat16().float()


def within(got, ref, err, what):
    diff = (c(got) - ref).abs()
    ratio = float((diff / err.clamp_min(1e-300)).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert torch.isfinite(got.float()).all() and ratio <= 1.0, (what, ratio)


def mlp_operands(M, seed=1):
    y2, hid = rand(M, 256, seed=seed).to(DEV), rand(M, 512, seed=seed + 1).to(DEV)
    W1, b1 = rand(512, 256, seed=seed + 2, scale=0.1).to(DEV), rand(512, seed=seed + 3).to(DEV)
    W2, b2 = rand(256, 512, seed=seed + 4, scale=0.1).to(DEV), rand(256, seed=seed + 5).to(DEV)
    return y2, hid, W1, b1, W2, b2


# ---- p = 0: the bits of the entries without dropout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one", [False, True])
def test_p0_attention_is_bit_identical(one):
    o, B, N = ops(), 2, 65
    nq = 1 if one else N
    qkv = rand(B, N, 768, seed=3).to(DEV)
    q, k, v = qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:]
    out, lse = o.mhsa_train(q, k, v, n_query_rows=nq)
    out0, lse0 = o.mhsa_train(q, k, v, n_query_rows=nq, dropout=(0.0, KEY_A))
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    dout = rand(B, nq, 256, seed=4).to(DEV)
    run = lambda **kw: (lambda d: o.mhsa_bwd(q, k, v, out, lse, dout, d[:, :nq, :256], d[:, :, 256:512], d[:, :, 512:], **kw))(torch.full_like(qkv, 7.0))
    for a, b in zip(run(), run(dropout=(0.0, KEY_A))):
        assert torch.equal(a, b)


def test_p0_row_sites_are_bit_identical():
    o, M = ops(), 129
    y2, hid, W1, b1, W2, b2 = mlp_operands(M)
    h1, pre1 = o.token_gemm_gelu_train(y2, W1, b1)
    h0, pre0 = o.token_gemm_dropout(y2, W1, b1, "gelu", (0.0, KEY_A))
    assert torch.equal(h1, h0) and torch.equal(pre1, pre0)
    resid = rand(M, 256, seed=9).to(DEV)
    x1 = o.token_gemm(hid, W2, b2, "residual", resid=resid, out=torch.empty_like(resid))
    x0 = o.token_gemm_dropout(hid, W2, b2, "residual", (0.0, KEY_A, 0, 7), resid=resid, out=torch.empty_like(resid))
    assert torch.equal(x1, x0)
    inplace = resid.clone()
    assert o.token_gemm_dropout(hid, W2, b2, "residual", (0.0, KEY_A), resid=inplace) is inplace and torch.equal(inplace, x1)
    G = rand(M, 256, seed=10).to(DEV)
    assert torch.equal(o.token_gemm_bwd_data(G, W2, F32, gate_pre=pre1), o.token_gemm_bwd_data(G, W2, F32, gate_pre=pre1, dropout=(0.0, KEY_A)))
    assert torch.equal(o.token_gemm_bwd_data(G, W2, F32), o.token_gemm_bwd_data(G, W2, F32, dropout=(0.0, KEY_B)))
    assert torch.equal(o.dropout_rows(G, (0.0, KEY_A)), G)


def test_refusals():
    o, L = ops(), __import__("causal_vae_amd._lib", fromlist=["CvaeError"])
    x = rand(4, 256).to(DEV)
    for bad in ((1.0, KEY_A), (-0.1, KEY_A), (0.1,), (0.1, KEY_A, 0), (0.1, -1), (0.1, KEY_A, 0, 0)):
        with pytest.raises(L.CvaeError):
            o.dropout_rows(x, bad)
    with pytest.raises(L.CvaeError, match="float32"):
        o.dropout_rows(x.bfloat16(), (0.1, KEY_A))
    qkv = rand(1, 4, 768).to(DEV).bfloat16()
    with pytest.raises(L.CvaeError, match="float32"):
        o.mhsa_train(qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:], dropout=(0.1, KEY_A))


# ---- the mask, revealed exactly ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(3, 256), (70, 512)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_rows_on_ones_is_the_mask(M, N, p):
    o = ops()
    s = dr.scale(p)
    ones = torch.ones(M, N, device=DEV)
    for row0, step in ((0, 1), (0, 7), (5, 3)):
        want = dr.keep_rows(M, N, p, KEY_A, row0, step).astype(np.float32) * s
        got = o.dropout_rows(ones, (p, KEY_A, row0, step))
        assert np.array_equal(got.cpu().numpy(), want), (M, N, p, row0, step)
    big = torch.ones(M, 2, N, device=DEV)                                   # strided rows, in place
    assert o.dropout_rows(big[:, 1], (p, KEY_B), out=big[:, 1]) is not None
    assert np.array_equal(big[:, 1].cpu().numpy(), dr.keep_rows(M, N, p, KEY_B).astype(np.float32) * s) and bool((big[:, 0] == 1).all())
    assert not torch.equal(o.dropout_rows(ones, (p, KEY_A)), o.dropout_rows(ones, (p, KEY_B)))


@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("N", [7, 32])
def test_attention_mask_revealed_by_one_hot_values(N, one):
    """q = k = 0: every probability is 1 / N; v[j] = one-hot(j) in every head: out[b, i, 32 h + j] = keep[b, h, i, j] / N * s, the fp32 quotient times the
    fp32 constant, one rounding of that product"""
    o, B, p = ops(), 2, 0.1
    nq = 1 if one else N
    qkv = torch.zeros(B, N, 768, device=DEV)
    for h in range(8):
        qkv[:, :, 512 + 32 * h:512 + 32 * h + N] = torch.eye(N, device=DEV)
    out, lse = o.mhsa_train(qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:], n_query_rows=nq, dropout=(p, KEY_A))
    keep = dr.keep_attn(B, N, p, KEY_A, nq)                                # [B, 8, nq, N]
    want = np.zeros((B, nq, 8, 32), dtype=np.float32)
    want[..., :N] = ((keep.astype(np.float32) / np.float32(N)) * dr.scale(p)).transpose(0, 2, 1, 3)
    assert np.array_equal(out.cpu().numpy().reshape(B, nq, 8, 32), want)
    assert 0 < keep.sum() < keep.size
    assert torch.equal(lse, o.mhsa_train(qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:], n_query_rows=nq)[1])


# ---- kernels against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("N", [7, 64, 65, 200])
def test_mhsa_dropout_against_float64(N, one, p):
    o, B = ops(), 2
    nq = 1 if one else N
    qkv = rand(B, N, 768, seed=N).to(DEV)
    q, k, v = qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:]
    out, lse = o.mhsa_train(q, k, v, n_query_rows=nq, dropout=(p, KEY_A))
    assert torch.equal(lse, o.mhsa_train(q, k, v, n_query_rows=nq)[1])      # the undropped rows' statistic, bit for bit
    m = dr.tmask(dr.keep_attn(B, N, p, KEY_A, nq), p)
    o64, _lse64 = dr.attn_fwd(c(q), c(k), c(v), m, nq)
    within(out, o64, dr.attn_fwd_bound(c(q), c(k), c(v), m, nq), f"mhsa_train dropout out N{N} nq{nq} p{p}")
    dout = rand(B, nq, 256, seed=N + 1).to(DEV)
    run = lambda: (lambda d: o.mhsa_bwd(q, k, v, out, lse, dout, d[:, :nq, :256], d[:, :, 256:512], d[:, :, 512:], dropout=(p, KEY_A)))(torch.full_like(qkv, 7.0))
    got = run()
    args = (c(q), c(k), c(v), c(out), c(lse) * LN2, c(dout), m)
    parts, ref = dr.attn_bwd(*args, parts=True), dr.attn_bwd(*args)
    for name, g, want, err in zip(("dq", "dk", "dv"), got, ref, dr.attn_bwd_bounds(parts)):
        assert g.shape == want.shape
        within(g, want, err, f"mhsa_bwd dropout {name} N{N} nq{nq} p{p}")
    for a, b in zip(got, run()):
        assert torch.equal(a, b)                                            # two runs: the same bits
    assert torch.equal(out, o.mhsa_train(q, k, v, n_query_rows=nq, dropout=(p, KEY_A))[0])
    assert not torch.equal(out, o.mhsa_train(q, k, v, n_query_rows=nq, dropout=(p, KEY_B))[0])


@pytest.mark.parametrize("rows", [(0, 1), (0, 7)])
@pytest.mark.parametrize("M", [1, 33, 200])
@pytest.mark.parametrize("K,N", [(256, 512), (512, 256)])
def test_token_gemm_dropout_against_float64(K, N, M, rows):
    o, p = ops(), 0.1
    x, W, b = rand(M, K, seed=M).to(DEV), rand(N, K, seed=K, scale=0.1).to(DEV), rand(N, seed=N + 1).to(DEV)
    m = dr.tmask(dr.keep_rows(M, N, p, KEY_A, *rows), p)
    hid, pre = o.token_gemm_dropout(x, W, b, "gelu", (p, KEY_A) + rows)
    y64, pre64, e_y, e_pre = dr.gelu_dropout(c(x), c(W), c(b), m)
    within(pre, pre64, e_pre, f"gelu dropout pre K{K} N{N} M{M} {rows}")
    within(hid, y64, e_y, f"gelu dropout y K{K} N{N} M{M} {rows}")
    assert bool((hid[(m == 0).to(DEV)] == 0).all())                        # dropped elements are exact zeros
    assert torch.equal(pre, o.token_gemm_gelu_train(x, W, b)[1])            # the pre-activation is stored undropped
    resid = rand(M, 3, N, seed=7).to(DEV)[:, 1]                             # strided rows
    got = o.token_gemm_dropout(x, W, b, "residual", (p, KEY_B) + rows, resid=resid, out=torch.empty(M, N, device=DEV))
    m2 = dr.tmask(dr.keep_rows(M, N, p, KEY_B, *rows), p)
    r64, e_r = dr.resid_dropout(c(x), c(W), c(b), c(resid), m2)
    within(got, r64, e_r, f"residual dropout K{K} N{N} M{M} {rows}")
    assert torch.equal(got[(m2 == 0).to(DEV)], resid[(m2 == 0).to(DEV)])   # a dropped product leaves the residual as it was
    # the data gradient of this GEMM: g [M, N] W [N, K] -> dx [M, K], mask and gate over dx
    g, gate = rand(M, N, seed=M + 3).to(DEV), rand(M, K, seed=M + 4).to(DEV)
    m3 = dr.tmask(dr.keep_rows(M, K, p, KEY_A, *rows), p)
    dx = o.token_gemm_bwd_data(g, W, F32, gate_pre=gate, dropout=(p, KEY_A) + rows)
    d64, e_d = dr.bwd_data_dropout(c(g), c(W), c(gate), m3)
    within(dx, d64, e_d, f"bwd_data dropout K{K} N{N} M{M} {rows}")
    assert torch.equal(dx, o.token_gemm_bwd_data(g, W, F32, gate_pre=gate, dropout=(p, KEY_A) + rows))
    assert torch.equal(hid, o.token_gemm_dropout(x, W, b, "gelu", (p, KEY_A) + rows)[0])


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------
IMG, DEPTH, B_WALK = (64, 96), 2, 3


def encoder(seed=0, keys_seed=77):
    from causal_vae_amd.vit.models import ViTVAEEncoder
    torch.manual_seed(seed)
    model = ViTVAEEncoder(img_size=IMG, depth=DEPTH, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    model.requires_grad_(False)
    model.dropout_keys = ops().DropoutKeys(seed=keys_seed)
    return model.to(DEV).eval()


def cotangents(B, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g)


def run_walk(model, x, cls_only, step=0):
    model._cls_only_last_block = cls_only
    model.dropout_keys.step = step
    params = model.train_transformer(dropout=True)
    model.zero_grad(set_to_none=True)
    collect = {}
    mu, lv = model.encode_with_grad(x, collect)
    gm, gl = cotangents(x.shape[0])
    torch.autograd.backward([mu, lv], [gm.to(DEV), gl.to(DEV)])
    got = {k: p.grad.clone() for (k, _p), p in zip(model._transformer_named(), params)}
    got["dstem"] = collect["dstem"]
    return mu.detach(), lv.detach(), got


def test_model_determinism_and_inference_untouched():
    x = vr.vit_inputs(B_WALK, *IMG, seed=5).to(DEV)
    a, b = encoder(), encoder()
    with torch.no_grad():
        mu0, lv0 = a.encode(x)
    mu_a, lv_a, g_a = run_walk(a, x, True)
    assert a.dropout_keys.step == 1                                          # one step per training forward
    mu_b, lv_b, g_b = run_walk(b, x, True)
    assert torch.equal(mu_a, mu_b) and torch.equal(lv_a, lv_b) and all(torch.equal(g_a[k], g_b[k]) for k in g_a)       # the same (seed, step): the same bits
    assert not torch.equal(mu_a, mu0)                                       # it did drop
    mu_c = a.encode_with_grad(x)[0]                                         # the next step: other masks
    assert a.dropout_keys.step == 2 and not torch.equal(mu_c.detach(), mu_a)
    mu_d, _lv, _g = run_walk(encoder(keys_seed=78), x, True)
    assert not torch.equal(mu_d, mu_a)                                      # another seed
    with torch.no_grad():
        mu1, lv1 = a.encode(x)
        assert torch.equal(a.cls_features_with_grad(x), a.cls_features(x))  # under no_grad: the inference walk, no dropout, no step drawn
    assert torch.equal(mu0, mu1) and torch.equal(lv0, lv1) and a.dropout_keys.step == 2
    a.freeze_transformer()
    assert torch.equal(a.encode_with_grad(x)[0], mu0) and a.dropout_keys.step == 2
    a.train_transformer(dropout=True)
    a.set_compute_dtype(torch.bfloat16)
    with pytest.raises(RuntimeError, match="float32"):
        a.encode_with_grad(x)


def walk_pair(dropout):
    """(result with the CLS-only last block, result with the full one) of one model and one step"""
    model = encoder()
    x = vr.vit_inputs(B_WALK, *IMG, seed=5).to(DEV)
    if dropout:
        return run_walk(model, x, True), run_walk(model, x, False)
    out = []
    for cls_only in (True, False):
        model._cls_only_last_block = cls_only
        params = model.train_transformer()
        model.zero_grad(set_to_none=True)
        mu, lv = model.encode_with_grad(x)
        gm, gl = cotangents(B_WALK)
        torch.autograd.backward([mu, lv], [gm.to(DEV), gl.to(DEV)])
        out.append((mu.detach(), lv.detach(), {k: p.grad.clone() for (k, _p), p in zip(model._transformer_named(), params)}))
    return out


def test_cls_only_last_block_features_agree_bit_for_bit_under_dropout():
    """the CLS-only last block (mask rows b N, query 0) gives the full block's CLS rows bit for bit, with dropout as without; and every gradient tensor on which
    the two forms agree bit for bit without dropout, they agree on with it: dropout adds no disagreement"""
    (mu_t, lv_t, got_t), (mu_f, lv_f, got_f) = walk_pair(True)
    assert torch.equal(mu_t, mu_f) and torch.equal(lv_t, lv_f)
    (_m, _l, plain_t), (_m2, _l2, plain_f) = walk_pair(False)
    same_plain = {k for k in plain_t if torch.equal(plain_t[k], plain_f[k])}
    same_drop = {k for k in plain_t if torch.equal(got_t[k], got_f[k])}
    print(f"bit-equal without dropout: {len(same_plain)} of {len(plain_t)} tensors; with dropout: {len(same_drop)}")
    assert same_plain and same_plain <= same_drop, sorted(same_plain - same_drop)


def test_cls_only_last_block_gradients_agree_bit_for_bit_under_dropout():
    """with _cls_only_last_block True and False every transformer gradient (and dstem) agrees bit for bit under dropout: the backward of a full last block is
    the CLS-only block's on the CLS rows of what it kept, with the mask rows b N and query 0"""
    (_mu_t, _lv_t, got_t), (_mu_f, _lv_f, got_f) = walk_pair(True)
    differ = []
    for k in got_t:
        d = float((got_t[k] - got_f[k]).abs().max())
        print(f"{k}: bit-equal {torch.equal(got_t[k], got_f[k])}, max |difference| {d:.3e}, max |gradient| {float(got_t[k].abs().max()):.3e}")
        if not torch.equal(got_t[k], got_f[k]):
            differ.append(k)
    assert not differ, differ


@pytest.mark.parametrize("cls_only", [True, False])
def test_walk_with_dropout_against_float64(cls_only):
    model = encoder()
    x = vr.vit_inputs(B_WALK, *IMG, seed=5).to(DEV)
    with torch.no_grad():
        stem = model._stem_cl(x).detach().cpu().double().view(B_WALK, -1, 256)
    N = stem.shape[1] + 1
    mu_t, lv_t, got = run_walk(model, x, cls_only)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    gm, gl = cotangents(B_WALK)
    K = ops().DropoutKeys
    masks = []
    for i, blk in enumerate(model.transformer):
        rates = (blk.attn.dropout, blk.mlp[2].p, blk.mlp[4].p)
        keys = tuple(model.dropout_keys.key(0, i, site) for site in (K.ATTN, K.MLP_ACT, K.MLP_OUT))
        masks.append(dr.block_masks(B_WALK, N, rates, keys, cls_only=(cls_only and i == DEPTH - 1)))
    r64, o64 = dr.transformer_vjp(sd, stem, DEPTH, gm, gl, masks, cls_only_last=cls_only, want_parts=True)
    r32, _o32 = dr.transformer_vjp(sd, stem, DEPTH, gm, gl, masks, dtype=F32, cls_only_last=cls_only)
    print(f"mu rel-L2 {gr.rel_l2(mu_t, o64['mu']):.3e}")
    assert gr.rel_l2(mu_t, o64["mu"]) < 1e-5 and gr.rel_l2(lv_t, o64["log_var"]) < 1e-5      # the masks of the restatement are the kernels'
    worst = []
    for k, g in got.items():
        assert g is not None and torch.isfinite(g.float()).all(), k
        a, ref, oth = c(g).reshape(r64[k].shape), r64[k], r32[k].double()
        if k.endswith("attn.in_proj_bias"):                                 # the k bias: zero in exact arithmetic, held to its rounding bound
            bound = dr.k_bias_bound(r64["k_bias_parts"][int(k.split(".")[1])])
            kr = float((a[256:512].abs() / bound).max())
            print(f"{k}[256:512]: max |got| / bound = {kr:.4f} (max |got| {float(a[256:512].abs().max()):.3e})")
            assert kr <= 1.0, (k, kr)
            keep = torch.ones(768, dtype=torch.bool)
            keep[256:512] = False
            a, ref, oth = a[keep], ref[keep], oth[keep]
        mine, yard = gr.rel_l2(a, ref), gr.rel_l2(oth, ref)
        ratio = mine / yard if yard > 0.0 else (0.0 if mine == 0.0 else float("inf"))
        print(f"{k}: rel-L2 {mine:.3e}, fp32 CPU evaluation {yard:.3e}, ratio {ratio:.3f} (allowed 4)")
        worst.append((ratio / 4.0, k))
    print("worst ratio / allowed", max(worst))
    assert max(worst)[0] <= 1.0, max(worst)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------------
def vitvae(seed=0):
    import vit_decoder_reference as vd
    from causal_vae_amd.vit.models import ViTVAE
    torch.manual_seed(seed)
    model = ViTVAE(img_size=IMG, depth=DEPTH, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    vd.randomize_decoder_bn(model.decoder, seed + 2)
    return model.to(DEV).eval()


def test_vitvae_train_all_with_dropout():
    from causal_vae_amd.vit import train_vit_vae, vit_vae_loss
    model = vitvae()
    x = vr.vit_inputs(2, *IMG, seed=9).to(DEV)
    with torch.no_grad():
        mu0, lv0 = model.encode(x)
    model.train_all(dropout=True)
    assert model._dropout and not model.training
    recons, _x, mu, lv = model.forward_train(x)
    assert not torch.equal(mu, mu0)
    vit_vae_loss(recons, x, mu, lv).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(model.encode(x), (mu0, lv0)))
    loader = [{"x": vr.vit_inputs(2, *IMG, seed=11 + i)} for i in range(2)]
    opt = torch.optim.Adam(model.parameters(), lr=0.0)                      # the parameters stay: encode can be compared afterwards
    step = model.dropout_keys.step
    losses = train_vit_vae(model, loader, opt, DEV, epochs=1, dropout=True)
    assert len(losses) == 1 and np.isfinite(losses[0]) and model.dropout_keys.step == step + 2 and model._dropout
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(model.encode(x), (mu0, lv0)))
    train_vit_vae(model, loader[:1], opt, DEV, epochs=1)                    # the default: no dropout, no step drawn
    assert not model._dropout and model.dropout_keys.step == step + 2


def test_causal_vitvae_train_adapters_with_dropout():
    import vit_decoder_reference as vd
    from causal_vae_amd.vessel.train import loss_function, total_loss
    from causal_vae_amd.vit.causal import CausalViTVAE
    torch.manual_seed(5)
    model = CausalViTVAE(img_size=IMG, depth=DEPTH)
    vd.randomize_decoder_bn(model.backbone.decoder, 6)
    vr.randomize_stem_bn(model.backbone.stem, 7)
    model = model.to(DEV)
    gen = torch.Generator().manual_seed(8)
    B = 3
    x = torch.rand(B, 1, *IMG, generator=gen).to(DEV)
    m, t = torch.randn(B, model.m_dim, generator=gen).to(DEV), torch.randn(B, model.t_dim, generator=gen).to(DEV)
    with torch.no_grad():
        mu0, lv0 = model.backbone.eval().encode(x)
    params = model.train_adapters(decoder=True, transformer=True, dropout=True)
    assert model.backbone._dropout and not model.backbone.training
    out = model.forward_train(x, m, t)
    total_loss(*loss_function(out[0], x, out[1], m, *out[2:])).backward()
    assert model.backbone.dropout_keys.step == 1
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(model.backbone.encode(x), (mu0, lv0)))
