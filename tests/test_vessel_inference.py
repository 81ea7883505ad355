"""CausalVesselVAE inference: encode / decode with BatchNorm2d folded into the convs (cvae_fold_bn_conv), the batched sweeps of
causal_vae_amd.vessel.analysis and counterfactual.batched_counterfactual on the vessel model, and the two reduction kernels
(cvae_row_diff_norms, cvae_stack_mean_std) — against the reference golden, the unfolded layer path, float64 CPU and torch written the
reference consumers' way.

Folded-vs-unfolded bounds (fp32 unit roundoff u = 2^-24, bf16 u_b = 2^-8).  Per layer the two paths compute the same real function with the
same conv kernel and summation order; they differ only in roundings: the folded weight w s (1 rounding per product), the folded bias
(b - mean) s + beta (3), and the BatchNorm epilogue (x - mean) rstd gamma + beta of the unfolded path (4) — at most 8 u relative to the
layer's output scale.  Seven layers add at most 7 x 8 u = 56 u = 3.3e-6 in relative L2 (BatchNorm keeps the gain per layer near 1; the
final sigmoid only shrinks differences).  bf16 activations: the two paths round the weights to bf16 independently (w vs w s) and the unfolded
one rounds the conv output once more before BatchNorm — at most 2 roundings of u_b / 2 per layer, 7 u_b = 2.7e-2 over the decoder.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    from causal_vae_amd import FusedAdam
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.counterfactual import batched_counterfactual
    from causal_vae_amd.vessel import CausalVesselVAE, ensemble_reconstruction, feature_importance, z_permutation_grid
    from causal_vae_amd.vessel import train_step as vessel_step

DEV = "cuda"
U32 = 2.0 ** -24
FP32_FOLD_REL_L2 = 7 * 8 * U32          # 3.3e-6 (module docstring)
BF16_FOLD_REL_L2 = 7 * 2.0 ** -8        # 2.7e-2


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def trained_model(golden):
    """seed-42 model with the golden's post-step state (weights after one Adam step, running statistics of one training forward): a BatchNorm
    whose statistics are not the init's 0 / 1, so the fold is not the identity."""
    g = golden("vessel2d_b4")
    torch.manual_seed(42)
    model = CausalVesselVAE().to(DEV)
    sd = model.state_dict()
    for k in g.keys("sd1"):
        sd[k].copy_(g.t("sd1/" + k).to(DEV))
    return model.eval()


def golden_batch(golden, name="vessel2d_b4_eval"):
    from conftest import vessel2d_inputs
    B, seed = (int(v) for v in golden(name).t("in/seed"))
    return tuple(v.to(DEV) for v in vessel2d_inputs(B, seed))


# ------------------------------------------------------------------------------------------------ 1. golden
def test_encode_decode_match_reference_golden(golden):
    """encode / decode (folded) of the eval-mode model against the reference class's own eval forward (vessel2d_b4_eval), at the tolerances of
    test_vessel2d_eval_mode_and_validate_match_reference_golden."""
    ge = golden("vessel2d_b4_eval")
    model = trained_model(golden)
    x, m, t, eps = golden_batch(golden)
    mu, logvar = model.encode(x, m, t)
    ge.check("eval", "mu", mu, rtol=1e-3, atol=2e-4)
    ge.check("eval", "logvar", logvar, rtol=1e-3, atol=2e-4)
    recon = model.decode(mu + eps * torch.exp(0.5 * logvar), m)
    ge.check("eval", "recon_x", recon, rtol=1e-3, atol=2e-4)


# ------------------------------------------------------------------------------------------------ 2. decode is forward's tail
def test_unfolded_paths_are_forward_bit_for_bit_and_folded_within_bound(golden):
    model = trained_model(golden)
    x, m, t, eps = golden_batch(golden)
    with torch.no_grad():
        recon, _mh, mu, logvar, _a, _b = model(x, m, t, eps=eps)
        z = model.reparameterize(mu, logvar, eps)
    mu_u, lv_u = model.encode(x, m, t, folded=False)
    assert torch.equal(mu_u, mu) and torch.equal(lv_u, logvar)
    assert torch.equal(model.decode(z, m, folded=False), recon)
    mu_f, lv_f = model.encode(x, m, t)
    dec_f = model.decode(z, m)
    e_mu, e_lv, e_dec = rel_l2(mu_f, mu), rel_l2(lv_f, logvar), rel_l2(dec_f, recon)
    print(f"fp32 folded vs unfolded rel-L2: mu {e_mu:.2e}  logvar {e_lv:.2e}  decode {e_dec:.2e}  (bound {FP32_FOLD_REL_L2:.2e})")
    assert e_dec <= FP32_FOLD_REL_L2, e_dec
    # enc_fc (Linear 61440 -> 1024, BatchNorm1d, Linear) sits between the folded encoder and mu: its own conditioning multiplies the encoder's
    # bound; the check here is that the folded encoder leaves mu as close as the decoder leaves the image, with 4x headroom for that head
    assert e_mu <= 4 * FP32_FOLD_REL_L2 and e_lv <= 4 * FP32_FOLD_REL_L2, (e_mu, e_lv)
    model.set_compute_dtype(torch.bfloat16)
    try:
        b_u, b_f = model.decode(z, m, folded=False), model.decode(z, m)
    finally:
        model.set_compute_dtype(torch.float32)
    e_b = rel_l2(b_f, b_u)
    print(f"bf16 folded vs bf16 unfolded decode rel-L2 {e_b:.2e} (bound {BF16_FOLD_REL_L2:.2e})")
    assert e_b <= BF16_FOLD_REL_L2, e_b
    assert model.training is False


def test_decode_checks_shapes_and_training_mode_uses_layer_path(golden):
    model = trained_model(golden)
    z, m = torch.randn(2, 128, device=DEV), torch.randn(2, 12, device=DEV)
    with pytest.raises(RuntimeError, match="decode"):
        model.decode(m, z)                                     # swapped arguments: 12 / 128 columns
    with pytest.raises(RuntimeError, match="decode"):
        model.decode(z, m[:1])
    model.train()
    a = model.decode(z, m)                                     # training mode: the layer path (batch statistics), whatever `folded` says
    b = model.decode(z, m, folded=False)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. the fold kernel
def _fold64(w, kind, bias, gamma, beta, mean, var, eps):
    w, bias = w.double().cpu(), bias.double().cpu()
    if kind == ops.FOLD_UPCONV_K3:
        A = torch.tensor([[0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0]], dtype=torch.float64)
        w = torch.einsum("ka,oiab,lb->iokl", A, w, A)                         # [Cin][Cout][4][4]
    if gamma is None:
        return w, bias
    s = gamma.double().cpu() / torch.sqrt(var.double().cpu() + eps)
    shape = (-1, 1, 1, 1) if kind == ops.FOLD_CONV_K4 else (1, -1, 1, 1)
    return w * s.view(shape), (bias - mean.double().cpu()) * s + beta.double().cpu()


@pytest.mark.parametrize("kind,cout,cin", [(0, 5, 3), (0, 64, 32), (0, 1, 1), (1, 7, 6), (1, 33, 20), (1, 1, 32), (1, 40, 17)],
                         ids=["k4-5x3", "k4-64x32", "k4-1x1", "k3-7x6", "k3-33x20", "k3-1x32", "k3-40x17"])
def test_fold_kernel_matches_float64(kind, cout, cin):
    g = torch.Generator().manual_seed(cout * 100 + cin + kind)
    k = 4 if kind == ops.FOLD_CONV_K4 else 3
    w = torch.randn(cout, cin, k, k, generator=g)
    b = torch.randn(cout, generator=g)
    for with_bn in (True, False):
        bn = torch.nn.BatchNorm2d(cout).eval()
        with torch.no_grad():
            bn.weight.copy_(torch.randn(cout, generator=g) * 2)
            bn.bias.copy_(torch.randn(cout, generator=g))
            bn.running_mean.copy_(torch.randn(cout, generator=g))
            bn.running_var.copy_(torch.rand(cout, generator=g) * 3 + 0.01)
        bn = bn.to(DEV)
        with torch.no_grad():
            (wo, bo), = ops.fold_bn_conv([(w.to(DEV), kind, b.to(DEV), bn if with_bn else None)])
        args = (bn.weight, bn.bias, bn.running_mean, bn.running_var) if with_bn else (None,) * 4
        w64, b64 = _fold64(w, kind, b, *args, bn.eps)
        # the bound is relative to the magnitude of what is summed: |A| |W3| |A^T| |s| (k3: up to 4 weights add), |b - mean| |s| + |beta|
        wa64, ba64 = _fold64(w.abs(), kind, b.abs(), *((a.abs() for a in args) if with_bn else args), bn.eps)
        if with_bn:
            s_abs = bn.weight.double().cpu().abs() / torch.sqrt(bn.running_var.double().cpu() + bn.eps)
            ba64 = (b.double().abs() + bn.running_mean.double().cpu().abs()) * s_abs + bn.bias.double().cpu().abs()
        assert tuple(wo.shape) == tuple(w64.shape)
        dw = (wo.double().cpu() - w64).abs()
        db = (bo.double().cpu() - b64).abs()
        assert bool((dw <= 1e-6 * wa64.abs() + 1e-30).all()), (with_bn, float((dw / wa64.abs().clamp_min(1e-30)).max()))
        assert bool((db <= 1e-6 * ba64.abs() + 1e-30).all()), (with_bn, float((db / ba64.abs().clamp_min(1e-30)).max()))
        if not with_bn:
            assert torch.equal(bo.cpu(), b)                                   # bias copied
            if kind == ops.FOLD_UPCONV_K3:
                with torch.no_grad():
                    assert torch.equal(wo, ops.Conv3ToK4.apply(w.to(DEV)))    # the plain transform: cvae_conv3_to_k4's bits


def test_fold_table_of_many_layers_in_one_launch():
    """A table mixing both kinds (the encoder + decoder shapes, shrunk), entries with and without BatchNorm, up to the 16-entry limit."""
    g = torch.Generator().manual_seed(5)
    table, refs = [], []
    for i in range(16):
        kind = i % 2
        cout, cin = 8 + 3 * i, 4 + 5 * i
        k = 4 if kind == 0 else 3
        w, b = torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g)
        bn = None
        if i % 3:
            bn = torch.nn.BatchNorm2d(cout).eval()
            with torch.no_grad():
                bn.weight.uniform_(0.5, 2.0, generator=g)
                bn.running_var.uniform_(0.1, 2.0, generator=g)
                bn.running_mean.normal_(generator=g)
            bn = bn.to(DEV)
        table.append((w.to(DEV), kind, b.to(DEV), bn))
        refs.append(_fold64(w, kind, b, *((bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else (None,) * 4), 1e-5))
    with torch.no_grad():
        outs = ops.fold_bn_conv(table)
    for (wo, bo), (w64, b64) in zip(outs, refs):
        assert rel_l2(wo, w64) < 1e-6 and rel_l2(bo, b64) < 1e-6
    with pytest.raises(CvaeError, match="1 to 16"):
        with torch.no_grad():
            ops.fold_bn_conv(table + table[:1])


def test_forward_only_helpers_raise_under_autograd():
    w = torch.randn(4, 2, 4, 4, device=DEV, requires_grad=True)
    with pytest.raises(CvaeError, match="forward-only"):
        ops.fold_bn_conv([(w, ops.FOLD_CONV_K4, None, None)])
    a = torch.randn(3, 5, device=DEV, requires_grad=True)
    with pytest.raises(CvaeError, match="forward-only"):
        ops.row_diff_norms(a, a.detach())
    with pytest.raises(CvaeError, match="forward-only"):
        ops.stack_mean_std([a, a.detach()])


# ------------------------------------------------------------------------------------------------ 4. no stale weights
def test_folded_decode_follows_a_training_step():
    """Parameters and running statistics are rewritten in place by HIP kernels (FusedAdam, bn2d_fwd) without moving tensor._version: the folded
    decode after a step must be the new state's, not a cached fold of the old one."""
    from conftest import vessel2d_inputs
    x, m, t, eps = (v.to(DEV) for v in vessel2d_inputs(2, 11))
    torch.manual_seed(42)
    model = CausalVesselVAE().to(DEV)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(3)
    z, mz = torch.randn(3, 128, generator=g).to(DEV), torch.randn(3, 12, generator=g).to(DEV)
    model.eval()
    before = model.decode(z, mz)
    model.train()
    vessel_step(model, opt, x, m, t, eps=eps)
    model.eval()
    after_f, after_u = model.decode(z, mz), model.decode(z, mz, folded=False)
    e = rel_l2(after_f, after_u)
    moved = float((after_f - before).abs().max())
    print(f"after one step: folded vs unfolded rel-L2 {e:.2e}; moved by {moved:.2e}")
    assert e <= FP32_FOLD_REL_L2, e
    assert moved > 1e-4 and rel_l2(before, after_u) > 1e3 * FP32_FOLD_REL_L2


# ------------------------------------------------------------------------------------------------ 5. sweeps
def _ref_decode(model, z_row, m_row, swap=False):
    """the reference consumers' decoder expression on today's (unfolded) eval layer path, one row"""
    with torch.no_grad():
        cat = torch.cat([z_row, m_row], 1) if swap else torch.cat([m_row, z_row], 1)
        return model.dec_conv(model.dec_fc(cat).view(-1, 512, 6, 10))


def test_batched_counterfactual_on_the_vessel_model(golden):
    model = trained_model(golden)
    g = torch.Generator().manual_seed(9)
    z, m = torch.randn(2, 128, generator=g).to(DEV), torch.randn(2, 12, generator=g).to(DEV)
    feats, vals = [0, 5], [-1.0, 1.5]
    out = batched_counterfactual(model, z, m, feats, vals)
    assert tuple(out.shape) == (2, 2, 2, 1, 768, 1280)
    worst, worst_abs, worst_swap = 0.0, 0.0, float("inf")
    for b in range(2):
        for fi, f in enumerate(feats):
            for vi, v in enumerate(vals):
                m1 = m[b:b + 1].clone()
                m1[0, f] = v
                ref = _ref_decode(model, z[b:b + 1], m1)
                worst = max(worst, rel_l2(out[b, fi, vi], ref[0]))
                worst_abs = max(worst_abs, float((out[b, fi, vi] - ref[0]).abs().max()))
                sw = _ref_decode(model, z[b:b + 1], m1, swap=True)          # a mis-dispatched decode: dec_fc(cat[z, m']), 140 columns too
                worst_swap = min(worst_swap, float((out[b, fi, vi] - sw[0]).abs().max()))
    print(f"sweep vs per-value loop rel-L2 {worst:.2e}, max |diff| {worst_abs:.2e}; nearest swapped decode max |diff| {worst_swap:.2e}")
    assert worst <= FP32_FOLD_REL_L2, worst
    # the swapped decode lies at least 1000x farther from the sweep than the right one does (and farther than fp32 noise on a [0, 1] image)
    assert worst_swap > 1e3 * max(worst_abs, 1e-7), (worst_swap, worst_abs)
    chunked = batched_counterfactual(model, z, m, feats, vals, chunk_rows=3)
    e = rel_l2(chunked, out)
    print(f"chunk_rows=3 vs one call: rel-L2 {e:.2e}, bit-equal {torch.equal(chunked, out)}")
    assert e <= 1e-6, e
    with pytest.raises(ValueError):
        batched_counterfactual(model, z, m, feats, vals, size=(384, 640))


def test_batched_counterfactual_existing_models_unchanged_by_chunking():
    from causal_vae_amd.mnist_baseline import CausalMorphVAE12
    torch.manual_seed(42)
    vae = CausalMorphVAE12().to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    zz, mm = torch.randn(3, 10, generator=g), torch.rand(3, 12, generator=g)
    whole = batched_counterfactual(vae, zz.to(DEV), mm.to(DEV), [1, 2], [0.0, 1.0])
    parts = batched_counterfactual(vae, zz.to(DEV), mm.to(DEV), [1, 2], [0.0, 1.0], chunk_rows=5)
    assert whole.shape == parts.shape
    torch.testing.assert_close(parts, whole, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 6. analysis
def _cpu_decode64(sd, z, m):
    """The decoder restated from the state dict with torch CPU float64 ops (models.py:58-60,108-134 of the reference, eval mode)."""
    sd = {k: v.detach().double().cpu() for k, v in sd.items()}
    h = torch.cat([m, z], 1).double().cpu()
    h = F.linear(h, sd["dec_fc.0.weight"], sd["dec_fc.0.bias"])
    h = F.batch_norm(h, sd["dec_fc.1.running_mean"], sd["dec_fc.1.running_var"], sd["dec_fc.1.weight"], sd["dec_fc.1.bias"], False, 0.0, 1e-5)
    h = F.leaky_relu(h, 0.2)
    h = F.relu(F.linear(h, sd["dec_fc.3.weight"], sd["dec_fc.3.bias"])).view(-1, 512, 6, 10)
    for i in range(7):
        j = 4 * i + 1
        h = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), sd[f"dec_conv.{j}.weight"], sd[f"dec_conv.{j}.bias"], padding=1)
        if i < 6:
            h = F.relu(F.batch_norm(h, sd[f"dec_conv.{j + 1}.running_mean"], sd[f"dec_conv.{j + 1}.running_var"], sd[f"dec_conv.{j + 1}.weight"],
                                    sd[f"dec_conv.{j + 1}.bias"], False, 0.0, 1e-5))
    return torch.sigmoid(h)


def test_feature_importance_matches_reference_loop(golden):
    model = trained_model(golden)
    g = torch.Generator().manual_seed(21)
    N = 4
    z, m = torch.randn(N, 128, generator=g).to(DEV), torch.randn(N, 12, generator=g).to(DEV)
    got = feature_importance(model, z, m, chunk_rows=16)
    again = feature_importance(model, z, m, chunk_rows=16)
    assert torch.equal(got, again)                                     # run-to-run bits
    x_base = model.decode(z, m)
    ref = []
    for i in range(12):                                                # analyze_vessel.py:98-117, on the same HIP decodes
        m_p = m.clone()
        m_p[:, i] += 1.0
        x_p = model.decode(z, m_p)
        ref.append((x_p - x_base).view(x_p.size(0), -1).norm(dim=1).mean())
    ref = torch.stack(ref)
    print("feature importance:", [f"{v:.4g}" for v in got.tolist()])
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-6)
    # one decode of the sweep against the decoder restated on CPU in float64
    cpu = _cpu_decode64(model.state_dict(), z[1:2].cpu(), m[1:2].cpu())
    e = rel_l2(x_base[1:2], cpu)
    print(f"HIP folded decode vs CPU float64 restatement: rel-L2 {e:.2e}, max |diff| {float((x_base[1:2].double().cpu() - cpu).abs().max()):.2e}")
    assert e <= 1e-5 and float((x_base[1:2].double().cpu() - cpu).abs().max()) <= 1e-4


def _models(k):
    out = []
    for s in range(k):
        torch.manual_seed(100 + s)
        mdl = CausalVesselVAE().to(DEV)
        with torch.no_grad():                                           # running statistics away from 0 / 1 so that every fold matters
            for mod in mdl.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.normal_(0.0, 0.1)
                    mod.running_var.uniform_(0.5, 1.5)
        out.append(mdl.eval())
    return out


def test_ensemble_reconstruction_matches_torch_stack():
    from conftest import vessel2d_inputs
    x, m, t, eps = (v.to(DEV) for v in vessel2d_inputs(2, 31))
    models = _models(5)
    recons = []
    for mdl in models:
        mu, lv = mdl.encode(x, m, t)
        recons.append(mdl.decode(mdl.reparameterize(mu, lv, eps), m))
    for k in (1, 2, 5):
        mean, std = ensemble_reconstruction(models[:k], x, m, t, eps=eps)
        st = torch.stack(recons[:k])
        torch.testing.assert_close(mean, st.mean(0), rtol=1e-6, atol=1e-7)           # ensemble_reconstruction.py:86-89
        if k == 1:
            assert bool(torch.isnan(std).all()) and bool(torch.isnan(st.std(0)).all())
        else:
            torch.testing.assert_close(std, st.std(0), rtol=1e-4, atol=1e-7)
    m2, s2 = ensemble_reconstruction(models, x, m, t, eps=eps)
    assert torch.equal(m2, mean) and torch.equal(s2, std)


def test_z_permutation_grid_matches_reference_triple_loop():
    from conftest import vessel2d_inputs
    x, m, t, _eps = (v.to(DEV) for v in vessel2d_inputs(3, 41))
    models = _models(2)
    grid = z_permutation_grid(models, x, m, t, scale=1.5, chunk_rows=4)
    assert tuple(grid.shape) == (3, 3, 1, 768, 1280)
    worst = 0.0
    with torch.no_grad():
        for i in range(3):                                              # check_mechanism_z_perm.py:100-125
            for j in range(3):
                preds = []
                for mdl in models:
                    _, _, mu, _lv, _, _ = mdl(x[j:j + 1], m[j:j + 1], t[j:j + 1])
                    h = mdl.dec_fc(torch.cat([m[i:i + 1], mu * 1.5], 1)).view(-1, 512, 6, 10)
                    preds.append(mdl.dec_conv(h))
                worst = max(worst, float((grid[i, j] - torch.stack(preds).mean(0)[0]).abs().max()))
    print(f"z-permutation grid vs reference loop: max |diff| {worst:.2e}")
    assert worst <= 1e-5, worst
    assert torch.equal(z_permutation_grid(models, x, m, t, scale=1.5, chunk_rows=4), grid)


# ------------------------------------------------------------------------------------------------ 7. reductions
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,n", [(1, 1), (3, 7), (5, 4097), (2, 16383), (4, 12288)])
def test_row_diff_norms_match_float64(rows, n, dtype):
    g = torch.Generator().manual_seed(rows * 7 + n)
    a = torch.randn(rows, n, generator=g).to(dtype)
    b = torch.randn(rows + 2, n, generator=g).to(dtype)
    ref = torch.randint(0, rows + 2, (rows,), generator=g)
    ad, bd = a.to(DEV), b.to(DEV)
    for r in (None, ref.to(DEV)):
        l2, ma = ops.row_diff_norms(ad, bd, r, want_mean_abs=True)
        bb = b[:rows] if r is None else b[r.cpu()]
        d = a.double() - bb.double()
        torch.testing.assert_close(l2.double().cpu(), d.norm(dim=1), rtol=1e-5, atol=1e-30)
        torch.testing.assert_close(ma.double().cpu(), d.abs().mean(dim=1), rtol=1e-5, atol=1e-30)
        l2b, mab = ops.row_diff_norms(ad, bd, r, want_mean_abs=True)
        assert torch.equal(l2, l2b) and torch.equal(ma, mab)                 # run-to-run bits
        one = ops.row_diff_norms(ad[-1:], bd, torch.full((1,), rows - 1, device=DEV) if r is None else r[-1:])[0]
        assert torch.equal(one, l2[-1:])                                     # a row's bits do not depend on the other rows of the call
    bad = torch.tensor([0] * (rows - 1) + [rows + 2], device=DEV)
    l2, _ = ops.row_diff_norms(ad, bd, bad)
    assert bool(torch.isnan(l2[-1])) and bool(torch.isfinite(l2[:-1]).all())   # a ref outside b: NaN, nothing read


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("n", [1, 7, 4099, 65539])
def test_stack_mean_std_matches_float64(k, n):
    g = torch.Generator().manual_seed(k * 1000 + n)
    xs = [torch.randn(n, generator=g) * 3 + 1 for _ in range(k)]
    xd = [v.to(DEV) for v in xs]
    mean, std = ops.stack_mean_std(xd)
    st = torch.stack(xs).double()
    torch.testing.assert_close(mean.double().cpu(), st.mean(0), rtol=1e-6, atol=1e-6)
    if k == 1:
        assert bool(torch.isnan(std).all())
    else:
        torch.testing.assert_close(std.double().cpu(), st.std(0), rtol=1e-5, atol=1e-6)
    m2, s2 = ops.stack_mean_std(xd)
    assert torch.equal(m2, mean) and (k == 1 or torch.equal(s2, std))
    # an unaligned view (offset by one float) takes the element-wise path: same values
    big = [torch.cat([torch.zeros(1), v]).to(DEV)[1:] for v in xs]
    mu, su = ops.stack_mean_std(big)
    torch.testing.assert_close(mu, mean, rtol=0, atol=0)
    if k > 1:
        torch.testing.assert_close(su, std, rtol=0, atol=0)
