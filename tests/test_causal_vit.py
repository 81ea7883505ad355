"""CausalViTVAE on the GPU.  The fused heads kernel (csrc/heads.hip) against float64 with the element-wise bound of tests/causal_vit_reference.py (its
docstring: c u sum|terms| with c counted from the operations the kernel issues), row independence, live parameters; the whole model against the fp32
golden and float64 within the composed bound, bf16 within twice the rounding-oracle gap; the reference's call patterns; the consumers against one row at
a time; cvae_latent_to_grid at the production latent width K = 512."""
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import causal_vit_reference as cr  # noqa: E402
from test_causal_vit_cpu import NAME, reference_state  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
BATCHES = (1, 8, 17, 64, 768)


def ops():
    from causal_vae_amd import ops as o
    return o


def within(got, ref, err, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = float(((got.detach().cpu().double() - ref).abs() / err).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


def strided(t, extra):
    """t's values as a column slice of a wider matrix on the GPU: unit column stride, row stride t.shape[1] + extra"""
    wide = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), device=DEV)
    wide[:, 3:3 + t.shape[1]] = t.to(DEV)
    return wide[:, 3:3 + t.shape[1]]


class Head:
    """One of the three served heads with weights that make the clamps bite, its inputs, and its float64 statement."""

    def __init__(self, kind, B, seed=0):
        from causal_vae_amd.vit import AdapterMLP
        g = torch.Generator().manual_seed(100 + seed)
        self.kind, self.B = kind, B
        self.clamp0 = self.clamp1 = self.eps = self.split = None
        if kind == "morph":
            torch.manual_seed(3)
            self.mods = nn.ModuleList([nn.Linear(19, 64), nn.Linear(64, 64), nn.Linear(64, 12), nn.Linear(64, 12)])
            with torch.no_grad():
                self.mods[3].weight[::2] *= 150.0                                   # every other logvar column far past +-10
            self.layers = [(self.mods[0], None, 0.2), (self.mods[1], None, 0.2), ((self.mods[2], self.mods[3]), None, None)]
            self.panels = [torch.randn(B, 19, generator=g)]
            self.split, self.clamp1 = 12, (-10.0, 10.0)
        else:
            torch.manual_seed(4)
            self.mods = AdapterMLP(287, 512, 256) if kind == "enc" else AdapterMLP(140, 256, 512)
            bn = self.mods[1]
            with torch.no_grad():
                bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=g))
                bn.bias.copy_(0.1 * torch.randn(bn.num_features, generator=g))
                bn.running_mean.copy_(0.1 * torch.randn(bn.num_features, generator=g))
                bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))
            self.layers = self.mods.head_layers()
            if kind == "enc":
                with torch.no_grad():
                    self.mods[3].weight[0:128:3] *= 2000.0                          # every third mu column past +-100
                    self.mods[3].weight[128:256:2] *= 150.0                         # every other logvar column past +-10
                self.panels = [torch.randn(B, w, generator=g) for w in (256, 12, 19)]
                self.split, self.clamp0, self.clamp1 = 128, (-100.0, 100.0), (-10.0, 10.0)
                self.eps = torch.randn(B, 128, generator=g)
            else:
                self.panels = [torch.randn(B, w, generator=g) for w in (12, 128)]
        self.mods.to(DEV).eval()

    @torch.no_grad()
    def run(self, rows=None):
        sl = (lambda t: t) if rows is None else (lambda t: t[rows])
        return ops().mlp_heads([strided(sl(p), 5 + i) for i, p in enumerate(self.panels)], self.layers, split=self.split, clamp0=self.clamp0,
                               clamp1=self.clamp1, eps=None if self.eps is None else strided(sl(self.eps), 7))

    def float64(self):
        """(pre-clamp values, bound) over all output columns"""
        d = lambda t: t.detach().cpu().double()
        lay = []
        for lin, bn, slope in self.layers:
            pair = lin if isinstance(lin, tuple) else (lin,)
            W, b = torch.cat([d(p.weight) for p in pair], 0), torch.cat([d(p.bias) for p in pair], 0)
            lay.append((W, b, None if bn is None else (d(bn.weight), d(bn.bias), d(bn.running_mean), d(bn.running_var), bn.eps), slope))
        x = torch.cat([p.double() for p in self.panels], 1)
        return cr.head_b(x, torch.zeros_like(x), lay)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", ["enc", "dec", "morph"])
def test_heads_kernel_against_float64(kind, B):
    h = Head(kind, B)
    first, second, z = h.run()
    y, e = h.float64()
    N = y.shape[1]
    S = h.split or N
    clamp = lambda v, c: v if c is None else v.clamp(*c)
    within(first, clamp(y[:, :S], h.clamp0), e[:, :S], f"{kind} B{B} first")
    if S < N:
        within(second, clamp(y[:, S:], h.clamp1), e[:, S:], f"{kind} B{B} second")
    else:
        assert second is None
    for c, v in ((h.clamp0, y[:, :S]), (h.clamp1, y[:, S:])):
        if c is not None:                                                           # the clamp bites on some values and leaves others alone
            assert bool((v > c[1] + 1).any()) and bool((v < c[0] - 1).any()) and bool(((v > c[0] + 1) & (v < c[1] - 1)).any()), (kind, c)
    if h.eps is not None:
        mu, lv = first.cpu().double(), second.cpu().double()
        assert bool((mu.abs() == 100).any()) and bool((lv.abs() == 10).any()) and bool((mu.abs() < 100).any()) and bool((lv.abs() < 10).any())
        zero = torch.zeros_like(mu)
        want, ez = cr.reparam_b(mu, zero, lv, zero, h.eps.double())                 # z from the kernel's OWN clamped outputs
        within(z, want, ez, f"{kind} B{B} z")
    else:
        assert z is None
    again = h.run()
    assert all(a is None or torch.equal(a, b) for a, b in zip(again, (first, second, z)))


@pytest.mark.parametrize("kind", ["enc", "dec", "morph"])
def test_a_row_of_a_768_row_call_equals_the_row_alone(kind):
    h = Head(kind, 768)
    full = h.run()
    for r in (0, 5, 15, 16, 401, 767):
        for a, b in zip(full, h.run(rows=slice(r, r + 1))):
            assert (a is None and b is None) or torch.equal(a[r:r + 1], b), (kind, r)
    for a, b in zip(full, h.run(rows=slice(760, 768))):
        assert (a is None and b is None) or torch.equal(a[760:], b), kind


def test_batchnorm_parameters_are_read_live():
    h = Head("dec", 8)
    before = h.run()[0].clone()
    with torch.no_grad():
        h.mods[1].running_var.mul_(4.0)                                              # in place, through the same storage: nothing may be cached
    after = h.run()[0]
    assert not torch.equal(before, after)
    y, e = h.float64()
    within(after, y, e, "dec after rewriting running_var")


@torch.no_grad()
def test_expanded_and_transposed_views_equal_their_copies():
    """The kernel addresses ptr + row * stride + col.  One row expanded over the batch (row stride 0: one eps draw or one m row shared by the rows) and a
    transposed view do not fit that; they are copied, not read past their storage."""
    B = 24
    h = Head("enc", B)
    cls_out, m, t = (p.to(DEV) for p in h.panels)
    eps = h.eps.to(DEV)
    kw = dict(split=h.split, clamp0=h.clamp0, clamp1=h.clamp1)
    m1, eps1 = m[:1].expand(B, -1), eps[:1].expand(B, -1)
    t_tr = t.t().contiguous().t()
    assert m1.stride() == (0, 1) and eps1.stride() == (0, 1) and t_tr.stride() == (1, B)
    got = ops().mlp_heads([cls_out, m1, t_tr], h.layers, eps=eps1, **kw)
    want = ops().mlp_heads([cls_out, m1.contiguous(), t], h.layers, eps=eps1.contiguous(), **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    for r in (0, 7, 23):                                                            # and the row alone, with the shared eps row
        alone = ops().mlp_heads([cls_out[r:r + 1], m[:1], t[r:r + 1]], h.layers, eps=eps[:1], **kw)
        assert all(torch.equal(a[r:r + 1], b) for a, b in zip(got, alone)), r
    d = Head("dec", B)
    md, zd = (p.to(DEV) for p in d.panels)
    z1 = zd[:1].expand(B, -1)
    assert torch.equal(ops().mlp_heads([md, z1], d.layers)[0], ops().mlp_heads([md, z1.contiguous()], d.layers)[0])


@torch.no_grad()
def test_unsupported_shapes_are_errors():
    from causal_vae_amd._lib import CvaeError
    x = torch.randn(4, 600, device=DEV)
    with pytest.raises(CvaeError, match="not supported"):
        ops().mlp_heads([x], [(nn.Linear(600, 8).to(DEV), None, None)])
    with pytest.raises(CvaeError, match="not supported"):
        ops().mlp_heads([x[:, :16]], [(nn.Linear(16, 513).to(DEV), None, None)])


# ---- the whole model -----------------------------------------------------------------------------------------------------------------
_STATE = {}


def state(golden):
    if not _STATE:
        g = golden(NAME)
        model, sd, inp, crop = reference_state(g)
        bound, ref = cr.composed_bound(sd, *inp, 6, key=NAME, crop=crop)
        _STATE.update(g=g, model=model.to(DEV).eval(), sd=sd, inp=inp, crop=crop, bound=bound, ref=ref)
    s = _STATE
    s["model"].set_compute_dtype(F32)
    return s


def run_model(model, inp, crop):
    x, m, t, eps = (v.to(DEV) for v in inp)
    recon, m_hat, mu, logvar, m_mu, m_logvar = model(x, m, t, eps)
    assert m_hat is m_mu and recon.shape == x.shape and recon.dtype == F32
    z = model.reparameterize(mu, logvar, eps)
    out = dict(mu=mu, logvar=logvar, m_mu=m_mu, m_logvar=m_logvar, z=z, z_vit=model.dec_adapter(torch.cat([m, z], 1)), recon_x=recon,
               recon_crop=recon[:, :, crop[0]:crop[1], crop[2]:crop[3]], cls_out=model.backbone.cls_features(x))
    return out


def test_whole_model_fp32_against_float64_and_golden(golden):
    s = state(golden)
    got = run_model(s["model"], s["inp"], s["crop"])
    for k in ("cls_out", "mu", "logvar", "m_mu", "m_logvar", "z", "z_vit", "recon_crop", "recon_x"):
        ratio = vr.fro_ratio(got[k], s["ref"][k], s["bound"][k])
        print(f"{k}: ||HIP fp32 - float64|| / bound = {ratio:.2e} (rel-L2 {vr.rel_l2(got[k].cpu(), s['ref'][k]):.3e})")
        assert ratio <= 1.0, (k, ratio)
        if s["g"].has("out/" + k):                                                   # both sit within the bound of float64: within twice it of each other
            assert vr.fro_ratio(got[k], s["g"].t("out/" + k).double(), 2 * s["bound"][k]) <= 1.0, (k, "against the fp32 golden")


def test_whole_model_bf16_within_twice_the_rounding_oracle_gap(golden):
    s = state(golden)
    orac = cr.forward_ref(s["sd"], *s["inp"], 6, rnd=vr.round_bf16)
    got = run_model(s["model"].set_compute_dtype(BF16), s["inp"], s["crop"])
    for k in ("mu", "logvar", "z_vit", "recon_x"):
        gap, mine = vr.rel_l2(orac[k], s["ref"][k]), vr.rel_l2(got[k].cpu(), s["ref"][k])
        print(f"bf16 {k}: rounding oracle vs float64 {gap:.3e}; HIP bf16 vs float64 {mine:.3e}")
        assert mine <= 2.0 * gap, (k, mine, gap)
    for k in ("m_mu", "m_logvar"):                                                   # the morph predictor never sees the backbone: fp32 in both modes
        assert vr.fro_ratio(got[k], s["ref"][k], s["bound"][k]) <= 1.0, k


def small_model(seed):
    from causal_vae_amd.vit import CausalViTVAE
    torch.manual_seed(seed)
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    vr.randomize_stem_bn(model.backbone.stem, seed + 1)
    cr.randomize_head_bn(model, seed + 2)
    return model.to(DEV).eval()


def test_reference_call_patterns(golden):
    model = small_model(11)
    x, m, t, eps = (v.to(DEV) for v in cr.causal_inputs(3, 64, 96, 21))
    mu, logvar = model.encode(x, m, t)
    z = model.reparameterize(mu, logvar, eps)
    by_hand = model.backbone.decode(model.dec_adapter(torch.cat([m, z], 1)))          # the consumers' expression (analyze_vessel.py)
    assert torch.equal(by_hand, model.decode(z, m))
    out = model(x, m, t, eps)
    assert torch.equal(out[2], mu) and torch.equal(out[3], logvar)
    zk = model.enc_adapter.fused([model.backbone.cls_features(x), m, t], split=128, clamp0=(-100.0, 100.0), clamp1=(-10.0, 10.0), eps=eps)[2]
    assert torch.equal(out[0], model.decode(zk, m))                                  # forward's image = decode of the z its own launch wrote
    within(zk, *cr.reparam_b(mu.cpu().double(), torch.zeros(3, 128, dtype=torch.float64), logvar.cpu().double(), torch.zeros(3, 128, dtype=torch.float64),
                             eps.cpu().double()), "z of the encoder launch")
    m_mu, m_lv = model.predict_morph(t)
    assert torch.equal(out[4], m_mu) and torch.equal(out[5], m_lv) and out[1] is out[4]
    # the sweeps' own expressions: one m row or one eps draw expanded over the batch
    m0, e0 = m[:1].expand(3, -1), eps[:1].expand(3, -1)
    assert torch.equal(model.decode(z, m0), model.decode(z, m0.contiguous()))
    assert torch.equal(model.decode(z[:1].expand(3, -1), m), model.decode(z[:1].expand(3, -1).contiguous(), m))
    for a_, b_ in zip(model(x, m0, t, e0), model(x, m0.contiguous(), t, e0.contiguous())):
        assert torch.equal(a_, b_)
    assert torch.equal(model.reparameterize(mu, logvar, e0), model.reparameterize(mu, logvar, e0.contiguous()))
    torch.manual_seed(5)
    a = model(x, m, t)
    torch.manual_seed(5)
    b = model(x, m, t, torch.randn(3, 128, device=DEV))
    assert torch.equal(a[0], b[0])                                                   # eps=None draws torch.randn on the device


def test_consumers_equal_one_row_at_a_time():
    from causal_vae_amd.counterfactual import batched_counterfactual, sweep_inputs
    from causal_vae_amd.vessel import analysis
    o = ops()
    model, other = small_model(11), small_model(31)
    x, m, t, eps = (v.to(DEV) for v in cr.causal_inputs(3, 64, 96, 22))
    z = torch.randn(3, 128, device=DEV)
    one = lambda mdl, zz, mm: torch.cat([mdl.decode(zz[r:r + 1], mm[r:r + 1]) for r in range(zz.shape[0])])
    # feature_importance: the same norms from single-row decodes
    feats = [0, 5, 11]
    fi = analysis.feature_importance(model, z, m, delta=0.7, features=feats, chunk_rows=4)
    rows = []
    for f in feats:
        mp = m.clone()
        mp[:, f] += 0.7
        rows.append(torch.cat([o.row_diff_norms(model.decode(z[r:r + 1], mp[r:r + 1]), model.decode(z[r:r + 1], m[r:r + 1]))[0] for r in range(3)]))
    assert torch.equal(fi, torch.stack(rows).mean(dim=1))
    # batched_counterfactual
    vals = [-1.0, 0.5]
    cf = batched_counterfactual(model, z, m, feats, vals, chunk_rows=5)
    z_rep, m_cf = sweep_inputs(z, m, feats, vals)
    assert torch.equal(cf.flatten(0, 2), one(model, z_rep, m_cf))
    # precision= reaches the backbone and the model's own choice is put back
    model.set_compute_dtype(BF16)
    assert torch.equal(batched_counterfactual(model, z, m, feats, vals), cf) and model.compute_dtype == BF16          # the default is the fp32 sweep
    cf16 = batched_counterfactual(model, z, m, feats, vals, precision="model")
    assert torch.equal(cf16.flatten(0, 2), model.decode(z_rep, m_cf)) and not torch.equal(cf16, cf)
    model.set_compute_dtype(F32)
    assert torch.equal(batched_counterfactual(model, z, m, feats, vals, precision="bf16"), cf16) and model.compute_dtype == F32
    # z_permutation_grid, two models
    grid = analysis.z_permutation_grid([model, other], x, m, t, scale=0.5, chunk_rows=4)
    per = []
    for mdl in (model, other):
        mus = torch.cat([mdl.encode(x[r:r + 1], m[r:r + 1], t[r:r + 1])[0] for r in range(3)]) * 0.5
        per.append(torch.stack([torch.cat([mdl.decode(mus[j:j + 1], m[i:i + 1]) for j in range(3)]) for i in range(3)]))
    assert torch.equal(grid, o.stack_mean_std([p.flatten(0, 1) for p in per])[0].view_as(grid))
    # ensemble_reconstruction, two models, shared eps
    mean, std = analysis.ensemble_reconstruction([model, other], x, m, t, eps)
    recs = [torch.cat([mdl(x[r:r + 1], m[r:r + 1], t[r:r + 1], eps[r:r + 1])[0] for r in range(3)]) for mdl in (model, other)]
    want_mean, want_std = o.stack_mean_std(recs)
    assert torch.equal(mean, want_mean) and torch.equal(std, want_std)


def test_validate_runs_the_model():
    from causal_vae_amd.vessel.train import validate, loss_function, total_loss
    from causal_vae_amd.vit import CausalViTVAE
    torch.manual_seed(13)
    model = CausalViTVAE(depth=1).to(DEV).eval()                                     # validate's loss is written for 768 x 1280 images
    data = [tuple(v[r] for v in cr.causal_inputs(4, 768, 1280, 23)[:3]) for r in range(4)]
    loader = torch.utils.data.DataLoader(data, batch_size=2)
    torch.manual_seed(7)
    got = validate(model, loader, device=DEV)
    torch.manual_seed(7)
    tot = 0.0
    for x, m, t in loader:
        x, m, t = x.to(DEV), m.to(DEV), t.to(DEV)
        recon_x, m_hat, mu, logvar, m_mu, m_logvar = model(x, m, t)
        tot = tot + total_loss(*loss_function(recon_x, x, m_hat, m, mu, logvar, m_mu, m_logvar), beta=0.5)
    assert got == float(tot) / 4 and got > 0 and got == got


# ---- cvae_latent_to_grid at the production latent width --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,P", [(1, 960), (2, 960), (19, 6), (64, 80)])
def test_latent_to_grid_at_k512_against_float64(dtype, B, P):
    K = 512
    g = torch.Generator().manual_seed(K + B + P)
    z, W, b = torch.randn(B, K, generator=g), torch.randn(256 * P, K, generator=g) * 0.05, torch.randn(256 * P, generator=g)
    got = ops().latent_to_grid(z.to(DEV), W.to(DEV), b.to(DEV), 256, dtype)
    ref = (z.double() @ W.double().T + b.double()).view(B, 256, P).transpose(1, 2)
    err = (K + 2) * vr.U32 * (z.double().abs() @ W.double().abs().T + b.double().abs()).view(B, 256, P).transpose(1, 2)
    err = err + (vr.UBF * ref.abs() if dtype == BF16 else 0.0)
    within(got, ref, err, f"latent_to_grid {dtype} K512 B{B} P{P}")
    one = ops().latent_to_grid(z[B - 1:].to(DEV), W.to(DEV), b.to(DEV), 256, dtype)
    assert torch.equal(one[0], got[B - 1])
