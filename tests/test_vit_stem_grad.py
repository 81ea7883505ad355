"""GPU tests of the ViT-VAE conv stem's gradients: cvae_conv_down_bwd_data, cvae_fold_bn_conv_bwd's kind CVAE_FOLD_CONV_K3S2, the gated
cvae_vit_tokens_bwd, ViTVAEEncoder.train_stem, ViTVAE.train_all / forward_train, vit_vae_loss / train_vit_vae and CausalViTVAE.train_adapters(stem=True).

cvae_conv_down_bwd_data alone: gate_act NONE / RELU are cvae_conv_up launches and must give its bits; fp32 LEAKY is the same multiplication of the same fp32
sum as cvae_conv_up followed by cvae_act_bwd, so it gives those bits too; and element-wise against float64 within the bound tests/test_conv_reference.py
uses for cvae_conv_up (oracle/conv64.py: C sqrt(K) U |S| . |w|) times |act'|, plus the one rounding of the product (fp32: U |dx|) or of the stored bf16 (half
an ulp).  The kernel forms the entry can reach, each at a small shape (FORMS; `up` never splits K, so the gated split-K finish cannot be reached).

The whole stem against the float64 restatement (tests/vit_stem_grad_reference.py after tests/vit_encoder_grad_reference.py) per tensor, by §16's rules: fp32
rel-L2 at most 4 x that of the fp32 CPU evaluation of the same restatement, bf16 at most 2 x the rounding-oracle gap.  Every ratio is printed before it is
asserted; DESIGN §17 holds the table measured on an MI355X.  The restatement takes the LeakyReLU masks of the HIP forward's own activations (checked against
float64 wherever the rounding bound decides a sign), as the decoder's does: at 64 x 96 one pre-activation of layer 1 is 1.7e-8 in float64 and an exact 0.0 in
fp32, and that one element moves the two lowest layers' gradients by 1e-3 of their norm.

Measured on the MI355X: cvae_conv_down_bwd_data max |error| / bound 0.03 - 0.09 (fp32), 0.92 - 0.99 (bf16: the half ulp of the stored value is nearly the whole
bound); the fold's way back <= 0.57; whole stem worst ratio / allowed 0.42 (fp32), 0.62 (bf16); ViTVAE end to end 0.41; CausalViTVAE 0.34; golden 2.09 of 6."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_encoder_grad_reference as gr  # noqa: E402
import vit_stem_grad_reference as sr  # noqa: E402
from oracle import conv64 as c64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SLOPE = {"leaky001": float(torch.tensor(0.01, dtype=F32)), "leaky02": float(torch.tensor(0.2, dtype=F32))}      # the kernels' fp32 constants


def ops():
    from causal_vae_amd import ops as o
    return o


# ---- cvae_conv_down_bwd_data -------------------------------------------------------------------------------------------------------------------------
STEM_PAIRS = [(64, 32), (128, 64), (256, 128), (256, 256)]      # (Cs, Cl) of the four data gradients of the stem
GRIDS = [(2, 3), (8, 10)]                                       # source grids: ragged against Tile<2,128> 8 x 16 and Tile<2,256> 16 x 16
# (dtype, Cs, Cl, source grid, (upfull, xpair), the kernel form the dispatch rules of conv_mfma.hip give it).  The stem's pairs on both grids with the
# library's own choice, then every other form forced: 32-channel tiles go to the whole-K kernel in bf16 when it exists for Cs (64, 128) and upfull allows,
# else to the data kernel; 64-channel tiles to the data kernel (bf16: per-wave weights, K-split waves); bf16 stages 32 channels (KH 2) from Cs 128 up;
# two samples per tile (XB 2): bf16, rows at most 8 wide, B >= 2.
FORMS = [(dt, Cs, Cl, grid, (-1, -1), "auto") for dt in ("f32", "bf16") for Cs, Cl in STEM_PAIRS for grid in GRIDS] + [
    ("f32", 64, 32, (8, 10), (0, 0), "data 32-ch fp32"), ("f32", 128, 64, (2, 3), (0, 0), "data 64-ch fp32"), ("f32", 16, 32, (2, 3), (-1, -1), "data 32-ch fp32, one k-step"),
    ("bf16", 64, 32, (2, 3), (1, -1), "whole-K KCH 4"), ("bf16", 64, 32, (8, 10), (1, -1), "whole-K KCH 4"), ("bf16", 128, 32, (8, 10), (1, -1), "whole-K KCH 8"),
    ("bf16", 256, 32, (2, 3), (1, 0), "data 32-ch KH 2 (no whole-K kernel for 256 channels)"),
    ("bf16", 64, 32, (8, 10), (0, 0), "data 32-ch KH 1"), ("bf16", 64, 32, (2, 3), (0, 1), "data 32-ch KH 1 XB 2"),
    ("bf16", 128, 32, (8, 10), (0, 0), "data 32-ch KH 2"), ("bf16", 128, 32, (2, 3), (0, 1), "data 32-ch KH 2 XB 2"),
    ("bf16", 64, 64, (8, 10), (-1, 0), "data 64-ch KH 1"), ("bf16", 64, 64, (2, 3), (-1, 1), "data 64-ch KH 1 XB 2"),
    ("bf16", 256, 128, (8, 10), (-1, 0), "data 64-ch KH 2"), ("bf16", 256, 128, (2, 3), (-1, 1), "data 64-ch KH 2 XB 2"), ("bf16", 256, 256, (2, 3), (-1, 1), "data 64-ch KH 2 XB 2"),
]


def gate_for(shape, dtype, seed):
    """an activation output of the result's shape: positive, negative and exactly-zero entries"""
    g = torch.Generator().manual_seed(seed)
    gate = torch.randn(*shape, generator=g)
    gate[torch.rand(*shape, generator=g) < 0.1] = 0.0
    gate = gate.to(dtype).to(F32)
    assert bool((gate > 0).any()) and bool((gate < 0).any()) and bool((gate == 0).any())
    return gate


class up_variant:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old, ops().UP_VARIANT = ops().UP_VARIANT, self.v

    def __exit__(self, *a):
        ops().UP_VARIANT = self.old


@pytest.mark.parametrize("i", range(len(FORMS)))
def test_conv_down_bwd_data(i):
    o = ops()
    dt, Cs, Cl, grid, variant, form = FORMS[i]
    dtype, B = {"f32": F32, "bf16": BF16}[dt], 2
    c = c64.make_case("up", 1700 + i, 2, B, Cl, Cs, grid, dtype, bias=False)
    gate = gate_for((B,) + c["l_dims"] + (Cl,), dtype, 1800 + i)
    g, gt = c["S"].to(DEV).to(dtype).contiguous(), gate.to(DEV).to(dtype).contiguous()
    wp = o.pack_weight(c["w"].to(DEV), 2, True, dtype)
    run = lambda act: o.conv_down_bwd_data(g, wp, gt if act else None, act, variant=variant)
    with up_variant(None if variant == (-1, -1) else variant + (0,)):
        plain = o._conv_up(g, wp, None, None, Cl, 2, None)
        masked = o._conv_up(g, wp, None, gt, Cl, 2, None)
    print(f"case {i}: {dt} {Cs} -> {Cl}, S {grid}, (upfull, xpair) {variant}: {form}")
    assert torch.equal(run(None), plain) and torch.equal(run("relu"), masked)
    ref, err, _pre, _e = c64.reference(c)
    for act in ("leaky001", "leaky02"):
        got = run(act)
        assert got.shape == gt.shape and got.dtype == dtype
        if dtype == F32:                                                     # the same multiplication of the same fp32 sum
            assert torch.equal(got, o._act_bwd(plain, gt, act)), act
        fac = torch.where(gate.double() > 0, 1.0, SLOPE[act])
        r, e = ref * fac, err * fac
        r, e = c64.out_bound(r, e + c64.U * r.abs(), dt)                     # the product's own rounding, then the stored dtype's
        ratio = c64.max_ratio(got, r, e)
        print(f"RATIO conv_down_bwd_data {dt} {act} [{form}] {ratio:.3f}")
        assert not c64.compare({"dx": got}, {"dx": r}, {"dx": e}), (act, ratio)
        assert torch.equal(got, run(act))                                    # fixed-order sums: the same bits


def test_conv_down_bwd_data_unsupported_shapes_do_not_launch():
    from causal_vae_amd import _lib as L
    o = ops()
    sentinel = lambda *s: torch.full(s, 7.0, device=DEV)
    UNSUPPORTED = -3                                                        # CVAE_E_UNSUPPORTED
    for Cs, Cl in ((24, 32), (64, 48), (64, 16)):
        g, w, gate, dx = sentinel(2, 2, 3, Cs), sentinel(Cs * Cl * 16), sentinel(2, 4, 6, Cl), sentinel(2, 4, 6, Cl)
        rc = L.lib.cvae_conv_down_bwd_data(g.data_ptr(), w.data_ptr(), gate.data_ptr(), dx.data_ptr(), 2, 2, 3, Cs, 4, 6, Cl, 2, 0, L.act_code("leaky001"), None, 0, -1,
                                           -1, o.stream())
        torch.cuda.synchronize()
        assert rc == L.lib.cvae_conv_down_bwd_data(None, None, None, None, 2, 2, 3, Cs, 4, 6, Cl, 2, 0, 0, None, 0, -1, -1, o.stream()) != 0      # decided before any pointer is looked at
        assert rc == UNSUPPORTED and float((dx - 7.0).abs().max()) == 0.0
        with pytest.raises(L.CvaeError):
            o.conv_down_bwd_data(g, w, gate, "leaky001")
    g, w, dx = sentinel(1, 2, 2, 2, 64), sentinel(64 * 32 * 64), sentinel(1, 4, 4, 4, 32)
    assert L.lib.cvae_conv_down_bwd_data(g.data_ptr(), w.data_ptr(), None, dx.data_ptr(), 1, 2, 2, 64, 4, 4, 32, 3, 0, 0, None, 0, -1, -1, o.stream()) != 0     # nd = 3
    assert L.lib.cvae_conv_down_bwd_data(g.data_ptr(), w.data_ptr(), dx.data_ptr(), dx.data_ptr(), 1, 2, 2, 64, 4, 4, 32, 2, 0, L.act_code("sigmoid"), None, 0, -1, -1,
                                         o.stream()) != 0
    torch.cuda.synchronize()
    assert float((dx - 7.0).abs().max()) == 0.0


# ---- the way back through the fold ---------------------------------------------------------------------------------------------------------------------
def fold_entry(cout, cin, seed, k=3):
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(cout, generator=g))
        bn.bias.copy_(0.1 * torch.randn(cout, generator=g))
        bn.running_mean.copy_(0.3 * torch.randn(cout, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(cout, generator=g))
    w, b = 0.2 * torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g)
    return w, b, bn.eval(), torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g)


def fold_check(what, quad, w, b, bn, dwf, dbf):
    """(dw, db, dgamma, dbeta) against float64 element-wise.  The kernel's operations on exact inputs (u = 2^-24): rstd = rsqrtf(var + eps) (one rounding of the
    sum, 2 ulp for the hardware reciprocal square root and its refinement), s = gamma rstd (1): |s - exact| <= 4 u |s|, so dw = s dwf and db = s dbf carry 5 u;
    dgamma = rstd (tot + dbf (b - mean)): tot is a sum of n = 9 Cin fused products in a fixed order ((n - 1) u sum |dwf w|, the fused product adds none), the
    bias term three roundings, the outer sum and product two more, rstd 3 u: (n + 2) u sum |dwf w| + 6 u |dbf (b - mean)| + 5 u |dgamma|, times rstd;
    dbeta = dbf exactly."""
    d = lambda t: t.detach().cpu().double()
    W, Bb, gam, mean, var = d(w), d(b), d(bn.weight), d(bn.running_mean), d(bn.running_var)
    rstd = 1.0 / torch.sqrt(var + bn.eps)
    s, u, n = gam * rstd, vr.U32, 9 * w.shape[1]
    G, gb = d(dwf), d(dbf)
    tot, bias_term = (G * W).sum((1, 2, 3)), gb * (Bb - mean)
    want = (G * s[:, None, None, None], gb * s, rstd * (tot + bias_term), gb)
    dgam_err = rstd * ((n + 2) * u * (G * W).abs().sum((1, 2, 3)) + 6 * u * bias_term.abs()) + 5 * u * want[2].abs()
    errs = (5 * u * want[0].abs(), 5 * u * want[1].abs(), dgam_err, torch.zeros_like(gb))
    for name, got, ref, err in zip(("dw", "db", "dgamma", "dbeta"), quad, want, errs):
        assert got.shape == ref.shape and got.dtype == F32, (what, name)
        diff = (d(got) - ref).abs()
        ratio = float((diff / err.clamp_min(1e-300)).max()) if float(err.max()) > 0 else float(diff.max())
        print(f"{what} {name}: max |got - float64| / bound = {ratio:.4f}")
        assert bool((diff <= err).all()), (what, name, ratio)


def test_fold_bn_conv_bwd_k3s2():
    o = ops()
    dims = [(32, 1), (64, 32), (128, 64), (256, 128), (256, 256)]           # the five stem layers: one launch; the first has Cin = 1
    cases = [fold_entry(co, ci, 50 + i) for i, (co, ci) in enumerate(dims)]
    table = []
    for w, b, bn, dwf, dbf in cases:
        k4 = torch.full(tuple(w.shape[:2]) + (4, 4), float("nan"))           # the fourth row and column: never read
        k4[:, :, :3, :3] = dwf
        table.append((w.to(DEV), o.FOLD_CONV_K3S2, b.to(DEV), bn.to(DEV), k4.to(DEV), dbf.to(DEV)))
    fold = torch.no_grad()(o.fold_bn_conv_bwd)                             # the BatchNorm parameters of the table ask for gradients: forward-only entry
    outs = fold(table)
    for i, (quad, case) in enumerate(zip(outs, cases)):
        fold_check(f"k3s2 layer {i}", quad, *case)
    again = fold(table)
    assert all(torch.equal(a, b) for qa, qb in zip(outs, again) for a, b in zip(qa, qb))
    # a mixed table: the existing kind's entry keeps the bits it has in a launch of its own
    w, b, bn, dwf, dbf = fold_entry(64, 64, 77)
    s1 = (w.to(DEV), o.FOLD_CONV_K3S1, b.to(DEV), bn.to(DEV), dwf.to(DEV), dbf.to(DEV))
    alone = fold([s1])[0]
    mixed = fold([table[1], s1, table[0]])
    assert all(torch.equal(a, b) for a, b in zip(alone, mixed[1]))
    assert all(torch.equal(a, b) for a, b in zip(outs[1], mixed[0])) and all(torch.equal(a, b) for a, b in zip(outs[0], mixed[2]))
    fold_check("k3s1 beside k3s2", mixed[1], w, b, bn, dwf, dbf)


# ---- gated token backward --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem_dtype", [F32, BF16])
@pytest.mark.parametrize("B", [1, 3])
def test_vit_tokens_bwd_gated(stem_dtype, B):
    o = ops()
    g = torch.Generator().manual_seed(B)
    dtok = (torch.randn(B, 7, 256, generator=g).bfloat16().float() * 1.0009765625).to(DEV)      # not bf16-exact: dstem is rounded
    gate = gate_for((B, 6, 256), stem_dtype, 30 + B).to(DEV).to(stem_dtype)
    dpos0, dcls0, dstem0 = o.vit_tokens_bwd(dtok, stem_dtype)
    assert torch.equal(o.vit_tokens_bwd(dtok, stem_dtype, gate=None, gate_act=None)[2], dstem0)
    for act in ("leaky001", "leaky02", "relu"):
        dpos, dcls, dstem = o.vit_tokens_bwd(dtok, stem_dtype, gate=gate, gate_act=act)
        assert torch.equal(dpos, dpos0) and torch.equal(dcls, dcls0)         # never gated
        slope = torch.tensor(SLOPE.get(act, 0.0), dtype=F32, device=DEV)
        want = (dtok[:, 1:] * torch.where(gate.float() > 0, torch.ones_like(slope), slope)).to(stem_dtype)      # the fp32 product, rounded once
        assert torch.equal(dstem, want), act
        assert torch.equal(dstem, o.vit_tokens_bwd(dtok, stem_dtype, gate=gate, gate_act=act)[2])
    with pytest.raises(Exception):
        o.vit_tokens_bwd(dtok, stem_dtype, gate=gate)                        # gate and gate_act come together


# ---- the whole stem ----------------------------------------------------------------------------------------------------------------------------------------
CASES = [((64, 96), 2), ((256, 320), 3)]
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


def stem_forward(sd, x, dtype=F64, rnd=None):
    """the stem's output [B, Np, 256] of the restatement in its folded form"""
    get = lambda k: sd[k].detach().to(dtype)
    h = x.to(dtype)
    for j in range(5):
        h, _e = vr.stem_layer_b(h, None, sd, j, get, rnd=rnd if rnd is not None else (lambda t: t))
    return h.flatten(2).transpose(1, 2)


def hip_masks(model, x, sd):
    """the LeakyReLU masks of the HIP forward's own five activations (NCHW bool), checked against float64 where the rounding bound decides the sign"""
    kept = {}
    with torch.no_grad():
        model._stem_cl(x, kept)
    ys = [y.detach().cpu().squeeze(1).permute(0, 3, 1, 2) for y in kept["ys"]]
    masks, undecided = sr.decided_masks(sd, x.cpu(), ys, model.compute_dtype == BF16)
    print(f"LeakyReLU masks of the HIP forward: {undecided} of {sum(m.numel() for m in masks)} signs undecided by the rounding bound")
    return masks


def chain(sd, x, depth, g_mu=None, g_lv=None, g_cls=None, dtype=F64, rnd=None, cls_only=False, masks=None, want_parts=False):
    """stem_vjp o transformer_vjp: {name: gradient} of the transformer's and the stem's tensors, `dstem` and `g0` (NHWC) from the cotangents; masks: the
    stem's LeakyReLU masks as arguments (hip_masks; tests/vit_stem_grad_reference.py says why); want_parts: `k_bias_parts` too, for gr.k_bias_bound"""
    grads = gr.transformer_vjp(sd, stem_forward(sd, x, dtype, rnd), depth, g_mu, g_lv, dtype=dtype, rnd=rnd, cls_only_last=cls_only, g_cls=g_cls,
                               want_parts=want_parts)[0]
    stem = sr.stem_vjp(sd, x, grads["dstem"], dtype=dtype, rnd=rnd, want_parts=True, masks=masks)
    grads["g0"] = stem.pop("g")[0].permute(0, 2, 3, 1)
    grads.update(stem)
    return grads


def references(img, B, bf, cls_only, model, x):
    """float64, its fp32 CPU evaluation and (bf16) the rounding oracle of one case, computed once and shared"""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if (img, B, bf, "masks") not in _REF:
        _REF[img, B, bf, "masks"] = hip_masks(model, x, sd)
    for kind in ("r64", "r32") + (("oracle",) if bf else ()):
        key = (img, B, bf, cls_only, kind)
        if key not in _REF:
            kw = dict(dtype=F32) if kind == "r32" else (dict(rnd=vr.round_bf16) if kind == "oracle" else {})
            _REF[key] = chain(sd, x.cpu(), 2, *cotangents(B), cls_only=cls_only, masks=_REF[img, B, bf, "masks"], **kw)
    return tuple(_REF.get((img, B, bf, cls_only, kind)) for kind in ("r64", "r32", "oracle"))


def check_rules(got, r64, r32, oracle, bf, label):
    """§16's rules per tensor: fp32 at most 4 x the fp32 CPU evaluation's rel-L2, bf16 at most 2 x the rounding-oracle gap (a zero gap: the fp32 rule).  The k
    third of an in_proj_bias is zero in exact arithmetic: it is held to its element-wise rounding bound (gr.k_bias_bound; r64 then carries `k_bias_parts`) and
    the rule to the q and v thirds, as tests/test_vit_encoder_grad.py does."""
    worst = []
    for k, g in got.items():
        assert g is not None and torch.isfinite(g.float()).all(), k
        a, ref = g.detach().cpu().double().reshape(r64[k].shape), r64[k].double()
        sel = slice(None)
        if k.endswith("attn.in_proj_bias"):
            parts = (oracle if bf else r64)["k_bias_parts"][int(k.split(".")[1])]
            kr = float((a[256:512].abs() / gr.k_bias_bound(parts, bf)).max())
            print(f"{k}[256:512] {label}: max |got| / bound = {kr:.4f} (max |got| {float(a[256:512].abs().max()):.3e})")
            assert kr <= 1.0, (k, kr)
            sel = torch.ones(768, dtype=torch.bool)
            sel[256:512] = False
        a, ref = a[sel], ref[sel]
        mine = sr.rel_l2(a, ref)
        yard, factor, rule = (sr.rel_l2(oracle[k].double()[sel], ref), 2.0, "rounding-oracle gap") if bf else (0.0, 4.0, "")
        if yard == 0.0:
            yard, factor, rule = sr.rel_l2(r32[k].double()[sel], ref), 4.0, "fp32 CPU evaluation"
        ratio = mine / yard if yard > 0.0 else (0.0 if mine == 0.0 else float("inf"))
        print(f"{k} {label}: rel-L2 {mine:.3e}, {rule} {yard:.3e}, ratio {ratio:.3f} (allowed {factor})")
        worst.append((ratio / factor, k))
    print(f"{label}: worst ratio / allowed", max(worst))
    assert max(worst)[0] <= 1.0, max(worst)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("cls_only", [True, False])
@pytest.mark.parametrize("img,B", CASES)
def test_stem_gradients_against_float64(img, B, dtype, cls_only):
    model = encoder(img).set_compute_dtype(dtype)
    model._cls_only_last_block = cls_only
    x = vr.vit_inputs(B, *img, seed=5).to(DEV)
    gm, gl = (t.to(DEV) for t in cotangents(B))
    with torch.no_grad():
        mu0, lv0 = model.encode(x)
    buffers = {k: v.clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
    tparams = model.train_transformer()                                     # first on a frozen stem: the bits the transformer side must keep
    frozen = {}
    mu, lv = model.encode_with_grad(x, frozen)
    torch.autograd.backward([mu, lv], [gm, gl])
    frozen_grads = [p.grad.clone() for p in tparams]
    model.zero_grad(set_to_none=True)
    sparams = model.train_stem()
    snames = [k for k, _p in model._stem_named()]
    assert snames == list(sr.STEM_KEYS)

    def run():
        model.zero_grad(set_to_none=True)
        col = {}
        mu, lv = model.encode_with_grad(x, col)
        assert torch.equal(mu, mu0) and torch.equal(lv, lv0)                # the training forward: the inference path's bits
        torch.autograd.backward([mu, lv], [gm, gl])
        return col, [p.grad.clone() for p in sparams], [p.grad.clone() for p in tparams]

    col, sgrads, tgrads = run()
    assert torch.equal(col["dstem"], frozen["dstem"]) and all(torch.equal(a, b) for a, b in zip(tgrads, frozen_grads))
    assert len(col["stem_g"]) == 5 and all(g.dtype == dtype for g in col["stem_g"])
    for k, v in model.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k                             # running statistics and num_batches_tracked: untouched
    col2, sgrads2, _t = run()
    assert all(torch.equal(a, b) for a, b in zip(sgrads, sgrads2)) and torch.equal(col["stem_g"][0], col2["stem_g"][0])
    bf = dtype == BF16
    r64, r32, oracle = references(img, B, bf, cls_only, model, x)
    got = dict(zip(snames, sgrads))
    got["g0"] = col["stem_g"][0].view(r64["g0"].shape)
    check_rules(got, r64, r32, oracle, bf, f"{dtype} cls_only={cls_only} {img} B{B}")


def test_stem_alone_and_a_parameter_rewritten_in_place():
    model = encoder((64, 96))
    x = vr.vit_inputs(2, 64, 96, seed=5).to(DEV)
    gm, gl = (t.to(DEV) for t in cotangents(2))
    both_t = model.train_transformer()
    both_s = model.train_stem()
    mu, lv = model.encode_with_grad(x)
    torch.autograd.backward([mu, lv], [gm, gl])
    want = [p.grad.clone() for p in both_s]
    model.zero_grad(set_to_none=True)
    model.freeze_transformer()                                              # train_stem() without train_transformer(): stem gradients only, the same bits
    mu, lv = model.encode_with_grad(x)
    torch.autograd.backward([mu, lv], [gm, gl])
    assert all(torch.equal(p.grad, w) for p, w in zip(both_s, want))
    assert all(p.grad is None for p in both_t)
    model.freeze_stem()
    with torch.no_grad():
        assert not model.cls_features_with_grad(x).requires_grad
    assert not model.cls_features_with_grad(x).requires_grad                # nothing asks: cls_features, nothing saved
    model.train_stem()
    mu, lv = model.encode_with_grad(x)
    with torch.no_grad():
        model.stem[4].weight.mul_(1.5)                                      # a BatchNorm weight rewritten between forward and backward
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.backward([mu, lv], [gm, gl])


def test_stem_gradients_against_the_golden(golden):
    """tests/golden/vitvae_stem_grad_64x96.npz: the reference class's fp32 CPU gradients.  The HIP fp32 result lies within 4 x the fp32 CPU evaluation's distance
    from float64 (this file's rule), the golden within 2 x (tests/test_vit_stem_grad_cpu.py's): so the two lie within 6 x of each other, per stored tensor."""
    from test_vit_reference_cpu import reference_state
    g = golden("vitvae_stem_grad_64x96")
    model, sd, x, depth = reference_state(g)
    z = g.z
    gm, gl = torch.from_numpy(z["in/g_mu"]), torch.from_numpy(z["in/g_lv"])
    model = model.to(DEV).eval()
    model.requires_grad_(False)
    model._cls_only_last_block = False                                      # the reference runs every block for every token
    model.train_transformer()
    params = model.train_stem()
    mu, lv = model.encode_with_grad(x.to(DEV))
    torch.autograd.backward([mu, lv], [gm.to(DEV), gl.to(DEV)])
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    masks = hip_masks(model, x.to(DEV), sd)
    r64, r32 = chain(sd, x, depth, gm, gl, masks=masks), chain(sd, x, depth, gm, gl, dtype=F32, masks=masks)
    for k, p in zip(sr.STEM_KEYS, params):
        want = torch.from_numpy(z["grad/" + k]).double()
        rows = torch.from_numpy(z[f"grad/{k}#rows"]) if f"grad/{k}#rows" in z.files else slice(None)
        got, a, b = p.grad.detach().cpu().double()[rows], r64[k][rows], r32[k].double()[rows]
        dist, own = float((got - want).norm()), float((a - b).norm())
        print(f"{k}: |HIP - golden| {dist:.3e}, |float64 - fp32 evaluation| {own:.3e}, ratio {dist / own:.3f} (allowed 6)")
        assert dist <= 6 * own, (k, dist, own)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------------
def vitvae(seed=3):
    from causal_vae_amd.vit import ViTVAE
    import vit_decoder_reference as dr
    torch.manual_seed(seed)
    model = ViTVAE(img_size=(64, 96), depth=2, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    dr.randomize_decoder_bn(model.decoder, seed + 2)
    return model.to(DEV).eval()


def test_vitvae_trains_end_to_end():
    import torch.nn.functional as F
    from causal_vae_amd.vit import vit_vae_loss
    o = ops()
    model = vitvae()
    B = 2
    gen = torch.Generator().manual_seed(8)
    x = vr.vit_inputs(B, 64, 96, seed=9).to(DEV)
    eps = torch.randn(B, 128, generator=gen).to(DEV)
    with torch.no_grad():
        mu0, lv0 = model.encode(x)
        rec0 = model.decode(o.Reparameterize.apply(mu0, lv0, eps))
    params = model.train_all()
    assert len(params) == len(list(model.parameters())) and not model.training
    recons, x_out, mu, lv = model.forward_train(x, eps)
    assert x_out is x and torch.equal(mu, mu0) and torch.equal(lv, lv0) and torch.equal(recons, rec0)      # the eval path's bits
    seen = {}
    mu.register_hook(lambda g: seen.__setitem__("g_mu", g.clone()))
    lv.register_hook(lambda g: seen.__setitem__("g_lv", g.clone()))
    loss = vit_vae_loss(recons, x, mu, lv, beta=0.5)
    want = F.mse_loss(recons, x) + 0.5 * (-0.5 * torch.mean(1 + lv - mu.pow(2) - lv.exp()))
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
    loss.backward()
    named = dict(model.named_parameters())
    for k, p in named.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0, k
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    gm, gl = seen["g_mu"].cpu().double(), seen["g_lv"].cpu().double()
    masks = hip_masks(model, x, sd)
    r64 = chain(sd, x.cpu(), 2, gm, gl, cls_only=True, masks=masks, want_parts=True)
    r32 = chain(sd, x.cpu(), 2, gm.float(), gl.float(), dtype=F32, cls_only=True, masks=masks)
    keys = [k for k in r64 if k in named]                                   # every stem and transformer-side tensor (the k bias: check_rules)
    assert set(sr.STEM_KEYS) <= set(keys) and len(keys) == 20 + 2 + 2 * 12 + 2 + 4
    check_rules({k: named[k].grad for k in keys}, r64, r32, None, False, "ViTVAE end to end fp32")
    recons2 = model.forward_train(x)[0]                                     # eps drawn with torch.randn
    assert recons2.shape == recons.shape and recons2.requires_grad


def test_train_vit_vae_one_epoch():
    from causal_vae_amd.vit import train_vit_vae
    model = vitvae(seed=4)
    loader = [{"x": vr.vit_inputs(2, 64, 96, seed=11 + i)} for i in range(2)]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    buffers = {k: v.clone() for k, v in model.state_dict().items() if k not in before}
    losses = train_vit_vae(model, loader, opt, DEV, epochs=1, beta=1.0)
    assert len(losses) == 1 and all(l == l and abs(l) < float("inf") for l in losses)
    assert not model.training
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]), k
    for k, v in model.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k                             # running statistics: not updated


def test_causal_vitvae_trains_the_stem_too():
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
    x = vr.vit_inputs(B, 64, 96, seed=10).to(DEV)
    m, t = torch.randn(B, model.m_dim, generator=gen).to(DEV), torch.randn(B, model.t_dim, generator=gen).to(DEV)
    eps = torch.randn(B, model.my_z_dim, generator=gen).to(DEV)
    seen = {}

    def step(**kw):
        state = {k: v.clone() for k, v in model.state_dict().items()}
        params = model.train_adapters(**kw)
        model.zero_grad(set_to_none=True)
        inner = model.backbone.cls_features_with_grad
        model.backbone.cls_features_with_grad = lambda xx: (lambda c: (c.register_hook(lambda g: seen.__setitem__("g_cls", g.clone())), c)[1])(inner(xx))
        out = model.forward_train(x, m, t, eps=eps)
        model.backbone.__dict__.pop("cls_features_with_grad", None)
        total_loss(*loss_function(out[0], x, out[1], m, *out[2:])).backward()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        model.load_state_dict(state)
        return params, grads

    base_params, base = step(decoder=True, transformer=True)
    params, grads = step(decoder=True, transformer=True, stem=True)
    assert len(params) == len(base_params) + 20 and len({id(p) for p in params}) == len(params)
    assert not any(k.startswith("backbone.stem.") for k in base)
    for k, g in base.items():                                               # everything else: the same bits as with a frozen stem
        assert torch.equal(grads[k], g), k
    sd = {k: v.detach().cpu() for k, v in model.backbone.state_dict().items()}
    g_cls = seen["g_cls"].detach().cpu().double()
    masks = hip_masks(model.backbone, x, sd)
    r64 = chain(sd, x.cpu(), 2, g_cls=g_cls, cls_only=True, masks=masks)
    r32 = chain(sd, x.cpu(), 2, g_cls=g_cls.float(), dtype=F32, cls_only=True, masks=masks)
    got = {k: grads["backbone." + k] for k in sr.STEM_KEYS}
    check_rules(got, r64, r32, None, False, "CausalViTVAE stem fp32")
