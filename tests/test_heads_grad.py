"""The training-mode heads on the GPU (cvae_mlp_heads_train_fwd / cvae_mlp_heads_bwd, ops.mlp_heads_train, CausalViTVAE.forward_train) against
tests/heads_grad_reference.py: the forward within the element-wise bounds of its docstring, every gradient's distance from the float64 VJP (with the HIP
forward's own masks) at most 4 x the distance of the float32 CPU evaluation of the same restatement (DESIGN §13's rule and margin), the masks, what the
comparison refuses, determinism, absent cotangents, and the wiring of forward_train.

Every comparison prints its figures before it asserts (rel-L2 against float64, HIP and float32 CPU, and their ratio); DESIGN §14 holds the record."""
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import heads_grad_reference as hr  # noqa: E402
import causal_vit_reference as cr  # noqa: E402
from test_causal_vit import strided, within  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
KINDS = ("enc", "dec", "morph", "tiny", "odd")
EXTRA_KINDS = ("one", "bn2")
BATCHES = (2, 8, 17, 33)
MARGIN = 4.0


def ops():
    from causal_vae_amd import ops as o
    return o


class TrainHead:
    """The three served heads and four synthetic ones (tiny: 2 + 3 -> 7 -> 3 | 3 with z, no BatchNorm; odd: 130 -> 129 (BatchNorm) -> 10: widths that cross the
    tiles and the padding; one: a single Linear 7 -> 5 with no panel gradient; bn2: 9 -> 12 (BatchNorm) -> 10 (BatchNorm) -> 6: three forward and three backward
    segments), weights scaled so that the clamps bite on some columns, some hidden values planted as exact zeros."""

    def __init__(self, kind, B, seed=0):
        from causal_vae_amd.vit import AdapterMLP
        g = torch.Generator().manual_seed(300 + seed)
        self.kind, self.B = kind, B
        self.clamp0 = self.clamp1 = self.eps = self.split = None
        self.grad_panels = ()
        torch.manual_seed(5)
        if kind == "morph":
            self.mods = nn.ModuleList([nn.Linear(19, 64), nn.Linear(64, 64), nn.Linear(64, 12), nn.Linear(64, 12)])
            self.layers = [(self.mods[0], None, 0.2), (self.mods[1], None, 0.2), ((self.mods[2], self.mods[3]), None, None)]
            widths, self.split, self.clamp1 = (19,), 12, (-10.0, 10.0)
            with torch.no_grad():
                self.mods[3].weight[::2] *= 150.0
                self.mods[0].weight[5].zero_(), self.mods[0].bias[5].zero_()                 # hidden column 5 of both layers: exact zeros
                self.mods[1].weight[5].zero_(), self.mods[1].bias[5].zero_()
        elif kind == "tiny":
            self.mods = nn.ModuleList([nn.Linear(5, 7), nn.Linear(7, 6)])
            self.layers = [(self.mods[0], None, 0.2), (self.mods[1], None, None)]
            widths, self.split, self.clamp0, self.clamp1 = (2, 3), 3, (-1.0, 1.0), (-0.5, 0.5)
            self.grad_panels = (0, 1)
            with torch.no_grad():
                self.mods[1].weight *= 3.0
                self.mods[0].weight[2].zero_(), self.mods[0].bias[2].zero_()
        elif kind == "one":
            self.mods = nn.ModuleList([nn.Linear(7, 5)])
            self.layers = [(self.mods[0], None, None)]
            widths, self.clamp0 = (7,), (-0.3, 0.3)
        elif kind == "bn2":
            self.mods = nn.ModuleList([nn.Linear(9, 12), nn.BatchNorm1d(12), nn.Linear(12, 10), nn.BatchNorm1d(10), nn.Linear(10, 6)])
            self.layers = [(self.mods[0], self.mods[1], 0.2), (self.mods[2], self.mods[3], 0.2), (self.mods[4], None, None)]
            widths, self.grad_panels, self.clamp0 = (9,), (0,), (-0.3, 0.3)
            with torch.no_grad():
                for bn in (self.mods[1], self.mods[3]):
                    bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=g))
                    bn.bias.copy_(0.1 * torch.randn(bn.num_features, generator=g))
                    bn.weight[3], bn.bias[3] = 0.0, 0.0
        else:
            dims = {"enc": (287, 512, 256), "dec": (140, 256, 512), "odd": (130, 129, 10)}[kind]
            self.mods = AdapterMLP(*dims)
            bn = self.mods[1]
            with torch.no_grad():
                bn.weight.copy_(0.5 + torch.rand(bn.num_features, generator=g))
                bn.bias.copy_(0.1 * torch.randn(bn.num_features, generator=g))
                bn.running_mean.copy_(0.1 * torch.randn(bn.num_features, generator=g))
                bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=g))
                bn.weight[3], bn.bias[3] = 0.0, 0.0                                          # hidden column 3: gamma x^ + beta is an exact zero
            self.layers = self.mods.head_layers()
            if kind == "enc":
                with torch.no_grad():
                    self.mods[3].weight[0:128:3] *= 2000.0
                    self.mods[3].weight[128:256:2] *= 150.0
                widths, self.split, self.clamp0, self.clamp1 = (256, 12, 19), 128, (-100.0, 100.0), (-10.0, 10.0)
            elif kind == "dec":
                widths, self.grad_panels = (12, 128), (1,)
            else:
                widths, self.grad_panels, self.clamp0 = (130,), (0,), (-0.3, 0.3)
        if kind in ("enc", "tiny"):
            self.eps = torch.randn(B, self.split, generator=g)
        self.panels = [torch.randn(B, w, generator=g) for w in widths]
        self.mods.to(DEV).train()
        N = sum(p.weight.shape[0] for p in (self.layers[-1][0] if isinstance(self.layers[-1][0], tuple) else (self.layers[-1][0],)))
        self.N, self.S = N, self.split or N
        self.cot = [torch.randn(B, self.S, generator=g), torch.randn(B, N - self.S, generator=g) if self.S < N else None,
                    torch.randn(B, self.S, generator=g) if self.eps is not None else None]
        self.layers64 = hr.layers_of(self.layers)              # before any forward: the running statistics as they are now
        self.x64 = torch.cat([p.double() for p in self.panels], 1)

    def params(self):
        return [p for p in self.mods.parameters()]

    def run(self, cot=None, grad_panels=None, collect=None):
        """one forward and one backward -> (outputs, {name: gradient})"""
        gp = self.grad_panels if grad_panels is None else grad_panels
        pans = [strided(p, 5 + i).requires_grad_(i in gp) for i, p in enumerate(self.panels)]
        outs = ops().mlp_heads_train(pans, self.layers, split=self.split, clamp0=self.clamp0, clamp1=self.clamp1,
                                     eps=None if self.eps is None else strided(self.eps, 7), collect=collect)
        cot = self.cot if cot is None else cot
        pairs = [(o, c.to(DEV)) for o, c in zip(outs, cot) if o is not None and c is not None]
        ins = self.params() + [pans[i] for i in gp]
        gs = torch.autograd.grad([o for o, _ in pairs], ins, [c for _, c in pairs], allow_unused=True)
        named = {}
        names = [k for k, _ in self.mods.named_parameters()]
        for k, gval in zip(names, gs[:len(names)]):
            named[k] = gval
        for i, gval in zip(gp, gs[len(names):]):
            named[f"panel{i}"] = gval
        return outs, named

    def reference_names(self, ref):
        """the restatement's gradients under the module's parameter names; `<bias>:scale` marks the bias in front of a BatchNorm layer (an exact zero) and
        holds the scale of its rounding bound (heads_grad_reference's docstring)"""
        name = {id(p): k for k, p in self.mods.named_parameters()}
        out = {}
        for l, (lin, bn, _slope) in enumerate(self.layers):
            off = 0
            for p in (lin if isinstance(lin, tuple) else (lin,)):
                n = p.weight.shape[0]
                out[name[id(p.weight)]], out[name[id(p.bias)]] = ref[f"dW{l}"][off:off + n], ref[f"db{l}"][off:off + n]
                off += n
            if bn is not None:
                out[name[id(bn.weight)]], out[name[id(bn.bias)]] = ref[f"dgamma{l}"], ref[f"dbeta{l}"]
                out[name[id(lin.bias)] + ":scale"] = ref[f"db_scale{l}"]
        k0 = 0
        for i, p in enumerate(self.panels):
            out[f"panel{i}"] = ref["dx"][:, k0:k0 + p.shape[1]]
            k0 += p.shape[1]
        return out

    def masks_of(self, collect):
        leaky = {l: collect[f"pre{l}"].cpu() > 0 for l in range(len(self.layers) - 1)}
        pc = collect["preclamp"].cpu()
        cm = torch.ones_like(pc, dtype=torch.bool)
        if self.clamp0 is not None:
            cm[:, :self.S] = (pc[:, :self.S] >= self.clamp0[0]) & (pc[:, :self.S] <= self.clamp0[1])
        if self.clamp1 is not None:
            cm[:, self.S:] = (pc[:, self.S:] >= self.clamp1[0]) & (pc[:, self.S:] <= self.clamp1[1])
        return dict(leaky=leaky, clamp=cm)

    def restate(self, masks, dtype, cot=None, **kw):
        ref = hr.head_grads(self.x64, self.layers64, self.S, self.clamp0, self.clamp1, None if self.eps is None else self.eps.double(),
                            self.cot if cot is None else cot, masks, dtype, **kw)
        return self.reference_names(ref)


def distance(a, b):
    return float((a.detach().cpu().double() - b.double()).norm())


def compare(h, got, masks, what, **kw):
    """rule 2: ||HIP - float64|| <= MARGIN ||float32 CPU - float64|| for every gradient (the same denominator on both sides of the rel-L2 ratio).  The bias
    in front of a BatchNorm layer is zero in exact arithmetic: it is held to the element-wise rounding bound of tests/heads_grad_reference.py instead.
    Returns the worst ratio; with kw (a wrong restatement as the reference) the caller asserts the opposite."""
    g64, g32 = h.restate(masks, F64, **kw), h.restate(masks, F32)
    true64 = h.restate(masks, F64) if kw else g64
    worst = 0.0
    for k, v in got.items():
        if k + ":scale" in true64:                 # zero in exact arithmetic: an absolute rounding bound instead of a ratio of two noises
            bound = ((2 * h.B + 16) * hr.U32 * true64[k + ":scale"]).clamp_min(1e-300)        # the planted gamma = 0 column: 0 <= 0
            r = float((v.detach().cpu().double().abs() / bound).max())
            print(f"{what} {k}: max |HIP| / rounding bound of an exact zero = {r:.4f}")
            assert r <= 1.0, (what, k, r)
            continue
        d_hip, d_32, n = distance(v, g64[k]), distance(g32[k], true64[k]), float(true64[k].norm())
        assert v.shape == g64[k].shape, (k, v.shape, g64[k].shape)
        ratio = d_hip / max(d_32, 1e-300)
        print(f"{what} {k}: rel-L2 vs float64 HIP {d_hip / max(n, 1e-300):.3e}  float32 CPU {d_32 / max(n, 1e-300):.3e}  ratio {ratio:.2f}")
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_backward_against_float64(kind, B):
    check_head(kind, B)


@pytest.mark.parametrize("B", (8, 17, 33))
@pytest.mark.parametrize("kind", EXTRA_KINDS)
def test_segment_loops_against_float64(kind, B):
    """A one-layer head without a panel gradient, and two BatchNorm layers in a row: every segment loop of the two entries runs.  B = 2 is left to the
    issue's five heads: behind two-row statistics x^ is +-1 and every gradient below is rounding scaled by eps / var, which says nothing about the loops."""
    check_head(kind, B)


def check_head(kind, B):
    h = TrainHead(kind, B)
    collect = {}
    (first, second, z), got = h.run(collect=collect)
    fw = hr.head_forward(h.x64, h.layers64, h.S, h.clamp0, h.clamp1, None if h.eps is None else h.eps.double(), want_bound=True)
    bd = fw["bound"]
    # 1. forward
    within(first, fw["first"], bd["first"], f"{kind} B{B} first")
    within(collect["preclamp"], fw["preclamp"], bd["preclamp"], f"{kind} B{B} preclamp")
    if second is not None:
        within(second, fw["second"], bd["second"], f"{kind} B{B} second")
    if z is not None:
        mu, lv = first.detach().cpu().double(), second.detach().cpu().double()
        zero = torch.zeros_like(mu)
        want, ez = cr.reparam_b(mu, zero, lv, zero, h.eps.double())
        within(z, want, ez, f"{kind} B{B} z")
    for c, v in ((h.clamp0, fw["preclamp"][:, :h.S]), (h.clamp1, fw["preclamp"][:, h.S:])):
        if c is not None and B >= 8:
            assert bool(((v > c[1]) | (v < c[0])).any()) and bool(((v > c[0]) & (v < c[1])).any()), (kind, c)
    for l, (_lin, bn, _s) in enumerate(h.layers[:-1]):
        within(collect[f"pre{l}"], fw["pre"][l], bd[f"pre{l}"].clamp_min(1e-300), f"{kind} B{B} pre{l}")
        assert bool((collect[f"pre{l}"] == 0).any()), "the planted exact zeros"
        if bn is not None:
            for name, val in (("mean", collect[f"mean{l}"]), ("rstd", collect[f"rstd{l}"]), ("xhat", collect[f"xhat{l}"]), ("running_mean", bn.running_mean),
                              ("running_var", bn.running_var)):
                within(val, fw[name][l], bd[f"{name}{l}"], f"{kind} B{B} {name}{l}")
            assert int(bn.num_batches_tracked) == fw["nbt"][l] == 1
    # 3. masks: HIP's differ from float64's only within the forward bound of zero / of the clamp edge
    masks, own = h.masks_of(collect), hr.own_masks(fw)
    for l in masks["leaky"]:
        diff = masks["leaky"][l] != own["leaky"][l]
        assert bool((fw["pre"][l].abs()[diff] <= bd[f"pre{l}"][diff]).all()), (kind, l, int(diff.sum()))
    diff = masks["clamp"] != own["clamp"]
    if bool(diff.any()):
        edge = torch.full_like(fw["preclamp"], float("inf"))
        for c, sl in ((h.clamp0, slice(0, h.S)), (h.clamp1, slice(h.S, h.N))):
            if c is not None:
                edge[:, sl] = torch.minimum((fw["preclamp"][:, sl] - c[0]).abs(), (fw["preclamp"][:, sl] - c[1]).abs())
        assert bool((edge[diff] <= bd["preclamp"][diff]).all()), (kind, int(diff.sum()))
    # 2. backward
    assert set(got) == set(k for k, _ in h.mods.named_parameters()) | {f"panel{i}" for i in h.grad_panels}
    worst = compare(h, got, masks, f"{kind} B{B}")
    print(f"{kind} B{B}: worst ratio {worst:.2f} of an allowed {MARGIN}")
    assert worst <= MARGIN, (kind, B, worst)


@pytest.mark.parametrize("kind", ["enc", "morph", "odd"])
def test_what_the_comparison_refuses(kind):
    """4. a wrong slope and a missing clamp mask, taken as the reference of rule 2, are refused.  running_var is no gradient, so rule 2 cannot see it: the
    biased-running_var restatement is refused by the forward's element-wise bound instead."""
    h = TrainHead(kind, 17)
    collect = {}
    _outs, got = h.run(collect=collect)
    masks = h.masks_of(collect)
    assert compare(h, got, masks, f"{kind} wrong slope", slope_override=0.01) > MARGIN
    assert compare(h, got, masks, f"{kind} no clamp mask", use_clamp_mask=False) > MARGIN
    if kind != "morph":
        fw = hr.head_forward(h.x64, h.layers64, h.S, h.clamp0, h.clamp1, None if h.eps is None else h.eps.double(), want_bound=True, biased_running=True)
        bn = h.layers[0][1]
        assert bool(((bn.running_var.cpu().double() - fw["running_var"][0]).abs() > fw["bound"]["running_var0"]).any())


@pytest.mark.parametrize("kind", KINDS + EXTRA_KINDS)
def test_two_runs_give_identical_bits_and_absent_cotangents_are_zeros(kind):
    """5. determinism; 6. a None cotangent equals a zero one, and a panel without a gradient changes no other result's bits"""
    h = TrainHead(kind, 33)
    o1, g1 = h.run()
    o2, g2 = h.run()
    assert all(torch.equal(g1[k], g2[k]) for k in g1) and all(a is None or torch.equal(a, b) for a, b in zip(o1, o2))
    for drop in (0, 1, 2):
        if h.cot[drop] is None:
            continue
        none = [None if i == drop else c for i, c in enumerate(h.cot)]
        if all(c is None for c in none):
            continue
        zero = [torch.zeros_like(c) if i == drop else c for i, c in enumerate(h.cot)]
        _o, ga = h.run(cot=none)
        _o, gb = h.run(cot=zero)
        assert all(torch.equal(ga[k], gb[k]) for k in ga), (kind, drop)
    if kind in ("morph", "tiny", "one"):                             # no BatchNorm: the training forward is the eval computation, bit for bit
        with torch.no_grad():
            ev = ops().mlp_heads([strided(p, 5 + i) for i, p in enumerate(h.panels)], h.layers, split=h.split, clamp0=h.clamp0, clamp1=h.clamp1,
                                 eps=None if h.eps is None else strided(h.eps, 7))
        assert all(a is None or torch.equal(a, b) for a, b in zip(ev, o1))
    if h.grad_panels:
        _o, g3 = h.run(grad_panels=())
        assert set(g3) == set(g1) - {f"panel{i}" for i in h.grad_panels} and all(torch.equal(g3[k], g1[k]) for k in g3)


# ---- 7 / 8: CausalViTVAE.forward_train ------------------------------------------------------------------------------------------------------------------
def small_model(dtype, seed=0):
    from causal_vae_amd.vit import CausalViTVAE
    torch.manual_seed(20 + seed)
    model = CausalViTVAE(img_size=(64, 96), depth=1)
    cr.randomize_head_bn(model, 5)
    model.to(DEV).set_compute_dtype(dtype)
    x, m, t, eps = cr.causal_inputs(3, 64, 96, 77)
    return model, x.to(DEV), m.to(DEV), t.to(DEV), eps.to(DEV)


def head_grads_of(model):
    return {k: p.grad.clone() for k, p in model.named_parameters() if not k.startswith("backbone.")}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_train_wiring(dtype):
    from causal_vae_amd.vessel.train import loss_function, total_loss
    model, x, m, t, eps = small_model(dtype)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    params = model.train_adapters()
    model.train()
    out = model.forward_train(x, m, t, eps)
    total_loss(*loss_function(out[0], x, out[1], m, *out[2:])).backward()
    got = head_grads_of(model)
    assert all(p.grad is None for p in model.backbone.parameters()) and all(p.grad is not None for p in params)
    # the same pieces called explicitly, on the same starting state
    model.load_state_dict(state)
    model.zero_grad(set_to_none=True)
    o = ops()
    cls_out = model.backbone.cls_features(x)
    ce, cd = {}, {}
    mu, logvar, z = o.mlp_heads_train([cls_out, m, t], model.enc_adapter.head_layers(), split=128, clamp0=(-100.0, 100.0), clamp1=(-10.0, 10.0), eps=eps,
                                      collect=ce)
    m_mu, m_logvar, _z = o.mlp_heads_train([t], model.morph_layers(), clamp1=(-10.0, 10.0))
    zd = z.detach().requires_grad_(True)
    z_vit, _s, _z = o.mlp_heads_train([m, zd], model.dec_adapter.head_layers(), collect=cd)
    recon = model.backbone.decode(z_vit.detach()).requires_grad_(True)
    assert torch.equal(recon, out[0].detach())
    mud, lvd = mu.detach().requires_grad_(True), logvar.detach().requires_grad_(True)
    total_loss(*loss_function(recon, x, m_mu, m, mud, lvd, m_mu, m_logvar)).backward()            # morph predictor, and the cotangents of recon, mu, logvar
    g_zvit = model.backbone.decode_vjp(z_vit.detach(), recon.grad)
    z_vit.backward(g_zvit)                                                                        # dec_adapter, and dz
    g_mu, g_lv = mud.grad, lvd.grad
    torch.autograd.backward([mu, logvar, z], [g_mu, g_lv, zd.grad])                               # enc_adapter: one call with all three cotangents
    want = head_grads_of(model)
    assert set(want) == set(got)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    # the heads chain on the HIP cls_out and the HIP decode_vjp cotangent against float64: rule 2 for every head parameter
    d = lambda v: v.detach().cpu().double()
    sd = {k: d(v) for k, v in state.items()}
    enc64, dec64 = hr.layers_of(model.enc_adapter.head_layers()), hr.layers_of(model.dec_adapter.head_layers())
    for lay, pre in ((enc64, "enc_adapter"), (dec64, "dec_adapter")):       # the starting running statistics (gradients do not read them)
        lay[0][2].update(running_mean=sd[pre + ".1.running_mean"], running_var=sd[pre + ".1.running_var"])
    masks_e = dict(leaky={0: ce["pre0"].cpu() > 0}, clamp=torch.cat([(ce["preclamp"][:, :128].abs() <= 100), (ce["preclamp"][:, 128:].abs() <= 10)], 1).cpu())
    masks_d = dict(leaky={0: cd["pre0"].cpu() > 0}, clamp=torch.ones(3, 512, dtype=torch.bool))
    res = {}
    for dt in (F64, F32):
        fe = hr.head_forward(torch.cat([d(cls_out), d(m), d(t)], 1), enc64, 128, (-100.0, 100.0), (-10.0, 10.0), d(eps), dt)
        fd = hr.head_forward(torch.cat([d(m).to(dt), fe["z"]], 1), dec64, 512, dtype=dt)
        gd = hr.head_vjp(fd, dec64, (d(g_zvit), None, None), masks_d)
        ge = hr.head_vjp(fe, enc64, (d(g_mu), d(g_lv), gd["dx"][:, 12:]), masks_e)
        res[dt] = {"enc_adapter.0.weight": ge["dW0"], "enc_adapter.0.bias": ge["db0"], "enc_adapter.1.weight": ge["dgamma0"],
                   "enc_adapter.1.bias": ge["dbeta0"], "enc_adapter.3.weight": ge["dW1"], "enc_adapter.3.bias": ge["db1"],
                   "dec_adapter.0.weight": gd["dW0"], "dec_adapter.0.bias": gd["db0"], "dec_adapter.1.weight": gd["dgamma0"],
                   "dec_adapter.1.bias": gd["dbeta0"], "dec_adapter.3.weight": gd["dW1"], "dec_adapter.3.bias": gd["db1"],
                   "enc_adapter.0.bias:scale": ge["db_scale0"], "dec_adapter.0.bias:scale": gd["db_scale0"]}
    worst = 0.0
    for k, v64 in res[F64].items():
        if k.endswith(":scale"):
            continue
        if k + ":scale" in res[F64]:               # the bias in front of a BatchNorm layer: an exact zero, held to its rounding bound
            r = float((got[k].cpu().double().abs() / ((2 * 3 + 16) * hr.U32 * res[F64][k + ":scale"]).clamp_min(1e-300)).max())
            print(f"chain {k}: max |HIP| / rounding bound of an exact zero = {r:.4f}")
            assert r <= 1.0, (k, r)
            continue
        d_hip, d_32, n = distance(got[k], v64), distance(res[F32][k], v64), float(v64.norm())
        print(f"chain {k}: rel-L2 vs float64 HIP {d_hip / max(n, 1e-300):.3e}  float32 CPU {d_32 / max(n, 1e-300):.3e}  ratio {d_hip / max(d_32, 1e-300):.2f}")
        worst = max(worst, d_hip / max(d_32, 1e-300))
    assert worst <= MARGIN, worst


def test_one_adam_step_moves_the_heads_only():
    from causal_vae_amd.vessel.train import loss_function, total_loss
    model, x, m, t, eps = small_model(torch.float32, seed=1)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.train_adapters(), lr=1e-4)
    out = model.forward_train(x, m, t, eps)
    terms = loss_function(out[0], x, out[1], m, *out[2:])
    total_loss(*terms).backward()
    opt.step()
    after = model.state_dict()
    for k, p in model.named_parameters():
        assert torch.equal(after[k], before[k]) == k.startswith("backbone."), k
    for k in before:
        if k.startswith("backbone."):
            assert torch.equal(after[k], before[k]), k
    for a in ("enc_adapter", "dec_adapter"):
        assert not torch.equal(after[a + ".1.running_mean"], before[a + ".1.running_mean"]) and int(after[a + ".1.num_batches_tracked"]) == 1
    model.eval()
    y = model(x, m, t, eps)
    assert bool(torch.isfinite(y[0]).all())
    model.enc_adapter[1].running_mean.add_(1.0)                          # the eval forward reads the live statistics
    assert not torch.equal(model(x, m, t, eps)[2], y[2])
