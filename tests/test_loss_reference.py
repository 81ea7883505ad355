"""csrc/losses.hip (scalar losses, BatchNorm1d and its rank-spanning split form, fused Adam, gradient clipping) through the raw C ABI against the float64
references of oracle/loss64.py: ONE launch and ONE comparison per case, with elementwise bounds derived there from the reduction structure
(C sqrt(K) U sum |terms|, C = 4, U = 2^-24, the measured ulp errors of the fp32 elementary functions, BatchNorm's 1 / sqrt(var + eps) amplification).
tests/test_loss_reference_cpu.py shows that the bounds are neither loose nor wrong, and holds the entry points' argument checks to include/cvae_hip.h.

The sizes are the smallest that cross each seam (RED_BLOCK 256, RED_MAX_BLOCKS 1024, the 256-block cap of reparam_kld / gauss_nll / the row losses,
latent_head's 4 x 1024 pass, ADAM_MULTI_SPAN 1024, SQM_MAX_TENSORS = ADAM_MAX_TENSORS = 64):
  sse / sum / sqnorm / bce   n = 1, 3, 4, 5, 1023, 1024, 1025, 2^20 + 3075 (second grid-stride trip plus tail) x {full scratch, NULL, one float short of the
                             grid} x {16-byte aligned, a view offset by one float: scalar path}; *out pre-filled with 3.25 (accumulate); sse / bce gradients
  reparam_kld / gauss_nll    n = 65536 + 300 and 1; z only / kld only / both; gradients with dz / gkld / gout absent
  wmse_sparsity              n = 262144 + 5, n_pos = n and 3 n, positive weight inside (1, 50) and on either clamp, two-row finish; g_recon / g_sp NULL
  latent_head                B x Z = 1x1, 1023x1, 1x1024, 41x25, 4095x1, 64x64, 17x241, 9001x1; one and two samples; *kld pre-filled (assigned, not added)
  softmax_ce / uniform_kl    C = 1, 2, 10, 63, 64 x B = 1, 37, 1061; logits of scale 30; targets 0 and C - 1; gout NULL and given
  BatchNorm1d                B = 2, 63, 64, 65, 129 x F = 1, 3, 64, 257; affine and running statistics given / NULL; eval; a zero-variance feature; the split
                             form on one device as 2 and 3 "ranks" against the float64 BatchNorm of the whole batch
  Adam                       cvae_adam_multi over 67 tensors (sizes 1, 1023, 1024, 1025, 4097 as a view offset by one float between canaries, 0, 7, and 60 small
                             ones: two table launches), host corrections and the device step counter, with and without a gradient scale, steps 1, 2, 3 and the
                             counter set to 1000 and 100000; cvae_adam_step at n = 5, 4099, aligned and offset
  sqnorm_multi               the same list with scratch for count + 1, 70 and all blocks; then clip_coef on both sides of max_norm, and scale
  weighted_sum (1 and 8 terms, g NULL and given), combine3, multi_copy, counter_add
Every family also runs STRUCTURED cases: small-integer inputs whose sums are exact in fp32, so the result must be bit-exact and a wrong index or a lost slot
is named, not bounded.  Every reduction is launched twice on the same inputs and must give the same bits (the promise of the kernel file's header).

Measured on the MI355X, max |got - ref| / err per family (the CPU fp32 stand-in of tests/test_loss_reference_cpu.py in brackets):
  sse / sum / sqnorm     0.0001 - 0.21 (n >= 1023: <= 0.02) [0.0001 - 0.21];  bce 0.0002 - 0.31 [0.0002 - 0.23];  gradients sse 0.14 - 0.40 [0.12 - 0.40], bce 0.14 - 0.46 [0.07 - 0.54]
  reparam_kld            kld 0.0000 - 0.04, z 0.11 - 0.97 [0.97];  gradients 0.05 - 0.90;  gauss_nll 0.11 - 0.44 [0.49]
  wmse_sparsity          sums 0.0002 - 0.001, dr 0.24 - 0.49 [0.24 - 0.49], the same inside (1, 50) and on either clamp
  latent_head            0.12 - 0.93 [0.12 - 0.93];  gradient 0.05 - 0.97
  softmax_ce             0.0000 (C = 1) - 0.77 [0.08 - 0.77];  uniform_kl 0.0000 (C = 1) - 0.47 [0.02 - 0.32]
  BatchNorm1d            train 0.012 - 0.45 [0.04 - 0.31];  eval 0.09 - 0.48 [0.03 - 0.48];  split form 0.009 - 0.44
  Adam                   cvae_adam_multi t = 1, 2, 3: 0.47 - 0.93 [0.53 - 0.83];  t = 1000, 100000: 0.96 [0.98 - 0.99];  cvae_adam_step 0.62 - 0.98
  sqnorm_multi           0.0001 - 0.002 [0.0002];  clip_coef <= 0.25 [0.11];  scale 0.99 [0.98];  weighted_sum <= 0.54 [0.54];  combine3 <= 0.06 [0.02]
No ratio is above 1, and no case of this file found a wrong result in csrc/losses.hip (the two findings are in the argument checks: see
tests/test_loss_reference_cpu.py).  Far below 1, as expected and not a sign of a loose bound per element: every long SUM (0.0001 - 0.02 from n = 1023 up).  The rule
C sqrt(K) U sum |terms| allows a random walk over K roundings, while the kernels add at most ~8 terms per thread and then a tree of depth ~20, so their
error is that of ~30 roundings whatever K is; the CPU stand-in (pairwise sums) sits as low.  What a sum's bound still rejects is shown in the CPU file: one
element of 1025, a tail of 3, one block slot of 1024.  The results with one or two roundings per element (z, scale, the Adam state) sit just under 1 by
construction: half an ulp of the stored value is nearly the whole bound and some element reaches it.
"""
import ctypes as C
import functools

import pytest
import torch

from causal_vae_amd import _lib as L
from oracle import loss64 as l64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
CANARY = -777.25
PRE = 3.25
BIG = (1 << 20) + 3075
RED_BLOCK, RED_MAX_BLOCKS = 256, 1024


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_KEEP = []                       # a c_void_p does not keep its tensor alive: every device copy lives until its test ends


def dev(t):
    if t is None:
        return None
    _KEEP.append(t.to(DEV).contiguous())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    _KEEP.clear()


def rnd(seed, *shape):
    return torch.randn(*shape, generator=l64.gen(seed))


def scalar(v):
    return dev(torch.tensor(float(v), dtype=F32))


def call(name, *args):
    rc = getattr(L.lib, name)(*args, None)
    assert rc == 0, f"{name}: {L.strerror(rc)}"
    torch.cuda.synchronize()


def offset_view(t, lead=1):
    """a copy of t as a view that starts `lead` floats into a canary-filled buffer (4-byte aligned only): (buffer, view)"""
    buf = torch.full((t.numel() + lead + 7,), CANARY, dtype=F32, device=DEV)
    view = buf[lead:lead + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == 4 * lead % 16
    return buf, view


def canaries_intact(buf, n, lead=1):
    return bool((buf[:lead] == CANARY).all()) and bool((buf[lead + n:] == CANARY).all())


def report(family, got, ref, err, keys=None):
    keys = keys or list(got.keys())
    worst = max(l64.max_ratio(got[k], ref[k], err[k]) for k in keys)
    print(f"RATIO {family} {worst:.4f}")
    bad = l64.compare(got, ref, err, keys)
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def scratch():
    return torch.empty(L.lib.cvae_reduce_workspace_bytes() // 4, dtype=F32, device=DEV)


def ws_args(mode, grid, nout=1):
    """(workspace, bytes) for a reduction whose full grid is `grid` blocks: all of it, none, or one float short of grid x nout"""
    if mode == "null":
        return None, 0
    return ptr(scratch()), (scratch().numel() * 4 if mode == "full" else (grid * nout - 1) * 4)


def grid_of(items, cap=RED_MAX_BLOCKS):
    return max(1, min((items + RED_BLOCK - 1) // RED_BLOCK, cap))


def twice(launch, nout=1):
    """run a reduction twice into fresh pre-filled outputs: the same bits both times; returns the output"""
    outs = []
    for _ in range(2):
        out = torch.full((nout,), PRE, dtype=F32, device=DEV)
        launch(out)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]), "two runs on the same inputs gave different bits"
    return outs[0] if nout > 1 else outs[0][0]


# ------------------------------------------------------------------------------------------------ sse / sum / sqnorm / bce
RED_N = [1, 3, 4, 5, 1023, 1024, 1025, BIG]
RED_FN = {"sse": "cvae_sse_fwd", "sum": "cvae_sum_fwd", "sqnorm": "cvae_sqnorm", "bce": "cvae_bce_fwd"}


@functools.lru_cache(maxsize=None)
def red_case(kind, n):
    a, b = l64.bce_inputs(n, n) if kind == "bce" else (rnd(n, n), rnd(n + 1, n))
    return a, b, l64.reduce2(kind, a, b, prefill=PRE)


def red_launch(kind, a, b, n, mode):
    ws, wsb = ws_args(mode, grid_of((n + 3) // 4))
    if kind in ("sum", "sqnorm"):
        return lambda out: call(RED_FN[kind], ptr(a), ptr(out), n, ws, wsb)
    return lambda out: call(RED_FN[kind], ptr(a), ptr(b), ptr(out), n, ws, wsb)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("mode", ["full", "null", "short"])
@pytest.mark.parametrize("n", RED_N)
@pytest.mark.parametrize("kind", list(RED_FN))
def test_reduce2(kind, n, mode, aligned):
    a, b, (ref, err) = red_case(kind, n)
    da, db = (dev(a), dev(b)) if aligned else (offset_view(a)[1], dev(b))
    out = twice(red_launch(kind, da, db, n, mode))
    report(f"{kind}", dict(out=out), ref, err)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("mode", ["full", "null", "short"])
@pytest.mark.parametrize("n", [5, 1025, BIG])
@pytest.mark.parametrize("kind", ["sse", "sum", "sqnorm"])
def test_reduce2_structured_exact(kind, n, mode, aligned):
    """integers in [-3, 3]: every partial sum is an integer below 2^24, so the result is exact whatever the order; with the 2.0 *out held before"""
    i = torch.arange(n)
    a, b = ((i * 3 + i // 1024) % 7 - 3).float(), ((i * 2 + i // 4096) % 3 - 1).float()
    want = {"sse": ((a - b).double() ** 2).sum(), "sum": a.double().sum(), "sqnorm": (a.double() ** 2).sum()}[kind] + 2.0
    da = dev(a) if aligned else offset_view(a)[1]
    out = torch.full((1,), 2.0, dtype=F32, device=DEV)
    red_launch(kind, da, dev(b), n, mode)(out)
    assert float(out[0]) == float(want), f"{kind} n={n}: got {float(out[0])} want {float(want)} (a lost block of 1024 elements changes it by ~{4 * 1024})"


@pytest.mark.parametrize("n", [5, 4099])
def test_sse_bce_gradients(n):
    a, b = rnd(1, n), rnd(2, n)
    for gout, sc in ((None, 1.0), (scalar(0.7), 0.25)):
        da = torch.full((n,), CANARY, dtype=F32, device=DEV)
        call("cvae_sse_bwd", ptr(dev(a)), ptr(dev(b)), ptr(gout), sc, ptr(da), n)
        report("sse_bwd", dict(da=da), *l64.sse_bwd(a, b, gout, sc))
    p, x = l64.bce_inputs(n, n)
    for gout in (None, scalar(-1.3)):
        dp = torch.full((n,), CANARY, dtype=F32, device=DEV)
        call("cvae_bce_bwd", ptr(dev(p)), ptr(dev(x)), ptr(gout), ptr(dp), n)
        report("bce_bwd", dict(dp=dp), *l64.bce_bwd(p, x, gout))


# ------------------------------------------------------------------------------------------------ reparameterise + KLD, Gaussian NLL
SCAN_N = [65536 + 300, 1]


@functools.lru_cache(maxsize=None)
def latent_case(n):
    return rnd(1, n), 0.5 * rnd(2, n), rnd(3, n), rnd(4, n), rnd(5, n)


@pytest.mark.parametrize("mode", ["full", "null", "short"])
@pytest.mark.parametrize("outs", ["z", "kld", "both"])
@pytest.mark.parametrize("n", SCAN_N)
def test_reparam_kld_fwd(n, outs, mode):
    mu, lv, eps, _dz, _m = latent_case(n)
    ref, err = l64.reparam_kld(mu, lv, eps, prefill=PRE)
    ws, wsb = ws_args(mode, grid_of(n, 256))
    dmu, dlv, deps = dev(mu), dev(lv), dev(eps)
    z = torch.full((n,), CANARY, dtype=F32, device=DEV) if outs != "kld" else None
    got = {}
    if outs == "z":
        call("cvae_reparam_kld_fwd", ptr(dmu), ptr(dlv), ptr(deps), ptr(z), None, n, ws, wsb)
    else:
        got["kld"] = twice(lambda out: call("cvae_reparam_kld_fwd", ptr(dmu), ptr(dlv), ptr(deps) if z is not None else None, ptr(z), ptr(out), n, ws, wsb))
    if z is not None:
        got["z"] = z
    report("reparam_kld", got, ref, err)


@pytest.mark.parametrize("with_dz,with_gk", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("n", SCAN_N)
def test_reparam_kld_bwd(n, with_dz, with_gk):
    mu, lv, eps, dz, _m = latent_case(n)
    gk = scalar(0.8) if with_gk else None
    ref, err = l64.reparam_kld(mu, lv, eps, dz=dz if with_dz else None, gkld=gk, gk_scale=0.5)
    dmu, dlv = (torch.full((n,), CANARY, dtype=F32, device=DEV) for _ in range(2))
    call("cvae_reparam_kld_bwd", ptr(dev(dz)) if with_dz else None, ptr(gk), 0.5, ptr(dev(mu)), ptr(dev(lv)), ptr(dev(eps)) if with_dz else None, ptr(dmu), ptr(dlv), n)
    report("reparam_kld_bwd", dict(dmu=dmu, dlogvar=dlv), ref, err)


@pytest.mark.parametrize("mode", ["full", "null", "short"])
@pytest.mark.parametrize("n", SCAN_N)
def test_gauss_nll(n, mode):
    mu, lv, _eps, _dz, m = latent_case(n)
    ws, wsb = ws_args(mode, grid_of(n, 256))
    dm, dmu_, dlv_ = dev(m), dev(mu), dev(lv)
    out = twice(lambda o: call("cvae_gauss_nll_fwd", ptr(dm), ptr(dmu_), ptr(dlv_), ptr(o), n, ws, wsb))
    for gout in (None, scalar(1.7)):
        ref, err = l64.gauss_nll(m, mu, lv, prefill=PRE, gout=gout)
        g1, g2 = (torch.full((n,), CANARY, dtype=F32, device=DEV) for _ in range(2))
        call("cvae_gauss_nll_bwd", ptr(dm), ptr(dmu_), ptr(dlv_), ptr(gout), ptr(g1), ptr(g2), n)
        report("gauss_nll", dict(out=out, dmu=g1, dlogvar=g2), ref, err)


# ------------------------------------------------------------------------------------------------ vessel recon terms
WM_N = (1 << 18) + 5


@pytest.mark.parametrize("mode", ["full", "null", "short"])
@pytest.mark.parametrize("kind,npm", [("general", 1), ("general", 3), ("zeros", 1), ("ones", 1), ("sparse", 1)])
def test_wmse_sparsity(kind, npm, mode):
    n, n_pos = WM_N, WM_N * npm
    r, x = l64.vessel_inputs(7, n, kind)
    dr_, dx_ = dev(r), dev(x)
    sum_x = torch.zeros(1, dtype=F32, device=DEV)
    call("cvae_sum_fwd", ptr(dx_), ptr(sum_x), n, ptr(scratch()), scratch().numel() * 4)          # as the header prescribes; exact (integers and few fractions)
    pw, _e, inside = l64.pos_weight(sum_x, n_pos)
    assert inside == (kind == "general") and (inside or float(pw) == (1.0 if kind == "ones" else 50.0))
    ws, wsb = ws_args(mode, grid_of(n), 2)
    out = twice(lambda o: call("cvae_wmse_sparsity_fwd", ptr(dr_), ptr(dx_), ptr(sum_x), ptr(o), n, n_pos, ws, wsb), nout=2)
    for gr, gs in ((None, scalar(-2.0)), (scalar(0.3), None), (scalar(0.3), scalar(-2.0))):
        ref, err = l64.wmse_sparsity(r, x, sum_x, n_pos, prefill=(PRE, PRE), g_recon=gr, g_sp=gs)
        g = torch.full((n,), CANARY, dtype=F32, device=DEV)
        call("cvae_wmse_sparsity_bwd", ptr(dr_), ptr(dx_), ptr(sum_x), ptr(gr), ptr(gs), ptr(g), n, n_pos)
        report(f"wmse_sparsity[{kind}]", dict(out=out, dr=g), ref, err)
    if kind == "zeros":                                      # every r with x < 0.1 counts: out[1] - 3.25 = sum |r|, and the gradient's sign is 0 at r == 0
        assert bool((g[::7] == 0).all())


def test_wmse_sparsity_structured_exact():
    """r, x integers (x binary, all ones: weight exactly 1): both rows exact, and distinct, so a swapped row or a lost slot shows"""
    n = WM_N
    i = torch.arange(n)
    r, x = ((i * 3 + i // 256) % 5 - 2).float(), torch.ones(n)
    x[::3] = 0.0
    sum_x = scalar(float(x.sum())).reshape(1)
    assert float(l64.pos_weight(sum_x, n)[0]) == 1.0
    out = torch.zeros(2, dtype=F32, device=DEV)
    call("cvae_wmse_sparsity_fwd", ptr(dev(r)), ptr(dev(x)), ptr(sum_x), ptr(out), n, n, ptr(scratch()), scratch().numel() * 4)
    assert out.tolist() == [float(((r - x).double() ** 2).sum()), float(r.double().abs()[x < 0.1].sum())]


# ------------------------------------------------------------------------------------------------ latent head
HEAD_SHAPES = [(1, 1), (1023, 1), (1, 1024), (41, 25), (4095, 1), (64, 64), (17, 241), (9001, 1)]


@pytest.mark.parametrize("with_kld", [True, False])
@pytest.mark.parametrize("samples", [1, 2])
@pytest.mark.parametrize("B,Z", HEAD_SHAPES)
def test_latent_head_fwd(B, Z, samples, with_kld):
    h = torch.cat([rnd(6, B, Z), 0.5 * rnd(7, B, Z)], 1)
    e1, e2 = rnd(8, B, Z), (rnd(9, B, Z) if samples == 2 else None)
    ref, err = l64.latent_head(h, e1, e2)
    dh, d1, d2 = dev(h), dev(e1), dev(e2)
    z1 = torch.full((B, Z), CANARY, dtype=F32, device=DEV)
    z2 = torch.full((B, Z), CANARY, dtype=F32, device=DEV) if samples == 2 else None
    klds = []
    for _ in range(2):
        kld = torch.full((1,), PRE, dtype=F32, device=DEV) if with_kld else None
        call("cvae_latent_head_fwd", ptr(dh), ptr(d1), ptr(d2), ptr(z1), ptr(z2), ptr(kld), B, Z)
        klds.append(None if kld is None else kld.cpu())
    got = dict(z1=z1)
    if samples == 2:
        got["z2"] = z2
    if with_kld:
        assert torch.equal(klds[0], klds[1])
        got["kld"] = klds[0][0]                              # assigned: the 3.25 it held is gone (the bound has no room for it)
    report("latent_head", got, ref, err)


@pytest.mark.parametrize("absent", ["none", "dz1", "dz2", "gkld"])
@pytest.mark.parametrize("B,Z", HEAD_SHAPES)
def test_latent_head_bwd(B, Z, absent):
    h = torch.cat([rnd(6, B, Z), 0.5 * rnd(7, B, Z)], 1)
    e1, e2, g1, g2 = rnd(8, B, Z), rnd(9, B, Z), rnd(10, B, Z), rnd(11, B, Z)
    gk = None if absent == "gkld" else scalar(0.6)
    if absent == "dz1":
        g1 = None
    if absent == "dz2":
        g2 = None
    ref, err = l64.latent_head(h, e1, e2, g1, g2, gk)
    out = torch.full((B, 2 * Z), CANARY, dtype=F32, device=DEV)
    call("cvae_latent_head_bwd", ptr(dev(g1)), ptr(dev(g2)), ptr(gk), ptr(dev(h)), ptr(dev(e1)) if g1 is not None else None,
         ptr(dev(e2)) if g2 is not None else None, ptr(out), B, Z)
    report("latent_head_bwd", dict(dh=out), ref, err)


def test_latent_head_structured_exact():
    """mu small integers, logvar 0 (e^0 = 1 exactly): z = mu + eps and kld = 0.5 sum mu^2 exactly, at the size that takes two passes and a ragged one"""
    for B, Z in ((17, 241), (64, 64)):
        i = torch.arange(B * Z).reshape(B, Z)
        mu, eps = ((i * 3 + i // 1024) % 5 - 2).float(), ((i * 7) % 3 - 1).float()
        h = torch.cat([mu, torch.zeros(B, Z)], 1)
        z, kld = torch.full((B, Z), CANARY, dtype=F32, device=DEV), torch.full((1,), PRE, dtype=F32, device=DEV)
        call("cvae_latent_head_fwd", ptr(dev(h)), ptr(dev(eps)), None, ptr(z), None, ptr(kld), B, Z)
        assert torch.equal(z.cpu(), mu + eps) and float(kld) == 0.5 * float((mu.double() ** 2).sum())


# ------------------------------------------------------------------------------------------------ softmax CE / uniform KL
@functools.lru_cache(maxsize=None)
def row_case(B, Cn):
    logits = 30.0 * rnd(B * 100 + Cn, B, Cn)
    target = torch.randint(0, Cn, (B,), generator=l64.gen(B + Cn))
    target[0], target[-1] = 0, Cn - 1
    return logits, target


@pytest.mark.parametrize("mode", ["full", "null"])
@pytest.mark.parametrize("Cn", [1, 2, 10, 63, 64])
@pytest.mark.parametrize("B", [1, 37, 1024 + 37])
def test_row_losses(B, Cn, mode):
    logits, target = row_case(B, Cn)
    dl, dt = dev(logits), dev(target)
    ws, wsb = ws_args(mode, grid_of(B * 64, 256))
    ce = twice(lambda o: call("cvae_softmax_ce_fwd", ptr(dl), ptr(dt), ptr(o), B, Cn, ws, wsb))
    kl = twice(lambda o: call("cvae_uniform_kl_fwd", ptr(dl), ptr(o), B, Cn, ws, wsb))
    for gout in (None, scalar(0.9)):
        g = torch.full((B, Cn), CANARY, dtype=F32, device=DEV)
        call("cvae_softmax_ce_bwd", ptr(dl), ptr(dt), ptr(gout), ptr(g), B, Cn)
        report("softmax_ce", dict(out=ce, dlogits=g), *l64.softmax_ce(logits, target, prefill=PRE, gout=gout))
        g = torch.full((B, Cn), CANARY, dtype=F32, device=DEV)
        call("cvae_uniform_kl_bwd", ptr(dl), ptr(gout), ptr(g), B, Cn)
        report("uniform_kl", dict(out=kl, dlogits=g), *l64.uniform_kl(logits, prefill=PRE, gout=gout))


def test_row_losses_structured_exact():
    """equal logits: softmax is exactly 1 / C for C a power of two, so the CE gradient is (1/C - onehot) / B exactly (B = 2048: a power of two, and a second trip of the 1024 rows a launch holds)"""
    B, Cn = 2048, 64
    target = (torch.arange(B) * 5) % Cn
    g = torch.full((B, Cn), CANARY, dtype=F32, device=DEV)
    call("cvae_softmax_ce_bwd", ptr(dev(torch.full((B, Cn), 7.0))), ptr(dev(target)), None, ptr(g), B, Cn)
    want = (torch.full((B, Cn), 1.0 / Cn) - torch.nn.functional.one_hot(target, Cn).float()) / B
    assert torch.equal(g.cpu(), want)


# ------------------------------------------------------------------------------------------------ BatchNorm1d
MOM, BN_EPS = 0.1, 1e-5
BN_B, BN_F = [2, 63, 64, 65, 129], [1, 3, 64, 257]


@functools.lru_cache(maxsize=None)
def bn_case(B, Fn):
    s = B * 1000 + Fn
    x = 1.5 + 2.0 * rnd(s, B, Fn)
    if Fn > 1:
        x[:, 0] = 1.5                                        # variance exactly 0
    return dict(x=x, w=1.0 + 0.5 * rnd(s + 1, Fn), b=rnd(s + 2, Fn), dy=rnd(s + 3, B, Fn), rm=0.1 * rnd(s + 4, Fn), rv=1.0 + torch.rand(Fn, generator=l64.gen(s + 5)))


def new(*shape):
    return torch.full(shape, CANARY, dtype=F32, device=DEV)


@pytest.mark.parametrize("affine,running", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("Fn", BN_F)
@pytest.mark.parametrize("B", BN_B)
def test_bn1d_train(B, Fn, affine, running):
    c = bn_case(B, Fn)
    w, b = (c["w"], c["b"]) if affine else (None, None)
    rm, rv = (c["rm"], c["rv"]) if running else (None, None)
    ref, err = l64.bn1d(c["x"], w, b, c["dy"], rm, rv, MOM, BN_EPS)
    x, dy, dw_, db_, drm, drv = dev(c["x"]), dev(c["dy"]), dev(w), dev(b), dev(rm), dev(rv)
    y, sm, sr, dx, gw, gb = new(B, Fn), new(Fn), new(Fn), new(B, Fn), new(Fn), new(Fn)
    call("cvae_bn1d_train_fwd", ptr(x), ptr(dw_), ptr(db_), ptr(y), ptr(sm), ptr(sr), ptr(drm), ptr(drv), B, Fn, MOM, BN_EPS)
    call("cvae_bn1d_train_bwd", ptr(dy), ptr(x), ptr(dw_), ptr(sm), ptr(sr), ptr(dx), ptr(gw), ptr(gb), B, Fn)
    y2, sm2, sr2 = new(B, Fn), new(Fn), new(Fn)                 # the same bits on a second run (running statistics left alone this time)
    call("cvae_bn1d_train_fwd", ptr(x), ptr(dw_), ptr(db_), ptr(y2), ptr(sm2), ptr(sr2), None, None, B, Fn, MOM, BN_EPS)
    assert torch.equal(y, y2) and torch.equal(sm, sm2) and torch.equal(sr, sr2)
    got = dict(y=y, save_mean=sm, save_rstd=sr, dx=dx, dw=gw, db=gb)
    if running:
        got.update(running_mean=drm, running_var=drv)
    report("bn1d_train", got, ref, err)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("Fn", BN_F)
@pytest.mark.parametrize("B", [1, 65])
def test_bn1d_eval(B, Fn, affine):
    c = bn_case(65, Fn)
    x = c["x"][:B]
    w, b = (c["w"], c["b"]) if affine else (None, None)
    y = new(B, Fn)
    call("cvae_bn1d_eval_fwd", ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(c["rm"])), ptr(dev(c["rv"])), ptr(y), B, Fn, BN_EPS)
    report("bn1d_eval", dict(y=y), *l64.bn1d_eval(x, w, b, c["rm"], c["rv"], BN_EPS))


@pytest.mark.parametrize("Fn", BN_F)
@pytest.mark.parametrize("B,ranks", [(2, 2), (6, 2), (6, 3), (63, 3), (64, 2), (129, 3), (390, 2), (390, 3)])
def test_bn1d_split_form(B, ranks, Fn):
    """the batch cut into equal "ranks" on one device; the rank sums are added with torch (the all-reduce): against the float64 BatchNorm of the whole batch"""
    c = bn_case(B, Fn)
    ref, err = l64.bn1d(c["x"], c["w"], c["b"], c["dy"], c["rm"], c["rv"], MOM, BN_EPS, split=ranks)
    Bl = B // ranks
    inv_n = 1.0 / B
    xs, dys = [dev(c["x"][r * Bl:(r + 1) * Bl]) for r in range(ranks)], [dev(c["dy"][r * Bl:(r + 1) * Bl]) for r in range(ranks)]
    w, b = dev(c["w"]), dev(c["b"])
    parts = [new(Fn) for _ in range(ranks)]
    for r in range(ranks):
        call("cvae_bn1d_stats", ptr(xs[r]), None, 0.0, ptr(parts[r]), Bl, Fn)
    s1 = torch.stack(parts).sum(0)
    for r in range(ranks):
        call("cvae_bn1d_stats", ptr(xs[r]), ptr(s1), inv_n, ptr(parts[r]), Bl, Fn)
    s2 = torch.stack(parts).sum(0)
    ys, dxs, sums = [new(Bl, Fn) for _ in range(ranks)], [new(Bl, Fn) for _ in range(ranks)], [new(2 * Fn) for _ in range(ranks)]
    sm, sr = new(Fn), new(Fn)
    for r in range(ranks):                                   # every rank holds its own copy of the running statistics: each must be right
        rm, rv = dev(c["rm"]), dev(c["rv"])
        call("cvae_bn1d_apply_stats", ptr(xs[r]), ptr(w), ptr(b), ptr(s1), ptr(s2), inv_n, ptr(ys[r]), ptr(sm), ptr(sr), ptr(rm), ptr(rv), Bl, Fn, MOM, BN_EPS)
        call("cvae_bn1d_bwd_sums", ptr(dys[r]), ptr(xs[r]), ptr(sm), ptr(sr), ptr(sums[r]), Bl, Fn)
        report("bn1d_split", dict(save_mean=sm, save_rstd=sr, running_mean=rm, running_var=rv), ref, err)
    total = torch.stack(sums).sum(0)
    for r in range(ranks):
        call("cvae_bn1d_bwd_apply", ptr(dys[r]), ptr(xs[r]), ptr(w), ptr(sm), ptr(sr), ptr(total), inv_n, ptr(dxs[r]), Bl, Fn)
    report("bn1d_split", dict(y=torch.cat(ys), dx=torch.cat(dxs), db=total[:Fn], dw=total[Fn:]), ref, err)


def test_bn1d_structured_exact():
    """x = 3 +- 2 (mean 3, centred sum of squares 4 B: powers of two with B = 64 and 128), dy small integers, the saved statistics given as mean 3, rstd 0.5:
    the batch sums, S1 = sum dy and S2 = sum dy xhat are exact, per feature, so a wrong row or feature index is named"""
    for B, Fn in ((64, 5), (128, 257)):
        i, f = torch.arange(B)[:, None], torch.arange(Fn)[None, :]
        sgn = (((i + f) % 2) * 2 - 1).float()
        x, dy = 3.0 + 2.0 * sgn, ((i * 3 + f * 5) % 7 - 3).float()
        dx_, ddy = dev(x), dev(dy)
        s1, s2, sums, gw, gb, gx = new(Fn), new(Fn), new(2 * Fn), new(Fn), new(Fn), new(B, Fn)
        call("cvae_bn1d_stats", ptr(dx_), None, 0.0, ptr(s1), B, Fn)
        assert torch.equal(s1.cpu(), torch.full((Fn,), 3.0 * B))
        call("cvae_bn1d_stats", ptr(dx_), ptr(s1), 1.0 / B, ptr(s2), B, Fn)
        assert torch.equal(s2.cpu(), torch.full((Fn,), 4.0 * B))
        mean, rstd = dev(torch.full((Fn,), 3.0)), dev(torch.full((Fn,), 0.5))
        call("cvae_bn1d_bwd_sums", ptr(ddy), ptr(dx_), ptr(mean), ptr(rstd), ptr(sums), B, Fn)
        want1, want2 = dy.sum(0), (dy * sgn).sum(0)
        assert torch.equal(sums.cpu(), torch.cat([want1, want2]))
        call("cvae_bn1d_train_bwd", ptr(ddy), ptr(dx_), None, ptr(mean), ptr(rstd), ptr(gx), ptr(gw), ptr(gb), B, Fn)
        assert torch.equal(gb.cpu(), want1) and torch.equal(gw.cpu(), want2)
        assert torch.equal(gx.cpu(), 0.5 * (dy - want1 / B - sgn * (want2 / B)))        # B a power of two: every operation exact


# ------------------------------------------------------------------------------------------------ Adam
LR, B1, B2, AEPS = 1e-3, 0.9, 0.999, 1e-8
SIZES = [1, 1023, 1024, 1025, 4097, 0, 7] + [1 + (k * 37) % 300 for k in range(60)]
OFFSET_AT = 4                                                # the 4097-element tensor: four full spans and a tail, as a view offset by one float


def ptr_table(ts):
    return (C.c_void_p * len(ts))(*[(t.data_ptr() if t.numel() else None) for t in ts])


class AdamList:
    def __init__(self, seed):
        self.cpu = [dict(p=rnd(seed + 4 * i, n), m=torch.zeros(n), v=torch.zeros(n)) for i, n in enumerate(SIZES)]
        self.bufs, self.dev = {}, []
        for i, c in enumerate(self.cpu):
            d = {}
            for k in ("p", "m", "v"):
                if i == OFFSET_AT:
                    self.bufs[k], d[k] = offset_view(c[k])
                else:
                    d[k] = dev(c[k])
            self.dev.append(d)
        self.n = (C.c_int64 * len(SIZES))(*SIZES)

    def grads(self, seed):
        return [rnd(seed + i, n) for i, n in enumerate(SIZES)]

    def step(self, g_dev, t, step_dev, gscale):
        bc1, bc2 = (0.0, 0.0) if step_dev is not None else (1.0 - l64.f32(B1) ** t, 1.0 - l64.f32(B2) ** t)
        call("cvae_adam_multi", ptr_table([d["p"] for d in self.dev]), ptr_table(g_dev), ptr_table([d["m"] for d in self.dev]), ptr_table([d["v"] for d in self.dev]),
             self.n, len(SIZES), LR, B1, B2, AEPS, bc1, bc2, ptr(step_dev), ptr(gscale))
        for k in ("p", "m", "v"):
            assert canaries_intact(self.bufs[k], SIZES[OFFSET_AT]), f"adam_multi wrote outside the offset view of {k}"

    def state(self, i):
        return {k: self.dev[i][k].cpu().clone() for k in ("p", "m", "v")}


@pytest.mark.parametrize("with_gscale", [False, True], ids=["noscale", "gscale"])
@pytest.mark.parametrize("device_step", [False, True], ids=["host_bc", "step_dev"])
def test_adam_multi(device_step, with_gscale):
    al = AdamList(100)
    gs = scalar(0.37) if with_gscale else None
    step_dev = torch.zeros((), dtype=torch.int32, device=DEV) if device_step else None
    hist = []
    for t in (1, 2, 3):                                      # cumulative: after t steps against t steps of the reference from the initial state
        g = al.grads(1000 * t)
        hist.append(g)
        if device_step:
            call("cvae_counter_add", ptr(step_dev), 1)
        al.step([dev(x) for x in g], t, step_dev, gs)
        assert not device_step or int(step_dev) == t
        worst = 0.0
        for i, n in enumerate(SIZES):
            if n:
                c = al.cpu[i]
                ref, err = l64.adam(c["p"], c["m"], c["v"], [h[i] for h in hist], LR, B1, B2, AEPS, device_step=device_step, gscale=gs)
                got = al.state(i)
                bad = l64.compare(got, ref, err)
                assert not bad, f"step {t}, tensor {i} (n = {n}): " + "\n".join(bad)
                worst = max(worst, max(l64.max_ratio(got[k], ref[k], err[k]) for k in "pmv"))
        print(f"RATIO adam_multi[t={t}] {worst:.4f}")
    for t in (1000, 100000):                                 # one step at a far step number, from the state the device holds
        before = [al.state(i) for i in range(len(SIZES))]
        g = al.grads(7 * t)
        if device_step:
            step_dev.fill_(t)
        al.step([dev(x) for x in g], t, step_dev, gs)
        worst = 0.0
        for i, n in enumerate(SIZES):
            if n:
                b = before[i]
                ref, err = l64.adam(b["p"], b["m"], b["v"], [g[i]], LR, B1, B2, AEPS, t0=t, device_step=device_step, gscale=gs)
                got = al.state(i)
                bad = l64.compare(got, ref, err)
                assert not bad, f"step {t}, tensor {i} (n = {n}): " + "\n".join(bad)
                worst = max(worst, max(l64.max_ratio(got[k], ref[k], err[k]) for k in "pmv"))
        print(f"RATIO adam_multi[t={t}] {worst:.4f}")


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [5, 4099])
def test_adam_step(n, aligned):
    p, m, v, g = rnd(1, n), 0.1 * rnd(2, n), 0.01 * rnd(3, n).abs(), rnd(4, n)
    t = 4
    for gs in (None, scalar(0.37)):
        ref, err = l64.adam(p, m, v, [g], LR, B1, B2, AEPS, t0=t, gscale=gs)
        bufs = {k: (offset_view(x) if not aligned else (None, dev(x))) for k, x in dict(p=p, m=m, v=v).items()}
        call("cvae_adam_step", ptr(bufs["p"][1]), ptr(dev(g)), ptr(bufs["m"][1]), ptr(bufs["v"][1]), n, LR, B1, B2, AEPS,
             1.0 - l64.f32(B1) ** t, 1.0 - l64.f32(B2) ** t, ptr(gs))
        report("adam_step", {k: bufs[k][1] for k in "pmv"}, ref, err)
        assert aligned or all(canaries_intact(bufs[k][0], n) for k in "pmv")


def test_adam_multi_structured_exact():
    """b1 = 0, b2 = 0.5, g = +-2, eps = 0, bc1 = 1, bc2 = 0.5, lr = 0.25: m = g, v = 2, sqrt(v) / sqrt(bc2) = 2 up to the rounding of sqrt(2)^2, so p moves by
    0.25 sign(g) to within 1e-6: every element of every tensor, the zero-length entry and the second table included, moved by its OWN gradient's sign"""
    sizes = SIZES
    ps = [dev(torch.zeros(n)) for n in sizes]
    gs = [dev((((torch.arange(n) + i) % 2) * 4 - 2).float()) for i, n in enumerate(sizes)]
    ms, vs = [dev(torch.zeros(n)) for n in sizes], [dev(torch.zeros(n)) for n in sizes]
    call("cvae_adam_multi", ptr_table(ps), ptr_table(gs), ptr_table(ms), ptr_table(vs), (C.c_int64 * len(sizes))(*sizes), len(sizes), 0.25, 0.0, 0.5, 0.0, 1.0, 0.5, None, None)
    for i, n in enumerate(sizes):
        assert torch.equal(ms[i], gs[i]) and bool((vs[i] == 2.0).all()), f"tensor {i}"
        assert bool(((ps[i] + 0.125 * gs[i]).abs() < 1e-6).all()), f"tensor {i} (n = {n}) moved by another tensor's gradient"


# ------------------------------------------------------------------------------------------------ sqnorm_multi, clip_coef, scale
@pytest.mark.parametrize("ws_floats", [len(SIZES) + 1, 70, None], ids=["count+1", "70", "full"])
def test_sqnorm_multi_clip_scale(ws_floats):
    tensors = [rnd(20 + i, n) for i, n in enumerate(SIZES)]
    d = [dev(t) for t in tensors]
    buf, d[OFFSET_AT] = offset_view(tensors[OFFSET_AT])
    ref, err = l64.sqnorm_multi(tensors, prefill=PRE)
    wsb = (scratch().numel() if ws_floats is None else ws_floats) * 4
    n_arr = (C.c_int64 * len(SIZES))(*SIZES)
    out = twice(lambda o: call("cvae_sqnorm_multi", ptr_table(d), n_arr, len(SIZES), ptr(o), ptr(scratch()), wsb))
    report("sqnorm_multi", dict(out=out), ref, err)
    sq = scalar(float(out) - PRE)
    norm = float(sq) ** 0.5
    for max_norm in (0.37 * norm, 2.0 * norm):                # clipped, and not
        coef = new(1)
        call("cvae_clip_coef", ptr(sq), ptr(coef), max_norm)
        cref, cerr = l64.clip_coef(sq, max_norm)
        report("clip_coef", dict(scale=coef[0]), cref, cerr)
        assert (float(coef) == 1.0) == (max_norm > norm)
        g = d[OFFSET_AT].clone()
        gb, gv = offset_view(g)
        call("cvae_scale", ptr(gv), SIZES[OFFSET_AT], ptr(coef))
        report("scale", dict(g=gv), *l64.scale(g, coef[0]))
        assert canaries_intact(gb, SIZES[OFFSET_AT])


@pytest.mark.parametrize("ws_floats", [len(SIZES) + 1, 70, None], ids=["count+1", "70", "full"])
def test_sqnorm_multi_structured_exact(ws_floats):
    """tensor i holds the integer (i % 3) + 1 throughout: the sum is sum_i n_i ((i % 3) + 1)^2 exactly; a tensor lost or read twice changes it"""
    d = [dev(torch.full((n,), float(i % 3 + 1))) for i, n in enumerate(SIZES)]
    out = torch.zeros(1, dtype=F32, device=DEV)
    wsb = (scratch().numel() if ws_floats is None else ws_floats) * 4
    call("cvae_sqnorm_multi", ptr_table(d), (C.c_int64 * len(SIZES))(*SIZES), len(SIZES), ptr(out), ptr(scratch()), wsb)
    assert float(out) == float(sum(n * (i % 3 + 1) ** 2 for i, n in enumerate(SIZES)))


# ------------------------------------------------------------------------------------------------ scalar combinations, copies, counters
@pytest.mark.parametrize("count", [1, 8])
def test_weighted_sum_combine3(count):
    terms = [scalar(float(rnd(40 + i, 1))) for i in range(count)]
    weights = [0.5, 1.0, -2.0, 1e-3, 3.0, 0.1, 7.0, 1.5][:count]
    w_arr = (C.c_float * count)(*weights)
    for g in (None, scalar(0.77)):
        ref, err = l64.weighted_sum(terms, weights, g)
        fwd, bwd = new(count + 2), new(count + 1)
        call("cvae_weighted_sum", ptr_table(terms), w_arr, count, None, ptr(fwd), 0)
        call("cvae_weighted_sum", None, w_arr, count, ptr(g), ptr(bwd), 1)
        report("weighted_sum", dict(fwd=fwd[:count + 1], bwd=bwd[:count]), ref, err)
        assert float(fwd[count + 1]) == CANARY and float(bwd[count]) == CANARY
    o4 = dev(rnd(50 + count, 4))
    ref, err = l64.combine3(o4, 0.1, 1e-4)
    call("cvae_combine3", ptr(o4), 0.1, 1e-4)
    report("combine3", dict(out4=o4), ref, err)


def test_multi_copy_and_counter():
    src = [dev(rnd(60 + i, n)) for i, n in enumerate(SIZES)]
    bufs = [offset_view(torch.zeros(n)) if n else (None, dev(torch.zeros(0))) for n in SIZES]
    call("cvae_multi_copy", ptr_table(src), ptr_table([v for _b, v in bufs]), (C.c_int64 * len(SIZES))(*SIZES), len(SIZES))
    for i, n in enumerate(SIZES):
        if n:
            assert torch.equal(bufs[i][1], src[i]) and canaries_intact(bufs[i][0], n), f"tensor {i}"
    c = torch.full((), 5, dtype=torch.int32, device=DEV)
    call("cvae_counter_add", ptr(c), 3)
    call("cvae_counter_add", ptr(c), -1)
    assert int(c) == 7
