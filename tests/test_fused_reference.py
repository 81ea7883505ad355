"""The fused bottleneck (csrc/bottleneck.hip) and the ELBO with the exact-2x resize folded in (csrc/recon_loss.hip) against float64 CPU
references (oracle/fused64.py), at the shapes, batch templates, widths and ABI options the kernels accept — not only the model's.

Every bound is derived in oracle/fused64.py from the reduction structure (C sqrt(K) U (|A| . |B|) per product-sum, carried through the graph;
BatchNorm's 1/sqrt(var + eps) amplification; half a bf16 ulp on bf16 outputs).  The cases' biases are nudged so that no ReLU pre-activation
lies within its bound of zero (asserted on the reference), so every ReLU mask must match exactly."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from causal_vae_amd import _lib as L
from causal_vae_amd import ops
from oracle import fused64 as f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
BN_EPS, MOM = 1e-5, 0.1
BADSHAPE = -1


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def cuda(c):
    return {k: ([p.to(DEV) for p in v] if isinstance(v, list) else v.to(DEV)) for k, v in c.items()}


def reference(c, out, training=True, g_none=False):
    ref, err, pre = f64.bottleneck(c["y_cl"], c["m"], c["t"], c["eps"], c["params"], c["rm"], c["rv"], MOM, BN_EPS, out, c["g_dec"],
                                   None if g_none else c["g_mu"], None if g_none else c["g_logvar"], None if g_none else c["g_mhat"], training=training)
    assert f64.mask_margin(pre) == {k: 0 for k in f64.RELU_PRE}, "a ReLU pre-activation lies within its bound of zero: the case cannot decide a mask"
    if c["y_cl"].dtype == torch.bfloat16:
        for k in ("dec_cl", "dy_cl"):
            err[k] = f64.bf16_out(err[k], ref[k])
    return ref, err


def assert_within(got, ref, err, names=None):
    bad = f64.compare(got, ref, err, names)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the raw C ABI (options ops does not expose)
class Raw:
    """One rank's buffers for cvae_bottleneck_fwd / _bwd (device tensors)."""

    def __init__(self, c, out, sl=slice(None), refused=False):
        self.c, self.out = c, out
        y = c["y_cl"][sl]
        M, D, H, W, Cc = y.shape
        T, HM, DM = c["t"].shape[1], c["params"][8].shape[0], c["m"].shape[1]
        N1, N2, Z = c["params"][0].shape[0], c["params"][2].shape[0], c["params"][4].shape[0]
        self.dims = L.BottleneckDims(M, D, H, W, Cc, *out, DM, T, N1, N2, Z, HM)
        sizes = [C.c_int64() for _ in range(5)]
        assert L.lib.cvae_bottleneck_sizes(C.byref(self.dims), *[C.byref(v) for v in sizes]) == (BADSHAPE if refused else 0)
        K1, K4, n_fwd, n_dzm, n_dx = (v.value for v in sizes)
        if refused:                                          # no sizes from the library: the largest each buffer could need
            F_ = Cc * out[0] * out[1] * out[2]
            K1, K4 = F_ + DM + T, Z + DM
            n_fwd, n_dzm, n_dx = 8 * M * N1, (F_ // 64) * M * K4, 64 * M * F_
        new = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
        self.y, self.m, self.t, self.labels, self.eps = y.contiguous(), c["m"][sl].contiguous(), c["t"][sl].contiguous(), c["labels"][sl].contiguous(), c["eps"][sl].contiguous()
        self.g_dec, self.g_mu, self.g_lv, self.g_mh = (c[k][sl].contiguous() for k in ("g_dec", "g_mu", "g_logvar", "g_mhat"))
        self.xcat, self.partial, self.dzm, self.dx, self.g1 = new(M, K1), new(n_fwd), new(n_dzm), new(n_dx), new(M * (N1 + N2))
        self.saved = dict(h1=new(M, N1), h2=new(M, N2), mu=new(M, Z), logvar=new(M, Z), xhat=new(M, HM), invstd=new(HM), a1n=new(M, HM), a2=new(M, HM),
                          m_hat=new(M, DM), zm=new(M, K4))
        self.dec = torch.empty(M, *out, Cc, dtype=y.dtype, device=DEV)
        self.grads = [torch.full_like(p, float("nan")) for p in c["params"]]
        self.dy = torch.empty_like(self.y)
        self.pstruct = L.BottleneckPtrs18(*[ptr(p) for p in c["params"]])
        self.gstruct = L.BottleneckPtrs18(*[ptr(g) for g in self.grads])
        self.sstruct = L.BottleneckSaved(*[ptr(self.saved[k]) for k in L.BOTTLENECK_SAVED])
        self.rm, self.rv, self.nbt = c["rm"].clone(), c["rv"].clone(), torch.zeros((), dtype=torch.int64, device=DEV)
        self.t_out = torch.full_like(self.t, float("nan"))

    def fwd(self, training=True, labels=True, rank_stats=None):
        t_arg = self.t_out if labels else self.t
        return L.lib.cvae_bottleneck_fwd(C.byref(self.dims), C.byref(self.pstruct), ptr(self.y), ptr(self.m), ptr(t_arg), ptr(self.labels) if labels else None,
                                         ptr(self.eps), ptr(self.rm), ptr(self.rv), ptr(self.nbt), MOM, BN_EPS, 1 if training else 0, ptr(self.xcat),
                                         ptr(self.partial), ptr(self.dzm), C.byref(self.sstruct), ptr(self.dec), L.dtype_code(self.y.dtype), ptr(rank_stats),
                                         0 if rank_stats is None else rank_stats.shape[0], None, None)

    def bwd(self, g_none=False, bn_dy=None, bn_sums=None):
        gm, gl, gh = (None, None, None) if g_none else (self.g_mu, self.g_lv, self.g_mh)
        return L.lib.cvae_bottleneck_bwd(C.byref(self.dims), C.byref(self.pstruct), C.byref(self.gstruct), C.byref(self.sstruct), ptr(self.g_dec), ptr(gm), ptr(gl),
                                         ptr(gh), ptr(self.t_out if self.t_out.isfinite().all() else self.t), ptr(self.eps), ptr(self.xcat), ptr(self.y), 1,
                                         ptr(self.dzm), ptr(self.g1), ptr(self.dx), ptr(self.dy), L.dtype_code(self.y.dtype), ptr(bn_dy), ptr(bn_sums), None)

    def outputs(self):
        got = dict(mu=self.saved["mu"], logvar=self.saved["logvar"], m_hat=self.saved["m_hat"], dec_cl=self.dec, dy_cl=self.dy)
        got.update({"d" + k: g for k, g in zip(f64.PARAMS, self.grads)})
        return got


def widths(c):
    """(m_dim, t_dim, N1, N2, Z, HM) of a case"""
    p = c["params"]
    return c["m"].shape[1], c["t"].shape[1], p[0].shape[0], p[2].shape[0], p[4].shape[0], p[8].shape[0]


def run_ops(c, out, labels=True):
    """through ops.BioBottleneck.apply and autograd, as the model calls it"""
    y = c["y_cl"].clone().requires_grad_(True)
    params = [p.clone().requires_grad_(True) for p in c["params"]]
    rm, rv, nbt = c["rm"].clone(), c["rv"].clone(), torch.zeros((), dtype=torch.int64, device=DEV)
    assert ops.BioBottleneck.supported(y, out, True, widths(c))
    mu, lv, mh, dec = ops.BioBottleneck.apply(y, c["m"], c["labels"] if labels else c["t"], c["eps"], *params, rm, rv, nbt, MOM, BN_EPS, out)
    torch.autograd.backward([dec, mu, lv, mh], [c["g_dec"], c["g_mu"], c["g_logvar"], c["g_mhat"]])
    got = dict(mu=mu, logvar=lv, m_hat=mh, dec_cl=dec, dy_cl=y.grad, running_mean=rm, running_var=rv)
    got.update({"d" + k: p.grad for k, p in zip(f64.PARAMS, params)})
    return got, int(nbt)


# ------------------------------------------------------------------------------------------------ bottleneck sweep
# (id, M, spatial, C, out_size, m_dim, t_dim, N1, N2, Z, HM): every batch template full and partial, the model shapes, non-model shapes / widths
MODEL = dict(m_dim=12, t_dim=19, N1=512, N2=256, Z=64, HM=64)
SPECS = [
    ("bench_8to4_M2", 2, (8, 8, 8), 256, (4, 4, 4), MODEL),                 # K1 = 16415: fwd_ksplit 4
    ("bench_8to4_M3", 3, (8, 8, 8), 256, (4, 4, 4), MODEL),
    ("3d_4to4_M4", 4, (4, 4, 4), 256, (4, 4, 4), MODEL),
    ("bench_8to4_M5", 5, (8, 8, 8), 256, (4, 4, 4), MODEL),
    ("vol256_16to4_M7", 7, (16, 16, 16), 256, (4, 4, 4), MODEL),
    ("bench_8to4_M8", 8, (8, 8, 8), 256, (4, 4, 4), MODEL),
    ("bench_8to4_M9", 9, (8, 8, 8), 256, (4, 4, 4), MODEL),
    ("2d_8to4_M13", 13, (1, 8, 8), 256, (1, 4, 4), MODEL),
    ("bench_8to4_M16", 16, (8, 8, 8), 256, (4, 4, 4), MODEL),
    ("2d_4x8to4_M3", 3, (1, 4, 8), 256, (1, 4, 4), MODEL),
    ("C64_win2x3", 5, (1, 4, 6), 64, (1, 2, 2), dict(m_dim=1, t_dim=40, N1=100, N2=33, Z=7, HM=100)),
    ("C128_642to321", 9, (6, 4, 2), 128, (3, 2, 1), dict(m_dim=12, t_dim=1, N1=4, N2=1, Z=1, HM=1)),       # t_dim 1: zero batch variance
    ("ksplit2_K1odd", 4, (4, 4, 4), 128, (4, 4, 4), dict(m_dim=12, t_dim=19, N1=100, N2=33, Z=116, HM=64)),   # K1 = 8223, Z + m_dim = 128
    ("ksplit8", 2, (4, 4, 8), 512, (4, 4, 8), dict(m_dim=1, t_dim=40, N1=100, N2=256, Z=7, HM=100)),       # K1 = 65577
    ("N1_4096_M10", 10, (2, 2, 2), 64, (1, 1, 1), dict(m_dim=12, t_dim=19, N1=4096, N2=33, Z=64, HM=64)),  # the largest N1 at its largest M
    ("HM_1024_M7", 7, (2, 2, 2), 64, (1, 1, 1), dict(m_dim=12, t_dim=40, N1=100, N2=256, Z=7, HM=1024)),  # the largest HM at its largest M
    ("N2_2048_M16", 16, (2, 2, 2), 64, (2, 1, 1), dict(m_dim=12, t_dim=19, N1=512, N2=2048, Z=64, HM=64)),
    # the mechanism FORWARD past the large-LDS opt-in: 4 M (t_dim + 2 HM) = 68544 bytes (its backward: 159540 + 2048 static of the 163840)
    ("HM_1024_M7_T400", 7, (2, 2, 2), 64, (1, 1, 1), dict(m_dim=12, t_dim=400, N1=100, N2=256, Z=7, HM=1024)),
]


def spec_case(spec, dtype, seed=0, labels=None, training=True):
    name, M, sp, Cc, out, w = spec
    c = f64.make_case(100 + seed + SPECS.index(spec), M, sp, Cc, out, w["m_dim"], w["t_dim"], w["N1"], w["N2"], w["Z"], w["HM"], y_dtype=dtype, labels=labels,
                      training=training)
    return c, out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("spec", SPECS, ids=[s[0] for s in SPECS])
def test_bottleneck_matches_float64(spec, dtype):
    c, out = spec_case(spec, dtype)
    ref, err = reference(c, out)
    got, nbt = run_ops(cuda(c), out, labels=SPECS.index(spec) % 2 == 0)      # int64 labels and float one-hot alternate
    assert nbt == 1
    assert_within(got, ref, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_bottleneck_labels_edges_and_zero_variance(dtype):
    """labels 0 and t_dim - 1 repeated; then every row one label: batch variance exactly 0 (xhat = 0, y = beta)"""
    spec = SPECS[5]
    for labels in ([0, 18, 0, 18, 18, 0, 7, 0], [4] * 8):
        c, out = spec_case(spec, dtype, seed=7, labels=labels)
        ref, err = reference(c, out)
        got, _ = run_ops(cuda(c), out, labels=True)
        assert_within(got, ref, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("labels", [True, False], ids=["labels", "onehot"])
@pytest.mark.parametrize("spec", [SPECS[1], SPECS[10]], ids=["bench_M3", "C64"])
def test_bottleneck_eval_forward_and_null_output_grads(spec, labels, dtype):
    """bn_training = 0 (running statistics, untouched), and a training step whose g_mu / g_logvar / g_mhat are NULL (the raw ABI)"""
    # eval-mode forward: a case whose biases are nudged for the running statistics, so that its masks are decided too
    c, out = spec_case(spec, dtype, seed=3, training=False)
    cg = cuda(c)
    ref, err = reference(c, out, training=False)
    r = Raw(cg, out)
    assert r.fwd(training=False, labels=labels) == 0
    torch.cuda.synchronize()
    assert_within(r.outputs(), ref, err, ["mu", "logvar", "m_hat", "dec_cl"])
    assert torch.equal(r.rm, cg["rm"]) and torch.equal(r.rv, cg["rv"]) and int(r.nbt) == 0
    if labels:
        assert torch.equal(r.t_out, cg["t"])
    # training forward + backward with NULL output gradients
    c, out = spec_case(spec, dtype, seed=3)
    cg = cuda(c)
    ref, err = reference(c, out, g_none=True)
    r = Raw(cg, out)
    assert r.fwd(training=True, labels=labels) == 0
    assert r.bwd(g_none=True) == 0
    torch.cuda.synchronize()
    got = r.outputs()
    got.update(running_mean=r.rm, running_var=r.rv)
    assert_within(got, ref, err)
    assert int(r.nbt) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("ranks,per_rank", [(2, 1), (3, 1), (2, 4), (3, 3)])
def test_bottleneck_syncbn_handoff_matches_whole_batch(ranks, per_rank, dtype):
    """SyncBatchNorm emulated in one process: local stats -> gathered -> forward; backward -> bn_dy / bn_local_sums -> summed -> bn_bwd_finish.
    The ranks' outputs and summed gradients equal the float64 whole-batch reference."""
    M = ranks * per_rank
    c = f64.make_case(55 + M, M, (4, 4, 4), 64, (2, 2, 2), 12, 19, 100, 33, 7, 64, y_dtype=dtype)
    out = (2, 2, 2)
    ref, err = reference(c, out)
    cg = cuda(c)
    HM, T = c["params"][8].shape
    rk = [Raw(cg, out, slice(r * per_rank, (r + 1) * per_rank)) for r in range(ranks)]
    local = torch.empty(ranks, 2, HM, device=DEV)
    for r, raw in enumerate(rk):
        assert L.lib.cvae_bottleneck_bn_local_stats(ptr(cg["params"][8]), ptr(cg["params"][9]), None, ptr(raw.labels), ptr(local[r]), per_rank, T, HM, None) == 0
    bn_dy = [torch.empty(per_rank, HM, device=DEV) for _ in rk]
    sums = torch.empty(ranks, 2, HM, device=DEV)
    for r, raw in enumerate(rk):
        assert raw.fwd(training=True, labels=True, rank_stats=local) == 0
        assert raw.bwd(bn_dy=bn_dy[r], bn_sums=sums[r]) == 0
    total = sums.sum(0).contiguous()
    for r, raw in enumerate(rk):
        assert L.lib.cvae_bottleneck_bn_bwd_finish(C.byref(raw.dims), C.byref(raw.pstruct), C.byref(raw.gstruct), C.byref(raw.sstruct), ptr(raw.t_out),
                                                   ptr(bn_dy[r]), ptr(total), ranks, None) == 0
    torch.cuda.synchronize()
    outs = [raw.outputs() for raw in rk]
    got = {k: torch.cat([o[k] for o in outs]) for k in ("mu", "logvar", "m_hat", "dec_cl", "dy_cl")}
    got.update({k: sum(o[k] for o in outs) for k in outs[0] if k.startswith("d") and k != "dec_cl" and k != "dy_cl"})
    for raw in rk:                                      # every rank updates its running statistics with the same global numbers
        assert torch.equal(raw.rm, rk[0].rm) and torch.equal(raw.rv, rk[0].rv) and int(raw.nbt) == 1
    got.update(running_mean=rk[0].rm, running_var=rk[0].rv)
    assert_within(got, ref, err)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kw", [dict(M=16, N1=4096), dict(M=11, N1=4096), dict(M=16, HM=1024), dict(M=8, HM=1024), dict(M=16, t_dim=4096)])
def test_bottleneck_lds_corners_are_refused_before_any_launch(kw, dtype):
    """beyond a workgroup's LDS every entry answers CVAE_E_BADSHAPE and writes nothing — the running statistics stay as they were — and
    BioBottleneck.supported, given the widths, says no"""
    w = dict(MODEL)
    w.update(kw)
    c = cuda(f64.make_case(9, w.pop("M"), (2, 2, 2), 64, (1, 1, 1), w["m_dim"], w["t_dim"], w["N1"], w["N2"], w["Z"], w["HM"], y_dtype=dtype))
    assert ops.BioBottleneck.supported(c["y_cl"], (1, 1, 1), True) and not ops.BioBottleneck.supported(c["y_cl"], (1, 1, 1), True, widths(c))
    r = Raw(c, (1, 1, 1), refused=True)                 # buffers of the full size all the same: nothing may be written to them
    assert r.fwd(training=True, labels=True) == BADSHAPE
    assert r.bwd() == BADSHAPE
    torch.cuda.synchronize()
    assert torch.equal(r.rm, c["rm"]) and torch.equal(r.rv, c["rv"]) and int(r.nbt) == 0
    assert r.saved["mu"].isnan().all() and r.grads[0].isnan().all()


# ------------------------------------------------------------------------------------------------ ElboUp2x / cvae_up2x_fwd
# (B, d, h, w): 2D when d == 0 (D = d = 1); grids of exactly one workgroup (B d h w / 4 == 256) and with a partial last one
UP_SHAPES = [(1, 1, 1, 4), (3, 2, 3, 8), (1, 5, 64, 68), (3, 0, 3, 68), (1, 0, 64, 8), (1, 2, 32, 16), (3, 1, 3, 4), (1, 0, 1, 4), (1, 2, 8, 64)]
assert any(B * max(d, 1) * h * w // 4 == 256 for B, d, h, w in UP_SHAPES)


def up_inputs(B, d, h, w, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    nd = 2 if d == 0 else 3
    dd = max(d, 1)
    src = torch.randn(B, dd, h, w, 1, generator=g).to(dtype)
    x = torch.randn(B, 1, *((2 * dd,) if nd == 3 else ()), 2 * h, 2 * w, generator=g)
    m_hat, m = torch.randn(B, 12, generator=g), torch.rand(B, 12, generator=g)
    mu, lv = torch.randn(B, 7, generator=g), 0.5 * torch.randn(B, 7, generator=g)
    return src, x, m_hat, m, mu, lv


@pytest.mark.parametrize("finish", [True, False], ids=["in_launch", "two_launch"])
@pytest.mark.parametrize("t1", [True, False], ids=["t1", "no_t1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=["x".join(map(str, s)) for s in UP_SHAPES])
def test_elbo_up2x_matches_float64(shape, dtype, t1, finish, monkeypatch):
    B, d, h, w = shape
    src, x, m_hat, m, mu, lv = up_inputs(B, d, h, w, dtype, seed=sum(shape))
    gamma, g_loss = 3.0, 0.7
    ref, err = f64.elbo_up2x(src, x, m_hat, m, mu, lv, gamma, g_loss)
    if dtype == torch.bfloat16:
        err["dsrc"] = f64.bf16_out(err["dsrc"], ref["dsrc"])
    monkeypatch.setattr(ops.ElboUp2x, "IN_LAUNCH_FINISH", finish)
    s, xg = src.to(DEV).requires_grad_(t1), x.to(DEV)
    mh, mug, lvg = (v.to(DEV).requires_grad_(t1) for v in (m_hat, mu, lv))
    assert ops.ElboUp2x.supported(s, xg)
    bump = torch.zeros(1, dtype=torch.int32, device=DEV)
    loss, recon, ml, kld = ops.ElboUp2x.apply(s, xg, mh, m.to(DEV), mug, lvg, gamma, bump)
    got = dict(loss=loss, recon=recon, m_loss=ml, kld=kld)
    if t1:
        (loss * g_loss).backward()
        got.update(dsrc=s.grad, d_mhat=mh.grad, dmu=mug.grad, dlv=lvg.grad)
    torch.cuda.synchronize()
    assert_within(got, ref, err, list(got))
    assert int(bump) == 1
    if finish:
        assert int(ops.ElboUp2x._tickets[xg.device].abs().sum()) == 0            # the last workgroup leaves the arrival words zero
        loss2 = ops.ElboUp2x.apply(s, xg, mh, m.to(DEV), mug, lvg, gamma, bump)[0]        # the same launch again: the same bits
        torch.cuda.synchronize()
        assert int(bump) == 2 and torch.equal(loss2.detach(), loss.detach())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=["x".join(map(str, s)) for s in UP_SHAPES])
def test_up2x_fwd_matches_float64_interpolate(shape, dtype):
    B, d, h, w = shape
    src = up_inputs(B, d, h, w, dtype, seed=sum(shape) + 1)[0]
    dd = max(d, 1)
    D, H, W = (2 * dd if d else 1), 2 * h, 2 * w
    s = src.to(DEV).contiguous()
    dst = torch.full((B, D * H * W), float("nan"), device=DEV)
    assert L.lib.cvae_up2x_fwd(ptr(s), ptr(dst), B, dd, h, w, D, H, W, L.dtype_code(dtype), None) == 0
    torch.cuda.synchronize()
    x = torch.zeros(B, 1, *((D,) if d else ()), H, W)
    z = torch.zeros(B, 1)
    ref, err = f64.elbo_up2x(src, x, z, z, z, z, 1.0, 1.0)
    assert_within(dict(up=dst), ref, err, ["up"])


@pytest.mark.parametrize("shape", [(2, 2, 4, 6), (1, 2, 4, 10), (1, 0, 3, 6)], ids=["w6", "w10", "2d_w6"])
def test_elbo_up2x_refuses_unsupported_shapes(shape):
    B, d, h, w = shape
    src, x = up_inputs(B, d, h, w, torch.float32, 0)[:2]
    assert not ops.ElboUp2x.supported(src.to(DEV), x.to(DEV))                        # w % 4 != 0
    src4 = torch.zeros(B, max(d, 1), h, 4, 1, device=DEV)
    x_bad = torch.zeros(B, 1, *((2 * d,) if d else ()), 2 * h + 2, 8, device=DEV)   # H != 2h
    assert not ops.ElboUp2x.supported(src4, x_bad)
