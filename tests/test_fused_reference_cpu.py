"""CPU self-tests of oracle/fused64.py, the float64 references tests/test_fused_reference.py compares the fused kernels with: the same graph
evaluated in fp32 lies within the derived bounds, and the reference with one term dropped (a K1 column, a pooled voxel, a batch row of a
weight-gradient sum, a mechanism_net unit) does not — a comparator that passed those would pass a subtly wrong kernel.  Also the host-side
LDS budget of the bottleneck's level launches: cvae_bottleneck_sizes refuses the corners whose launches would not fit."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import fused64 as f64  # noqa: E402

BADSHAPE = -1
OUT = (2, 2, 2)


def _args(c, out=OUT):
    return (c["y_cl"], c["m"], c["t"], c["eps"], c["params"], c["rm"], c["rv"], 0.1, 1e-5, out, c["g_dec"], c["g_mu"], c["g_logvar"], c["g_mhat"])


@pytest.fixture(scope="module")
def case():
    c = f64.make_case(1, 5, (4, 4, 4), 64, OUT, 12, 19, 100, 33, 7, 64)
    ref, err, pre = f64.bottleneck(*_args(c))
    return c, ref, err, pre


def test_masks_are_clear_of_their_bounds(case):
    _, _, _, pre = case
    assert f64.mask_margin(pre) == {k: 0 for k in f64.RELU_PRE}


def test_fp32_evaluation_is_within_the_bounds(case):
    c, ref, err, _ = case
    got, _, _ = f64.bottleneck(*_args(c), dtype=torch.float32)
    assert f64.compare(got, ref, err) == []


def test_zero_variance_batch_is_within_the_bounds():
    """every row with the same label: BatchNorm's batch variance is exactly 0 and the rounding in h - mean is amplified by 1/sqrt(bn_eps)"""
    c = f64.make_case(2, 4, (4, 4, 4), 64, OUT, 12, 19, 100, 33, 7, 64, labels=[3, 3, 3, 3])
    ref, err, pre = f64.bottleneck(*_args(c))
    assert f64.mask_margin(pre) == {k: 0 for k in f64.RELU_PRE}
    got, _, _ = f64.bottleneck(*_args(c), dtype=torch.float32)
    assert f64.compare(got, ref, err) == []


@pytest.mark.parametrize("drop,expect", [(("k1_col", 3), "mu"), (("pool_voxel", (0, 1, 0, 1)), "dec_cl"), (("wgrad_row", 1), "dW1"),
                                         (("hm_unit", 2), "m_hat")])
def test_a_dropped_term_fails_the_comparison(case, drop, expect):
    c, ref, err, _ = case
    got, _, _ = f64.bottleneck(*_args(c), drop=drop)
    bad = f64.compare(got, ref, err)
    assert any(b.startswith(expect + ":") for b in bad), bad


@pytest.fixture(scope="module")
def model_case():
    """the benchmark's shape (C = 256, 8^3 -> 4^3, the model's widths) at M = 8, the full MT = 8 template: K1 = 16415 (fwd_ksplit 4), NS = 32
    backward slabs of 16 enc_fc.0 rows"""
    out = (4, 4, 4)
    c = f64.make_case(108, 8, (8, 8, 8), 256, out, 12, 19, 512, 256, 64, 64)
    ref, err, pre = f64.bottleneck(*_args(c, out))
    return c, out, ref, err, pre


def test_model_shape_fp32_evaluation_is_within_the_bounds(model_case):
    c, out, ref, err, pre = model_case
    assert f64.mask_margin(pre) == {k: 0 for k in f64.RELU_PRE}
    got, _, _ = f64.bottleneck(*_args(c, out), dtype=torch.float32)
    assert f64.compare(got, ref, err) == []


@pytest.mark.parametrize("name", ["mu", "logvar", "dec_cl", "dy_cl", "dW1", "db1", "dWd"])
@pytest.mark.parametrize("scale", [0.97, 1.02])
def test_model_shape_a_few_percent_fails_the_comparison(model_case, name, scale):
    """the bounds stay tight at the model shape: a uniform 2-3 % error in the encoder's input gradient, the decoder's input or the latent fails"""
    _, _, ref, err, _ = model_case
    got = dict(ref)
    got[name] = ref[name] * scale
    assert f64.compare(got, ref, err, [name]) != []


@pytest.mark.parametrize("slab", [(0, 16), (256, 272), (496, 512)])
def test_model_shape_a_missing_backward_slab_fails_the_comparison(model_case, slab):
    """one NS slab (16 rows of enc_fc.0) missing from the partial sums of d(xcat), hence from dy_cl"""
    c, out, ref, err, _ = model_case
    got, _, _ = f64.bottleneck(*_args(c, out), drop=("dy_slab", slab))
    assert any(b.startswith("dy_cl:") for b in f64.compare(got, ref, err, ["dy_cl"]))


def test_bf16_bound_covers_the_rounding():
    x = torch.randn(1000, dtype=torch.float64) * 10
    got = x.to(torch.bfloat16)
    assert f64.compare({"v": got}, {"v": x}, {"v": f64.bf16_out(torch.zeros_like(x), x)}) == []
    assert f64.compare({"v": got}, {"v": x}, {"v": torch.zeros_like(x)}) != []


def test_elbo_up2x_reference_is_consistent():
    """the float64 ELBO reference against an fp32 evaluation of the same graph, and a dropped voxel of x fails it"""
    g = torch.Generator().manual_seed(3)
    B, d, h, w = 2, 2, 3, 8
    src = torch.randn(B, d, h, w, 1, generator=g)
    x = torch.randn(B, 1, 2 * d, 2 * h, 2 * w, generator=g)
    m_hat, m, mu, lv = (torch.randn(B, 12, generator=g), torch.rand(B, 12, generator=g), torch.randn(B, 7, generator=g), 0.3 * torch.randn(B, 7, generator=g))
    ref, err = f64.elbo_up2x(src, x, m_hat, m, mu, lv, 3.0, 0.7)
    import torch.nn.functional as F
    from oracle.functional import cascade_loss
    s = src.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    up = F.interpolate(s, size=x.shape[2:], mode="trilinear", align_corners=False)
    loss, recon, ml, kld = cascade_loss(up, x, m_hat, m, mu, lv, 3.0)
    (gs,) = torch.autograd.grad(loss * 0.7, s)
    got = dict(loss=loss, recon=recon, m_loss=ml, kld=kld, dsrc=gs.permute(0, 2, 3, 4, 1))
    assert f64.compare(got, ref, err, names=list(got)) == []
    x2 = x.clone()
    x2[1, 0, 3, 5, 2] += 1.0
    ref2, _ = f64.elbo_up2x(src, x2, m_hat, m, mu, lv, 3.0, 0.7)
    assert f64.compare(ref2, ref, err, names=["recon", "dsrc"]) != []


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "causal_vae_amd", "libcvae_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    from causal_vae_amd import _lib
    return _lib


def _sizes(L, M, N1=512, N2=256, HM=64, t_dim=19, Z=64, m_dim=12, C_=64):
    dims = L.BottleneckDims(M, 4, 4, 4, C_, 2, 2, 2, m_dim, t_dim, N1, N2, Z, HM)
    out = [C.c_int64() for _ in range(5)]
    return L.lib.cvae_bottleneck_sizes(C.byref(dims), *[C.byref(v) for v in out])


@pytest.mark.parametrize("kw", [dict(M=16, N1=4096), dict(M=11, N1=4096), dict(M=16, HM=1024), dict(M=8, HM=1024), dict(M=16, t_dim=4096),
                                dict(M=2, t_dim=65537)])
def test_lds_corners_are_refused(lib, kw):
    """a level launch whose dynamic LDS would not fit in the 160 KiB of a CU is refused before anything runs"""
    assert _sizes(lib, **kw) == BADSHAPE


@pytest.mark.parametrize("kw", [dict(M=16, N1=2048), dict(M=10, N1=4096), dict(M=7, HM=1024), dict(M=2, t_dim=4096), dict(M=16, N2=2048, N1=512),
                                dict(M=16)])
def test_lds_budget_accepts_the_rest(lib, kw):
    assert _sizes(lib, **kw) == 0


@pytest.mark.parametrize("M,N1,ok", [(10, 4096, True), (11, 4096, False), (16, 512, True)])
def test_supported_asks_the_library_about_widths(lib, M, N1, ok):
    from causal_vae_amd import ops
    y = torch.empty(M, 4, 4, 4, 64)
    assert ops.BioBottleneck.supported(y, (2, 2, 2), True)                                   # shapes alone
    assert ops.BioBottleneck.supported(y, (2, 2, 2), True, widths=(12, 19, N1, 256, 64, 64)) == ok
