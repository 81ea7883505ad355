"""csrc/bn2d_batch.hip (cvae_bn2d_batch_fwd: batch-statistics BatchNorm2d + LeakyReLU(0.01) that reads its input twice) through ops.bn2d_batch_fwd,
and cvae_bn2d_bwd fed with its outputs through ops.bn2d_bwd, against float64 on the stored values with the element-wise bounds of
tests/bn2d_batch_reference.py (derived there from the kernel's sums; tests/test_bn2d_batch_cpu.py shows that an fp32 evaluation of the same formulas meets them).

Shapes: C in {32, 64, 128, 256} (the stem's widths) x P in {2, 12, 257, 3077}: the smallest legal P, the stem's last layer at 64 x 96 (2 x 3 positions, batch 2), a
chunk of 256 rows plus one row (two workgroups, the second with one row), and 13 workgroups with a ragged tail of 5 rows; fp32 and bf16.
  forward        mean, rstd, a, running_mean, running_var element-wise within their bounds; num_batches_tracked up by one; two runs give equal bits
  cancellation   fp32 channels 1000 + 0.01 N(0, 1), P = 3077: every output within the same bounds, and the variance itself, read back from the running variance,
                 within its bound.  On this input the float32 formula E[y^2] - E[y]^2 misses the float64 variance (1.0e-4) by 0.25, 2.1e4 times the bound
                 (computed on the CPU by the test itself, and in tests/test_bn2d_batch_cpu.py): the case discriminates.  The bound is wide there, 0.53 of the
                 variance: the mean, 1000, is stored in fp32 (half an ulp is 3e-5, a third of a percent of the standard deviation) and every merge rounds it again.
  backward       ops.bn2d_bwd on (y, dy, a, gamma, mean, rstd) of the HIP forward against float64 autograd of a = where(mask, v, 0.01 v), v = batch_norm(y), with the
                 masks of the HIP forward's own `a`, checked against float64 wherever |v| exceeds its bound (the idiom of tests/vit_stem_grad_reference.py)

Measured on the MI355X, max |got - ref| / bound (the RATIO lines of the run), over all 16 shapes:
  forward fp32    mean 0.016 - 0.93 (P = 2: one rounding is the whole bound), rstd 0.010 - 0.16, a 0.015 - 0.80, running_mean 0.016 - 0.41, running_var 0.045 - 0.44
  forward bf16    mean <= 0.33, rstd <= 0.11, a 0.86 - 0.99 (half a bf16 ulp of the stored value is nearly the whole bound), running_mean <= 0.45, running_var <= 0.37
  cancellation    mean 0.11, rstd 0.001, a 0.11, running_var 0.079; the variance 0.079 of its bound, the naive fp32 formula 21332 bounds
  backward fp32   dx 0.013 - 0.60, dgamma 0.0005 - 0.61, dbeta 0.0008 - 0.12 (the large ratios at P = 2);  bf16  dx 0.54 - 0.99, dgamma <= 0.08, dbeta <= 0.12
  masks           at most 28 of 393856 signs undecided by the rounding bound (bf16, P = 3077); where decided, every sign is float64's
No ratio is above 1."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bn2d_batch_reference as br  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHANNELS, ROWS = (32, 64, 128, 256), (2, 12, 257, 3077)
MOM, EPS = 0.1, 1e-5
_REF = {}


def module(d, Cc, track=True):
    bn = torch.nn.BatchNorm2d(Cc, eps=EPS, momentum=MOM, track_running_stats=track)
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]), bn.bias.copy_(d["beta"])
        if track:
            bn.running_mean.copy_(d["rm"]), bn.running_var.copy_(d["rv"])
            bn.num_batches_tracked.fill_(7)
    return bn.to(DEV).eval()


def case(P, Cc, bf16, cancel=False):
    """the inputs and the float64 reference of one shape, computed once and shared"""
    key = (P, Cc, bf16, cancel)
    if key not in _REF:
        d = br.inputs(P, Cc, 100 + P + Cc, bf16, cancel)
        _REF[key] = (d,) + br.forward(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], MOM, EPS, bf16=bf16)
    return _REF[key]


def run_forward(d, Cc):
    from causal_vae_amd import ops
    bn = module(d, Cc)
    with torch.no_grad():
        a, mean, rstd = ops.bn2d_batch_fwd(d["y"].to(DEV), bn, "leaky001")
    torch.cuda.synchronize()
    return bn, dict(a=a, mean=mean, rstd=rstd, running_mean=bn.running_mean, running_var=bn.running_var)


def hold(label, got, ref, err, keys):
    ratios = {k: br.max_ratio(got[k], ref[k], err[k]) for k in keys}
    print(f"RATIO {label} " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (label, k, v)


FWD_KEYS = ("mean", "rstd", "a", "running_mean", "running_var")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_forward_against_float64(Cc, P, bf16):
    d, ref, err = case(P, Cc, bf16)
    bn, got = run_forward(d, Cc)
    assert got["a"].dtype == d["y"].dtype and got["a"].shape == d["y"].shape and int(bn.num_batches_tracked) == 8
    hold(f"forward C{Cc} P{P} {'bf16' if bf16 else 'f32'}", got, ref, err, FWD_KEYS)
    _bn2, again = run_forward(d, Cc)                                   # no atomics, a grid that depends on P alone: the same bits
    for k in FWD_KEYS:
        assert torch.equal(got[k], again[k]), k


def test_cancellation_case():
    P, Cc = 3077, 32
    d, ref, err = case(P, Cc, False, cancel=True)
    naive = br.naive_var_fp32(d["y"])                                  # on the CPU: the formula the kernel must not use breaks the bound on this input
    assert br.max_ratio(naive, ref["var"], err["var"]) > 100.0
    _bn, got = run_forward(d, Cc)
    hold("cancellation C32 P3077 f32", got, ref, err, FWD_KEYS)
    # the variance itself, from the running variance (momentum m, unbiased): var = (running_var - (1 - m) rv) / m (P - 1) / P, held to var's own bound plus
    # the rounding of the stored running value
    m = br.f32(MOM)
    var = (got["running_var"].cpu().double() - (1.0 - m) * d["rv"].double()) / m * (P - 1) / P
    bound = err["running_var"] / m * (P - 1) / P
    r = br.max_ratio(var, ref["var"], bound)
    print(f"RATIO cancellation variance {r:.4f} (bound / var {float((bound / ref['var']).max()):.3f}, naive fp32 formula {br.max_ratio(naive, ref['var'], bound):.1f})")
    assert r <= 1.0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_backward_against_float64_autograd(Cc, P, bf16):
    from causal_vae_amd import ops
    d, ref, err = case(P, Cc, bf16)
    bn = module(d, Cc, track=False)
    y, dy = d["y"].to(DEV), d["dy"].to(DEV)
    with torch.no_grad():
        a, mean, rstd = ops.bn2d_batch_fwd(y, bn, "leaky001")
        assert bn.running_mean is None                                   # untracked: statistics of the batch, nothing else written
        gy, dgamma, dbeta = ops.bn2d_bwd(y, dy, a, bn.weight, mean, rstd, "leaky001")
    mask = a.cpu().double() > 0
    decided = ref["v"].abs() > err["v"]
    assert bool(((mask == (ref["v"] > 0)) | ~decided).all()), "a LeakyReLU sign differs from float64's where the rounding bound decides it"
    print(f"masks C{Cc} P{P}: {int((~decided).sum())} of {mask.numel()} signs undecided by the rounding bound")
    bref, berr = br.backward(d["y"], d["dy"], mask, d["gamma"], ref["mean"], ref["rstd"], err["mean"], err["rstd"], bf16=bf16)
    auto = br.autograd_backward(d["y"], d["dy"], mask, d["gamma"], d["beta"], EPS)
    for k in auto:                                                       # the restatement that carries the bound IS autograd's function
        assert float((auto[k] - bref[k]).abs().max()) <= 1e-10 * max(float(auto[k].abs().max()), 1e-30), k
    hold(f"backward C{Cc} P{P} {'bf16' if bf16 else 'f32'}", dict(dx=gy, dgamma=dgamma, dbeta=dbeta), auto, berr, ("dx", "dgamma", "dbeta"))


def test_momentum_none_and_width_mismatch_raise():
    from causal_vae_amd import ops
    from causal_vae_amd._lib import CvaeError
    y = torch.zeros(4, 32, device=DEV)
    with torch.no_grad():
        with pytest.raises(CvaeError, match="momentum"):
            ops.bn2d_batch_fwd(y, torch.nn.BatchNorm2d(32, momentum=None).to(DEV).eval(), "leaky001")
        with pytest.raises(CvaeError, match="32 channels"):
            ops.bn2d_batch_fwd(y, torch.nn.BatchNorm2d(64).to(DEV).eval(), "leaky001")
