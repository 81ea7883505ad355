"""csrc/bn2d_batch.hip's decoder entries on the GPU: cvae_bn2d_batch_bwd through ops.bn2d_batch_bwd and cvae_bn2d_batch_fwd_res through
ops.bn2d_batch_fwd(.., resid=), against float64 on the stored values with the element-wise bounds of tests/bn2d_batch_bwd_reference.py (derived there from the
kernels' sums; tests/test_bn2d_batch_bwd_cpu.py shows that an fp32 evaluation of the same formulas in the kernels' order meets them and that two wrong kernels
do not).

Shapes: C in {8, 16, 32, 64, 128} x P in {2, 24, 257, 3077}: the smallest legal P, the decoder's first stage at 64 x 96 with B = 1, a chunk of 256 rows plus one
row, and 13 workgroups with a ragged tail; activations none / leaky02 / leaky001; fp32 and bf16.  One more: C = 16, P = 262401 — the chunk grows to 512 rows,
513 chunks with a ragged last one, and the finish walks runs of 33.
  backward   ops.bn2d_batch_bwd on (y, dy, a, gamma, mean, rstd) of the HIP forward against float64 autograd of a = where(mask, v, slope v), v = batch_norm(y), with
             the masks of the HIP forward's own `a`; dx, dgamma, dbeta element-wise within their bounds; two runs give equal bits
  forward    the plain entry at C = 8 and 16 (widths the stem's tests do not reach) and the residual entry at every width: a, mean, rstd, running statistics
             within their bounds, the counter up by one, two runs equal bits; a residual with an activation is refused

Measured on the MI355X, max |got - ref| / bound over all shapes (the RATIO lines of the run):
  backward fp32   dx 0.013 - 0.58, dgamma <= 0.76, dbeta <= 0.17;  bf16  dx 0.066 - 0.99 (half a bf16 ulp of the stored value is nearly the whole bound), dgamma <= 0.065,
                  dbeta <= 0.21;  P = 262401: dx 0.0056 (fp32) / 0.98 (bf16), dgamma and dbeta below 0.001
  forward         C = 8, 16 and P = 262401: fp32 mean <= 0.60, rstd <= 0.11, a <= 0.34, running statistics <= 0.36; bf16 a 0.75 - 0.97, the rest <= 0.37
  residual        fp32 mean <= 0.93 (P = 2), a <= 0.80, running statistics <= 0.41; bf16 a 0.83 - 0.995, the rest <= 0.45
No ratio is above 1."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bn2d_batch_reference as br  # noqa: E402
import bn2d_batch_bwd_reference as bb  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHANNELS, ROWS, ACTS = (8, 16, 32, 64, 128), (2, 24, 257, 3077), (None, "leaky02", "leaky001")
BIG = (262401, 16)
MOM, EPS = 0.1, 1e-5
FWD_KEYS = ("mean", "rstd", "a", "running_mean", "running_var")
_REF = {}


def module(d, Cc, track=True):
    bn = torch.nn.BatchNorm2d(Cc, eps=EPS, momentum=MOM, track_running_stats=track)
    with torch.no_grad():
        bn.weight.copy_(d["gamma"]), bn.bias.copy_(d["beta"])
        if track:
            bn.running_mean.copy_(d["rm"]), bn.running_var.copy_(d["rv"])
            bn.num_batches_tracked.fill_(7)
    return bn.to(DEV).eval()


def case(P, Cc, bf16, act):
    """the inputs and the forward's float64 reference of one shape and activation, computed once and shared"""
    key = (P, Cc, bf16, act)
    if key not in _REF:
        d = br.inputs(P, Cc, 100 + P + Cc, bf16)
        slope = bb.SLOPES[act]
        _REF[key] = (d, slope) + br.forward(d["y"], d["gamma"], d["beta"], d["rm"], d["rv"], MOM, EPS, slope=1.0 if slope is None else slope, bf16=bf16)
    return _REF[key]


def hold(label, got, ref, err, keys):
    ratios = {k: br.max_ratio(got[k], ref[k], err[k]) for k in keys}
    print(f"RATIO {label} " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 1.0, (label, k, v)


def run_backward(Cc, P, act, bf16):
    from causal_vae_amd import ops
    d, slope, ref, err = case(P, Cc, bf16, act)
    bn = module(d, Cc, track=False)
    y, dy = d["y"].to(DEV), d["dy"].to(DEV)
    with torch.no_grad():
        a, mean, rstd = ops.bn2d_batch_fwd(y, bn, act)
        outs = [ops.bn2d_batch_bwd(y, dy, a if act is not None else None, bn.weight, mean, rstd, act) for _ in range(2)]
    torch.cuda.synchronize()
    for u, v in zip(*outs):                                              # no atomics, a grid that depends on P alone: the same bits
        assert torch.equal(u, v)
    gy, dgamma, dbeta = outs[0]
    assert gy.dtype == y.dtype and gy.shape == y.shape and dgamma.dtype == dbeta.dtype == torch.float32
    mask = None
    if slope is not None:                                                # the masks of the HIP forward's own `a`
        mask = a.cpu().double() > 0
        decided = ref["v"].abs() > err["v"]
        assert bool(((mask == (ref["v"] > 0)) | ~decided).all()), "a LeakyReLU sign differs from float64's where the rounding bound decides it"
    bref, berr = bb.backward(d["y"], d["dy"], mask, d["gamma"], ref["mean"], ref["rstd"], err["mean"], err["rstd"], slope, bf16)
    auto = bb.autograd_backward(d["y"], d["dy"], mask, d["gamma"], d["beta"], EPS, slope)
    for k in auto:                                                       # the restatement that carries the bound IS autograd's function
        assert float((auto[k] - bref[k]).abs().max()) <= 1e-10 * max(float(auto[k].abs().max()), 1e-30), k
    hold(f"backward C{Cc} P{P} {act} {'bf16' if bf16 else 'f32'}", dict(dx=gy, dgamma=dgamma, dbeta=dbeta), auto, berr, ("dx", "dgamma", "dbeta"))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", ACTS, ids=["none", "leaky02", "leaky001"])
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_backward_against_float64_autograd(Cc, P, act, bf16):
    run_backward(Cc, P, act, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_backward_with_513_chunks_of_512_rows(bf16):
    P, Cc = BIG
    assert (br.chunk_rows(P), br.parts(P), P - 512 * 512) == (512, 513, 257) and bb.runs(513)[0] == (0, 33)
    run_backward(Cc, P, "leaky001", bf16)


def run_forward(d, Cc, act, resid=None):
    from causal_vae_amd import ops
    bn = module(d, Cc)
    with torch.no_grad():
        a, mean, rstd = ops.bn2d_batch_fwd(d["y"].to(DEV), bn, act, **({} if resid is None else {"resid": resid.to(DEV)}))
    torch.cuda.synchronize()
    assert a.dtype == d["y"].dtype and a.shape == d["y"].shape and int(bn.num_batches_tracked) == 8
    return dict(a=a, mean=mean, rstd=rstd, running_mean=bn.running_mean, running_var=bn.running_var)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("P,Cc", [(P, Cc) for Cc in (8, 16) for P in ROWS] + [BIG])
def test_plain_forward_at_the_narrow_widths(P, Cc, bf16):
    d, _slope, ref, err = case(P, Cc, bf16, "leaky001")
    got = run_forward(d, Cc, "leaky001")
    hold(f"forward C{Cc} P{P} {'bf16' if bf16 else 'f32'}", got, ref, err, FWD_KEYS)
    again = run_forward(d, Cc, "leaky001")
    for k in FWD_KEYS:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_residual_forward_against_float64(Cc, P, bf16):
    d, _slope, _ref, _err = case(P, Cc, bf16, None)
    resid = d["dy"]                                                      # any tensor of y's shape and dtype
    ref, err = bb.forward_res(d["y"], resid, d["gamma"], d["beta"], d["rm"], d["rv"], MOM, EPS, bf16)
    got = run_forward(d, Cc, None, resid)
    hold(f"residual forward C{Cc} P{P} {'bf16' if bf16 else 'f32'}", got, ref, err, FWD_KEYS)
    again = run_forward(d, Cc, None, resid)
    for k in FWD_KEYS:
        assert torch.equal(got[k], again[k]), k
    plain = run_forward(d, Cc, None)                                     # the same moments and finish launches: the statistics' bits are the plain entry's
    for k in ("mean", "rstd", "running_mean", "running_var"):
        assert torch.equal(got[k], plain[k]), k


def test_a_residual_with_an_activation_is_refused():
    from causal_vae_amd import _lib as L, ops
    y = torch.zeros(24, 16, device=DEV)
    bn = torch.nn.BatchNorm2d(16).to(DEV).eval()
    with torch.no_grad():
        for act in ("leaky02", "leaky001", "relu"):
            with pytest.raises(L.CvaeError, match="residual"):
                ops.bn2d_batch_fwd(y, bn, act, resid=y)
        with pytest.raises(L.CvaeError, match="resid"):
            ops.bn2d_batch_fwd(y, bn, None, resid=torch.zeros(24, 8, device=DEV))
        with pytest.raises(L.CvaeError, match="needed"):
            ops.bn2d_batch_bwd(y, y, None, bn.weight, bn.running_mean, bn.running_var, "leaky001")
        mean, rstd = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
        _scratch = torch.zeros(2 * 16, device=DEV)
        p = lambda t: t.data_ptr()
        rc = L.lib.cvae_bn2d_batch_fwd_res(p(y), p(bn.weight), p(bn.bias), p(torch.empty_like(y)), p(mean), p(rstd), None, None, 24, 16, 0.1, 1e-5, 4, 0,
                                           p(_scratch), _scratch.numel() * 4, None, p(y))
    assert rc == -3 and int(bn.num_batches_tracked) == 0                 # CVAE_E_UNSUPPORTED, before any launch
