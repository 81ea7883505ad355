"""CPU self-tests of oracle/plumbing64.py, the float64 references and bounds that tests/test_plumbing_reference.py holds csrc/elementwise.hip and csrc/vessel2d.hip to.

  1. WITHIN THE BOUNDS: every reference evaluated in fp32 on the CPU (the stand-in for a correct kernel) lies within its bound at every shape family of the GPU
     file; the ratio max |fp32 - float64| / bound is printed per family (`RATIO <family> <value>`, the bracketed figures of the GPU file's docstring).  The pure
     moves have no bound: their reference is checked against torch (permute, cat, one_hot, clamp, .bfloat16()) bit for bit.  The resize reference is checked
     against F.interpolate in float64 at the ratios where the fp32 and the float64 scale agree exactly (2x, 1/2x, 1x).
  2. ONE WRONG TERM FAILS: every entry of plumbing64._MUTATIONS is rejected at the shapes the GPU file relies on.  What catches it:
       last_row            the bound at P <= 7000 (C = 12, 40, 19); at 16385 x 1028 the bound still rejects the tensor, but only the STRUCTURED case (integers, exact
                           sums) differs in every channel whose dropped element is not 0
       unclipped_div       bound and structured at 7 -> 3 and (5, 6, 9) -> 4; identical at 8 -> 4 (the nominal window is the real one)
       pm1                 THE RULE csrc/elementwise.hip SHIPPED for the pool backward (candidates floor(i O / I) - 1 .. + 1): rejected by bound and structured at
                           1 -> 3, 2 -> 7, 2 -> 5 / 1 -> 4; bit-identical to the exact rule at every O <= I shape (8 -> 4, 7 -> 3, (5, 6, 9) -> 4, 66 -> 65)
       align_corners       bound, at (16, 16) -> (9, 11), the 3D case and exact 2x; identical at 8 -> 8 and 1 -> 5 (not a fault there)
       swap_taps           bound, at the same shapes
       biased_running_var  bound on running_var, at P = 3 and at P = 4097
       one_pass_var        bound on rstd and y, in the channel of mean 50 and std 0.1 (the other channels pass: that is why the channel is there), at every shape of
                           the GPU file with P <= 1361 but 817 x 40 (0.73 of the bound) and barely at 4097 x 8 (1.3): the two-pass bound itself grows like sqrt(P) |mean|
       dx_no_dgamma        bound on dx
       tile_edge           bits, at C or S or V = 65 and 130; nothing to catch at <= 64
       bf16_trunc          bits, on the exact ties of plumbing64.specials() and on Gaussian values (half of them round up)
  3. The reference's BRANCH ASSERTIONS fire: an activation output within 2^-6 of zero, a sigmoid argument beyond 8.  The resize has no assertion: a tap position
     within rounding of an integer (3 -> 7, 300 -> 420: s = 1, 2 at o = 3 with an inexact fp32 scale; 8 -> 8, 5 -> 1: exact integers) may flip the kernel's tap
     index, and test_resize_tap_positions_moved_by_their_rounding moves every position by +- 0.99 eps_s, flips included, and finds the result inside the bound.
  4. ARGUMENT CHECKS of the 20 entry points of both files, each against what include/cvae_hip.h says, in the idiom of tests/test_loss_reference_cpu.py: valid
     arguments get past every check, which without a device ends as CVAE_E_LAUNCH; every rule has its code; no byte of any buffer changes.  Skipped where a
     device exists.  Header and code disagreed; fixed with this file:
       cvae_clamp_fwd          the header says torch.clamp, the kernel's fminf(fmaxf(x, lo), hi) turned a NaN into lo: the kernel keeps the NaN now
       cvae_adaptive_avgpool_bwd  the header says "sum over windows containing (d, h, w)", the kernel looked at three candidates per axis and lost terms whenever
                               an output axis is more than about twice its input: the kernel visits floor(i O / I) .. ceil((i + 1) O / I) - 1 now
       cvae_bn2d_fwd           the header lets running_mean / running_var be NULL; the kernel wrote running_var whenever running_mean was given: each on its own
                               now.  The header did not give the limits the code has (8 <= C <= 2048, training P >= 2), the 16-byte alignment its loads need,
                               the codes of a missing or short workspace, or that the forward is satisfied with half of cvae_bn2d_workspace_bytes: stated now
  5. cvae_channel_sum_workspace_bytes and cvae_bn2d_workspace_bytes are at least what every path asks for, the block counts recomputed in Python from the rules of
     the .hip files (plumbing64.channel_sum_geometry, aligned and misaligned; bn2d_blocks), at every shape the GPU file uses; and the replayed geometry is the one
     the shape tables name."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import plumbing64 as p64

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
WORST = {}
KINDS = ["random", "structured"]


def ratio(name, fn, *args, **kw):
    """the fp32 evaluation of fn against its float64 reference: asserts it within the bounds, prints and returns the largest ratio"""
    ref, err = fn(*args, **kw)
    got, _ = fn(*args, dtype=F32, **kw)
    bad = p64.compare(got, ref, err)
    worst = max(p64.max_ratio(got[k], ref[k], err[k]) for k in ref)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"RATIO {name} {worst:.4f}")
    assert not bad, "\n".join(bad)
    return worst


def rejected(got, ref, err, keys=None):
    bad = p64.compare(got, ref, err, keys)
    assert bad, f"the wrong result passed the comparison of {keys or list(ref)}"
    return bad


def exact32(fn, *args, **kw):
    """the structured case: the fp32 stand-in gives the float64 result bit for bit (a LeakyReLU's slope product: that result correctly rounded to fp32, once)"""
    ref, _ = fn(*args, **kw)
    got, _ = fn(*args, dtype=F32, **kw)
    ref = {k: v.to(F32).to(F64) for k, v in ref.items()}
    for k in ref:
        assert torch.equal(got[k], ref[k]), f"{k}: the structured case is not exact in fp32"
    return ref


def structured_catches(fn, args, drop, **kw):
    ref = exact32(fn, *args, **kw)
    got, _ = fn(*args, dtype=F32, drop=drop, **kw)
    assert any(not torch.equal(got[k], ref[k]) for k in ref), f"{drop[0]} left the structured result unchanged"


def pool_dout(kind, seed, B, Cc, out):
    """structured: 27 x integers, so that every quotient by a window of 2^a 3^b (b <= 3) voxels is exact"""
    v = p64.operands(kind, seed, B, Cc * out[0] * out[1] * out[2])
    return 27.0 * v if kind == "structured" else v


# ------------------------------------------------------------------------------------------------ 1. the fp32 stand-in lies within the bounds
def test_pure_moves_against_torch():
    sp = p64.specials()
    x = torch.cat([sp, torch.randn(4000, generator=p64.gen(3)) * 10.0 ** torch.randint(-30, 30, (4000,), generator=p64.gen(4)).float()])
    assert bool(p64.same_bits(p64.bf16_rne(x), x.to(BF16)).all()), "bf16_rne is not torch's round-to-nearest-even"
    assert float(p64.bf16_rne(torch.tensor([1.0 + 2.0 ** -8]))[0]) == 1.0 and float(p64.bf16_rne(torch.tensor([1.0 + 3 * 2.0 ** -8]))[0]) == 1.0 + 2.0 ** -6
    assert torch.isinf(p64.bf16_rne(torch.tensor([3.4028234663852886e38]))[0])
    assert bool(p64.same_bits(p64.cast(x.to(BF16), F32)[0]["dst"], x.to(BF16).float()).all())
    t = p64.operands("structured", 1, 3, 65, 70)
    assert torch.equal(p64.ncs_to_nsc(t)[0]["dst"], t.permute(0, 2, 1).contiguous()) and torch.equal(p64.nsc_to_ncs(p64.ncs_to_nsc(t)[0]["dst"])[0]["dst"], t)
    fl = p64.flatten_fwd(t)[0]["out"]                              # t as [B][V = 65][C = 70]
    assert torch.equal(fl, t.permute(0, 2, 1).reshape(3, -1))      # nn.Flatten on NC(D)HW
    mask = p64.operands("structured", 2, 3, 65, 70)
    mask[0, 0, 0] = -0.0
    dx = p64.flatten_bwd(fl, mask, 65, 70)[0]["dx"]
    assert torch.equal(dx, torch.where(mask > 0, t, torch.zeros_like(t))) and float(dx[0, 0, 0]) == 0.0
    pan = [p64.operands("random", s, 4, w) for s, w in ((1, 3), (2, 0), (3, 5))]
    wide = torch.full((4, 12), -1.0)
    w = p64.copy_panels(pan, wide, 2, 0)[0]["wide"]
    assert torch.equal(w[:, 2:10], torch.cat(pan, 1)) and bool((w[:, :2] == -1).all()) and bool((w[:, 10:] == -1).all())
    back = p64.copy_panels(pan, w, 2, 1)[0]
    assert all(torch.equal(back[f"p{i}"], pan[i]) for i in range(3))
    tt = torch.tensor([0, 4, -1, 5, 2])
    oh = p64.onehot_panel(tt, 5)[0]["dst"]
    assert torch.equal(oh[[0, 1, 4]], F.one_hot(tt[[0, 1, 4]], 5).float()) and float(oh[2].sum()) == 0.0 and float(oh[3].sum()) == 0.0
    y = p64.clamp_fwd(sp, -0.5, 0.75)[0]["y"]
    assert bool(p64.same_bits(y, torch.clamp(sp, -0.5, 0.75)).all()) and bool(torch.isnan(y[4])) and float(y[2]) == 0.75 and float(y[3]) == -0.5
    g = torch.arange(1.0, sp.numel() + 1)
    dx = p64.clamp_bwd(sp, g, -0.25, 0.75)[0]["dx"]
    assert float(dx[4]) == 0.0 and float(dx[-1]) == float(g[-1]) and float(dx[-2]) == float(g[-2]) and float(dx[2]) == 0.0      # NaN: no gradient; x == hi, x == lo pass


def test_act_fp32_within_bounds():
    for n in p64.N_ELEMENTWISE[:2] + [4099]:
        for act in p64.ACTS:
            for bf in (False, True):
                x = p64.act_input("random", 1, n)
                ratio("act_fwd", p64.act_fwd, p64.bf16(x) if bf else x, act, out_bf16=bf)
                dy, y = p64.operands("random", 2, n), p64.act_output("random", 5, n, act)
                if act != p64.NONE:
                    ratio("act_bwd", p64.act_bwd, p64.bf16(dy) if bf else dy, p64.bf16(y) if bf else y, act, out_bf16=bf)
    for act in (p64.NONE, p64.RELU, p64.LEAKY02, p64.LEAKY001):
        x = p64.act_input("structured", 1, 257)
        ref = exact32(p64.act_fwd, x, act)
        if act == p64.RELU:
            assert not bool(torch.signbit(ref["y"]).any())        # v > 0 ? v : 0 gives +0 for -0.0
        if act == p64.LEAKY02:
            assert bool(torch.signbit(ref["y"][-1]))               # 0.2f * -0.0 is -0.0
        exact32(p64.act_bwd, p64.operands("structured", 2, 257), p64.act_output("structured", 5, 257, act), act)


def test_channel_sum_fp32_within_bounds():
    for P, Cc, bf, _off, _why in p64.CHANNEL_SUM:
        x = p64.operands("random", 1, P, Cc)
        ratio("channel_sum", p64.channel_sum, p64.bf16(x) if bf else x)
        s = p64.operands("structured", 1, P, Cc)
        ref = exact32(p64.channel_sum, s)
        assert float(ref["out"].abs().max()) < 2 ** 24 and torch.equal(p64.bf16(s), s)


@pytest.mark.parametrize("case", p64.POOL, ids=lambda c: f"{c[1]}->{c[3]}".replace(" ", ""))
def test_pool_fp32_within_bounds(case):
    B, dims, Cc, out, _why = case
    for bf in (False, True):
        x = p64.operands("random", 1, B, *dims, Cc)
        x = p64.bf16(x) if bf else x
        ratio("pool_fwd", p64.pool_fwd, x, out)
        dout = pool_dout("random", 2, B, Cc, out)
        ratio("pool_bwd", p64.pool_bwd, dout, None, dims, out, out_bf16=bf)
        ratio("pool_bwd", p64.pool_bwd, dout, x, dims, out, out_bf16=bf)
    xs = p64.operands("structured", 1, B, *dims, Cc)
    ref, _ = p64.pool_fwd(xs, out)
    got, _ = p64.pool_fwd(xs, out, dtype=F32)
    assert torch.equal(got["out"], ref["out"].to(F32).to(F64))     # an exact sum and ONE correctly rounded division
    exact32(p64.pool_bwd, pool_dout("structured", 2, B, Cc, out), xs, dims, out)


def test_pool_windows_are_torch_s():
    for dims, out in (((1, 7, 7), (1, 3, 3)), ((5, 6, 9), (4, 4, 4)), ((1, 2, 2), (1, 7, 7)), ((1, 1, 1), (1, 3, 3)), ((2, 2, 1), (5, 5, 4))):
        x = torch.randn(2, *dims, 3, dtype=F64, generator=p64.gen(7), requires_grad=True)
        ref, _ = p64.pool_fwd(x, out)
        want = F.adaptive_avg_pool3d(x.permute(0, 4, 1, 2, 3), out)
        assert torch.allclose(ref["out"], want.reshape(2, -1), rtol=1e-13, atol=1e-13)
        g = torch.randn(2, 3 * out[0] * out[1] * out[2], dtype=F64, generator=p64.gen(8))
        want.reshape(2, -1).backward(g)
        assert torch.allclose(p64.pool_bwd(g, None, dims, out)[0]["dx"], x.grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("case", p64.RESIZE, ids=lambda c: f"{c[1]}->{c[3]}".replace(" ", ""))
def test_resize_fp32_within_bounds(case):
    B, dims, Cc, out, _why = case
    for bf in (False, True):
        src = p64.operands("random", 1, B, *dims, Cc)
        ratio("resize_fwd", p64.resize_fwd, p64.bf16(src) if bf else src, out)
        ratio("resize_bwd", p64.resize_bwd, p64.operands("random", 2, B, *out, Cc), dims, out_bf16=bf)


@pytest.mark.parametrize("dims,out", [((1, 3, 300), (1, 7, 420)), ((1, 8, 5), (1, 8, 1)), ((1, 16, 16), (1, 9, 11)), ((3, 5, 4), (8, 6, 9)), ((1, 4, 3), (1, 8, 6)),
                                      ((1, 16, 1), (1, 3, 5))])
def test_resize_tap_positions_moved_by_their_rounding(dims, out):
    """the float64 nest with every tap position moved by its eps_s, up or down, stays within the tap term of the bound: also where that flips a tap index"""
    src, g = p64.operands("random", 1, 2, *dims, 3), p64.operands("random", 2, 2, *out, 3)
    flips = 0
    for i, o in zip(dims, out):
        A, _dA, _e, dA2 = p64.taps(i, o)
        for sh in (-0.99, 0.99):                                   # (at +- 1 exactly the tap term is met with equality, up to float64's own rounding)
            flips += int((((p64.taps(i, o, shift=sh)[0] != 0) != (A != 0)).any(1)).sum())
        assert (dA2 is not None) == ((i, o) in ((3, 7), (300, 420), (8, 8), (5, 1))), (i, o)
    assert (flips > 0) == (dims[1:] in ((3, 300), (8, 5)))
    ref, err = p64.resize_fwd(src, out)
    refb, errb = p64.resize_bwd(g, dims)
    for sh in (-0.99, 0.99):                                   # (at +- 1 exactly the tap term is met with equality, up to float64's own rounding)
        assert not p64.compare(p64.resize_fwd(src, out, shift=sh)[0], ref, err)
        assert not p64.compare(p64.resize_bwd(g, dims, shift=sh)[0], refb, errb)
        ratio("resize_fwd", p64.resize_fwd, src, out)
        ratio("resize_bwd", p64.resize_bwd, g, dims)


def test_resize_2x_fp32_within_bounds():
    for B, dims, out, _why in p64.RESIZE_2X:
        ratio("resize2x_fwd", p64.resize_fwd, p64.operands("random", 1, B, *dims, 1), out)
        ratio("resize2x_bwd", p64.resize_bwd, p64.operands("random", 2, B, *out, 1), dims)
        # exact 2x: every weight is a multiple of 1 / 4 per axis, so integers times 64 stay exact
        exact32(p64.resize_fwd, 64.0 * p64.operands("structured", 1, B, *dims, 1), out)
        exact32(p64.resize_bwd, 64.0 * p64.operands("structured", 2, B, *out, 1), dims)


def test_resize_reference_is_f_interpolate_where_the_scales_agree():
    for dims, out in (((1, 5, 6), (1, 10, 12)), ((3, 5, 6), (6, 10, 12)), ((1, 8, 12), (1, 4, 6)), ((4, 6, 8), (2, 3, 4)), ((1, 8, 8), (1, 8, 8)), ((1, 4, 3), (1, 8, 6))):
        x = torch.randn(2, *dims, 3, dtype=F64, generator=p64.gen(9), requires_grad=True)
        ncdhw = x.permute(0, 4, 1, 2, 3)
        want = F.interpolate(ncdhw[:, :, 0], size=out[1:], mode="bilinear", align_corners=False)[:, :, None] if dims[0] == out[0] == 1 else \
            F.interpolate(ncdhw, size=out, mode="trilinear", align_corners=False)
        ref, _ = p64.resize_fwd(x, out)
        assert torch.allclose(ref["dst"], want.permute(0, 2, 3, 4, 1), rtol=1e-13, atol=1e-13)
        g = torch.randn(2, *out, 3, dtype=F64, generator=p64.gen(10))
        want.backward(g.permute(0, 4, 1, 2, 3))
        assert torch.allclose(p64.resize_bwd(g, dims)[0]["dsrc"], x.grad, rtol=1e-13, atol=1e-13)


def test_k3_k4_fp32_within_bounds_and_adjoint():
    for Cout, Cin in p64.K34:
        w3, g = p64.operands("random", 1, Cout, Cin, 3, 3), p64.operands("random", 2, Cin, Cout, 4, 4)
        ratio("k3_k4", p64.conv3_to_k4, w3)
        ratio("k3_k4", p64.k4_to_conv3_grad, g)
        k4, dw3 = p64.conv3_to_k4(w3)[0]["k4"], p64.k4_to_conv3_grad(g)[0]["dw3"]
        assert abs(float((k4 * g.double()).sum() - (w3.double() * dw3).sum())) < 1e-10 * float(k4.abs().sum())
        exact32(p64.conv3_to_k4, p64.operands("structured", 1, Cout, Cin, 3, 3))
        exact32(p64.k4_to_conv3_grad, p64.operands("structured", 2, Cin, Cout, 4, 4))
    # nearest x2 then a 3x3 / pad 1 cross-correlation IS the transposed k4 / s2 / p1 product with K4 = A W3 A^T
    x, w3 = torch.randn(1, 5, 4, 6, dtype=F64, generator=p64.gen(11)), torch.randn(3, 5, 3, 3, dtype=F64, generator=p64.gen(12))
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w3, padding=1)
    assert torch.allclose(F.conv_transpose2d(x, p64.conv3_to_k4(w3)[0]["k4"], stride=2, padding=1), want, rtol=1e-12, atol=1e-12)


def bn_args(c, training, act, running=True):
    return (c["x"], c["gamma"], c["beta"], c["rm"] if running else None, c["rv"] if running else None, 0.1, 1e-5, training, act)


def saved_stats(c, eps=1e-5):
    """mean and rstd as the forward leaves them: the float64 statistics rounded to fp32 (inputs of the eval forward and of the backward)"""
    ref, _ = p64.bn2d_fwd(*bn_args(c, 1, p64.NONE))
    return ref["mean"].to(F32), ref["rstd"].to(F32)


@pytest.mark.parametrize("Cc", p64.BN_C)
def test_bn2d_fp32_within_bounds(Cc):
    for P in p64.bn_P(Cc):
        for bf in (False, True):
            c = p64.bn_case("random", 1, P, Cc, bf)
            mean, rstd = saved_stats(c)
            for act in p64.ACTS:
                ratio("bn2d_fwd_train", p64.bn2d_fwd, *bn_args(c, 1, act, running=act != p64.LEAKY02), out_bf16=bf)
                ratio("bn2d_fwd_eval", p64.bn2d_fwd, *bn_args(c, 0, act), mean=mean, rstd=rstd, out_bf16=bf)
                y = p64.act_output("random", 5, P * Cc, act)
                y = None if y is None else (p64.bf16(y) if bf else y).reshape(P, Cc)
                ratio("bn2d_bwd", p64.bn2d_bwd, c["x"], c["dy"], c["x"] if y is None else y, c["gamma"], mean, rstd, act, out_bf16=bf)


def test_bn2d_reference_is_torch_batch_norm():
    c = p64.bn_case("random", 1, 37, 8)
    x = c["x"].double().clone().requires_grad_(True)
    gamma = c["gamma"].double().clone().requires_grad_(True)
    rm, rv = c["rm"].double().clone(), c["rv"].double().clone()
    mom, eps = p64.f32(0.1), p64.f32(1e-5)
    y = F.batch_norm(x, rm, rv, gamma, c["beta"].double(), True, mom, eps)
    ref, _ = p64.bn2d_fwd(*bn_args(c, 1, p64.NONE))
    for k, v in (("y", y), ("running_mean", rm), ("running_var", rv)):
        assert torch.allclose(ref[k], v, rtol=1e-11, atol=1e-11), k
    y.backward(c["dy"].double())
    b, _ = p64.bn2d_bwd(c["x"], c["dy"], c["x"], c["gamma"], ref["mean"], ref["rstd"], p64.NONE)
    assert torch.allclose(b["dx"], x.grad, rtol=1e-9, atol=1e-9) and torch.allclose(b["dgamma"], gamma.grad, rtol=1e-10, atol=1e-10)
    assert torch.allclose(b["dbeta"], c["dy"].double().sum(0), rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. every mutation is rejected
def test_every_mutation_is_named():
    assert set(p64._MUTATIONS) == {"last_row", "unclipped_div", "pm1", "align_corners", "swap_taps", "biased_running_var", "one_pass_var", "dx_no_dgamma", "tile_edge",
                                   "bf16_trunc"}
    with pytest.raises(ValueError):
        p64.channel_sum(torch.ones(3, 4), drop=("no_such",))


def test_fault_channel_sum_without_its_last_row():
    for P, Cc, bf, _off, _why in p64.CHANNEL_SUM:
        x = p64.operands("random", 1, P, Cc)
        x = p64.bf16(x) if bf else x
        ref, err = p64.channel_sum(x)
        got, _ = p64.channel_sum(x, dtype=F32, drop=("last_row",))
        if Cc > 1 or P <= 4096:                                  # 66560 x 1: ONE output, whose bound (sqrt(P) of it) hides one element: the structured case's
            rejected(got, ref, err)
        else:
            assert float(p64.operands("structured", 1, P, Cc)[-1]) != 0
        if P <= 7000 and Cc > 1:
            assert float(((got["out"] - ref["out"]).abs() > err["out"]).double().mean()) > 0.5
        s = p64.operands("structured", 1, P, Cc)
        if bool((s[-1] != 0).any()):                             # (1 x 19: an all-zero result is still wrong wherever the row is not 0)
            structured_catches(p64.channel_sum, (s,), ("last_row",))
    s = p64.operands("structured", 1, 16385, 1028)
    ref, _ = p64.channel_sum(s)
    got, _ = p64.channel_sum(s, dtype=F32, drop=("last_row",))
    assert bool(((got["out"] != ref["out"]) == (s[-1] != 0)).all()) and float((s[-1] != 0).double().mean()) > 0.7


def test_fault_pool_divisor_from_the_unclipped_window():
    for B, dims, Cc, out, _why in p64.POOL[:3]:
        x = p64.operands("random", 1, B, *dims, Cc)
        ref, err = p64.pool_fwd(x, out)
        got, _ = p64.pool_fwd(x, out, dtype=F32, drop=("unclipped_div",))
        if dims == (1, 8, 8):
            assert not p64.compare(got, ref, err)
        else:
            rejected(got, ref, err)
            xs = p64.operands("structured", 1, B, *dims, Cc)
            assert not torch.equal(p64.pool_fwd(xs, out, dtype=F32, drop=("unclipped_div",))[0]["out"], p64.pool_fwd(xs, out, dtype=F32)[0]["out"])


def test_fault_the_shipped_candidate_rule_of_the_pool_backward():
    """the parent's rule (windows among floor(i O / I) - 1 .. + 1) loses terms at 1 -> 3, 2 -> 7, 2 -> 5 / 1 -> 4 and is complete at every O <= I"""
    hit = 0
    for B, dims, Cc, out, _why in p64.POOL:
        for kind in KINDS:
            dout = pool_dout(kind, 2, B, Cc, out)
            ref, err = p64.pool_bwd(dout, None, dims, out)
            assert not p64.compare(p64.pool_bwd(dout, None, dims, out, dtype=F32)[0], ref, err)                 # the new rule: accepted
            got, _ = p64.pool_bwd(dout, None, dims, out, dtype=F32, drop=("pm1",))
            if (B, dims, Cc, out, _why) in p64.POOL_LEGACY_COMPLETE:
                assert torch.equal(got["dx"], p64.pool_bwd(dout, None, dims, out, dtype=F32)[0]["dx"])          # not one bit changes where O <= I
            elif any(o >= 3 * i for i, o in zip(dims, out)):
                rejected(got, ref, err)
                hit += 1
            else:
                assert torch.equal(got["dx"], p64.pool_bwd(dout, None, dims, out, dtype=F32)[0]["dx"])          # 3 -> 4: at most two windows, both among the candidates
    assert hit == 6 and len(p64.POOL_LEGACY_COMPLETE) == 4
    # the arithmetic of the parent's kernel itself, replayed: at 1 -> 3 the voxel's candidates are o = 0, 1 of 3 windows; at 2 -> 7 voxel 0 has windows 0 .. 3, candidates 0, 1
    for I, O, i, windows, cands in ((1, 3, 0, [0, 1, 2], [0, 1]), (2, 7, 0, [0, 1, 2, 3], [0, 1]), (2, 7, 1, [3, 4, 5, 6], [2, 3, 4]), (8, 4, 3, [1], [0, 1, 2])):
        wn = p64.windows(I, O)
        assert [o for o in range(O) if wn[o][0] <= i < wn[o][1]] == windows == list(range((i * O) // I, -((-(i + 1) * O) // I)))
        assert [o for o in range(O) if abs(o - (i * O) // I) <= 1] == cands


def test_the_window_range_is_exact_for_every_pair():
    for I in range(1, 25):
        for O in list(range(1, 70)) + [128, 257]:
            wn = p64.windows(I, O)
            for i in range(I):
                assert [o for o in range(O) if wn[o][0] <= i < wn[o][1]] == list(range((i * O) // I, ((i + 1) * O - 1) // I + 1)), (I, O, i)


RESIZE_FAULT = [p64.RESIZE[0], p64.RESIZE[5], (2, (1, 5, 6), 1, (1, 10, 12), "exact 2x")]


@pytest.mark.parametrize("mut", ["align_corners", "swap_taps"])
def test_fault_resize_taps(mut):
    for B, dims, Cc, out, _why in RESIZE_FAULT:
        src, g = p64.operands("random", 1, B, *dims, Cc), p64.operands("random", 2, B, *out, Cc)
        ref, err = p64.resize_fwd(src, out)
        rejected(p64.resize_fwd(src, out, dtype=F32, drop=(mut,))[0], ref, err)
        ref, err = p64.resize_bwd(g, dims)
        rejected(p64.resize_bwd(g, dims, dtype=F32, drop=(mut,))[0], ref, err)
    src = p64.operands("random", 1, 2, 1, 8, 8, 3)                  # the identity: align_corners is the same map there
    ref, err = p64.resize_fwd(src, (1, 8, 8))
    assert not p64.compare(p64.resize_fwd(src, (1, 8, 8), dtype=F32, drop=("align_corners",))[0], ref, err)


def test_fault_bn2d_statistics():
    for P in (3, 4097):
        c = p64.bn_case("random", 1, P, 8)
        ref, err = p64.bn2d_fwd(*bn_args(c, 1, p64.NONE))
        got, _ = p64.bn2d_fwd(*bn_args(c, 1, p64.NONE), dtype=F32, drop=("biased_running_var",))
        rejected(got, ref, err, ["running_var"])
        assert not p64.compare(got, ref, err, ["y", "mean", "rstd", "running_mean"])
    caught = 0
    for Cc in p64.BN_C:                                          # every shape of the GPU file
        for P in p64.bn_P(Cc):
            c = p64.bn_case("random", 1, P, Cc)
            ref, err = p64.bn2d_fwd(*bn_args(c, 1, p64.NONE))
            got, _ = p64.bn2d_fwd(*bn_args(c, 1, p64.NONE), dtype=F32, drop=("one_pass_var",))
            r = (got["rstd"] - ref["rstd"]).abs() / err["rstd"]
            print(f"ONE_PASS {P} x {Cc}: channel 1 at {float(r[1]):.2f} bounds, the ordinary channels at most {float(torch.cat([r[:1], r[3:]]).max()):.2f}")
            caught += float(r[1]) > 1.0
            if P <= 255:                                         # the two-pass bound grows like sqrt(P) |mean| U rstd: at P in the thousands a one-pass variance fits into it
                assert float(r[1]) > 1.0, (P, Cc)
                rejected(got, ref, err, ["rstd"])
                rejected(got, ref, err, ["y"])
            if P >= 50:
                assert float(torch.cat([r[:1], r[3:]]).max()) < 0.1  # the ordinary channels cannot tell the two variances apart: that is why channel 1 is there
    assert caught >= 17


def test_fault_bn2d_dx_without_its_dgamma_term():
    for P, Cc in ((3, 8), (84, 24), (4097, 8)):
        c = p64.bn_case("random", 1, P, Cc)
        mean, rstd = saved_stats(c)
        args = (c["x"], c["dy"], c["x"], c["gamma"], mean, rstd, p64.NONE)
        ref, err = p64.bn2d_bwd(*args)
        got, _ = p64.bn2d_bwd(*args, dtype=F32, drop=("dx_no_dgamma",))
        rejected(got, ref, err, ["dx"])
        assert not p64.compare(got, ref, err, ["dgamma", "dbeta"])


def test_fault_tile_edge_dropped():
    for Cc, S in ((65, 63), (63, 65), (130, 200), (65, 65)):
        x = p64.operands("structured", 1, 2, Cc, S, lo=1, hi=5)
        for fn in (p64.ncs_to_nsc, p64.nsc_to_ncs):
            assert not bool(p64.same_bits(fn(x, drop=("tile_edge",))[0]["dst"], fn(x)[0]["dst"]).all())
        assert not torch.equal(p64.flatten_fwd(x, drop=("tile_edge",))[0]["out"], p64.flatten_fwd(x)[0]["out"])
        g = p64.flatten_fwd(x)[0]["out"]
        assert not torch.equal(p64.flatten_bwd(g, None, Cc, S, drop=("tile_edge",))[0]["dx"], p64.flatten_bwd(g, None, Cc, S)[0]["dx"])
    x = p64.operands("structured", 1, 2, 64, 64, lo=1, hi=5)
    assert torch.equal(p64.ncs_to_nsc(x, drop=("tile_edge",))[0]["dst"], p64.ncs_to_nsc(x)[0]["dst"])


def test_fault_bf16_truncation():
    sp = p64.specials()
    t, r = p64.cast(sp, BF16, drop=("bf16_trunc",))[0]["dst"], p64.cast(sp, BF16)[0]["dst"]
    same = p64.same_bits(t, r)
    assert not bool(same[11]) and not bool(same[13]) and not bool(same[14]) and bool(same[10])       # 1 + 3/256 (tie, odd) and above a tie round up; 1 + 1/256 (tie, even) down
    x = p64.operands("random", 1, 2, 65, 70)
    for fn in (p64.ncs_to_nsc, p64.nsc_to_ncs):
        assert float(p64.same_bits(fn(x, BF16, drop=("bf16_trunc",))[0]["dst"], fn(x, BF16)[0]["dst"]).double().mean()) < 0.6
    g = p64.flatten_fwd(x)[0]["out"]
    assert float(p64.same_bits(p64.flatten_bwd(g, None, 65, 70, BF16, drop=("bf16_trunc",))[0]["dx"], p64.flatten_bwd(g, None, 65, 70, BF16)[0]["dx"]).double().mean()) < 0.6


# ------------------------------------------------------------------------------------------------ 3. the reference's own assertions
def test_branch_margins_are_asserted():
    dy = p64.operands("random", 1, 64)
    y = p64.act_output("random", 5, 64, p64.RELU)
    y[7] = 2.0 ** -8
    for act in (p64.RELU, p64.LEAKY02, p64.LEAKY001):
        with pytest.raises(AssertionError):
            p64.act_bwd(dy, y, act)
        with pytest.raises(AssertionError):
            p64.bn2d_bwd(dy.reshape(8, 8), dy.reshape(8, 8), y.reshape(8, 8), torch.ones(8), torch.zeros(8), torch.ones(8), act)
    p64.act_bwd(dy, y, p64.SIGMOID)                                # no branch: no assertion
    with pytest.raises(AssertionError):
        p64.act_fwd(torch.tensor([0.5, 8.5]), p64.SIGMOID)
    p64.act_fwd(torch.tensor([0.5, 8.0, -8.0]), p64.SIGMOID)
    with pytest.raises(AssertionError):
        p64.bn2d_fwd(torch.tensor([[30.0] * 8, [-30.0] * 8]), 9.0 * torch.ones(8), torch.zeros(8), None, None, 0.1, 1e-5, 1, p64.SIGMOID)
    for act in (p64.RELU, p64.LEAKY02, p64.LEAKY001):
        v = p64.act_output("random", 9, 4096, act)
        assert bool(((v == 0) | (v.abs() >= p64.BRANCH_MARGIN)).all()) and bool((v > 0).any()) and bool((v < 0).any() or act == p64.RELU)
        assert bool((v == 0).any()) and bool(torch.signbit(v[v == 0]).any())


# ------------------------------------------------------------------------------------------------ 4. argument checks before any launch
HAS_DEVICE = torch.cuda.is_available()
needs_no_device = pytest.mark.skipif(HAS_DEVICE, reason="host pointers stand in for device memory: only where no launch can succeed")
OK, BADSHAPE, DTYPE, UNSUPPORTED, WORKSPACE, LAUNCH, NULLPTR = 0, -1, -2, -3, -4, -5, -6

_buf = (C.c_float * (1 << 14))(*([3.25] * (1 << 14)))           # never read or written through: no launch succeeds here
P = (C.addressof(_buf) + 15) & ~15
_panels = (C.c_void_p * 3)(P, P, P)
_panels_hole = (C.c_void_p * 3)(P, None, P)
_widths = (C.c_int64 * 3)(3, 0, 5)
_widths_neg = (C.c_int64 * 3)(3, -1, 5)
_strides = (C.c_int64 * 3)(4, 0, 5)
_strides_short = (C.c_int64 * 3)(2, 0, 5)
_widths_hole = (C.c_int64 * 3)(3, 2, 5)
_strides_hole = (C.c_int64 * 3)(4, 2, 5)


def A(arr):
    return C.cast(arr, C.c_void_p)


def R(*pos):
    return [({i: None}, NULLPTR) for i in pos]


BN_WS = 2 * 1 * 8 * 4                                           # cvae_bn2d_workspace_bytes(64, 8): one row block
# entry point -> (valid arguments, [({position: value}, expected code)])
CHECKS = {
    # src, dst, n, src_dtype, dst_dtype, stream
    "cvae_cast": ((P, P, 100, 0, 1, None), R(0, 1) + [({2: -1}, BADSHAPE), ({2: 0}, OK), ({2: 0, 0: None}, OK), ({3: 2}, DTYPE), ({4: 2}, DTYPE), ({3: -1}, DTYPE), ({4: 7}, DTYPE)]),
    # src, dst, B, C, S, src_dtype, dst_dtype, stream
    "cvae_ncs_to_nsc": ((P, P, 2, 65, 63, 0, 1, None),
                        R(0, 1) + [({2: -1}, BADSHAPE), ({3: 0}, BADSHAPE), ({3: -1}, BADSHAPE), ({4: -1}, BADSHAPE), ({2: 0}, OK), ({4: 0}, OK), ({2: 65536}, BADSHAPE),
                                   ({2: 65535}, LAUNCH), ({3: 1}, LAUNCH), ({3: 1, 2: 65536}, LAUNCH), ({5: 2}, DTYPE), ({6: 2}, DTYPE), ({3: 1, 5: 2}, DTYPE)]),
    "cvae_nsc_to_ncs": ((P, P, 2, 65, 63, 1, 0, None),
                        R(0, 1) + [({2: -1}, BADSHAPE), ({3: 0}, BADSHAPE), ({4: -1}, BADSHAPE), ({2: 0}, OK), ({4: 0}, OK), ({2: 65536}, BADSHAPE), ({3: 1}, LAUNCH),
                                   ({5: 2}, DTYPE), ({6: 3}, DTYPE)]),
    # panels, widths, strides, count, wide, B, wide_stride, col0, gather, stream (the first three are HOST arrays)
    "cvae_copy_panels": ((A(_panels), A(_widths), A(_strides), 3, P, 4, 12, 2, 0, None),
                         R(0, 1, 2, 4) + [({3: 0}, BADSHAPE), ({3: 9}, BADSHAPE), ({5: -1}, BADSHAPE), ({7: -1}, BADSHAPE), ({1: A(_widths_neg)}, BADSHAPE),
                                          ({2: A(_strides_short)}, BADSHAPE), ({6: 9}, BADSHAPE), ({6: 10}, LAUNCH), ({5: 0}, OK), ({8: 1}, LAUNCH), ({0: A(_panels_hole)}, LAUNCH),
                                          ({0: A(_panels_hole), 1: A(_widths_hole), 2: A(_strides_hole), 6: 20}, NULLPTR),
                                          ({0: A(_panels_hole), 1: A(_widths_hole), 2: A(_strides_hole), 6: 20, 5: 0}, OK), ({3: 1, 6: 5}, LAUNCH)]),
    # t, dst, B, n_classes, dst_stride, col0, stream
    "cvae_onehot_panel": ((P, P, 4, 19, 30, 5, None),
                          R(0, 1) + [({2: -1}, BADSHAPE), ({3: 0}, BADSHAPE), ({5: -1}, BADSHAPE), ({4: 23}, BADSHAPE), ({4: 24}, LAUNCH), ({2: 0}, OK), ({2: 0, 0: None}, OK)]),
    # x, y, n, act, dtype, stream
    "cvae_act_fwd": ((P, P, 100, 4, 0, None), R(0, 1) + [({2: -1}, BADSHAPE), ({2: 0}, OK), ({4: 2}, DTYPE), ({4: 1}, LAUNCH), ({3: 0}, LAUNCH)]),
    # dy, y, dx, n, act, dtype, stream
    "cvae_act_bwd": ((P, P, P, 100, 2, 1, None), R(0, 1, 2) + [({3: -1}, BADSHAPE), ({3: 0}, OK), ({5: 2}, DTYPE), ({5: 0}, LAUNCH)]),
    # x, out, P, C, dtype, workspace, workspace_bytes, stream
    "cvae_channel_sum": ((P, P, 300, 12, 0, None, 0, None),
                         R(0, 1) + [({2: -1}, BADSHAPE), ({3: 0}, BADSHAPE), ({3: -1}, BADSHAPE), ({4: 2}, DTYPE), ({4: 1}, LAUNCH), ({5: P, 6: 4}, LAUNCH), ({5: P, 6: 1 << 16}, LAUNCH),
                                    ({0: P + 4}, LAUNCH), ({2: 0, 1: None}, NULLPTR), ({3: 1}, LAUNCH), ({3: 19}, LAUNCH), ({3: 256 * 65536 + 1}, BADSHAPE), ({3: 256 * 65536}, LAUNCH)]),
    # x, out, B, D, H, W, C, OD, OH, OW, out_stride, dtype, stream
    "cvae_adaptive_avgpool_fwd": ((P, P, 2, 1, 7, 7, 4, 1, 3, 3, 40, 0, None),
                                  R(0, 1) + [({i: 0}, BADSHAPE) for i in range(3, 10)] + [({2: -1}, BADSHAPE), ({2: 0}, OK), ({10: 35}, BADSHAPE), ({10: 36}, LAUNCH),
                                                                                            ({11: 2}, DTYPE), ({11: 1}, LAUNCH), ({8: 7, 9: 7, 10: 196}, LAUNCH),
                                                                                            ({8: 7, 9: 7, 10: 196, 11: 2}, DTYPE), ({8: 7, 9: 7, 10: 195}, BADSHAPE)]),
    # dout, relu_mask_x, dx, B, D, H, W, C, OD, OH, OW, dout_stride, dtype, stream
    "cvae_adaptive_avgpool_bwd": ((P, None, P, 2, 1, 2, 2, 3, 1, 7, 7, 150, 0, None),
                                  R(0, 2) + [({i: 0}, BADSHAPE) for i in range(4, 11)] + [({3: -1}, BADSHAPE), ({3: 0}, OK), ({11: 146}, BADSHAPE), ({11: 147}, LAUNCH),
                                                                                            ({1: P}, LAUNCH), ({12: 2}, DTYPE), ({12: 1}, LAUNCH), ({9: 2, 10: 2, 11: 12}, LAUNCH),
                                                                                            ({9: 2, 10: 2, 11: 11}, BADSHAPE)]),
    # src, dst, B, d, h, w, D, H, W, C, dtype, stream
    "cvae_upsample_linear_fwd": ((P, P, 2, 1, 16, 16, 1, 9, 11, 3, 0, None),
                                 R(0, 1) + [({i: 0}, BADSHAPE) for i in range(3, 10)] + [({2: -1}, BADSHAPE), ({2: 0}, OK), ({10: 2}, DTYPE), ({10: 1}, LAUNCH),
                                                                                           ({4: 1, 5: 2, 7: 2, 8: 4, 9: 1}, LAUNCH), ({4: 1, 5: 2, 7: 2, 8: 4, 9: 1, 10: 2}, DTYPE)]),
    "cvae_upsample_linear_bwd": ((P, P, 2, 1, 16, 16, 1, 9, 11, 3, 1, None),
                                 R(0, 1) + [({i: 0}, BADSHAPE) for i in range(3, 10)] + [({2: -1}, BADSHAPE), ({2: 0}, OK), ({10: 2}, DTYPE), ({10: 0}, LAUNCH),
                                                                                           ({4: 1, 5: 2, 7: 2, 8: 4, 9: 1}, LAUNCH)]),
    # w3, k4, Cout, Cin, stream
    "cvae_conv3_to_k4": ((P, P, 17, 16, None), R(0, 1) + [({2: 0}, BADSHAPE), ({3: 0}, BADSHAPE), ({2: -1}, BADSHAPE), ({2: 1 << 14, 3: (1 << 14) + 1}, BADSHAPE), ({2: 1, 3: 1}, LAUNCH)]),
    "cvae_k4_to_conv3_grad": ((P, P, 17, 16, None), R(0, 1) + [({2: 0}, BADSHAPE), ({3: 0}, BADSHAPE), ({3: -1}, BADSHAPE), ({2: 1 << 14, 3: (1 << 14) + 1}, BADSHAPE), ({2: 1, 3: 1}, LAUNCH)]),
    # x, y, lo, hi, n, stream
    "cvae_clamp_fwd": ((P, P, 0.0, 1.0, 100, None), R(0, 1) + [({4: -1}, BADSHAPE), ({4: 0}, OK), ({4: 0, 0: None}, OK)]),
    # x, g, dx, lo, hi, n, stream
    "cvae_clamp_bwd": ((P, P, P, 0.0, 1.0, 100, None), R(0, 1, 2) + [({5: -1}, BADSHAPE), ({5: 0}, OK)]),
    # x, gamma, beta, y, mean, rstd, running_mean, running_var, P, C, momentum, eps, training, act, dtype, workspace, workspace_bytes, stream
    "cvae_bn2d_fwd": ((P, P, P, P, P, P, P, P, 64, 8, 0.1, 1e-5, 1, 1, 0, P, BN_WS, None),
                      R(0, 1, 2, 3, 4, 5, 15) + [({6: None}, LAUNCH), ({7: None}, LAUNCH), ({6: None, 7: None}, LAUNCH), ({8: 0}, BADSHAPE), ({8: 1}, BADSHAPE), ({8: 1, 12: 0}, LAUNCH),
                                                 ({8: 2}, LAUNCH), ({9: 0}, BADSHAPE), ({9: 4}, BADSHAPE), ({9: 12}, BADSHAPE), ({9: 2056}, BADSHAPE), ({9: 2048, 16: 1 << 15}, LAUNCH), ({9: 2048, 16: (1 << 15) - 4}, WORKSPACE),
                                                 ({16: BN_WS // 2}, LAUNCH), ({16: BN_WS // 2 - 4}, WORKSPACE), ({16: 0}, WORKSPACE), ({12: 0, 15: None, 16: 0}, LAUNCH),
                                                 ({14: 2}, DTYPE), ({14: 1}, LAUNCH)]),
    # x, dy, y, gamma, mean, rstd, dx, dgamma, dbeta, P, C, act, dtype, workspace, workspace_bytes, stream
    "cvae_bn2d_bwd": ((P, P, P, P, P, P, P, P, P, 64, 8, 1, 0, P, BN_WS, None),
                      R(0, 1, 2, 3, 4, 5, 6, 7, 8, 13) + [({9: 0}, BADSHAPE), ({9: 1}, LAUNCH), ({10: 0}, BADSHAPE), ({10: 12}, BADSHAPE), ({10: 2056}, BADSHAPE),
                                                          ({14: BN_WS - 4}, WORKSPACE), ({14: BN_WS // 2}, WORKSPACE), ({14: 0}, WORKSPACE), ({12: 2}, DTYPE), ({12: 1}, LAUNCH)]),
}
VALUES = {
    "cvae_channel_sum_workspace_bytes": [((0, 12, 0), 0), ((300, 0, 0), 0), ((-1, 12, 0), 0), ((340, 12, 0), 0), ((70, 1024, 0), 3 * 1024 * 4), ((16385, 1028, 0), 512 * 1028 * 4),
                                         ((2000, 19, 0), 3 * 19 * 4), ((130, 257, 0), 3 * 257 * 4), ((300, 64, 0), 2 * 64 * 4), ((66560, 1, 0), 5 * 4)],
    "cvae_bn2d_workspace_bytes": [((0, 8), 0), ((64, 4), 0), ((64, 12), 0), ((64, 2056), 0), ((64, 8), BN_WS), ((4097, 8), 2 * 2 * 8 * 4), ((16385, 2048), 2 * 1024 * 2048 * 4),
                                  ((17, 2048), 2 * 2 * 2048 * 4)],
}
FLAT = [(name, k) for name, (_a, muts) in CHECKS.items() for k in range(len(muts))]


@needs_no_device
@pytest.mark.parametrize("name", list(CHECKS))
def test_valid_arguments_reach_the_launch(name):
    from causal_vae_amd import _lib
    args, _ = CHECKS[name]
    assert len(args) == len(_lib.SIGNATURES[name])
    assert getattr(_lib.lib, name)(*args) == LAUNCH, f"{name}: the arguments are not otherwise valid"


@needs_no_device
@pytest.mark.parametrize("name,k", FLAT, ids=[f"{n}-{k}" for n, k in FLAT])
def test_argument_check(name, k):
    from causal_vae_amd import _lib
    args, muts = CHECKS[name]
    change, want = muts[k]
    bad = list(args)
    for i, v in change.items():
        bad[i] = v
    before = bytes(_buf)
    assert getattr(_lib.lib, name)(*bad) == want, f"{name} with {change}"
    assert bytes(_buf) == before                                  # no buffer written


@pytest.mark.parametrize("name", list(VALUES))
def test_value_entry_points(name):
    from causal_vae_amd import _lib
    for args, want in VALUES[name]:
        assert getattr(_lib.lib, name)(*args) == want, f"{name}{args}"


def test_the_table_names_every_entry_point_of_both_files():
    from causal_vae_amd import _lib
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    entries = set()
    for f in ("elementwise.hip", "vessel2d.hip"):
        entries |= set(re.findall(r'extern "C" (?:int|size_t) (cvae_\w+)\(', open(os.path.join(csrc, f)).read()))
    assert len(entries) == 20 and entries == set(CHECKS) | set(VALUES)


def test_the_header_states_what_the_code_checks():
    from causal_vae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    text = " ".join(open(os.path.join(root, "include", "cvae_hip.h")).read().split())
    for s in ("8 <= C <= 2048", "training: P >= 2", "16-byte aligned", "either may be NULL, each on its own", "satisfied with half", "sum over windows containing (d, h, w)",
              "torch.clamp(x, lo, hi)"):
        assert s in text.replace(" * ", " "), s


# ------------------------------------------------------------------------------------------------ 5. the advertised workspace covers every path
def test_the_replayed_geometry_is_the_one_the_tables_name():
    g = p64.channel_sum_geometry
    assert g(340, 12)["rows"] == 85 and g(340, 12)["groups"] == 3 and g(340, 12)["gx"] == 1 and g(7000, 12)["gx"] == 3
    assert g(204, 40, True)["rows"] == 51 and g(204, 40, True)["groups"] == 5
    assert g(9, 1024)["rows"] == 1 and g(70, 1024)["gx"] == 3 and g(9, 1028)["gy"] == 2
    assert g(16385, 1028) == dict(path="vec", fold=0, gx=512, gy=2, rows=1, groups=257, ws_floats=512 * 1028)
    assert g(4096, 1)["fold"] == 1 and g(66560, 1)["gx"] == 3 and g(66560, 1)["ws_floats"] == 3 and g(16, 1, True)["fold"] == 1
    assert g(1001, 1)["path"] == "scalar" and g(1001, 1)["rows"] == 256
    assert g(50, 19)["rows"] == 13 and 50 < 8 * 13 and g(2000, 19)["gx"] == 3 and g(130, 257)["gy"] == 2 and g(130, 257)["gx"] == 3
    assert g(300, 64)["path"] == "vec" and g(300, 64, aligned=False) == dict(path="scalar", fold=0, gx=2, gy=1, rows=4, groups=0, ws_floats=128)
    for P, rem in ((340, {0}), (428, {1, 2}), (600, {0, 3})):     # trips of a thread's row walk modulo the 4-deep loop
        assert {len(range(ri, P, 85)) % 4 for ri in range(85)} == rem
    for P, rem in ((204, {0}), (260, {1, 2}), (359, {0, 3})):
        assert {len(range(ri, P, 51)) % 4 for ri in range(51)} == rem
    assert [p64.bn2d_blocks(1, c)[1] for c in p64.BN_C] == [256, 85, 51, 7, 1]
    assert p64.bn_P(8) == [2, 3, 255, 4097] and p64.bn_P(2048) == [2, 3, 17] and p64.bn_P(264) == [2, 3, 6, 113]
    assert all(p64.bn2d_blocks(16 * p64.bn2d_blocks(1, c)[1] + 1, c)[0] == 2 for c in p64.BN_C)
    assert -(-p64.BN_CAP[0] // 16) == 1025 and p64.bn2d_blocks(*p64.BN_CAP)[0] == 1024
    assert p64.grid_1d(p64.N_ELEMENTWISE[2]) == 2048 and p64.N_ELEMENTWISE[2] > 2048 * 256
    B, dims, Cc, out, _ = p64.POOL[-1]
    assert B * Cc * out[1] * out[2] > 2048 * 256 and B * Cc * dims[1] * dims[2] > 2048 * 256
    assert all(b * c * max(d[0] * d[1] * d[2], o[0] * o[1] * o[2]) > 2048 * 256 for b, d, c, o, _ in p64.RESIZE[-2:])
    b, d, o = p64.RESIZE_2X_BIG_FWD
    assert b * o[0] * o[1] * o[2] // 4 > 8192 * 256 and o[2] % 4 == 0 and b * o[0] * o[1] * o[2] * 4 < 36e6
    b, d, o = p64.RESIZE_2X_BIG_BWD
    assert b * d[0] * d[1] * d[2] > 8192 * 256 and o[2] % 4 == 0 and b * o[0] * o[1] * o[2] * 4 < 68e6
    assert 17 * 16 == 272 > 256


def test_workspace_bytes_cover_every_path():
    from causal_vae_amd import _lib
    adv = _lib.lib.cvae_channel_sum_workspace_bytes
    split = 0
    for P, Cc, bf, _off, _why in p64.CHANNEL_SUM:
        for aligned in (True, False):
            need = 4 * p64.channel_sum_geometry(P, Cc, bf, aligned)["ws_floats"]
            split += need > 0
            assert adv(P, Cc, 1 if bf else 0) >= need, (P, Cc, bf, aligned)
    assert split >= 12
    adv = _lib.lib.cvae_bn2d_workspace_bytes
    for Cc in p64.BN_C:
        for P in p64.bn_P(Cc) + [p64.BN_CAP[0]]:
            assert adv(P, Cc) == 4 * p64.bn2d_workspace_floats(P, Cc, True) == 8 * p64.bn2d_workspace_floats(P, Cc, False)


def test_zz_worst_ratios():
    for k in sorted(WORST):
        print(f"WORST {k} {WORST[k]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
