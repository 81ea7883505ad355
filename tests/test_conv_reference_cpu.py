"""CPU self-tests of oracle/conv64.py, the float64 reference tests/test_conv_reference.py compares the k4 / s2 / p1 convolution kernels with.

For every case family of the GPU file (at reduced size): a plain fp32 aten evaluation of the same product — rounded to bf16 for a bf16 result, to e4m3 for
an fp8 code result — lies within the bound, and each deliberately wrong variant of the product (conv64._MUTATIONS, plus a bf16 result scaled by
1 +- 2^-7) does NOT: a comparison that let those pass would let a subtly wrong kernel pass.  The ReLU-bit cases must leave at most 0.1 % of their
elements undecided.

max |stand-in - ref| / err of the fp32 aten stand-in, as printed by test_fp32_aten_standin_is_within_the_bound (CPU, this file):
  down 0.004 - 0.16, up 0.013 - 0.07, wgrad dW 0.007 - 0.11, dbias <= 0.008; rounded to bf16 / e4m3 as the kernels store it 0.92 - 0.999 (the half ulp of
  the stored value is nearly the whole bound then)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import conv64 as c64  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
# family id -> make_case arguments (kind, seed, nd, B, Cl, Cs, size, dtype) + options; the same families, at full size, in tests/test_conv_reference.py
FAMILIES = {
    "down3d-f32": (("down", 11, 3, 2, 32, 64, (8, 6, 10), F32), dict(masked=True)),
    "down3d-bf16": (("down", 12, 3, 1, 128, 64, (4, 6, 4), BF16), {}),
    "down3d-odd": (("down", 13, 3, 1, 32, 64, (9, 8, 11), BF16), {}),
    "down2d-f32": (("down", 14, 2, 3, 48, 64, (14, 10), F32), {}),
    "down2d-bf16": (("down", 15, 2, 3, 96, 128, (7, 9), BF16), dict(masked=True)),
    "down-c1-3d": (("down", 16, 3, 2, 1, 32, (8, 8, 16), BF16), {}),
    "down-c1-2d-f32": (("down", 17, 2, 2, 1, 32, (12, 20), F32), {}),
    "up3d-f32": (("up", 21, 3, 2, 64, 32, (3, 4, 5), F32), {}),
    "up3d-bf16": (("up", 22, 3, 1, 64, 128, (4, 3, 4), BF16), dict(masked=True)),
    "up3d-odd": (("up", 23, 3, 1, 32, 64, (4, 4, 5), BF16), dict(odd_l=True)),
    "up2d-bf16-32ch": (("up", 24, 2, 3, 96, 64, (7, 7), BF16), {}),
    "up2d-f32-odd": (("up", 25, 2, 2, 64, 64, (3, 6), F32), dict(odd_l=True)),
    "up-c1-3d": (("up", 26, 3, 2, 1, 32, (4, 5, 9), BF16), {}),
    "wgrad3d-f32": (("wgrad", 31, 3, 2, 32, 64, (4, 4, 5), F32), {}),
    "wgrad3d-bf16": (("wgrad", 32, 3, 3, 64, 64, (8, 8, 8), BF16), {}),
    "wgrad2d-bf16-odd": (("wgrad", 33, 2, 2, 32, 64, (6, 4), BF16), dict(odd_l=True)),
    "wgrad-c1": (("wgrad", 34, 3, 2, 1, 32, (4, 4, 16), BF16), {}),
}
ACTS = {"down3d-f32": "relu", "down3d-bf16": "leaky02", "down2d-bf16": "relu", "up3d-bf16": "relu", "up-c1-3d": "sigmoid", "up2d-bf16-32ch": "sigmoid"}


def case_of(name, **over):
    args, kw = FAMILIES[name]
    return c64.make_case(*args, **{**kw, **over})


def aten32(c, act=None, dbias_side=None):
    """the product through aten in fp32 on NC(D)HW tensors: the stand-in for a correct kernel"""
    nd = c["nd"]
    nc = lambda t: t.float().permute(0, 4, 1, 2, 3)[:, :, 0] if nd == 2 else t.float().permute(0, 4, 1, 2, 3)
    cl = lambda t: (t.unsqueeze(2) if nd == 2 else t).permute(0, 2, 3, 4, 1)
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    w = c["w_ref"].float()
    if c["kind"] == "wgrad":
        L = nc(c["L"]).requires_grad_(False)
        wz = torch.zeros_like(w).requires_grad_(True)
        S = nc(c["S"])
        out = conv(L, wz, None, stride=2, padding=1)
        (dW,) = torch.autograd.grad(out, wz, S[(..., *[slice(0, n) for n in out.shape[2:]])])
        got = {"dW": dW}
        if dbias_side is not None:
            t = c["L"] if dbias_side else c["S"]
            got["dbias"] = t.float().reshape(-1, t.shape[-1]).sum(0)
        return got
    if c["kind"] == "down":
        pre = conv(nc(c["L"]), w, c["bias"], stride=2, padding=1)
    else:
        opad = tuple(l - 2 * s for l, s in zip(c["l_dims"], c["s_dims"]))[3 - nd:]
        pre = convT(nc(c["S"]), w, c["bias"], stride=2, padding=1, output_padding=opad)
    y = {None: lambda v: v, "relu": F.relu, "sigmoid": torch.sigmoid, "leaky02": lambda v: F.leaky_relu(v, 0.2)}[act](pre)
    y = cl(y)
    return y * (c["mask"] > 0) if c["mask"] is not None else y


def stored(c):
    return "bf16" if (c["dtype"] == BF16 and c["kind"] != "wgrad") else "f32"


@pytest.mark.parametrize("name", list(FAMILIES))
def test_fp32_aten_standin_is_within_the_bound(name):
    c = case_of(name)
    act = ACTS.get(name)
    if c["kind"] == "wgrad":
        for side in (0, 1):
            ref, err = c64.reference(c, dbias_side=side)
            got = aten32(c, dbias_side=side)
            print(name, side, {k: round(c64.max_ratio(got[k], ref[k], err[k]), 3) for k in ref})
            assert c64.compare(got, ref, err) == []
        return
    ref, err, _, _ = c64.reference(c, act)
    got = aten32(c, act)
    print(name, "fp32", round(c64.max_ratio(got, ref, err), 3))
    assert c64.compare({"y": got}, {"y": ref}, {"y": err}) == []
    if stored(c) == "bf16":
        r, e = c64.out_bound(ref, err, "bf16")
        gb = got.to(BF16)
        print(name, "bf16", round(c64.max_ratio(gb, r, e), 3))
        assert c64.compare({"y": gb}, {"y": r}, {"y": e}) == []


def mutations_of(c):
    """every mutation that applies to the case's product (the issue's list), with arguments that fit its channel counts"""
    nd, cin = c["nd"], (c["Cl"] if c["kind"] == "down" else c["Cs"])
    tap = 5 if nd == 2 else 21                      # an inner tap: (1, 1) / (1, 1, 1)
    m = []
    if c["kind"] in ("down", "up"):
        m.append(("product", (cin // 2, tap)))
        if cin >= 16:
            m.append(("kstep", (16 * ((cin // 16) // 2), tap)))
        m += [("replicate_face", 2), ("replicate_face", 1)] + ([("replicate_face", 0)] if nd == 3 else [])
        m.append(("bias_per_split", 2))
    if c["kind"] == "down" and cin >= 32:
        m.append(("slab_bf16", 2))
    if c["kind"] == "up":
        m.append(("parity_shift", (1, 0, 1)))
    if c["kind"] == "wgrad":
        m += [("ragged_last",), ("slab_bf16", 4), ("replicate_face", 2)]
    return m


@pytest.mark.parametrize("name", list(FAMILIES))
def test_every_mutation_fails_the_comparison(name):
    c = case_of(name)
    act = ACTS.get(name)
    muts = mutations_of(c)
    assert muts
    for drop in muts:
        if c["kind"] == "wgrad":
            ref, err = c64.reference(c, dbias_side=0)
            bad, _ = c64.reference(c, dbias_side=0, drop=drop)
            assert c64.compare({"dW": bad["dW"]}, ref, err, ["dW"]) != [], (name, drop)
            continue
        ref, err, _, _ = c64.reference(c, act)
        r, e = c64.out_bound(ref, err, stored(c))
        bad = c64.reference(c, act, drop=drop)[0]
        if stored(c) == "bf16":
            bad = bad.to(BF16)
        assert c64.compare({"y": bad}, {"y": r}, {"y": e}) != [], (name, drop)


@pytest.mark.parametrize("name", [n for n in FAMILIES if FAMILIES[n][0][7] == BF16 and FAMILIES[n][0][0] != "wgrad"])
@pytest.mark.parametrize("sign", [1, -1])
def test_a_bf16_result_scaled_by_one_ulp_fails(name, sign):
    """got = bf16(ref) (1 +- 2^-7): every element is one bf16 ulp off"""
    c = case_of(name)
    ref, err, _, _ = c64.reference(c, ACTS.get(name))
    r, e = c64.out_bound(ref, err, "bf16")
    got = (ref.to(BF16).double() * (1 + sign * 2.0 ** -7)).to(BF16)
    assert c64.compare({"y": got}, {"y": r}, {"y": e}) != []
    assert c64.compare({"y": ref.to(BF16)}, {"y": r}, {"y": e}) == []


def _fp8_case(seed, up, nd, B, Cin, Cout, size):
    """decoded e4m3 codes times their scales on both operands (what a cvae_conv_fp8 reference is handed)"""
    kind = "up" if up else "down"
    Cl, Cs = (Cout, Cin) if up else (Cin, Cout)
    c = c64.make_case(kind, seed, nd, B, Cl, Cs, size, F32)
    q = lambda t: (t / (float(t.abs().max()) / 448.0)).to(torch.float8_e4m3fn).float() * (float(t.abs().max()) / 448.0)
    key = "S" if up else "L"
    c[key] = q(c[key].abs())
    c["w_ref"] = q(c["w"])
    return c


@pytest.mark.parametrize("up,nd,Cin,Cout,size", [(False, 3, 32, 64, (6, 8, 8)), (True, 3, 64, 32, (3, 4, 5)), (True, 2, 128, 64, (5, 6))])
def test_fp8_products_and_code_output(up, nd, Cin, Cout, size):
    c = _fp8_case(41, up, nd, 2, Cin, Cout, size)
    ref, err, _, _ = c64.reference(c, "relu", f8_mfma=True)                # with the truncation term of the fp8 MFMA: the mutations below must still fail
    assert float((err / c64.reference(c, "relu")[1]).max()) > 1.0
    got = aten32(c, "relu")
    assert c64.compare({"y": got}, {"y": ref}, {"y": err}) == []
    scale = 0.5 * float(ref.abs().max()) / 448.0                    # half the range: the upper half of the values saturates at 448
    r, e = c64.out_bound(ref, err, "e4m3", scale)
    codes = (got.float() * (1.0 / scale)).clamp(-448, 448).to(torch.float8_e4m3fn).float() * scale
    print("fp8", up, nd, round(c64.max_ratio(codes, r, e), 3))
    assert c64.compare({"y": codes}, {"y": r}, {"y": e}) == []
    assert float(r.max()) == pytest.approx(448 * scale)
    for drop in [("product", (Cin // 2, 5)), ("kstep", (16, 5)), ("replicate_face", 2), ("bias_per_split", 2)] + ([] if up else [("slab_bf16", 2)]):      # split-K slabs: down only
        bad = c64.reference(c, "relu", drop=drop)[0]
        r16, e16 = c64.out_bound(ref, err, "bf16")
        assert c64.compare({"y": bad.to(BF16)}, {"y": r16}, {"y": e16}) != [], drop
    one_up = (codes / scale).to(torch.float8_e4m3fn).view(torch.uint8)
    bumped = torch.where((one_up & 0x7f) < 0x7d, one_up + 1, one_up).view(torch.float8_e4m3fn).float() * scale       # every code one step up
    assert c64.compare({"y": bumped}, {"y": r}, {"y": e}) != []


def test_e4m3_half_ulp_steps():
    x = torch.tensor([0.0, 2.0 ** -9, 2.0 ** -6, 1.0, 1.9, 2.0, 300.0, 448.0, 1e4], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -10, 2.0 ** -4, 2.0 ** -4, 2.0 ** -3, 16.0, 16.0, 16.0], dtype=torch.float64)
    assert torch.equal(c64.e4m3_half_ulp(x), want)


BIT_CASES = [c[:6] + ({"f32": F32, "bf16": BF16}[c[6]],) for c in c64.BIT_CASES]        # the very cases (and seed) the GPU file runs


@pytest.mark.parametrize("kind,nd,B,Cl,Cs,size,dtype", BIT_CASES)
def test_relu_bit_cases_leave_at_most_a_thousandth_undecided(kind, nd, B, Cl, Cs, size, dtype):
    c = c64.make_case(kind, c64.BIT_SEED, nd, B, Cl, Cs, size, dtype, bits=True)
    _, _, pre, e_pre = c64.reference(c, "relu")
    assert c64.undecided_fraction(pre, e_pre) <= 1e-3
    # relu_bits reads the words as the kernels write them: element 32 i + j = bit j of word i
    bits = (pre.reshape(-1, 32) > 0).long()
    words = (bits << torch.arange(32)).sum(1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    assert c64.relu_bits(words, pre, e_pre)[0] == 0
    flipped = words ^ 1                                              # bit 0 of every word wrong
    assert c64.relu_bits(flipped, pre, e_pre)[0] > 0.9 * words.numel()


def test_structured_case_names_the_coordinate():
    """one-hot weight, small-integer inputs: every output is ONE input element, exact in bf16 — and a swapped pair of axes shows at once"""
    c = c64.make_case("down", 0, 3, 2, 32, 64, (8, 6, 10), BF16, bias=False, structure=True)
    ref, err, _, _ = c64.reference(c)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 15
    assert torch.equal(aten32(c).double(), ref)
    swapped = dict(c, L=c["L"].transpose(2, 3).contiguous().reshape(c["L"].shape))
    assert not torch.equal(c64.reference(swapped)[0], ref)
