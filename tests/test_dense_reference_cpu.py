"""CPU self-tests of oracle/dense64.py, the float64 references and bounds that tests/test_dense_reference.py holds csrc/linear.hip and csrc/small_dense.hip to.

  1. WITHIN THE BOUNDS: every reference evaluated in fp32 on the CPU (the stand-in for a correct kernel) lies within its bound at every shape family of the
     GPU file; the ratio max |fp32 - float64| / bound is printed per family (`RATIO <family> <value>`, the bracketed figures of the GPU file's docstring).
  2. ONE WRONG TERM FAILS: every entry of dense64._MUTATIONS, a named restatement of the fp32 stand-in, is rejected by the same comparison at the shapes where
     the GPU file relies on the bound.  Where the bound alone is not enough the STRUCTURED case (integers in [-2, 2], exact sums) catches it bit for bit, and
     that is the reason those cases exist.  The one-missing-k mutation is such a case: the bound C sqrt(K) U sum |terms| grows like K^(1/2) x K^(1/2) terms of
     size K^(-1/2), i.e. like sqrt(K) U, against a missing term of size K^(-1/2).  Share of the ELEMENTS of y whose bound rejects a dropped last k
     (`LAST_K_SHARE K share`, Gaussian operands, 256 x 256 outputs), measured here:
         K = 130: 0.997   449: 0.995   1100: 0.983   2100: 0.951   3000: 0.926   4000: 0.903   5000: 0.837   8000: 0.753   16415: 0.563
     Below 90 % from K ~ 4000 - 5000 on; `compare` still rejects the tensor while ANY element is outside, so what can escape is a product with few outputs
     (1 x 64 x 1: one element; 17 x 5000 x 3: 51).  At every K the structured case differs from the exact result in every element whose dropped product is not 0.
  3. The reference's BRANCH ASSERTIONS fire on inputs that straddle them (an activation output within 2^-6 of zero, a sigmoid pre-activation beyond 8).
  4. ARGUMENT CHECKS of the nine entry points, each against what include/cvae_hip.h says, in the idiom of tests/test_loss_reference_cpu.py: valid arguments get
     past every check, which without a device ends as CVAE_E_LAUNCH; every rule has its code; no byte of the buffer changes.  Skipped where a device exists.
     Header and code disagreed; fixed with this file: the header gave cvae_small_dense_*'s limit as K, N <= 512 where the code has 128 (the header was
     wrong: ops.py asks cvae_small_dense_supported); cvae_linear_bwd_weight refused db on a strided dy (M > 16) only AFTER the dW GEMM had been launched (now
     before any launch, and stated in the header); cvae_linear_bwd_weight answered CVAE_OK for N == 0 where the other two entries answer CVAE_E_BADSHAPE, and
     cvae_linear_bwd_data with y_act, M <= 16 and K == 0 launched an empty grid (CVAE_E_LAUNCH): both CVAE_E_BADSHAPE now, as the header states.
  5. cvae_linear_workspace_bytes(M, K, N, op) is at least what each path of that op asks for, with the split counts recomputed in Python from the rules of
     csrc/linear.hip (dense64.gemm_splits, gemm_t128_splits, skinny_fwd_chunks, skinny_bwd_chunks), at every shape the GPU file uses; and those replayed
     counts are the ones its docstring names."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import dense64 as d64

F32, F64 = torch.float32, torch.float64
WORST = {}


def ratio(name, fn, *args, **kw):
    """the fp32 evaluation of fn against its float64 reference: asserts it within the bounds, prints and returns the largest ratio"""
    ref, err = fn(*args, **kw)
    got, _ = fn(*args, dtype=F32, **kw)
    bad = d64.compare(got, ref, err)
    worst = max(d64.max_ratio(got[k], ref[k], err[k]) for k in ref)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"RATIO {name} {worst:.4f}")
    assert not bad, "\n".join(bad)
    return worst


def rejected(got, ref, err, keys=None):
    bad = d64.compare(got, ref, err, keys)
    assert bad, f"the wrong result passed the comparison of {keys or list(ref)}"
    return bad


def share_outside(got, ref, err, k):
    return float(((got[k].double() - ref[k]).abs() > err[k]).double().mean())


# ------------------------------------------------------------------------------------------------ 1. the fp32 stand-in lies within the bounds
FWD = [("fwd_skinny", d64.FWD_SKINNY, False), ("fwd_gemm_f32", d64.FWD_GEMM, False), ("fwd_bf16_t64", d64.FWD_BF16_64, True), ("fwd_bf16_t128", d64.FWD_BF16_128, True),
       ("small_dense_fwd", [(M, K, N) for M in (17, 1000) for K, N in d64.SD_KN], False)]


@pytest.mark.parametrize("family,shapes,bf", FWD, ids=[f[0] for f in FWD])
def test_fwd_fp32_within_bounds(family, shapes, bf):
    for M, K, N in shapes:
        c = d64.operands("random", 1, M, K, N)
        x, W = (d64.bf16(c["x"]), d64.bf16(c["W"])) if bf else (c["x"], c["W"])
        for act in d64.ACTS:
            ratio(family, d64.fwd, x, W, c["b"] if act != d64.LEAKY02 else None, act)


BWD_DATA = [("bwd_data_skinny", d64.BWD_DATA_WIDE + d64.BWD_DATA_NARROW, False), ("bwd_data_gemm_f32", d64.BWD_DATA_GEMM, False),
            ("bwd_data_bf16", d64.BWD_DATA_BF16, True), ("small_dense_bwd_data", [(M, K, N) for M in (17, 1000) for K, N in d64.SD_KN], False)]


@pytest.mark.parametrize("family,shapes,bf", BWD_DATA, ids=[f[0] for f in BWD_DATA])
def test_bwd_data_fp32_within_bounds(family, shapes, bf):
    for M, K, N in shapes:
        c = d64.operands("random", 1, M, K, N)
        dy, W = (d64.bf16(c["dy"]), d64.bf16(c["W"])) if bf else (c["dy"], c["W"])
        for i, act in enumerate(d64.ACTS):
            in_act = d64.ACTS[(i + 2) % 5]
            ratio(family, d64.bwd_data, dy, W, d64.act_output("random", 5, M, N, act), act, d64.act_output("random", 6, M, K, in_act), in_act)


BWD_WEIGHT = [("bwd_weight_rows", d64.BWD_WEIGHT_ROWS, False), ("bwd_weight_flat", d64.BWD_WEIGHT_FLAT, False), ("bwd_weight_gemm_f32", d64.BWD_WEIGHT_GEMM, False),
              ("bwd_weight_bf16", d64.BWD_WEIGHT_BF16_64 + d64.BWD_WEIGHT_BF16_128, True),
              ("small_dense_bwd_weight", [(M, K, N) for M in (17, 1000) for K, N in d64.SD_KN], False)]


@pytest.mark.parametrize("family,shapes,bf", BWD_WEIGHT, ids=[f[0] for f in BWD_WEIGHT])
def test_bwd_weight_fp32_within_bounds(family, shapes, bf):
    for M, K, N in shapes:
        c = d64.operands("random", 1, M, K, N)
        dy, x = (d64.bf16(c["dy"]), d64.bf16(c["x"])) if bf else (c["dy"], c["x"])
        for act in (d64.ACTS if N < 10000 else (d64.RELU,)):
            ratio(family, d64.bwd_weight, dy, x, d64.act_output("random", 5, M, N, act), act, dy_db=c["dy"] if bf else None)


def test_structured_operands_are_exact_in_fp32_and_bf16():
    """integers in [-2, 2]: the float64 result is an integer below 2^24 (fp32-exact), the operands survive the rounding to bf16, and every index matters"""
    for M, K, N in ((17, 5000, 3), (2, 255, 300), (129, 400, 133)):
        c = d64.operands("structured", 1, M, K, N)
        for v in c.values():
            assert torch.equal(d64.bf16(v), v) and float(v.abs().max()) == 2.0
        for fn, args in ((d64.fwd, (c["x"], c["W"], c["b"], d64.RELU)), (d64.bwd_data, (c["dy"], c["W"], d64.act_output("structured", 5, M, N, d64.RELU), d64.RELU, None, 0)),
                         (d64.bwd_weight, (c["dy"], c["x"], d64.act_output("structured", 5, M, N, d64.LEAKY02), d64.LEAKY02))):
            ref, _ = fn(*args)
            got, _ = fn(*args, dtype=F32)
            for k in ref:
                assert float(ref[k].abs().max()) < 2 ** 24 and torch.equal(ref[k], ref[k].round()) and torch.equal(got[k], ref[k])
                assert float(ref[k].std()) > 0.5


# ------------------------------------------------------------------------------------------------ 2. every mutation is rejected
def fwd_case(kind, M, K, N, act=d64.NONE):
    c = d64.operands(kind, 1, M, K, N)
    return (c["x"], c["W"], c["b"], act)


def structured_catches(fn, args, drop):
    """the structured case: the mutated fp32 result differs in bits from the exact one"""
    ref, _ = fn(*args)
    got, _ = fn(*args, dtype=F32, drop=drop)
    good, _ = fn(*args, dtype=F32)
    assert all(torch.equal(good[k], ref[k]) for k in ref)
    assert any(not torch.equal(got[k], ref[k]) for k in ref), f"{drop[0]} left the structured result unchanged"


def test_every_mutation_is_named():
    assert set(d64._MUTATIONS) == {"last_k", "kstep", "slab", "bias_per_split", "last_row", "edge_col", "yact_rowlen"}
    with pytest.raises(ValueError):
        d64.fwd(*fwd_case("random", 3, 8, 2), drop=("no_such",))


@pytest.mark.parametrize("K", [130, 1100, 2100, 5000, 16415])
def test_fault_last_k_dropped(K):
    """see the module docstring: the share of elements whose bound rejects it falls with K; the structured case catches it at every K"""
    args = fwd_case("random", 256, K, 256)
    ref, err = d64.fwd(*args)
    got, _ = d64.fwd(*args, dtype=F32, drop=("last_k",))
    share = share_outside(got, ref, err, "y")
    print(f"LAST_K_SHARE {K} {share:.4f}")
    assert (share > 0.9) == (K <= 2100) and share > 0.4
    rejected(got, ref, err)
    structured_catches(d64.fwd, fwd_case("structured", 64, K, 64), ("last_k",))


@pytest.mark.parametrize("shape", [(1, 64, 1), (65, 130, 67), (3, 1100, 7), (17, 5000, 3), (129, 131, 133)])
def test_fault_last_k_at_the_shapes_of_the_gpu_file(shape):
    """rejected by the bound except where the product has too few outputs for one to be surely outside; the structured case catches every one"""
    args = fwd_case("random", *shape)
    ref, err = d64.fwd(*args)
    got, _ = d64.fwd(*args, dtype=F32, drop=("last_k",))
    if shape[0] * shape[2] >= 21:
        rejected(got, ref, err)
    structured_catches(d64.fwd, fwd_case("structured", *shape), ("last_k",))
    for fn, a in ((d64.bwd_data, lambda c: (c["dy"], c["W"], None, 0, None, 0)), (d64.bwd_weight, lambda c: (c["dy"], c["x"], None, 0))):
        structured_catches(fn, a(d64.operands("structured", 1, *shape)), ("last_k",))


@pytest.mark.parametrize("shape,k0", [((65, 113, 67), 64), ((65, 113, 67), 96), ((17, 5000, 3), 4992), ((129, 400, 133), 384), ((5, 2100, 3), 1728)])
def test_fault_one_k_step_dropped(shape, k0):
    for act in (d64.NONE, d64.SIGMOID):
        args = fwd_case("random", *shape, act)
        ref, err = d64.fwd(*args)
        assert not d64.compare(d64.fwd(*args, dtype=F32)[0], ref, err)
        rejected(d64.fwd(*args, dtype=F32, drop=("kstep", k0))[0], ref, err)
    structured_catches(d64.fwd, fwd_case("structured", *shape), ("kstep", k0))


def test_fault_one_slab_dropped():
    """the second of 2 splits (65 x 130 x 67: 80 + 50), the last, short, one of 63 (17 x 5000 x 3), the last k-chunk of 4 (5 x 2100 x 3), one n-chunk of the skinny
    backward-data (16 x 1500 x 200: 12 chunks of 17), one workgroup's partial of small_dense's weight gradient (M = 145: 10 workgroups of 16 rows)"""
    for shape, per, s in (((65, 130, 67), 80, 1), ((17, 5000, 3), 80, 62), ((5, 2100, 3), 576, 3)):
        assert d64.gemm_splits(shape[0], shape[2], shape[1]) == (s + 1, per) or d64.skinny_fwd_chunks(shape[1], shape[2]) == (s + 1, per)
        args = fwd_case("random", *shape)
        ref, err = d64.fwd(*args)
        rejected(d64.fwd(*args, dtype=F32, drop=("slab", (s, per)))[0], ref, err)
        structured_catches(d64.fwd, fwd_case("structured", *shape), ("slab", (s, per)))
    c = d64.operands("random", 1, 16, 1500, 200)
    ref, err = d64.bwd_data(c["dy"], c["W"], None, 0, None, 0)
    rejected(d64.bwd_data(c["dy"], c["W"], None, 0, None, 0, dtype=F32, drop=("slab", (11, 17)))[0], ref, err)
    c = d64.operands("random", 1, 145, 10, 64)
    ref, err = d64.bwd_weight(c["dy"], c["x"], None, 0)
    got, _ = d64.bwd_weight(c["dy"], c["x"], None, 0, dtype=F32, drop=("slab", (9, 16)))
    rejected(got, ref, err, ["dW"])
    rejected(got, ref, err, ["db"])


def test_fault_bias_added_once_per_split():
    for shape, n in (((65, 113, 67), 2), ((17, 5000, 3), 63), ((3, 1100, 7), 2)):
        for act in (d64.NONE, d64.RELU) + ((d64.SIGMOID,) if n == 2 else ()):       # (63 biases would leave the sigmoid's measured range)
            args = fwd_case("random", *shape, act)
            ref, err = d64.fwd(*args)
            rejected(d64.fwd(*args, dtype=F32, drop=("bias_per_split", n))[0], ref, err)
        structured_catches(d64.fwd, fwd_case("structured", *shape), ("bias_per_split", n))


@pytest.mark.parametrize("M", [17, 145, 1000, 1031])
def test_fault_last_row_missing_from_the_weight_gradient(M):
    """M = 17: the second workgroup of small_dense holds this one row; M = 1031: the last term of the GEMM's sum over the batch"""
    K, N = 20, 10
    c = d64.operands("random", 1, M, K, N)
    ya = d64.act_output("random", 5, M, N, d64.LEAKY02)
    ref, err = d64.bwd_weight(c["dy"], c["x"], ya, d64.LEAKY02)
    got, _ = d64.bwd_weight(c["dy"], c["x"], ya, d64.LEAKY02, dtype=F32, drop=("last_row",))
    rejected(got, ref, err, ["dW"])
    rejected(got, ref, err, ["db"])
    s = d64.operands("structured", 1, M, K, N)
    structured_catches(d64.bwd_weight, (s["dy"], s["x"], d64.act_output("structured", 5, M, N, d64.RELU), d64.RELU), ("last_row",))


def test_fault_tile_edge_column_from_its_neighbour():
    for shape, col in (((65, 113, 67), 64), ((129, 131, 133), 128), ((133, 400, 129), 128)):
        args = fwd_case("random", *shape)
        ref, err = d64.fwd(*args)
        rejected(d64.fwd(*args, dtype=F32, drop=("edge_col", col))[0], ref, err)
        structured_catches(d64.fwd, fwd_case("structured", *shape), ("edge_col", col))
    c = d64.operands("random", 1, 400, 131, 257)                  # dW [257][131]: column 128 of the (row, row) 128-tile form
    ref, err = d64.bwd_weight(c["dy"], c["x"], None, 0)
    rejected(d64.bwd_weight(c["dy"], c["x"], None, 0, dtype=F32, drop=("edge_col", 128))[0], ref, err, ["dW"])
    c = d64.operands("random", 1, 65, 67, 130)
    ref, err = d64.bwd_data(c["dy"], c["W"], None, 0, None, 0)
    rejected(d64.bwd_data(c["dy"], c["W"], None, 0, None, 0, dtype=F32, drop=("edge_col", 64))[0], ref, err)


@pytest.mark.parametrize("act", [d64.RELU, d64.SIGMOID, d64.LEAKY02, d64.LEAKY001])
def test_fault_y_act_read_with_the_row_length(act):
    """y_act on dy's stride N + 3, the gaps holding the GPU file's canary: the skinny backward-data (4 x 1030 x 40) and the rows kernel (16 x 1030 x 5)"""
    for M, K, N in ((4, 1030, 40), (16, 1030, 5)):
        c = d64.operands("random", 1, M, K, N)
        ya = d64.act_output("random", 5, M, N, act)
        buf = torch.full((M, N + 3), -777.25)
        buf[:, :N] = ya
        ref, err = d64.bwd_data(c["dy"], c["W"], ya, act, None, 0)
        rejected(d64.bwd_data(c["dy"], c["W"], ya, act, None, 0, dtype=F32, drop=("yact_rowlen", buf))[0], ref, err)
        ref, err = d64.bwd_weight(c["dy"], c["x"], ya, act)
        got, _ = d64.bwd_weight(c["dy"], c["x"], ya, act, dtype=F32, drop=("yact_rowlen", buf))
        rejected(got, ref, err, ["dW"])
        rejected(got, ref, err, ["db"])


def test_fault_wrong_activation_slope_and_missing_in_act():
    """LeakyReLU(0.01) where 0.2 belongs, and the in_act epilogue left out"""
    c = d64.operands("random", 1, 65, 67, 112)
    ref, err = d64.fwd(c["x"], c["W"], c["b"], d64.LEAKY02)
    rejected(d64.fwd(c["x"], c["W"], c["b"], d64.LEAKY001, dtype=F32)[0], ref, err)
    xin = d64.act_output("random", 6, 65, 67, d64.SIGMOID)
    ref, err = d64.bwd_data(c["dy"], c["W"], None, 0, xin, d64.SIGMOID)
    rejected(d64.bwd_data(c["dy"], c["W"], None, 0, None, 0, dtype=F32)[0], ref, err)


# ------------------------------------------------------------------------------------------------ 3. the reference's own assertions
def test_branch_margins_are_asserted():
    c = d64.operands("random", 1, 3, 7, 3)
    ya = d64.act_output("random", 5, 3, 3, d64.RELU)
    ya[1, 1] = 2.0 ** -8
    for act in (d64.RELU, d64.LEAKY02, d64.LEAKY001):
        with pytest.raises(AssertionError):
            d64.bwd_data(c["dy"], c["W"], ya, act, None, 0)
        with pytest.raises(AssertionError):
            d64.bwd_weight(c["dy"], c["x"], ya, act)
    xin = d64.act_output("random", 6, 3, 7, d64.RELU)
    xin[2, 0] = -2.0 ** -7
    with pytest.raises(AssertionError):
        d64.bwd_data(c["dy"], c["W"], None, 0, xin, d64.RELU)
    with pytest.raises(AssertionError):
        d64.fwd(20.0 * c["x"], 20.0 * c["W"], c["b"], d64.SIGMOID)
    d64.bwd_data(c["dy"], c["W"], ya, d64.SIGMOID, None, 0)           # no branch: no assertion
    for act in (d64.RELU, d64.LEAKY02, d64.LEAKY001):
        v = d64.act_output("random", 9, 64, 64, act)
        assert bool(((v == 0) | (v.abs() >= d64.BRANCH_MARGIN)).all()) and bool((v > 0).any()) and bool((v <= 0).any())


# ------------------------------------------------------------------------------------------------ 4. argument checks before any launch
HAS_DEVICE = torch.cuda.is_available()
needs_no_device = pytest.mark.skipif(HAS_DEVICE, reason="host pointers stand in for device memory: only where no launch can succeed")
OK, BADSHAPE, UNSUPPORTED, WORKSPACE, LAUNCH, NULLPTR = 0, -1, -3, -4, -5, -6

_buf = (C.c_float * (1 << 14))(*([3.25] * (1 << 14)))           # never read or written through: no launch succeeds here
P = (C.addressof(_buf) + 15) & ~15


def R(*pos):
    return [({i: None}, NULLPTR) for i in pos]


SD_WS = 2 * (10 * 64 + 64) * 4                                   # cvae_small_dense_workspace_bytes(17, 10, 64)
# entry point -> (valid arguments, [({position: value}, expected code)])
CHECKS = {
    # x, W, b, y, M, K, N, x_stride, y_stride, act, bf16_math, workspace, workspace_bytes, stream
    "cvae_linear_fwd": ((P, P, None, P, 4, 64, 3, 64, 3, 0, 0, None, 0, None),
                        R(0, 1, 3) + [({7: 63}, BADSHAPE), ({8: 2}, BADSHAPE), ({4: -1}, BADSHAPE), ({4: 0}, OK), ({5: 0, 7: 0}, BADSHAPE), ({6: 0, 8: 0}, BADSHAPE),
                                      ({10: 1}, UNSUPPORTED), ({10: 1, 4: 16}, UNSUPPORTED), ({10: 1, 4: 17}, LAUNCH), ({10: 1, 8: 2}, BADSHAPE), ({4: 17}, LAUNCH),
                                      ({4: 17, 0: None}, NULLPTR), ({4: 17, 1: None}, NULLPTR), ({4: 17, 3: None}, NULLPTR), ({4: 17, 8: 2}, BADSHAPE),
                                      ({2: P, 9: 4}, LAUNCH), ({5: 63, 7: 63}, LAUNCH)]),
    # dy, W, dx, M, K, N, dy_stride, dx_stride, y_act, act, x_in, x_stride, in_act, bf16_math, workspace, workspace_bytes, stream
    "cvae_linear_bwd_data": ((P, P, P, 4, 1024, 3, 3, 1024, None, 0, None, 0, 0, 0, None, 0, None),
                             R(0, 1, 2) + [({6: 2}, BADSHAPE), ({7: 1023}, BADSHAPE), ({3: -1}, BADSHAPE), ({3: 0}, OK), ({8: P, 9: 1}, LAUNCH),
                                           ({3: 17, 8: P, 9: 1}, UNSUPPORTED), ({3: 17, 8: P, 9: 0}, LAUNCH), ({3: 17}, LAUNCH), ({3: 17, 2: None}, NULLPTR),
                                           ({4: 7, 7: 7, 8: P, 9: 3}, LAUNCH), ({10: P, 11: 1024, 12: 1}, UNSUPPORTED), ({3: 17, 10: None, 11: 1024, 12: 1}, NULLPTR),
                                           ({3: 17, 10: P, 11: 1023, 12: 1}, BADSHAPE), ({3: 17, 10: P, 11: 1024, 12: 2}, LAUNCH), ({13: 1}, UNSUPPORTED),
                                           ({3: 17, 13: 1}, LAUNCH), ({3: 17, 13: 1, 7: 1023}, BADSHAPE), ({4: 0, 7: 0, 8: P, 9: 1}, BADSHAPE),
                                           ({4: 0, 7: 0}, BADSHAPE), ({5: 0, 6: 0}, BADSHAPE)]),
    # dy, x, dW, db, M, K, N, dy_stride, x_stride, y_act, act, bf16_math, workspace, workspace_bytes, stream
    "cvae_linear_bwd_weight": ((P, P, P, P, 4, 256, 3, 3, 256, None, 0, 0, None, 0, None),
                               R(0, 1, 2) + [({3: None}, LAUNCH), ({7: 2}, BADSHAPE), ({8: 255}, BADSHAPE), ({4: 0}, BADSHAPE), ({4: -1}, BADSHAPE), ({11: 1}, UNSUPPORTED),
                                             ({9: P, 10: 2}, LAUNCH), ({7: 5, 9: P, 10: 1}, LAUNCH), ({5: 10, 8: 10}, LAUNCH), ({4: 17}, LAUNCH), ({4: 17, 0: None}, NULLPTR),
                                             ({4: 17, 9: P, 10: 1}, UNSUPPORTED), ({4: 17, 9: P, 10: 0}, LAUNCH), ({4: 17, 7: 5}, UNSUPPORTED), ({4: 17, 7: 5, 3: None}, LAUNCH),
                                             ({4: 17, 11: 1}, LAUNCH), ({4: 17, 11: 1, 7: 5}, UNSUPPORTED), ({6: 0, 7: 0}, BADSHAPE), ({5: 0, 8: 0}, BADSHAPE),
                                             ({4: 17, 6: 0, 7: 0}, BADSHAPE), ({4: 17, 5: 0, 8: 0}, BADSHAPE)]),
    # x, W, b, y, M, K, N, x_stride, y_stride, act, stream
    "cvae_small_dense_fwd": ((P, P, None, P, 17, 10, 64, 10, 64, 0, None),
                             R(0, 1, 3) + [({4: 16}, BADSHAPE), ({4: 1 << 30}, BADSHAPE), ({5: 129, 7: 129}, BADSHAPE), ({6: 129, 8: 129}, BADSHAPE), ({5: 0}, BADSHAPE),
                                           ({6: 0}, BADSHAPE), ({5: 128, 6: 97, 7: 128, 8: 97}, BADSHAPE), ({5: 128, 6: 96, 7: 128, 8: 96}, LAUNCH), ({7: 9}, BADSHAPE),
                                           ({8: 63}, BADSHAPE), ({9: 5}, BADSHAPE), ({9: -1}, BADSHAPE), ({9: 4, 2: P}, LAUNCH)]),
    # dy, W, dx, y_act, act, x_in, in_act, M, K, N, dy_stride, dx_stride, y_stride, x_stride, stream
    "cvae_small_dense_bwd_data": ((P, P, P, None, 0, None, 0, 17, 10, 64, 64, 10, 0, 0, None),
                                  R(0, 1, 2) + [({7: 16}, BADSHAPE), ({8: 129, 11: 129}, BADSHAPE), ({10: 63}, BADSHAPE), ({11: 9}, BADSHAPE), ({4: 5}, BADSHAPE), ({6: 5}, BADSHAPE),
                                                ({3: P, 4: 1, 12: 63}, BADSHAPE), ({3: P, 4: 1, 12: 64}, LAUNCH), ({3: P, 4: 0, 12: 0}, LAUNCH), ({4: 4}, LAUNCH),
                                                ({5: P, 6: 2, 13: 9}, BADSHAPE), ({5: P, 6: 2, 13: 10}, LAUNCH), ({5: P, 6: 0, 13: 0}, LAUNCH)]),
    # dy, x, dW, db, y_act, act, M, K, N, dy_stride, x_stride, y_stride, workspace, workspace_bytes, stream
    "cvae_small_dense_bwd_weight": ((P, P, P, P, None, 0, 17, 10, 64, 64, 10, 0, P, SD_WS, None),
                                    R(0, 1, 2, 12) + [({3: None}, LAUNCH), ({13: SD_WS - 4}, WORKSPACE), ({13: 0}, WORKSPACE), ({6: 16}, BADSHAPE), ({9: 63}, BADSHAPE),
                                                      ({10: 9}, BADSHAPE), ({5: 5}, BADSHAPE), ({4: P, 5: 1, 11: 63}, BADSHAPE), ({4: P, 5: 1, 11: 64}, LAUNCH),
                                                      ({4: P, 5: 0}, LAUNCH), ({6: 33, 13: SD_WS}, WORKSPACE), ({6: 32}, LAUNCH)]),
}
# the three entry points that answer a value, not a code: (arguments, value)
VALUES = {
    "cvae_small_dense_supported": [((17, 128, 96), 1), ((17, 96, 128), 1), ((17, 1, 1), 1), ((16, 10, 10), 0), ((17, 129, 1), 0), ((17, 1, 129), 0), ((17, 128, 97), 0),
                                   ((17, 0, 5), 0), ((17, 5, 0), 0), ((17, 512, 20), 0), ((1 << 30, 4, 4), 0), ((-1, 4, 4), 0)],
    "cvae_small_dense_workspace_bytes": [((17, 10, 64), SD_WS), ((32, 10, 64), SD_WS), ((33, 10, 64), 3 * (10 * 64 + 64) * 4), ((1000, 128, 96), 63 * (12288 + 96) * 4),
                                         ((16, 10, 64), 0), ((17, 129, 1), 0), ((17, 512, 20), 0)],
    "cvae_linear_workspace_bytes": [((0, 5, 5, 0), 0), ((4, 0, 5, 1), 0), ((4, 5, 0, 2), 0), ((4, 64, 3, 0), 0), ((3, 1100, 7, 0), 2 * 3 * 7 * 4), ((65, 130, 67, 0), 2 * 65 * 67 * 4),
                                    ((65, 112, 67, 0), 0), ((17, 5000, 3, 0), 63 * 17 * 3 * 4), ((4, 1030, 40, 1), 2 * 4 * 1030 * 4), ((16, 1030, 5, 2), 0), ((4, 64, 3, 7), 0)],
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
    assert bytes(_buf) == before                                  # no output written (M == 0 returns OK and leaves them alone)


@pytest.mark.parametrize("name", list(VALUES))
def test_value_entry_points(name):
    from causal_vae_amd import _lib
    for args, want in VALUES[name]:
        assert getattr(_lib.lib, name)(*args) == want, f"{name}{args}"


def test_small_dense_limits_match_the_header():
    """the header's sentence on the limits names the numbers of the code (it said K, N <= 512)"""
    from causal_vae_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__)))
    text = open(os.path.join(root, "include", "cvae_hip.h")).read()
    assert "1 <= K, N <= 128 and N * K <= 12288" in text and "K, N <= 512" not in text
    assert (d64.SD_MAX_DIM, d64.SD_MAX_NK) == (128, 12288)
    for K, N in d64.SD_KN:
        assert all(_lib.lib.cvae_small_dense_supported(M, K, N) == 1 for M in d64.SD_M)


def test_the_table_names_every_entry_point_of_linear_hip_and_small_dense_hip():
    from causal_vae_amd import _lib
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    entries = set()
    for f in ("linear.hip", "small_dense.hip"):
        entries |= set(re.findall(r'extern "C" (?:int|size_t) (cvae_\w+)\(', open(os.path.join(csrc, f)).read()))
    assert len(entries) == 9 and entries == set(CHECKS) | set(VALUES)
    assert {e for e in entries if re.search(r'extern "C" int ' + e + r"\(", open(os.path.join(csrc, "linear.hip")).read() + open(os.path.join(csrc, "small_dense.hip")).read())} \
        == set(CHECKS) | {"cvae_small_dense_supported"}


# ------------------------------------------------------------------------------------------------ 5. the advertised workspace covers every path
def test_the_replayed_dispatch_gives_the_documented_splits():
    assert d64.skinny_fwd_chunks(1023, 7) == (1, 1024) and d64.skinny_fwd_chunks(1100, 7) == (2, 576) and d64.skinny_fwd_chunks(2100, 3) == (4, 576)
    assert d64.gemm_splits(65, 67, 112)[0] == 1 and d64.gemm_splits(65, 67, 113) == (2, 64) and d64.gemm_splits(65, 67, 130) == (2, 80)
    assert d64.gemm_splits(17, 3, 5000) == (63, 80) and d64.gemm_splits(17, 5, 20)[0] == 1 and d64.gemm_splits(100, 130, 200) == (3, 80)
    assert d64.gemm_t128_splits(128, 128, 128) == (1, 128) and d64.gemm_t128_splits(129, 133, 131) == (1, 160) and d64.gemm_t128_splits(129, 133, 400) == (3, 160)
    assert d64.skinny_bwd_chunks(1024, 5, True) == (1, 5) and d64.skinny_bwd_chunks(1030, 40, True) == (2, 20) and d64.skinny_bwd_chunks(1500, 200, True) == (12, 17)
    assert d64.skinny_bwd_chunks(7, 3, False) == (1, 3) and d64.skinny_bwd_chunks(70, 23, False) == (2, 12) and d64.skinny_bwd_chunks(300, 3000, False) == (250, 12)
    assert d64.gemm_splits(65, 67, 130) == (2, 80) and d64.gemm_splits(10, 20, 1031) == (13, 80)                 # the weight gradients: split over M
    assert d64.gemm_t128_splits(129, 133, 400) == (3, 160) and d64.gemm_t128_splits(257, 131, 400) == (3, 160)
    assert 255 * 16449 > 16384 * 256 > 255 * 16448                                                                # the flat kernel's second grid-stride trip


def test_linear_workspace_bytes_covers_every_path():
    from causal_vae_amd import _lib
    adv = _lib.lib.cvae_linear_workspace_bytes
    split = 0
    for op, shapes in ((0, d64.FWD_SKINNY + d64.FWD_GEMM + d64.FWD_BF16_64 + d64.FWD_BF16_128),
                       (1, d64.BWD_DATA_WIDE + d64.BWD_DATA_NARROW + d64.BWD_DATA_GEMM + d64.BWD_DATA_BF16),
                       (2, d64.BWD_WEIGHT_ROWS + d64.BWD_WEIGHT_FLAT + d64.BWD_WEIGHT_GEMM + d64.BWD_WEIGHT_BF16_64 + d64.BWD_WEIGHT_BF16_128)):
        for M, K, N in shapes:
            for bf in ((False, True) if M > d64.SK_M else (False,)):
                for y_act in ((False, True) if op == 1 and M <= d64.SK_M else (False,)):
                    for in_act in ((False, True) if op == 1 and M > d64.SK_M else (False,)):
                        need = 4 * d64.workspace_floats(op, M, K, N, bf, y_act, in_act)
                        split += need > 0
                        assert adv(M, K, N, op) >= need, f"op {op} {M}x{K}x{N} bf16 {bf} y_act {y_act}: advertised {adv(M, K, N, op)} < {need}"
            if op == 2 and M > d64.SK_M:
                assert adv(M, K, N, 2) >= _lib.lib.cvae_channel_sum_workspace_bytes(M, N, _lib.F32)
    assert split >= 30


def test_zz_worst_ratios():
    for k in sorted(WORST):
        print(f"WORST {k} {WORST[k]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
