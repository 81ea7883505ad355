"""csrc/linear.hip and csrc/small_dense.hip through the raw C ABI against the float64 references of oracle/dense64.py: ONE launch and ONE comparison per
case, with elementwise bounds derived there (C sqrt(T) U (sum |a| |b| + |bias|), C = 4, U = 2^-24, T the element's real term count; the activation's
Lipschitz constant, the measured error of __expf for the sigmoid, the roundings of g = dy act'(y_act) and of the in_act epilogue).
tests/test_dense_reference_cpu.py shows that the bounds are neither loose nor wrong, replays the launch dispatch, and holds the entry points' argument checks
to include/cvae_hip.h.

Every output lives inside a canary-filled buffer, so the gaps of a strided output and both ends are checked intact; strided INPUTS hold the canary in
their gaps too, so a read with the wrong stride shows.  Every case runs twice on the same inputs and must give the same bits, and in two kinds:
  random       Gaussian operands, W scaled by 1 / sqrt(K): held to the bound (`RATIO <family> <worst>` is printed);
  structured   integers in [-2, 2] (bias and gradients too; saved activation outputs with a derivative of exactly 0 or 1): every sum is exact in fp32 and in
               bf16, so the result must be bit-exact and the failure names the first wrong (row, column).  A missing term in a long sum, which the bound
               cannot see in every element (tests/test_dense_reference_cpu.py), is seen here.  No sigmoid; LeakyReLU derivatives on the branch '1' only.
The shapes (oracle/dense64.py) are the smallest that cross each seam of the dispatch:
  cvae_linear_fwd         skinny 1x64x1 .. 5x2100x3 (tail loop only, one unrolled trip, 1 / 2 / 4 k-chunks with a short last one; workspace full, NULL, one
                          float short); fp32 GEMM 7x10x64 .. 17x5000x3 (unsplit kernel epilogue, 2 splits of 64 + 49 and 80 + 50, 63 slabs: the slab sum's 8-wide
                          walk with a remainder; NULL / short workspace: unsplit); bf16 64-tile; bf16 128-tile (1 split of 4 stages, 5 stages: the zero-stashed
                          padding stage, 3 splits with a short last one, n_slow either way; odd strides under the dword-aligned vector loads and stores, and
                          once with both operands offset by one float: 4-byte aligned only, in all three bf16 products)
  cvae_linear_bwd_data    skinny wide (1, 2, 12 n-chunks) and narrow (1, 2, 250 chunks), y_act on dy's stride; the GEMM with in_act in the kernel epilogue
                          (unsplit) and in the slab sum (split); the (k-contiguous, row-contiguous) 128-tile instantiation
  cvae_linear_bwd_weight  rows kernel, flat kernel up to N K = 4 194 495 (the grid-stride second trip past 16384 x 256), GEMM with A = dy^T, the (row, row)
                          128-tile instantiation with N and K a 128-multiple + 1 / + 3 (the clamped loads' shifts 1 and 3)
  cvae_small_dense_*      M = 17, 32, 145, 1000 x K x N = 1x1 .. 128x96 / 96x128 (N K = 12288: more than 48 KB of LDS); x 16-byte aligned, offset by one float
                          (scalar copy), x_stride = K + 1; every activation code for act and in_act; y_stride != dy_stride
Row strides are x_stride = K + 3, y_stride = N + 5, dy_stride = N + 3, dx_stride = K + 1 unless the table says otherwise.

Measured on the MI355X, max |got - ref| / err per family (the CPU fp32 stand-in of tests/test_dense_reference_cpu.py in brackets):
  cvae_linear_fwd         skinny 0.0000 - 0.032 [0.051];  fp32 GEMM 0.0005 - 0.149 [0.139];  bf16 64-tile 0.010 - 0.034 [0.040];  bf16 128-tile 0.007 - 0.030 [0.039]
  cvae_linear_bwd_data    skinny 0.003 - 0.315 [0.236];  fp32 GEMM 0.0005 - 0.141 [0.135];  bf16 64-tile 0.012 - 0.042, 128-tile 0.007 - 0.033 [both 0.112]
  cvae_linear_bwd_weight  rows 0.0000 - 0.311 [0.311];  flat 0.086 - 0.359 [0.331];  fp32 GEMM 0.001 - 0.067 [0.132];  bf16 64-tile 0.017 - 0.028, 128-tile 0.005 - 0.026 [both 0.141]
  cvae_small_dense_*      fwd 0.009 - 0.309 [0.321];  bwd_data 0.043 - 0.333 [0.333];  bwd_weight 0.0000 - 0.273 [0.273]
__expf, measured for the sigmoid's bound: 7.75 ulp over [-8, 8] (oracle/dense64.py ULP).
No ratio is above 1, every structured case is bit-exact, every pair of runs gives the same bits and every canary is intact: no case of this file found a
wrong result in csrc/linear.hip or csrc/small_dense.hip (the findings are in the argument checks: see tests/test_dense_reference_cpu.py).  The ratios near 0.3
belong to results of few terms (M <= 16 batch sums, K or N of 1 - 10, the three roundings of a sigmoid derivative), where one or two roundings are a third of
the bound, and the CPU stand-in reaches the same figures; the long sums sit far below (0.0005 - 0.15), as in the loss file: the rule allows a random walk over
all K roundings, while the MFMA tiles, the wave-wide trees of the skinny forward (0.03) and the slab sums add short chains.  The exact 0.0000 are one-term sums
(1 x 256 x 1, K = 1) and all-zero gradients.  What the bound cannot see in a long sum the structured cases do (tests/test_dense_reference_cpu.py, part 2).
"""
import ctypes as C
import functools

import pytest
import torch

from causal_vae_amd import _lib as L
from oracle import dense64 as d64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
CANARY = -777.25
UNSUPPORTED, WORKSPACE = -3, -4
KINDS = ["random", "structured"]


class Mat:
    """an [R][Cc] matrix of row stride `stride`, `lead` floats into a canary-filled device buffer (gaps, lead and tail hold the canary)"""

    def __init__(self, R, Cc, stride=None, lead=0, src=None):
        self.R, self.Cc, self.stride, self.lead = R, Cc, stride or Cc, lead
        self.buf = torch.full((lead + R * self.stride + 8,), CANARY, dtype=F32, device=DEV)
        if src is not None:
            self.view(self.buf).copy_(src)

    def view(self, buf):
        return buf[self.lead:self.lead + self.R * self.stride].view(self.R, self.stride)[:, :self.Cc]

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.lead)

    def reset(self):
        self.buf.fill_(CANARY)

    def get(self):
        return self.view(self.buf).cpu().clone()

    def intact(self):
        b = self.buf.clone()
        self.view(b).fill_(CANARY)
        return bool((b == CANARY).all())

    def untouched(self):
        return bool((self.buf == CANARY).all())


def mat(t, stride=None, lead=0):
    return None if t is None else Mat(t.shape[0], t.shape[1], stride, lead, src=t)


def vec(t):
    return None if t is None else Mat(1, t.numel(), src=t.reshape(1, -1))


def p(m):
    return None if m is None else m.ptr


class Workspace:
    """`floats` of device scratch followed by canaries; mode 'full': all of it, 'null': none, 'short': one float less than `need`"""

    def __init__(self, floats):
        self.floats = floats
        self.buf = torch.full((floats + 16,), CANARY, dtype=F32, device=DEV)

    def args(self, mode, need=0):
        if mode == "null":
            return None, 0
        if mode == "short":
            assert 0 < need <= self.floats, "this case never splits: there is no workspace to fall short of"
            return C.c_void_p(self.buf.data_ptr()), (need - 1) * 4
        return C.c_void_p(self.buf.data_ptr()), self.floats * 4

    def intact(self):
        return bool((self.buf[self.floats:] == CANARY).all())


def linear_ws(op, M, K, N):
    return Workspace(L.lib.cvae_linear_workspace_bytes(M, K, N, op) // 4)


def launch_twice(name, args, outs, ws=None):
    """the call twice into re-filled outputs: rc 0, canaries intact, the same bits; returns the outputs of the first run"""
    runs = []
    for _ in range(2):
        for o in outs:
            o.reset()
        rc = getattr(L.lib, name)(*args, None)
        assert rc == 0, f"{name}: {L.strerror(rc)}"
        torch.cuda.synchronize()
        runs.append([o.get() for o in outs])
        assert all(o.intact() for o in outs), f"{name} wrote outside its output"
        assert ws is None or ws.intact(), f"{name} wrote past the advertised workspace"
    for a, b in zip(*runs):
        assert torch.equal(a, b), f"{name}: two runs on the same inputs gave different bits"
    return runs[0]


def refused(name, args, outs, want):
    rc = getattr(L.lib, name)(*args, None)
    torch.cuda.synchronize()
    assert rc == want, f"{name}: {rc} ({L.strerror(rc)}), expected {want}"
    assert all(o.untouched() for o in outs), f"{name} refused the call but wrote"


WORST = {}


def check(family, kind, got, ref, err):
    """random: within the bounds (RATIO printed); structured: bit-exact, the first wrong (row, column) named"""
    for k, g in got.items():
        want = ref[k].reshape(g.shape)
        if kind == "structured":
            w32 = want.to(F32)                                   # exact, but for a forward LeakyReLU's slope product: one correctly rounded fp32 product of an exact sum
            if not torch.equal(g, w32):
                r, c = (int(v) for v in torch.nonzero(g != w32)[0])
                pytest.fail(f"{family} {k}: {int((g != w32).sum())}/{g.numel()} wrong; first at (row {r}, column {c}): got {float(g[r, c])} want {float(w32[r, c])}")
        else:
            worst = d64.max_ratio(g, ref[k], err[k])
            WORST[family] = max(WORST.get(family, 0.0), worst)
            print(f"RATIO {family} {worst:.4f}")
            bad = d64.compare({k: g}, ref, err, [k])
            assert not bad, f"{family}: " + "\n".join(bad)


@functools.lru_cache(maxsize=64)
def case(kind, M, K, N):
    return d64.operands(kind, 1, M, K, N)


def acts_of(kind):
    return [a for a in d64.ACTS if not (kind == "structured" and a == d64.SIGMOID)]


def rounded(bf16_math, *ts):
    return tuple(d64.bf16(t) if bf16_math else t for t in ts)


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(fn, family, kind, M, K, N, act, bias, mode="full", bf16_math=0, xs=3, ys=5, lead=0):
    c = case(kind, M, K, N)
    b = c["b"] if bias else None
    x, W, bv, y = mat(c["x"], K + xs, lead), mat(c["W"], None, lead), vec(b), Mat(M, N, N + ys)
    if fn == "cvae_linear_fwd":
        ws = linear_ws(0, M, K, N)
        wsp, wsb = ws.args(mode, d64.workspace_floats(0, M, K, N, bool(bf16_math)))
        args = (x.ptr, W.ptr, p(bv), y.ptr, M, K, N, x.stride, y.stride, act, bf16_math, wsp, wsb)
    else:
        ws = None
        args = (x.ptr, W.ptr, p(bv), y.ptr, M, K, N, x.stride, y.stride, act)
    got, = launch_twice(fn, args, [y], ws)
    xr, Wr = rounded(bf16_math, c["x"], c["W"])
    check(family, kind, dict(y=got), *d64.fwd(xr, Wr, b, act))


FWD_SKINNY_MODES = [(s, "full") for s in d64.FWD_SKINNY] + [((3, 1100, 7), "null"), ((3, 1100, 7), "short"), ((5, 2100, 3), "null")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", FWD_SKINNY_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in FWD_SKINNY_MODES])
def test_linear_fwd_skinny(shape, mode, kind):
    assert d64.path(0, *shape) == "skinny"
    for act in acts_of(kind):
        for bias in (True, False):
            run_fwd("cvae_linear_fwd", "fwd_skinny", kind, *shape, act, bias, mode)


FWD_GEMM_MODES = [(s, "full") for s in d64.FWD_GEMM] + [((65, 130, 67), "null"), ((65, 130, 67), "short"), ((17, 5000, 3), "null")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", FWD_GEMM_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in FWD_GEMM_MODES])
def test_linear_fwd_gemm_f32(shape, mode, kind):
    assert d64.path(0, *shape) == "gemm64"
    for act in acts_of(kind):
        for bias in (True, False):
            run_fwd("cvae_linear_fwd", "fwd_gemm_f32", kind, *shape, act, bias, mode)


FWD_BF16_MODES = [(s, "full") for s in d64.FWD_BF16_64 + d64.FWD_BF16_128] + [((100, 200, 130), "null"), ((129, 400, 133), "null"), ((129, 400, 133), "short")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", FWD_BF16_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in FWD_BF16_MODES])
def test_linear_fwd_bf16(shape, mode, kind):
    family = "fwd_bf16_t128" if shape in d64.FWD_BF16_128 else "fwd_bf16_t64"
    assert d64.path(0, *shape, bf16_math=True) == ("gemm128" if shape in d64.FWD_BF16_128 else "gemm64")
    for act in acts_of(kind):
        for bias in (True, False):
            run_fwd("cvae_linear_fwd", family, kind, *shape, act, bias, mode, bf16_math=1, xs=3, ys=5)     # x_stride and y_stride odd for the 128-tile shapes' odd K / N too
    run_fwd("cvae_linear_fwd", family, kind, *shape, d64.RELU, True, mode, bf16_math=1, xs=0, ys=0)
    run_fwd("cvae_linear_fwd", family, kind, *shape, d64.NONE, True, mode, bf16_math=1, xs=0, ys=0, lead=1)             # x and W 4-byte aligned only


def test_linear_fwd_bf16_refuses_the_skinny_range():
    c = case("random", 16, 64, 8)
    x, W, y = mat(c["x"]), mat(c["W"]), Mat(16, 8)
    ws = linear_ws(0, 16, 64, 8)
    refused("cvae_linear_fwd", (x.ptr, W.ptr, None, y.ptr, 16, 64, 8, 64, 8, 0, 1, *ws.args("full")), [y], UNSUPPORTED)


# ------------------------------------------------------------------------------------------------ backward-data
def run_bwd_data(fn, family, kind, M, K, N, act, with_y, in_act=0, mode="full", bf16_math=0, dys=3, dxs=1, ys=None, xs=2, lead=0):
    c = case(kind, M, K, N)
    ya = d64.act_output(kind, 5, M, N, act) if with_y else None
    xin = d64.act_output(kind, 6, M, K, in_act)
    ys = dys if ys is None else ys
    dy, W, dx, yam, xim = mat(c["dy"], N + dys, lead), mat(c["W"], None, lead), Mat(M, K, K + dxs), mat(ya, N + ys), mat(xin, K + xs)
    if fn == "cvae_linear_bwd_data":
        ws = linear_ws(1, M, K, N)
        wsp, wsb = ws.args(mode, d64.workspace_floats(1, M, K, N, bool(bf16_math), ya is not None, in_act != 0))
        args = (dy.ptr, W.ptr, dx.ptr, M, K, N, dy.stride, dx.stride, p(yam), act, p(xim), K + xs, in_act, bf16_math, wsp, wsb)
    else:
        ws = None
        args = (dy.ptr, W.ptr, dx.ptr, p(yam), act, p(xim), in_act, M, K, N, dy.stride, dx.stride, N + ys, K + xs)
    got, = launch_twice(fn, args, [dx], ws)
    dyr, Wr = rounded(bf16_math, c["dy"], c["W"])
    check(family, kind, dict(dx=got), *d64.bwd_data(dyr, Wr, ya, act, xin, in_act))


WIDE_MODES = [(s, "full") for s in d64.BWD_DATA_WIDE] + [((4, 1030, 40), "null"), ((4, 1030, 40), "short"), ((16, 1500, 200), "null")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", WIDE_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in WIDE_MODES])
def test_linear_bwd_data_skinny_wide(shape, mode, kind):
    assert d64.path(1, *shape) == "skinny"
    for act in acts_of(kind):
        for with_y in (True, False):
            run_bwd_data("cvae_linear_bwd_data", "bwd_data_skinny", kind, *shape, act, with_y, mode=mode)


NARROW_MODES = [(s, "full") for s in d64.BWD_DATA_NARROW] + [((16, 70, 23), "null"), ((2, 300, 3000), "short")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", NARROW_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in NARROW_MODES])
def test_linear_bwd_data_skinny_narrow(shape, mode, kind):
    assert d64.path(1, *shape, y_act=True) == "skinny"
    for act in acts_of(kind)[1:]:
        run_bwd_data("cvae_linear_bwd_data", "bwd_data_skinny", kind, *shape, act, True, mode=mode)


GEMM_DATA_MODES = [(s, "full") for s in d64.BWD_DATA_GEMM] + [((65, 67, 130), "null"), ((65, 67, 130), "short")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", GEMM_DATA_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in GEMM_DATA_MODES])
def test_linear_bwd_data_gemm_f32(shape, mode, kind):
    assert d64.path(1, *shape) == "gemm64"
    run_bwd_data("cvae_linear_bwd_data", "bwd_data_gemm_f32", kind, *shape, 0, False, mode=mode)
    if shape[0] > d64.SK_M:
        for in_act in acts_of(kind)[1:]:                         # (65, 67, 112): in the kernel epilogue; (65, 67, 130): in the slab sum, or unsplit without workspace
            run_bwd_data("cvae_linear_bwd_data", "bwd_data_gemm_f32", kind, *shape, 0, False, in_act=in_act, mode=mode)


BF16_DATA_MODES = [(s, "full") for s in d64.BWD_DATA_BF16] + [((100, 130, 200), "null"), ((129, 133, 400), "null")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,mode", BF16_DATA_MODES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{m}" for s, m in BF16_DATA_MODES])
def test_linear_bwd_data_bf16(shape, mode, kind):
    big = shape[0] >= 128
    assert d64.path(1, *shape, bf16_math=True) == ("gemm128" if big else "gemm64")
    family = "bwd_data_bf16_t128" if big else "bwd_data_bf16_t64"
    run_bwd_data("cvae_linear_bwd_data", family, kind, *shape, 0, False, mode=mode, bf16_math=1)
    run_bwd_data("cvae_linear_bwd_data", family, kind, *shape, 0, False, mode=mode, bf16_math=1, dys=0, dxs=0, lead=1)   # dy and W 4-byte aligned only
    for in_act in (d64.RELU, d64.LEAKY02) + (() if kind == "structured" else (d64.SIGMOID,)):
        run_bwd_data("cvae_linear_bwd_data", family, kind, *shape, 0, False, in_act=in_act, mode=mode, bf16_math=1)


def test_linear_bwd_data_refuses_y_act_above_the_skinny_range():
    c = case("random", 17, 20, 5)
    ya = d64.act_output("random", 5, 17, 5, d64.RELU)
    dy, W, dx, yam = mat(c["dy"]), mat(c["W"]), Mat(17, 20), mat(ya)
    ws = linear_ws(1, 17, 20, 5)
    refused("cvae_linear_bwd_data", (dy.ptr, W.ptr, dx.ptr, 17, 20, 5, 5, 20, yam.ptr, d64.RELU, None, 0, 0, 0, *ws.args("full")), [dx], UNSUPPORTED)


# ------------------------------------------------------------------------------------------------ backward-weight
def run_bwd_weight(fn, family, kind, M, K, N, act, with_y, with_db, bf16_math=0, dys=3, xs=3, ys=None, mode="full", lead=0):
    c = case(kind, M, K, N)
    ya = d64.act_output(kind, 5, M, N, act) if with_y else None
    ys = dys if ys is None else ys
    dy, x, yam, dW, db = mat(c["dy"], N + dys, lead), mat(c["x"], K + xs, lead), mat(ya, N + ys), Mat(N, K), Mat(1, N)
    if fn == "cvae_linear_bwd_weight":
        ws = linear_ws(2, M, K, N)
        wsp, wsb = ws.args(mode, d64.workspace_floats(2, M, K, N, bool(bf16_math)))
        args = (dy.ptr, x.ptr, dW.ptr, db.ptr if with_db else None, M, K, N, dy.stride, x.stride, p(yam), act, bf16_math, wsp, wsb)
    else:
        ws = Workspace(L.lib.cvae_small_dense_workspace_bytes(M, K, N) // 4)
        args = (dy.ptr, x.ptr, dW.ptr, db.ptr if with_db else None, p(yam), act, M, K, N, dy.stride, x.stride, N + ys, *ws.args("full"))
    got = launch_twice(fn, args, [dW, db], ws)
    assert with_db or db.untouched()
    dyr, xr = rounded(bf16_math, c["dy"], c["x"])
    ref, err = d64.bwd_weight(dyr, xr, ya, act, dy_db=c["dy"] if bf16_math else None)
    check(family, kind, dict(dW=got[0], db=got[1]) if with_db else dict(dW=got[0]), ref, err)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", d64.BWD_WEIGHT_ROWS + d64.BWD_WEIGHT_FLAT, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_linear_bwd_weight_skinny(shape, kind):
    family = "bwd_weight_rows" if shape in d64.BWD_WEIGHT_ROWS else "bwd_weight_flat"
    if shape[2] > 10000:                                        # N K = 4 194 495: the flat kernel's second grid-stride trip; one pass each way
        run_bwd_weight("cvae_linear_bwd_weight", family, kind, *shape, d64.RELU, True, True)
        run_bwd_weight("cvae_linear_bwd_weight", family, kind, *shape, 0, False, False)
        return
    for act in acts_of(kind):
        for with_y in (True, False):
            for with_db in (True, False):
                run_bwd_weight("cvae_linear_bwd_weight", family, kind, *shape, act, with_y, with_db)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["full", "null"])
@pytest.mark.parametrize("shape", d64.BWD_WEIGHT_GEMM, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_linear_bwd_weight_gemm_f32(shape, mode, kind):
    assert d64.path(2, *shape) == "gemm64"
    run_bwd_weight("cvae_linear_bwd_weight", "bwd_weight_gemm_f32", kind, *shape, 0, False, False, mode=mode)                 # dy_stride = N + 3: db NULL
    run_bwd_weight("cvae_linear_bwd_weight", "bwd_weight_gemm_f32", kind, *shape, 0, False, True, dys=0, mode=mode)          # db through cvae_channel_sum


def test_linear_bwd_weight_refuses_db_on_a_strided_dy_before_any_launch():
    M, K, N = 130, 67, 65
    c = case("random", M, K, N)
    dy, x, dW, db = mat(c["dy"], N + 3), mat(c["x"]), Mat(N, K), Mat(1, N)
    ws = linear_ws(2, M, K, N)
    refused("cvae_linear_bwd_weight", (dy.ptr, x.ptr, dW.ptr, db.ptr, M, K, N, N + 3, K, None, 0, 0, *ws.args("full")), [dW, db], UNSUPPORTED)


BF16_WEIGHT = d64.BWD_WEIGHT_BF16_64 + d64.BWD_WEIGHT_BF16_128


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["full", "null"])
@pytest.mark.parametrize("shape", BF16_WEIGHT, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_linear_bwd_weight_bf16(shape, mode, kind):
    big = shape in d64.BWD_WEIGHT_BF16_128
    assert d64.path(2, *shape, bf16_math=True) == ("gemm128" if big else "gemm64")
    family = "bwd_weight_bf16_t128" if big else "bwd_weight_bf16_t64"
    run_bwd_weight("cvae_linear_bwd_weight", family, kind, *shape, 0, False, False, bf16_math=1, mode=mode)
    run_bwd_weight("cvae_linear_bwd_weight", family, kind, *shape, 0, False, True, bf16_math=1, dys=0, xs=0, mode=mode)
    run_bwd_weight("cvae_linear_bwd_weight", family, kind, *shape, 0, False, False, bf16_math=1, dys=0, xs=0, mode=mode, lead=1)      # dy and x 4-byte aligned only


# ------------------------------------------------------------------------------------------------ small_dense
LAYOUTS = {"aligned": dict(xs=0, lead=0), "offset": dict(xs=0, lead=1), "strided": dict(xs=1, lead=0)}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("K,N", d64.SD_KN)
@pytest.mark.parametrize("M", d64.SD_M)
def test_small_dense_fwd(M, K, N, layout, kind):
    assert L.lib.cvae_small_dense_supported(M, K, N) == 1
    for act in acts_of(kind):
        run_fwd("cvae_small_dense_fwd", "small_dense_fwd", kind, M, K, N, act, act != d64.LEAKY02, ys=5, **LAYOUTS[layout])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("K,N", d64.SD_KN)
@pytest.mark.parametrize("M", d64.SD_M)
def test_small_dense_bwd_data(M, K, N, layout, kind):
    lead = LAYOUTS[layout]["lead"]
    acts = acts_of(kind)
    for i, act in enumerate(acts):                               # every act with y_act, every in_act with x_in, each once without its tensor
        in_act = acts[(i + 2) % len(acts)]
        run_bwd_data("cvae_small_dense_bwd_data", "small_dense_bwd_data", kind, M, K, N, act, True, in_act=in_act, ys=7, lead=lead)
    run_bwd_data("cvae_small_dense_bwd_data", "small_dense_bwd_data", kind, M, K, N, d64.RELU, False, in_act=0, ys=7, lead=lead)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("K,N", d64.SD_KN)
@pytest.mark.parametrize("M", d64.SD_M)
def test_small_dense_bwd_weight(M, K, N, layout, kind):
    lo = LAYOUTS[layout]
    for act in acts_of(kind):
        run_bwd_weight("cvae_small_dense_bwd_weight", "small_dense_bwd_weight", kind, M, K, N, act, True, act != d64.LEAKY001, xs=lo["xs"], ys=7, lead=lo["lead"])
    run_bwd_weight("cvae_small_dense_bwd_weight", "small_dense_bwd_weight", kind, M, K, N, d64.RELU, False, True, xs=lo["xs"], ys=7, lead=lo["lead"])


def test_small_dense_limits():
    sup, wsb = L.lib.cvae_small_dense_supported, L.lib.cvae_small_dense_workspace_bytes
    for M, K, N, ok in ((17, 128, 96, 1), (17, 96, 128, 1), (16, 10, 10, 0), (17, 129, 1, 0), (17, 1, 129, 0), (17, 128, 97, 0), (17, 0, 5, 0), (1 << 30, 4, 4, 0)):
        assert sup(M, K, N) == ok, (M, K, N)
        assert wsb(M, K, N) == (((M + 15) // 16) * (N * K + N) * 4 if ok else 0), (M, K, N)
    M, K, N = 145, 10, 64
    c = case("random", M, K, N)
    dy, x, dW, db = mat(c["dy"]), mat(c["x"]), Mat(N, K), Mat(1, N)
    ws = Workspace(wsb(M, K, N) // 4)
    refused("cvae_small_dense_bwd_weight", (dy.ptr, x.ptr, dW.ptr, db.ptr, None, 0, M, K, N, N, K, N, C.c_void_p(ws.buf.data_ptr()), wsb(M, K, N) - 4), [dW, db], WORKSPACE)
    assert bool((ws.buf == CANARY).all())


def test_zz_worst_ratios():
    """the summary line per family of the module docstring (runs last in this file)"""
    for k in sorted(WORST):
        print(f"WORST {k} {WORST[k]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
