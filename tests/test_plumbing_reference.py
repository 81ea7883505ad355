"""csrc/elementwise.hip and csrc/vessel2d.hip through the raw C ABI against the float64 references of oracle/plumbing64.py: ONE launch and ONE comparison per
case, with the elementwise bounds derived there (U = 2^-24, C = 4: C sqrt(T) U sum |terms| for a sum of T terms, one U per fp32 operation, the measured ulps of
__expf / div / sqrtf, the tap-position term of the resize, the two-pass rule of the BatchNorm).  tests/test_plumbing_reference_cpu.py shows that the bounds are
neither loose nor wrong, replays the launch geometry, and holds the entry points' argument checks to include/cvae_hip.h.

Every output lives inside a canary-filled buffer, so the gaps of a strided output, its lead and its tail are checked intact; strided INPUTS hold the canary in their
gaps too.  Every case runs twice on the same inputs and must give the same bits (both files promise sums without float atomics), and in two kinds:
  random       Gaussian operands: held to the bound (`RATIO <family> <worst>` is printed);
  structured   small integers (pool gradients 27 x integers, exact-2x resize 64 x integers): every sum and quotient is exact in fp32, so the result must be
               bit-exact (one correctly rounded product, division or bf16 conversion at the end) and the failure names the first wrong index.  A dropped row of a
               16385-row channel sum, which the bound cannot see in every channel, is seen here.  Where a family has no exact form (a resize at a ratio other than
               1, 2, 1/2; the BatchNorm statistics) the structured operands are held to the bound.
The pure moves (cast, transposes, panels, one-hot, flatten, clamp) are bit-exact in BOTH kinds and for all four dtype pairs: float -> bf16 is round-to-nearest-even,
+-0, +-inf, NaN, denormals and exact ties included (a NaN must stay a NaN; its payload is free).
The shapes (oracle/plumbing64.py, the seam named next to each row) are the smallest that cross each seam: n = 1, 257, 524 293 (past the 2048 x 256 grid cap);
transposes C x S over the 64-tile's 63 / 64 / 65 and three tiles; flatten V x C likewise with strides above C V; the channel sum's vector / fold / scalar paths with
their idle threads, non-power-of-two trees, loop remainders, second blockIdx.y, row blocks with the finish pass, the 1024 / gy cap (67 MB), a misaligned x, and the
workspace full, NULL and one float short; pools with divisible, overlapping and OUTPUT-LARGER windows; resizes at non-integer ratios, 1 -> 5, 5 -> 1, 3D, at
3 -> 7 (a tap position within rounding of an integer), and the exact-2x kernels up to more than 8192 x 256 work items (34 MB and 68 MB); k3 <-> k4 with a block
tail; BatchNorm2d at C = 8, 24, 40, 264, 2048 x P = 2, 3, R - 1, 16 R + 1 and once over the scratch's 1024-row cap (67 MB of bf16).

FINDINGS (all fixed with this file; tests/test_plumbing_reference_cpu.py lists the header's side):
  avgpool_bwd_kernel    looked for the windows containing input index i only among floor(i O / I) - 1 .. + 1 and lost gradient terms whenever an output axis is more
                        than about twice its input (1 -> 3, 2 -> 5, 2 -> 7 ...): test_pool_bwd at (1, 2, 2) -> (1, 7, 7), (1, 1, 1) -> (1, 3, 3) and (2, 2, 1) -> (5, 5, 4)
                        fails on the former arithmetic (plumbing64's 'pm1' mutation IS that arithmetic).  The kernel visits exactly floor(i O / I) ..
                        ceil((i + 1) O / I) - 1 now, without a membership test; test_pool_bwd_bits_of_the_sequential_sum holds every O <= I case to the bits of the
                        same ascending fp32 sum, which is what the former rule computed there.
  clamp_fwd_kernel      fminf(fmaxf(x, lo), hi) turned a NaN into lo; torch.clamp (the header's contract) keeps it: the kernel does now (test_clamp).
  bn2d_finalize_rstd_kernel  wrote running_var whenever running_mean was given, though the header lets either be NULL: each on its own now (test_bn2d_running_mean_alone).

Measured on the MI355X, max |got - ref| / err per family, fp32 outputs / bf16 outputs (the CPU fp32 stand-in of tests/test_plumbing_reference_cpu.py in brackets):
  act_fwd          0.985 / 0.996 [0.965]     act_bwd         0.985 / 0.996 [0.963]     channel_sum    0.179 [0.179]          k3 <-> k4       0.288 [0.218]
  pool_fwd         0.249 [0.188]             pool_bwd        0.241 / 0.996 [0.199]     resize_fwd     0.370 [0.482]          resize_bwd      0.297 / 0.987 [0.314]
  resize2x_fwd     0.127 [0.141]             resize2x_bwd    0.035 / 0.845 [0.036]
  bn2d_fwd_train   0.466 / 0.995 [0.466]     bn2d_fwd_eval   0.652 / 0.995 [0.813]     bn2d_bwd       0.364 / 0.996 [0.364]
No ratio is above 1, every structured and pure-move case is bit-exact, every pair of runs gives the same bits and every canary is intact (350 cases, 16 s).
The ratios near 1 are results of ONE rounding, where that rounding is the whole bound: a LeakyReLU's slope product (U |y| against an error of up to U |y|; the CPU
stand-in reaches 0.965 the same way), and every bf16 output, whose half bf16 ulp (2^-8 |y|) is 250 times the fp32 part of its bound; they cannot pass 1 while
the conversion rounds to nearest.  The BatchNorm figures (0.36 - 0.65) belong to P = 2 and 3 and to the eval forward: three to five roundings against a bound of
about as many, and the CPU stand-in reaches the same or more; resize_fwd's 0.37 is the 3 -> 7 case, where the tap term of a position next to an
integer is most of a small bound (the stand-in: 0.48).  The sums sit at 0.03 - 0.3, as in the dense and loss files: the rule allows a random walk over all
roundings, while the kernels' trees and row blocks add short chains.
"""
import ctypes as C
import functools

import pytest
import torch

from causal_vae_amd import _lib as L
from oracle import plumbing64 as p64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
CANARY = -776.0                                                  # exact in bf16
WORKSPACE = -4
KINDS = ["random", "structured"]
DT = {F32: L.F32, BF16: L.BF16}
DTYPES = [F32, BF16]


class Buf:
    """[rows][cols] elements of `dtype` at columns col0 .. of rows of `stride` elements, `lead` elements into a canary-filled device buffer (gaps, lead and tail hold
    the canary); ptr is the address of row 0, column 0 of the strided matrix"""

    def __init__(self, rows, cols, dtype=F32, stride=None, lead=0, col0=0, src=None):
        self.rows, self.cols, self.stride, self.lead, self.col0, self.dtype = rows, cols, stride or (col0 + cols), lead, col0, dtype
        self.buf = torch.full((lead + rows * self.stride + 16,), CANARY, dtype=dtype, device=DEV)
        if src is not None:
            self.view(self.buf).copy_(src.reshape(rows, cols).to(dtype))

    def view(self, buf):
        return buf[self.lead:self.lead + self.rows * self.stride].view(self.rows, self.stride)[:, self.col0:self.col0 + self.cols]

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.buf.element_size() * self.lead)

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


def flat(t, dtype=F32, lead=0):
    return None if t is None else Buf(1, t.numel(), dtype, lead=lead, src=t.reshape(1, -1))


def p(b):
    return None if b is None else b.ptr


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
        assert bool(p64.same_bits(a, b).all()), f"{name}: two runs on the same inputs gave different bits"
    return runs[0]


def refused(name, args, outs, want):
    rc = getattr(L.lib, name)(*args, None)
    torch.cuda.synchronize()
    assert rc == want, f"{name}: {rc} ({L.strerror(rc)}), expected {want}"
    assert all(o.untouched() for o in outs), f"{name} refused the call but wrote"


WORST = {}


def exact(family, got, want):
    """bit-exact (a NaN for a NaN); the failure names the first wrong flat index"""
    want = want.reshape(got.shape)
    same = p64.same_bits(got, want)
    if not bool(same.all()):
        i = int(torch.nonzero(~same.reshape(-1))[0])
        pytest.fail(f"{family}: {int((~same).sum())}/{same.numel()} wrong; first at flat {i}: got {float(got.reshape(-1)[i])} want {float(want.reshape(-1)[i])}")


def check(family, kind, got, ref, err, bound_only=False):
    """random: within the bounds (RATIO printed); structured: bit-exact after the one final rounding"""
    for k, g in got.items():
        if kind == "structured" and not bound_only:
            want = ref[k].to(F32)
            exact(f"{family} {k}", g, want if g.dtype == F32 else want.to(BF16))
        else:
            fam = family + ("/bf16" if g.dtype == BF16 else "")          # a bf16 output's one rounding is most of its bound: kept apart
            worst = p64.max_ratio(g.float(), ref[k], err[k])
            WORST[fam] = max(WORST.get(fam, 0.0), worst)
            print(f"RATIO {fam} {worst:.4f}")
            bad = p64.compare({k: g.float()}, ref, err, [k])
            assert not bad, f"{family}: " + "\n".join(bad)


def rounded(dtype, *ts):
    return tuple(p64.bf16(t) if dtype == BF16 and t is not None else t for t in ts)


def with_specials(v):
    sp = p64.specials()
    if v.numel() >= 2 * sp.numel():
        v = v.clone()
        v.reshape(-1)[:sp.numel()] = sp
    return v


# ------------------------------------------------------------------------------------------------ cast, activation, clamp
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", p64.N_ELEMENTWISE)
def test_cast(n, kind):
    x = with_specials(p64.operands(kind, 1, n) if n > 1 else torch.tensor([-0.0]))
    for sd in DTYPES:
        for dd in DTYPES:
            src, dst = flat(x, sd), Buf(1, n, dd)
            got, = launch_twice("cvae_cast", (src.ptr, dst.ptr, n, DT[sd], DT[dd]), [dst])
            exact(f"cast {sd} -> {dd}", got, p64.cast(src.get(), dd)[0]["dst"])


def acts_of(kind):
    return [a for a in p64.ACTS if not (kind == "structured" and a == p64.SIGMOID)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", p64.N_ELEMENTWISE)
def test_act(n, kind):
    for dt in DTYPES:
        for act in acts_of(kind):
            x, = rounded(dt, p64.act_input(kind, 1, n))
            xb, yb = flat(x, dt), Buf(1, n, dt)
            got, = launch_twice("cvae_act_fwd", (xb.ptr, yb.ptr, n, act, DT[dt]), [yb])
            check("act_fwd", kind, dict(y=got), *p64.act_fwd(x, act, out_bf16=dt == BF16))
            ya = p64.act_output(kind, 5, n, act)
            dy, y = rounded(dt, p64.operands(kind, 2, n), x if ya is None else ya)
            dyb, yb, dxb = flat(dy, dt), flat(y, dt), Buf(1, n, dt)
            got, = launch_twice("cvae_act_bwd", (dyb.ptr, yb.ptr, dxb.ptr, n, act, DT[dt]), [dxb])
            check("act_bwd", kind, dict(dx=got), *p64.act_bwd(dy, y, act, out_bf16=dt == BF16))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", p64.N_ELEMENTWISE)
def test_clamp(n, kind):
    """torch.clamp: a NaN stays a NaN (the kernel answered lo), x == lo and x == hi pass the gradient, +-inf clamp"""
    lo, hi = -0.5, 0.75
    x = with_specials(p64.operands(kind, 1, n) if n > 1 else torch.tensor([float("nan")]))
    if n > 100:
        x[60], x[61] = lo, hi
    g = p64.operands(kind, 2, n)
    xb, gb, yb, dxb = flat(x), flat(g), Buf(1, n), Buf(1, n)
    got, = launch_twice("cvae_clamp_fwd", (xb.ptr, yb.ptr, lo, hi, n), [yb])
    exact("clamp_fwd", got, p64.clamp_fwd(x, lo, hi)[0]["y"])
    got, = launch_twice("cvae_clamp_bwd", (xb.ptr, gb.ptr, dxb.ptr, lo, hi, n), [dxb])
    exact("clamp_bwd", got, p64.clamp_bwd(x, g, lo, hi)[0]["dx"])


# ------------------------------------------------------------------------------------------------ transposes, flatten
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", p64.TRANSPOSE_S)
@pytest.mark.parametrize("Cc", p64.TRANSPOSE_C)
def test_transposes(Cc, S, kind):
    for B in p64.TRANSPOSE_B:
        x = with_specials(p64.operands(kind, 1, B, Cc, S))
        for sd in DTYPES:
            for dd in DTYPES:
                src, dst = flat(x, sd), Buf(1, B * S * Cc, dd)
                got, = launch_twice("cvae_ncs_to_nsc", (src.ptr, dst.ptr, B, Cc, S, DT[sd], DT[dd]), [dst])
                exact(f"ncs_to_nsc {sd} -> {dd}", got, p64.ncs_to_nsc(src.get().reshape(B, Cc, S), dd)[0]["dst"])
                got, = launch_twice("cvae_nsc_to_ncs", (src.ptr, dst.ptr, B, Cc, S, DT[sd], DT[dd]), [dst])
                exact(f"nsc_to_ncs {sd} -> {dd}", got, p64.nsc_to_ncs(src.get().reshape(B, S, Cc), dd)[0]["dst"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cc", p64.FLATTEN_C)
@pytest.mark.parametrize("V", p64.FLATTEN_V)
def test_flatten(V, Cc, kind):
    """the bare Flatten (1-voxel windows) of cvae_adaptive_avgpool_fwd / _bwd, strides above C V, the mask NULL and given (0, -0.0 and negatives in it)"""
    B, stride = 3, Cc * V + 3
    for dt in DTYPES:
        x = p64.operands(kind, 1, B, V, Cc)
        x.reshape(-1)[0] = -0.0
        xb, out = flat(x, dt), Buf(B, Cc * V, F32, stride)
        got, = launch_twice("cvae_adaptive_avgpool_fwd", (xb.ptr, out.ptr, B, 1, 1, V, Cc, 1, 1, V, stride, DT[dt]), [out])
        exact("flatten_fwd", got, p64.flatten_fwd(xb.get().reshape(B, V, Cc))[0]["out"])
        g = Buf(B, Cc * V, F32, stride, src=p64.operands(kind, 2, B, Cc * V))
        for mask in (None, xb):
            dx = Buf(1, B * V * Cc, dt)
            got, = launch_twice("cvae_adaptive_avgpool_bwd", (g.ptr, p(mask), dx.ptr, B, 1, 1, V, Cc, 1, 1, V, stride, DT[dt]), [dx])
            exact("flatten_bwd", got, p64.flatten_bwd(g.get(), None if mask is None else xb.get().reshape(B, V, Cc), V, Cc, dt)[0]["dx"])


# ------------------------------------------------------------------------------------------------ concat panels, one-hot
PANELS = [
    ("one", 5, [(7, 7)], 7, 0),
    ("one-strided", 5, [(7, 9)], 12, 3),
    ("three-with-a-zero-width", 4, [(3, 4), (0, 0), (5, 5)], 12, 2),
    ("eight", 3, [(1, 1), (2, 5), (3, 3), (4, 4), (5, 9), (6, 6), (7, 7), (8, 8)], 40, 1),
    ("second-grid-stride-trip", 4100, [(64, 66), (66, 66)], 131, 1),              # B total = 533 000 > 524 288
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gather", [0, 1])
@pytest.mark.parametrize("name,B,panels,ws,col0", PANELS, ids=[c[0] for c in PANELS])
def test_copy_panels(name, B, panels, ws, col0, gather, kind):
    tot = sum(w for w, _ in panels)
    vals = [p64.operands(kind, 1 + i, B, w) for i, (w, _) in enumerate(panels)]
    wide_v = p64.operands(kind, 20, B, tot)
    n = len(panels)
    if gather:
        pb = [Buf(B, w, F32, max(s, 1)) for w, s in panels]
        wide = Buf(B, tot, F32, ws, col0=col0, src=wide_v)
        outs = pb
    else:
        pb = [Buf(B, w, F32, max(s, 1), src=v) for (w, s), v in zip(panels, vals)]
        wide = Buf(B, tot, F32, ws, col0=col0)
        outs = [wide]
    ptrs = (C.c_void_p * n)(*[b.ptr for b in pb])
    widths, strides = (C.c_int64 * n)(*[w for w, _ in panels]), (C.c_int64 * n)(*[s for _, s in panels])
    got = launch_twice("cvae_copy_panels", (C.cast(ptrs, C.c_void_p), C.cast(widths, C.c_void_p), C.cast(strides, C.c_void_p), n, wide.ptr, B, ws, col0, gather), outs)
    if gather:
        ref, _ = p64.copy_panels(vals, torch.cat([torch.zeros(B, col0), wide_v], 1), col0, 1)
        for i, g in enumerate(got):
            exact(f"copy_panels gather {i}", g, ref[f"p{i}"])
    else:
        ref, _ = p64.copy_panels(vals, torch.zeros(B, col0 + tot), col0, 0)
        exact("copy_panels", got[0], ref["wide"][:, col0:])


@pytest.mark.parametrize("B,nc,ds,col0", [(1, 1, 1, 0), (7, 19, 30, 5), (700, 19, 19, 0), (30000, 19, 21, 1)])
def test_onehot_panel(B, nc, ds, col0):
    """ds > col0 + nc; a class outside [0, nc) gives an all-zero row; B nc = 570 000 > 524 288 once"""
    t = torch.randint(0, nc, (B,), generator=p64.gen(5))
    if B > 3:
        t[1], t[2], t[3] = -1, nc, nc + 5
    tb = t.to(DEV)
    dst = Buf(B, nc, F32, ds, col0=col0)
    got, = launch_twice("cvae_onehot_panel", (C.c_void_p(tb.data_ptr()), dst.ptr, B, nc, ds, col0), [dst])
    exact("onehot_panel", got, p64.onehot_panel(t, nc)[0]["dst"])
    assert B <= 3 or float(got[1:4].sum()) == 0.0


# ------------------------------------------------------------------------------------------------ channel sum
def run_channel_sum(kind, P, Cc, bf, off, mode):
    dt = BF16 if bf else F32
    x, = rounded(dt, p64.operands(kind, 1, P, Cc))
    xb, out = flat(x, dt, lead=off), Buf(1, Cc)
    geo = p64.channel_sum_geometry(P, Cc, bf, aligned=off == 0)
    ws = Workspace(L.lib.cvae_channel_sum_workspace_bytes(P, Cc, DT[dt]) // 4)
    assert ws.floats >= geo["ws_floats"]
    wsp, wsb = ws.args(mode, geo["ws_floats"])
    got, = launch_twice("cvae_channel_sum", (xb.ptr, out.ptr, P, Cc, DT[dt], wsp, wsb), [out], ws)
    check("channel_sum", kind, dict(out=got), *p64.channel_sum(x))


CS_CASES = [(c, m) for c in p64.CHANNEL_SUM for m in (("full", "null", "short") if p64.channel_sum_geometry(c[0], c[1], c[2], c[3] == 0)["ws_floats"] and c[0] < 16385
                                                      else ("full", "null") if c[0] < 16385 else ("full",))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case,mode", CS_CASES, ids=[f"{c[0]}x{c[1]}{'-bf16' if c[2] else ''}{'-off' if c[3] else ''}-{m}" for c, m in CS_CASES])
def test_channel_sum(case, mode, kind):
    """the same bound in every workspace mode (without scratch ONE row block sums everything); the structured kind is bit-exact: a dropped row shows"""
    run_channel_sum(kind, case[0], case[1], case[2], case[3], mode)


def test_channel_sum_of_no_rows_is_zero():
    out = Buf(1, 19)
    got, = launch_twice("cvae_channel_sum", (None, out.ptr, 0, 19, L.F32, None, 0), [out])
    exact("channel_sum P = 0", got, torch.zeros(1, 19))


# ------------------------------------------------------------------------------------------------ adaptive average pool (generic kernels)
def pool_dout(kind, seed, B, Cc, out):
    v = p64.operands(kind, seed, B, Cc * out[0] * out[1] * out[2])
    return 27.0 * v if kind == "structured" else v             # every quotient by a window of 2^a 3^b voxels is exact


POOL_IDS = [f"{c[1]}->{c[3]}".replace(" ", "") for c in p64.POOL]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", p64.POOL, ids=POOL_IDS)
def test_pool_fwd(case, kind):
    B, dims, Cc, out, _why = case
    OV = out[0] * out[1] * out[2]
    for dt in DTYPES:
        x, = rounded(dt, p64.operands(kind, 1, B, *dims, Cc))
        xb, ob = flat(x, dt), Buf(B, Cc * OV, F32, Cc * OV + 3)
        got, = launch_twice("cvae_adaptive_avgpool_fwd", (xb.ptr, ob.ptr, B, *dims, Cc, *out, ob.stride, DT[dt]), [ob])
        check("pool_fwd", kind, dict(out=got), *p64.pool_fwd(x, out))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", p64.POOL, ids=POOL_IDS)
def test_pool_bwd(case, kind):
    """every window that contains the voxel: (1, 2, 2) -> (1, 7, 7), (1, 1, 1) -> (1, 3, 3) and (2, 2, 1) -> (5, 5, 4) fail on the former three-candidate rule"""
    B, dims, Cc, out, _why = case
    OV = out[0] * out[1] * out[2]
    for dt in DTYPES:
        dout = pool_dout(kind, 2, B, Cc, out)
        x, = rounded(dt, p64.operands(kind, 1, B, *dims, Cc))
        x.reshape(-1)[0] = -0.0
        gb, xb = Buf(B, Cc * OV, F32, Cc * OV + 3, src=dout), flat(x, dt)
        for mask in (None, xb):
            dxb = Buf(1, x.numel(), dt)
            got, = launch_twice("cvae_adaptive_avgpool_bwd", (gb.ptr, p(mask), dxb.ptr, B, *dims, Cc, *out, gb.stride, DT[dt]), [dxb])
            check("pool_bwd", kind, dict(dx=got), *p64.pool_bwd(dout, None if mask is None else x, dims, out, out_bf16=dt == BF16))


@pytest.mark.parametrize("case", p64.POOL, ids=POOL_IDS)
def test_pool_bwd_bits_of_the_sequential_sum(case):
    """the kernel's result IS the ascending fp32 sum of correctly rounded quotients; at the O <= I cases (plumbing64.POOL_LEGACY_COMPLETE, the overlapping windows
    among them) that is what the former candidate rule computed, so making the window range exact changed no bit there"""
    B, dims, Cc, out, _why = case
    dout = pool_dout("random", 2, B, Cc, out)
    gb, dxb = flat(dout), Buf(1, B * dims[0] * dims[1] * dims[2] * Cc)
    got, = launch_twice("cvae_adaptive_avgpool_bwd", (gb.ptr, None, dxb.ptr, B, *dims, Cc, *out, dout.shape[1], L.F32), [dxb])
    exact("pool_bwd sequential", got, p64.pool_bwd_sequential_f32(dout, dims, out))


# ------------------------------------------------------------------------------------------------ linear resize
def resize_exact(dims, out):
    return all(o in (i, 2 * i) or 2 * o == i for i, o in zip(dims, out))


def run_resize(family, kind, B, dims, Cc, out, dtypes=DTYPES):
    scale = 64.0 if kind == "structured" else 1.0
    bound_only = not resize_exact(dims, out)
    for dt in dtypes:
        src, = rounded(dt, scale * p64.operands(kind, 1, B, *dims, Cc))
        sb, db = flat(src, dt), Buf(1, B * out[0] * out[1] * out[2] * Cc)
        got, = launch_twice("cvae_upsample_linear_fwd", (sb.ptr, db.ptr, B, *dims, *out, Cc, DT[dt]), [db])
        check(family + "_fwd", kind, dict(dst=got), *p64.resize_fwd(src, out), bound_only=bound_only)
        del sb, db
        g = scale * p64.operands(kind, 2, B, *out, Cc)
        gb, sb = flat(g), Buf(1, src.numel(), dt)
        got, = launch_twice("cvae_upsample_linear_bwd", (gb.ptr, sb.ptr, B, *dims, *out, Cc, DT[dt]), [sb])
        check(family + "_bwd", kind, dict(dsrc=got), *p64.resize_bwd(g, dims, out_bf16=dt == BF16), bound_only=bound_only)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", p64.RESIZE, ids=[f"{c[1]}->{c[3]}".replace(" ", "") for c in p64.RESIZE])
def test_resize_generic(case, kind):
    B, dims, Cc, out, _why = case
    run_resize("resize", kind, B, dims, Cc, out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", p64.RESIZE_2X, ids=[f"{c[1]}->{c[2]}".replace(" ", "") for c in p64.RESIZE_2X])
def test_resize_exact_2x(case, kind):
    """C = 1, W % 4 == 0: upsample2x_fwd_kernel / upsample2x_bwd_kernel of elementwise.hip itself (ops.UpsampleLinear sends this shape to recon_loss.hip)"""
    B, dims, out, _why = case
    run_resize("resize2x", kind, B, dims, 1, out)


@pytest.mark.parametrize("kind", KINDS)
def test_resize_exact_2x_forward_past_the_grid_cap(kind):
    B, dims, out = p64.RESIZE_2X_BIG_FWD
    scale = 64.0 if kind == "structured" else 1.0
    src = scale * p64.operands(kind, 1, B, *dims, 1)
    sb, db = flat(src), Buf(1, B * out[0] * out[1] * out[2])
    got, = launch_twice("cvae_upsample_linear_fwd", (sb.ptr, db.ptr, B, *dims, *out, 1, L.F32), [db])
    check("resize2x_fwd", kind, dict(dst=got), *p64.resize_fwd(src, out))


@pytest.mark.parametrize("kind", KINDS)
def test_resize_exact_2x_backward_past_the_grid_cap(kind):
    B, dims, out = p64.RESIZE_2X_BIG_BWD
    scale = 64.0 if kind == "structured" else 1.0
    g = scale * p64.operands(kind, 2, B, *out, 1)
    gb, sb = flat(g), Buf(1, B * dims[0] * dims[1] * dims[2])
    got, = launch_twice("cvae_upsample_linear_bwd", (gb.ptr, sb.ptr, B, *dims, *out, 1, L.F32), [sb])
    check("resize2x_bwd", kind, dict(dsrc=got), *p64.resize_bwd(g, dims))


# ------------------------------------------------------------------------------------------------ k3 <-> k4
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Cout,Cin", p64.K34)
def test_k3_k4(Cout, Cin, kind):
    w3, g = p64.operands(kind, 1, Cout, Cin, 3, 3), p64.operands(kind, 2, Cin, Cout, 4, 4)
    wb, kb = flat(w3), Buf(1, Cin * Cout * 16)
    k4, = launch_twice("cvae_conv3_to_k4", (wb.ptr, kb.ptr, Cout, Cin), [kb])
    check("k3_k4", kind, dict(k4=k4), *p64.conv3_to_k4(w3))
    gb, db = flat(g), Buf(1, Cout * Cin * 9)
    dw3, = launch_twice("cvae_k4_to_conv3_grad", (gb.ptr, db.ptr, Cout, Cin), [db])
    check("k3_k4", kind, dict(dw3=dw3), *p64.k4_to_conv3_grad(g))
    # the adjoint identity <A W A^T, G> = <W, A^T G A> in float64 on the device outputs: each side carries its outputs' bounds
    lhs, rhs = (k4.double().reshape(-1) * g.double().reshape(-1)).sum(), (w3.double().reshape(-1) * dw3.double().reshape(-1)).sum()
    tol = (p64.conv3_to_k4(w3)[1]["k4"].reshape(-1) * g.double().reshape(-1).abs()).sum() + (p64.k4_to_conv3_grad(g)[1]["dw3"].reshape(-1) * w3.double().reshape(-1).abs()).sum()
    assert abs(float(lhs - rhs)) <= float(tol), (float(lhs), float(rhs), float(tol))


# ------------------------------------------------------------------------------------------------ BatchNorm2d
MOM, EPS = 0.1, 1e-5


@functools.lru_cache(maxsize=8)
def bn_case(kind, P, Cc, bf):
    c = p64.bn_case(kind, 1, P, Cc, bf)
    ref, _ = p64.bn2d_fwd(c["x"], c["gamma"], c["beta"], None, None, MOM, EPS, 1, p64.NONE)
    c["mean"], c["rstd"] = ref["mean"].to(F32), ref["rstd"].to(F32)            # what a forward leaves: the inputs of the eval forward and of the backward
    return c


def bn_ws(P, Cc):
    return Workspace(L.lib.cvae_bn2d_workspace_bytes(P, Cc) // 4)


def run_bn_fwd(kind, P, Cc, dt, act, training, running=True, rv_only_mean=False, ws_mode="full"):
    c = bn_case(kind, P, Cc, dt == BF16)
    xb, yb = flat(c["x"], dt), Buf(1, P * Cc, dt)
    gb, bb = flat(c["gamma"]), flat(c["beta"])
    ws = bn_ws(P, Cc)
    if training:
        mb, rb = Buf(1, Cc), Buf(1, Cc)
        rmb, rvb = (flat(c["rm"]), flat(c["rv"])) if running else (None, None)
        outs = [yb, mb, rb]
        wsp, wsb = ws.args(ws_mode)
        if ws_mode == "half":
            wsp, wsb = ws.args("full")[0], ws.floats * 2
    else:
        mb, rb, rmb, rvb, outs, (wsp, wsb) = flat(c["mean"]), flat(c["rstd"]), None, None, [yb], (None, 0)
    args = (xb.ptr, gb.ptr, bb.ptr, yb.ptr, mb.ptr, rb.ptr, p(rmb), p(rvb), P, Cc, MOM, EPS, training, act, DT[dt], wsp, wsb)
    runs = []
    for _ in range(2):                                           # launch_twice, with the running statistics re-filled too: they are updated in place
        for b, v in ((rmb, c["rm"]), (rvb, c["rv"])):
            if b is not None:
                b.view(b.buf).copy_(v.reshape(1, -1))
        for o in outs:
            o.reset()
        rc = L.lib.cvae_bn2d_fwd(*args, None)
        assert rc == 0, L.strerror(rc)
        torch.cuda.synchronize()
        runs.append([o.get() for o in outs] + ([rmb.get(), rvb.get()] if running and training else []))
        assert all(o.intact() for o in outs) and ws.intact() and (rmb is None or (rmb.intact() and rvb.intact()))
    for a, b in zip(*runs):
        assert bool(p64.same_bits(a, b).all()), "cvae_bn2d_fwd: two runs on the same inputs gave different bits"
    r = runs[0]
    got = dict(y=r[0])
    if training:
        got.update(mean=r[1], rstd=r[2])
        if running:
            got.update(running_mean=r[3], running_var=r[4])
    ref, err = p64.bn2d_fwd(c["x"], c["gamma"], c["beta"], c["rm"] if running else None, c["rv"] if running else None, MOM, EPS, training, act,
                            mean=None if training else c["mean"], rstd=None if training else c["rstd"], out_bf16=dt == BF16)
    check("bn2d_fwd_train" if training else "bn2d_fwd_eval", "random", got, ref, err)     # the statistics have no exact form: structured operands are held to the bound


def run_bn_bwd(kind, P, Cc, dt, act):
    c = bn_case(kind, P, Cc, dt == BF16)
    ya = p64.act_output("random", 5, P * Cc, act)
    y, = rounded(dt, c["x"] if ya is None else ya.reshape(P, Cc))
    xb, dyb, yb, gb, mb, rb = flat(c["x"], dt), flat(c["dy"], dt), flat(y, dt), flat(c["gamma"]), flat(c["mean"]), flat(c["rstd"])
    dxb, dgb, dbb = Buf(1, P * Cc, dt), Buf(1, Cc), Buf(1, Cc)
    ws = bn_ws(P, Cc)
    got = launch_twice("cvae_bn2d_bwd", (xb.ptr, dyb.ptr, yb.ptr, gb.ptr, mb.ptr, rb.ptr, dxb.ptr, dgb.ptr, dbb.ptr, P, Cc, act, DT[dt], *ws.args("full")), [dxb, dgb, dbb], ws)
    ref, err = p64.bn2d_bwd(c["x"], c["dy"], y, c["gamma"], c["mean"], c["rstd"], act, out_bf16=dt == BF16)
    check("bn2d_bwd", "random", dict(dx=got[0], dgamma=got[1], dbeta=got[2]), ref, err)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", p64.BN_C)
def test_bn2d(Cc, dt, kind):
    """training with and without the running-statistics pointers, eval mode, the backward: every activation code, at P = 2, 3, R - 1, 16 R + 1"""
    for P in p64.bn_P(Cc):
        for act in p64.ACTS:
            run_bn_fwd(kind, P, Cc, dt, act, 1, running=act != p64.LEAKY02)
            run_bn_fwd(kind, P, Cc, dt, act, 0)
            run_bn_bwd(kind, P, Cc, dt, act)


def test_bn2d_eval_structured_is_exact():
    """integer mean, gamma and beta, rstd a power of two: y = act((x - mean) rstd gamma + beta) is exact"""
    for Cc, P in ((8, 255), (40, 817), (264, 6)):
        x = p64.operands("structured", 1, P, Cc, lo=-8, hi=8)
        gamma, beta, mean = (p64.operands("structured", s, Cc, lo=-3, hi=3) for s in (2, 3, 4))
        rstd = 2.0 ** p64.operands("structured", 5, Cc, lo=-2, hi=2)
        for dt in DTYPES:
            for act in (p64.NONE, p64.RELU):
                xb, yb = flat(x, dt), Buf(1, P * Cc, dt)
                gb, bb, mb, rb = flat(gamma), flat(beta), flat(mean), flat(rstd)
                got, = launch_twice("cvae_bn2d_fwd", (xb.ptr, gb.ptr, bb.ptr, yb.ptr, mb.ptr, rb.ptr, None, None, P, Cc, MOM, EPS, 0, act, DT[dt], None, 0), [yb])
                assert mb.intact() and rb.intact() and torch.equal(mb.get(), mean.reshape(1, -1)) and torch.equal(rb.get(), rstd.reshape(1, -1))      # eval: inputs
                ref, err = p64.bn2d_fwd(x, gamma, beta, None, None, MOM, EPS, 0, act, mean=mean, rstd=rstd)
                check("bn2d_fwd_eval", "structured", dict(y=got), ref, err)


def test_bn2d_running_mean_alone():
    """the header lets either running statistic be NULL: running_var == NULL with running_mean given used to be written through"""
    P, Cc = 50, 40
    c = bn_case("random", P, Cc, False)
    xb, yb, gb, bb, mb, rb, rmb = flat(c["x"]), Buf(1, P * Cc), flat(c["gamma"]), flat(c["beta"]), Buf(1, Cc), Buf(1, Cc), flat(c["rm"])
    ws = bn_ws(P, Cc)
    rc = L.lib.cvae_bn2d_fwd(xb.ptr, gb.ptr, bb.ptr, yb.ptr, mb.ptr, rb.ptr, rmb.ptr, None, P, Cc, MOM, EPS, 1, 0, L.F32, *ws.args("full"), None)
    torch.cuda.synchronize()
    assert rc == 0 and rmb.intact() and ws.intact()
    ref, err = p64.bn2d_fwd(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], MOM, EPS, 1, 0)
    check("bn2d_fwd_train", "random", dict(y=yb.get(), running_mean=rmb.get()), ref, err)


def test_bn2d_over_the_scratch_row_cap():
    """C = 2048, P = 16385 in bf16: 1025 row blocks wanted, 1024 scratch rows (67 MB per tensor); forward in training mode and backward"""
    P, Cc = p64.BN_CAP
    assert p64.bn2d_blocks(P, Cc)[0] == 1024
    run_bn_fwd("random", P, Cc, BF16, p64.RELU, 1)
    run_bn_bwd("random", P, Cc, BF16, p64.RELU)


def test_bn2d_workspace():
    """one float short: CVAE_E_WORKSPACE with every buffer untouched; the forward is satisfied with half of cvae_bn2d_workspace_bytes, the backward is not"""
    P, Cc = 113, 264
    c = bn_case("random", P, Cc, False)
    ws = bn_ws(P, Cc)
    assert ws.floats == p64.bn2d_workspace_floats(P, Cc, True) == 2 * p64.bn2d_workspace_floats(P, Cc, False)
    xb, dyb, gb, bb = flat(c["x"]), flat(c["dy"]), flat(c["gamma"]), flat(c["beta"])
    outs = [Buf(1, P * Cc), Buf(1, Cc), Buf(1, Cc)]
    wsp = ws.args("full")[0]
    fwd = lambda nbytes: (xb.ptr, gb.ptr, bb.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, None, None, P, Cc, MOM, EPS, 1, 0, L.F32, wsp, nbytes)   # noqa: E731
    refused("cvae_bn2d_fwd", fwd(ws.floats * 2 - 4), outs, WORKSPACE)
    assert bool((ws.buf == CANARY).all())
    run_bn_fwd("random", P, Cc, F32, p64.NONE, 1, ws_mode="half")
    mb, rb = flat(c["mean"]), flat(c["rstd"])
    bwd = lambda nbytes: (xb.ptr, dyb.ptr, xb.ptr, gb.ptr, mb.ptr, rb.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, P, Cc, 0, L.F32, wsp, nbytes)   # noqa: E731
    for nbytes in (ws.floats * 4 - 4, ws.floats * 2):
        refused("cvae_bn2d_bwd", bwd(nbytes), outs, WORKSPACE)
    assert bool((ws.buf == CANARY).all())


def test_zz_worst_ratios():
    """the summary line per family of the module docstring (runs last in this file)"""
    for k in sorted(WORST):
        print(f"WORST {k} {WORST[k]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
