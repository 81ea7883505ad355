"""Float64 references of the dense layers (csrc/linear.hip: cvae_linear_fwd / _bwd_data / _bwd_weight; csrc/small_dense.hip: cvae_small_dense_fwd / _bwd_data /
_bwd_weight) with derived elementwise error bounds, in the style and with the constants of oracle/fused64.py (U = 2^-24, C = 4; `compare` and `max_ratio`
are the same functions).

  fwd(x, W, b, act)                               y  = act(x W^T + b)                                   x [M][K], W [N][K], b [N] or None
  bwd_data(dy, W, y_act, act, x_in, in_act)       dx = (g W) * in_act'(x_in),  g = dy * act'(y_act)      y_act [M][N] / x_in [M][K] or None
  bwd_weight(dy, x, y_act, act)                   dW = g^T x,  db = column sums of g

Every function returns (ref, err): dicts of float64 CPU tensors, err[k] an elementwise bound on how far an fp32 evaluation of the same sums may lie from ref[k].
The operands are exactly what the caller passes.  Activations are the CVAE_ACT_* codes of include/cvae_hip.h (0 none, 1 ReLU, 2 sigmoid, 3 LeakyReLU(0.2),
4 LeakyReLU(0.01)).  The rules:
  a product-sum          an element summed over T terms gets C sqrt(T) U (sum |a| |b| + |bias|), T that element's real term count: K for y, N for dx, M for dW
                         and db.  K-splits, slabs, n-chunks, k-chunks and per-workgroup partials reorder the same sum and do not change T.
  through an activation  ReLU and the LeakyReLUs are 1-Lipschitz (the slope product adds one rounding); sigmoid is 1/4-Lipschitz plus its own evaluation,
                         1.f / (1.f + __expf(-v)) in apply_act (common.h): ULP['__expf'] ulps of e = exp(-v) weighted by d sigmoid / d e = s (1 - s) / e, one
                         rounding of 1 + e and the (correctly rounded, loss64.ULP['div']) division.  __expf was measured over [-8, 8] only, so a sigmoid
                         pre-activation beyond SIG_RANGE = 8 is refused by the reference.
  g = dy * act'(y_act)   act' is read off the activation's OUTPUT (act_grad_from_out): the factors 0 / 1 are exact, 0.2f / 0.01f cost the product's one rounding,
                         y (1 - y) costs two roundings before the product (three in all).  The error of g enters the sums as a term error, as in loss64._sum.
                         The in_act epilogue multiplies the finished sum by the same kind of factor: its error times |sum|, plus one rounding.
  branches               y > 0 of the ReLU / LeakyReLU derivative is decided on an INPUT of the call (y_act, x_in), so it is exact for any input; the
                         generators nevertheless keep every such value at 0 or |v| >= 2^-6 and the reference asserts it (`BRANCH_MARGIN`), so that the same
                         inputs stay valid for a kernel that recomputes the activation.
  bf16-operand forms     (bf16_math) the caller passes operands already rounded to bf16 (`bf16`): x and W for the forward, dy and W for dx, dy and x for dW;
                         products of bf16 numbers are exact in fp32 and the accumulation is fp32, so the same bound applies (oracle/conv64.py records that
                         neither MFMA adds a term of its own).  db stays the fp32 column sum of the UNROUNDED dy (`dy_db`).  Both conversions in the kernels,
                         (bf16) x and pack2_bf16 (__builtin_convertvector to __bf16, common.h), are float -> __bf16 conversions of the language, which round
                         to nearest-even like torch's .bfloat16().
dtype = torch.float32 evaluates the same formulas in fp32 on the CPU (the stand-in for a correct kernel of tests/test_dense_reference_cpu.py; the bounds
returned with it are meaningless).  drop= (self-tests only) evaluates a deliberately wrong variant, see _MUTATIONS.

The second half of the file replays the launch dispatch of csrc/linear.hip in Python (gemm_splits, gemm_t128_splits, skinny_fwd_chunks, skinny_bwd_chunks,
workspace_floats) and holds the shape tables both test files walk: the smallest shapes that cross each seam of the dispatch.
"""
import math

import torch

from .conv64 import max_ratio  # noqa: F401  (re-exported: the tests take it from here)
from .fused64 import C, U, _ps, compare  # noqa: F401
from .loss64 import ULP as _LOSS_ULP
from .loss64 import f32, gen  # noqa: F401

F64, F32 = torch.float64, torch.float32
NONE, RELU, SIGMOID, LEAKY02, LEAKY001 = 0, 1, 2, 3, 4
ACTS = (NONE, RELU, SIGMOID, LEAKY02, LEAKY001)
SLOPE = {LEAKY02: f32(0.2), LEAKY001: f32(0.01)}           # the fp32 values of the kernel's 0.2f / 0.01f
SIG_RANGE = 8.0                                             # |pre-activation| of a sigmoid case: the range __expf was measured over
BRANCH_MARGIN = 2.0 ** -6

# Maximum error of the device functions apply_act calls, in ulps of the result, MEASURED as loss64.ULP was (tools/probes/math_ulp_probe.hip on the MI355X, 2^26
# arguments per range; the entry is the next integer at or above twice the largest error seen).
ULP = {
    "__expf": 16,    # measured 7.746 ulp over [-8, 8] (7.746 in [7, 8], 7.627 in [-8, -7], 1.465 in [-1, 1]): it grows with |x|, the rounding of x log2(e)
    "div": _LOSS_ULP["div"],
}

_MUTATIONS = {
    "last_k": "('last_k',): the last term of every sum missing (the last k of y, the last n of dx, the last m of dW and db)",
    "kstep": "('kstep', k0): the 16 terms k0 .. k0 + 15 of every sum missing (one k-step of the fp32 MFMA tile)",
    "slab": "('slab', (s, per)): the terms s per .. (s + 1) per - 1 missing: one split's slab, one chunk, one workgroup's partial",
    "bias_per_split": "('bias_per_split', n): the bias added once per split, n times in all  [fwd]",
    "last_row": "('last_row',): the last batch row (the only row of the last 16-row block at M = 16 j + 1) missing from dW and db  [bwd_weight]",
    "edge_col": "('edge_col', c): output column c (the first of a 64- or 128-wide tile) taken from column c - 1",
    "yact_rowlen": "('yact_rowlen', buf): y_act read as buf.reshape(-1)[m N + n] from its padded buffer buf [M][stride], i.e. with the row length where "
                   "its stride belongs  [bwd_data, bwd_weight]",
}


def _t(v, dtype):
    return None if v is None else v.detach().to("cpu", dtype)


def _out(ref, err):
    return {k: v.detach().to(F64) for k, v in ref.items()}, {k: v.detach().to(F64) for k, v in err.items()}


def bf16(v):
    """v rounded to bf16 (nearest-even), as fp32: what a bf16_math kernel multiplies"""
    return None if v is None else v.detach().to(F32).to(torch.bfloat16).to(F32)


def _keep(T, drop, dtype):
    """0 / 1 over the T terms of a sum: the terms a mutation leaves out"""
    keep = torch.ones(T, dtype=dtype)
    if not drop:
        return keep
    if drop[0] not in _MUTATIONS:
        raise ValueError(drop[0])
    if drop[0] in ("last_k", "last_row"):
        keep[-1] = 0.0
    elif drop[0] == "kstep":
        keep[drop[1]:drop[1] + 16] = 0.0
    elif drop[0] == "slab":
        s, per = drop[1]
        keep[s * per:(s + 1) * per] = 0.0
    return keep


def _edge(v, drop):
    if drop and drop[0] == "edge_col":
        v = v.clone()
        v[..., drop[1]] = v[..., drop[1] - 1]
    return v


def _act(pre, e_pre, act):
    """act(pre) and its bound"""
    if act == NONE:
        return pre, e_pre
    if act == RELU:
        return pre.clamp_min(0.0), e_pre
    if act in SLOPE:
        r = torch.where(pre > 0, pre, SLOPE[act] * pre)
        return r, e_pre + U * r.abs()
    if act == SIGMOID:
        assert float(pre.abs().max()) <= SIG_RANGE, f"a sigmoid pre-activation lies beyond {SIG_RANGE}: __expf was not measured there"
        e = torch.exp(-pre)
        s = 1.0 / (1.0 + e)
        return s, 0.25 * e_pre + s * ((1.0 - s) * ULP["__expf"] * 2.0 * U + U + ULP["div"] * 2.0 * U)
    raise ValueError(act)


def _act_grad(y, act):
    """act'(y) from the activation's output y, and the roundings its product with a gradient costs (relative, in units of U)"""
    if act == NONE or y is None:
        return None, 0.0
    if act == SIGMOID:
        return y * (1.0 - y), 3.0
    if act == RELU or act in SLOPE:
        ok = (y == 0) | (y.abs() >= BRANCH_MARGIN)
        assert bool(ok.all()), "an activation output lies within 2^-6 of zero without being zero: the branch y > 0 is not decided clear of rounding"
        one = torch.ones_like(y)
        return torch.where(y > 0, one, (0.0 if act == RELU else SLOPE[act]) * one), (0.0 if act == RELU else 1.0)
    raise ValueError(act)


def _g(dy, y_act, act, drop):
    """g = dy * act'(y_act) and its own error"""
    if drop and drop[0] == "yact_rowlen" and y_act is not None:
        M, N = dy.shape
        y_act = drop[1].detach().to("cpu", dy.dtype).reshape(-1)[:M * N].reshape(M, N)
    f, r = _act_grad(y_act, act)
    if f is None:
        return dy, torch.zeros_like(dy)
    g = dy * f
    return g, r * U * g.abs()


def fwd(x, W, b, act, dtype=F64, drop=None):
    x, W, b = (_t(v, dtype) for v in (x, W, b))
    K = x.shape[1]
    keep = _keep(K, drop, dtype)
    pre = (x * keep) @ W.t()
    mag = x.abs() @ W.abs().t()
    if b is not None:
        pre = pre + b * (drop[1] if drop and drop[0] == "bias_per_split" else 1.0)
        mag = mag + b.abs()
    y, e_y = _act(pre, _ps(K) * mag, act)
    return _out(dict(y=_edge(y, drop)), dict(y=e_y))


def bwd_data(dy, W, y_act, act, x_in, in_act, dtype=F64, drop=None):
    dy, W, y_act, x_in = (_t(v, dtype) for v in (dy, W, y_act, x_in))
    N = dy.shape[1]
    g, e_g = _g(dy, y_act, act, drop)
    keep = _keep(N, drop, dtype)
    s = (g * keep) @ W
    e_s = _ps(N) * (g.abs() @ W.abs()) + e_g @ W.abs()
    f, r = _act_grad(x_in, in_act)
    if f is not None:
        e_s = f.abs() * e_s + (r + 1.0) * U * (s * f).abs()
        s = s * f
    return _out(dict(dx=_edge(s, drop)), dict(dx=e_s))


def bwd_weight(dy, x, y_act, act, dy_db=None, dtype=F64, drop=None):
    """dy_db: the dy whose column sums are db, where it differs from the dy of the product (bf16_math: the unrounded one)"""
    dy, x, y_act, dy_db = (_t(v, dtype) for v in (dy, x, y_act, dy_db))
    M = dy.shape[0]
    g, e_g = _g(dy, y_act, act, drop)
    gb, e_gb = (g, e_g) if dy_db is None else _g(dy_db, y_act, act, drop)
    keep = _keep(M, drop, dtype)[:, None]
    dW = (g * keep).t() @ x
    e_dW = _ps(M) * (g.abs().t() @ x.abs()) + e_g.t() @ x.abs()
    db = (gb * keep).sum(0)
    e_db = _ps(M) * gb.abs().sum(0) + e_gb.sum(0)
    return _out(dict(dW=_edge(dW, drop), db=db), dict(dW=e_dW, db=e_db))


# ------------------------------------------------------------------------------------------------ operands
def _ints(seed, R, Cc, lo=-2, hi=2):
    """small integers f(seed, row, column) in [lo, hi], distinct enough along both axes that a swapped or repeated index shows"""
    i, j = torch.arange(R, dtype=torch.int64)[:, None], torch.arange(Cc, dtype=torch.int64)[None, :]
    v = (i * (7 + 2 * seed) + j * 13 + (i * j) % 11 + (i // 16) * 3 + (j // 16) * 5 + seed) % (hi - lo + 1) + lo
    return v.to(F32)


def operands(kind, seed, M, K, N):
    """x [M][K], W [N][K], b [N], dy [M][N].  'random': Gaussian, W scaled by 1 / sqrt(K).  'structured': integers in [-2, 2], so that every sum is an
    integer below 2^24, exact in fp32 and in bf16 whatever the order."""
    if kind == "structured":
        return dict(x=_ints(seed, M, K), W=_ints(seed + 1, N, K), b=_ints(seed + 2, 1, N)[0], dy=_ints(seed + 3, M, N))
    g = gen(seed * 7919 + M * 31 + K * 17 + N)
    return dict(x=torch.randn(M, K, generator=g), W=torch.randn(N, K, generator=g) / math.sqrt(K), b=0.5 * torch.randn(N, generator=g),
                dy=torch.randn(M, N, generator=g))


def act_output(kind, seed, R, Cc, act):
    """a tensor that could be the saved OUTPUT of `act`, every ReLU / LeakyReLU branch decided by BRANCH_MARGIN.  'structured': integers whose derivative
    factor is exactly 0 or 1 (ReLU: 0, 1, 2; LeakyReLU: 1 .. 3, the branch '1' only: the slopes 0.2 / 0.01 would break exactness)."""
    if act == NONE:
        return None
    if kind == "structured":
        assert act != SIGMOID
        return _ints(seed, R, Cc, -2, 2).clamp_min(0.0) if act == RELU else _ints(seed, R, Cc, 1, 3)
    v = torch.randn(R, Cc, generator=gen(seed * 104729 + R * 13 + Cc))
    if act == SIGMOID:
        return torch.sigmoid(2.0 * v)
    v = torch.where(v.abs() < BRANCH_MARGIN, torch.full_like(v, BRANCH_MARGIN), v)
    return v.clamp_min(0.0) if act == RELU else torch.where(v > 0, v, SLOPE[act] * v - BRANCH_MARGIN).to(F32)


# ------------------------------------------------------------------------------------------------ the launch dispatch of csrc/linear.hip, replayed
SK_M = 16


def _cdiv(a, b):
    return (a + b - 1) // b


def gemm_splits(M, N, K):
    """(splits, k_per_split) of gemm_f32's 64-tile kernels for an [M][N] result over K"""
    tiles, ksteps, splits = _cdiv(M, 64) * _cdiv(N, 64), _cdiv(K, 16), 1
    if tiles < 512 and ksteps >= 8:
        splits = max(1, min(512 // tiles, ksteps // 4, 1024))
    kps = _cdiv(ksteps, splits) * 16
    return _cdiv(K, kps), kps


def gemm_t128_splits(M, N, K):
    tiles, stages = _cdiv(M, 128) * _cdiv(N, 128), _cdiv(K, 32)
    splits = max(1, min(256 // tiles, stages // 4))
    kps = _cdiv(stages, splits) * 32
    return _cdiv(K, kps), kps


def is_t128(M, N, K):
    return M >= 128 and N >= 128 and K >= 128


def skinny_fwd_chunks(K, N):
    chunks = max(1, min(_cdiv(4096, N), K // 512))
    kchunk = _cdiv(_cdiv(K, chunks), 64) * 64
    return _cdiv(K, kchunk), kchunk


def skinny_bwd_chunks(K, N, wide):
    kb = _cdiv(K, 256)
    chunks = max(1, min(_cdiv(2048, kb), N // 16) if wide else min(N // 8, 256))
    nchunk = _cdiv(N, chunks)
    return _cdiv(N, nchunk), nchunk


def _gemm_floats(m, n, k, bf16_math):
    s = gemm_t128_splits(m, n, k)[0] if bf16_math and is_t128(m, n, k) else gemm_splits(m, n, k)[0]
    return s * m * n if s > 1 else 0


def path(op, M, K, N, bf16_math=False, y_act=False, in_act=False):
    """the kernel family a call takes: 'skinny', 'gemm64', 'gemm128' (op 0 fwd, 1 bwd_data, 2 bwd_weight)"""
    if op == 0 and not bf16_math and M <= SK_M and K >= 64:
        return "skinny"
    if op == 1 and not bf16_math and not in_act and M <= SK_M and (K >= 1024 or y_act):
        return "skinny"
    if op == 2 and M <= SK_M:
        return "skinny"
    m, n, k = {0: (M, N, K), 1: (M, K, N), 2: (N, K, M)}[op]
    return "gemm128" if bf16_math and is_t128(m, n, k) else "gemm64"


def workspace_floats(op, M, K, N, bf16_math=False, y_act=False, in_act=False):
    """the floats of workspace the path of this call asks for, to run split (0: it never splits)"""
    if path(op, M, K, N, bf16_math, y_act, in_act) == "skinny":
        if op == 0:
            c = skinny_fwd_chunks(K, N)[0]
            return c * M * N if c > 1 else 0
        if op == 1:
            c = skinny_bwd_chunks(K, N, K >= 1024)[0]
            return c * M * K if c > 1 else 0
        return 0
    m, n, k = {0: (M, N, K), 1: (M, K, N), 2: (N, K, M)}[op]
    return _gemm_floats(m, n, k, bf16_math)


# ------------------------------------------------------------------------------------------------ the shapes (M, K, N) both test files walk
FWD_SKINNY = [(1, 64, 1), (16, 67, 5), (3, 449, 6), (4, 1023, 7), (3, 1100, 7), (5, 2100, 3)]
FWD_GEMM = [(7, 10, 64), (17, 20, 5), (65, 112, 67), (65, 113, 67), (65, 130, 67), (17, 5000, 3)]
FWD_BF16_64 = [(17, 33, 5), (100, 200, 130)]
FWD_BF16_128 = [(128, 128, 128), (129, 131, 133), (129, 400, 133), (133, 400, 129)]
BWD_DATA_WIDE = [(4, 1024, 5), (4, 1030, 40), (16, 1500, 200)]
BWD_DATA_NARROW = [(3, 7, 3), (16, 70, 23), (2, 300, 3000)]
BWD_DATA_GEMM = [(M, N, K) for M, K, N in FWD_GEMM]           # the forward's products with the roles of K and N exchanged
BWD_DATA_BF16 = [(M, N, K) for M, K, N in FWD_BF16_64 + FWD_BF16_128]
BWD_WEIGHT_ROWS = [(1, 256, 1), (16, 1030, 5)]
BWD_WEIGHT_FLAT = [(4, 10, 64), (16, 255, 300), (2, 255, 16449)]
BWD_WEIGHT_GEMM = [(17, 5, 3), (130, 67, 65), (1031, 20, 10)]
BWD_WEIGHT_BF16_64 = [(100, 130, 200)]
BWD_WEIGHT_BF16_128 = [(128, 128, 128), (400, 133, 129), (400, 131, 257)]
SD_M = [17, 32, 145, 1000]
SD_KN = [(1, 1), (3, 5), (10, 64), (64, 10), (128, 96), (96, 128), (127, 96), (128, 12)]
SD_MAX_DIM, SD_MAX_NK = 128, 12288
