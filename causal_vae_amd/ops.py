"""torch.autograd.Function wrappers over the C ABI (include/cvae_hip.h).

The reference reaches its arithmetic through autograd (`loss.backward()`, causal_cascade/train.py:33), so the kernels hook
in here: every Function.forward / backward enqueues HIP kernels on torch's current stream and nothing else.  Conv
activations are channels-last [B, D, H, W, C] (D = 1 for 2D) in the compute dtype (float32 or bfloat16); linear layers,
losses, BN and sampling are fp32.
"""
import ctypes as C_
import functools
import math

import torch

from . import _lib as L
from ._lib import lib, check, ptr, stream


_SIDE = {}
FORK_BACKWARD = False      # True: weight-gradient kernels run on a side stream next to the data-gradient kernels
FORK_MAX_POSITIONS = 0     # > 0: only layers with at most this many S positions per batch fork (the small, latency-bound layers)
DEFER_JOIN = False         # True: the side stream is not joined after each layer but once, by join_side_streams(), before the gradients are
                           # consumed (exchange / optimizer): the weight gradients then trail the data-gradient chain instead of gating it
_PENDING = {}              # device key -> tensors produced on the side stream since the last join (kept alive until then)


class _Fork:
    """`with _Fork() as f:` runs its body on a side HIP stream that first waits for the current stream; f.join() makes
    the current stream wait for the side work.  The weight gradient of a layer and the data gradient of the same layer
    only share inputs, so the two kernels (often too small to fill 256 CUs each) overlap.  Captured graphs record the
    fork/join as dependencies."""

    def __init__(self, device, positions=None):
        self.main = torch.cuda.current_stream(device)
        key = (device.index if device.index is not None else torch.cuda.current_device())
        self.key = key
        if key not in _SIDE:
            _SIDE[key] = torch.cuda.Stream(device=device)
        on = FORK_BACKWARD and (FORK_MAX_POSITIONS <= 0 or positions is None or positions <= FORK_MAX_POSITIONS)
        self.side = _SIDE[key] if on else None
        self.ctx = None

    def __enter__(self):
        if self.side is not None:
            self.side.wait_stream(self.main)
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False

    def join(self, *tensors):
        if self.side is None:
            return
        if DEFER_JOIN:
            _PENDING.setdefault(self.key, []).extend(t for t in tensors if t is not None)
            return
        self.main.wait_stream(self.side)
        for t in tensors:
            if t is not None:
                t.record_stream(self.main)


def join_side_streams():
    """Make the current stream wait for every weight gradient still running on a side stream (DEFER_JOIN).  Called before anything reads
    `.grad`: the gradient exchange, clip_grad_norm_, optimizer.step()."""
    for key, tensors in list(_PENDING.items()):
        if not tensors:
            continue
        main = torch.cuda.current_stream(tensors[0].device)
        main.wait_stream(_SIDE[key])
        for t in tensors:
            t.record_stream(main)
        tensors.clear()


def _cl_dims(t):
    assert t.dim() == 5 and t.is_contiguous(), "channels-last [B, D, H, W, C] contiguous tensor expected"
    return t.shape


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


_ZERO_POOL = [None, 0]


class zero_pool:
    """`with ops.zero_pool(n):` — the accumulating scalar reductions inside the block (loss sums: `*out += ...` kernels) take their zeroed 0-dim outputs
    from ONE torch.zeros(n) made on entry instead of one fill launch each.  The fill belongs to the step that uses it, so a captured step stays
    replayable; more than n requests fall back to their own zeros."""

    def __init__(self, n, like):
        self.n, self.like = int(n), like

    def __enter__(self):
        self.prev = list(_ZERO_POOL)
        _ZERO_POOL[0], _ZERO_POOL[1] = torch.zeros(self.n, dtype=torch.float32, device=self.like.device), 0
        return self

    def __exit__(self, *exc):
        _ZERO_POOL[0], _ZERO_POOL[1] = self.prev
        return False


def _scalar(like):
    pool, used = _ZERO_POOL
    if pool is not None and used < pool.numel() and pool.device == like.device:
        _ZERO_POOL[1] = used + 1
        return pool[used]
    return torch.zeros((), dtype=torch.float32, device=like.device)


def _scratch(nbytes, like):
    """(pointer, bytes) of `nbytes` of device scratch for one call (None, 0 when nbytes == 0).  Reductions leave their per-workgroup partial
    sums here and add them in a fixed order (no float atomics).  A fresh block per call: safe on any stream, and inside a capture it
    comes from the graph's pool."""
    if not nbytes:
        return None, None, 0
    t = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=like.device)
    return t, t.data_ptr(), nbytes


_RED_WS = None


def _red_ws(like):
    """Scratch of cvae_reduce_workspace_bytes() for the scalar loss reductions."""
    global _RED_WS
    if _RED_WS is None:
        _RED_WS = int(lib.cvae_reduce_workspace_bytes())
    return _scratch(_RED_WS, like)


_ONES = {}


def cached_one(loss):
    """A ones scalar like `loss`, kept per (device, dtype): seeds a backward without the fill kernel autograd launches for the implicit 1."""
    key = (loss.device, loss.dtype)
    one = _ONES.get(key)
    if one is None:
        one = torch.ones((), dtype=loss.dtype, device=loss.device)
        if not (loss.is_cuda and torch.cuda.is_current_stream_capturing()):      # a tensor born inside a capture lives in that graph's pool
            _ONES[key] = one
    return one


def backward_from(loss):
    """loss.backward() seeded with cached_one(loss)."""
    loss.backward(cached_one(loss))


# ------------------------------------------------------------------------------------------------ layout plumbing
class ToChannelsLast(torch.autograd.Function):
    """NC(D)HW fp32 -> channels-last [B, D, H, W, C] in `dtype` (cvae_ncs_to_nsc)."""

    @staticmethod
    def forward(ctx, x, dtype):
        L.require_gpu(x)
        x = x.contiguous()
        B, C = x.shape[0], x.shape[1]
        sp = tuple(x.shape[2:])
        S = 1
        for s in sp:
            S *= s
        d5 = (1,) + sp if len(sp) == 2 else sp
        out = _empty((B,) + d5 + (C,), dtype, x)
        check(lib.cvae_ncs_to_nsc(ptr(x), ptr(out), B, C, S, L.dtype_code(x.dtype), L.dtype_code(dtype), stream()), "ncs_to_nsc")
        ctx.meta = (x.shape, x.dtype, S)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, dt, S = ctx.meta
        g = g.contiguous()
        out = _empty(shape, dt, g)
        check(lib.cvae_nsc_to_ncs(ptr(g), ptr(out), shape[0], shape[1], S, L.dtype_code(g.dtype), L.dtype_code(dt), stream()), "nsc_to_ncs")
        return out, None


class FromChannelsLast(torch.autograd.Function):
    """channels-last [B, D, H, W, C] -> NC(D)HW fp32; nd selects whether D is dropped."""

    @staticmethod
    def forward(ctx, x, nd):
        L.require_gpu(x)
        B, D, H, W, Cc = _cl_dims(x)
        sp = (H, W) if nd == 2 else (D, H, W)
        out = _empty((B, Cc) + sp, torch.float32, x)
        check(lib.cvae_nsc_to_ncs(ptr(x), ptr(out), B, Cc, D * H * W, L.dtype_code(x.dtype), L.F32, stream()), "nsc_to_ncs")
        ctx.meta = (x.shape, x.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, dt = ctx.meta
        g = g.contiguous()
        out = _empty(shape, dt, g)
        B, D, H, W, Cc = shape
        check(lib.cvae_ncs_to_nsc(ptr(g), ptr(out), B, Cc, D * H * W, L.dtype_code(g.dtype), L.dtype_code(dt), stream()), "ncs_to_nsc")
        return out, None


def _copy_panels(panels, wide, col0, gather):
    """cvae_copy_panels on fp32 [B, w_i] matrices (row strides taken from the tensors) and the wide matrix they sit side by side in."""
    import ctypes as C
    k = len(panels)
    check(lib.cvae_copy_panels((C.c_void_p * k)(*[t.data_ptr() for t in panels]), (C.c_int64 * k)(*[t.shape[1] for t in panels]), (C.c_int64 * k)(*[t.stride(0) for t in panels]),
                               k, ptr(wide), wide.shape[0], wide.stride(0), col0, int(gather), stream()), "copy_panels")


def _as_panel(t):
    """A [B, w] fp32 matrix whose rows are contiguous (a column slice of a wider matrix qualifies: its row stride travels with it)."""
    if t.dtype != torch.float32 or t.dim() != 2:
        raise L.CvaeError("cat: fp32 [B, n] matrices expected")
    return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) or t.shape[1] == 0 else t.contiguous()


class Cat(torch.autograd.Function):
    """torch.cat(tensors, dim=1) for fp32 [B, n_i] matrices: one launch (cvae_copy_panels), one more for all the gradients."""

    @staticmethod
    def forward(ctx, *ts):
        L.require_gpu(*ts)
        if len(ts) > 8:
            raise L.CvaeError("cat: at most 8 tensors")
        ts = [_as_panel(t) for t in ts]
        B = ts[0].shape[0]
        widths = [t.shape[1] for t in ts]
        out = _empty((B, sum(widths)), torch.float32, ts[0])
        _copy_panels(ts, out, 0, False)
        ctx.widths = widths
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        B = g.shape[0]
        need = [i for i in range(len(ctx.widths)) if ctx.needs_input_grad[i]]
        outs = [None] * len(ctx.widths)
        if need:
            # the needed pieces are gathered in one launch: consecutive runs of needed columns would be simplest, but any subset works by
            # giving the skipped pieces a width-0 panel... they still shift the offsets, so gather run by run
            col, runs, cur = 0, [], None
            for i, w in enumerate(ctx.widths):
                if ctx.needs_input_grad[i]:
                    outs[i] = _empty((B, w), torch.float32, g)
                    if cur is None:
                        cur = (col, [])
                        runs.append(cur)
                    cur[1].append(outs[i])
                else:
                    cur = None
                col += w
            for col0, panels in runs:
                _copy_panels(panels, g, col0, True)
        return tuple(outs)


def cat(tensors):
    return Cat.apply(*tensors)


def one_hot(t, n_classes):
    """F.one_hot(t, n).float() (causal_cascade/models.py:71)."""
    L.require_gpu(t)
    t = t.contiguous()
    if t.dtype != torch.int64:
        raise L.CvaeError("class index tensor must be int64")
    out = _empty((t.shape[0], n_classes), torch.float32, t)
    check(lib.cvae_onehot_panel(ptr(t), ptr(out), t.shape[0], n_classes, n_classes, 0, stream()), "onehot_panel")
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    out = torch.empty_like(x, dtype=dtype)
    check(lib.cvae_cast(ptr(x), ptr(out), x.numel(), L.dtype_code(x.dtype), L.dtype_code(dtype), stream()), "cast")
    return out


class Cast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return cast(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return cast(g.contiguous(), ctx.src), None


# ------------------------------------------------------------------------------------------------ conv family
def _taps(nd):
    return 64 if nd == 3 else 16


def pack_weight(w, nd, for_up, dtype):
    """fp32 [Cs][Cl][k..] -> MFMA operand panels (cvae_conv_pack_weight); the fp32 weight itself when Cl == 1."""
    Cs, Cl = w.shape[0], w.shape[1]
    w = w.contiguous()
    if Cl == 1:
        return w
    out = torch.empty(Cs * Cl * _taps(nd), dtype=dtype, device=w.device)
    check(lib.cvae_conv_pack_weight(ptr(w), ptr(out), Cs, Cl, nd, int(for_up), L.dtype_code(dtype), stream()), "conv_pack_weight")
    return out


def pack_weights(weights, nd, dtype, f8spec=None):
    """Pack the weights of several conv layers for BOTH directions in one launch (cvae_conv_pack_weight_pairs).
    Returns [(packed_down, packed_up)] per weight; a Cl == 1 layer gets its fp32 weight back for both (not packed).
    f8spec (fp8 training forward, causal_vae_amd.fp8): {id(weight): (f8dir, f8out, inv_scale_dev, amax)} — that weight's forward-direction panel
    (f8dir 1 = down, 2 = up) is written as fp8 codes into f8out instead of bf16 (its entry in the returned pair is None), max |w| recorded."""
    import ctypes as C
    outs, ws, pd, pu, cs, cl, fd, fo, fi, fa = [], [], [], [], [], [], [], [], [], []
    for w0 in weights:
        w = w0.contiguous()
        Cs, Cl = w.shape[0], w.shape[1]
        if Cl == 1:
            outs.append((w, w))
            continue
        n = Cs * Cl * _taps(nd)
        spec = f8spec.get(id(w0)) if f8spec else None
        if spec is not None:
            one = torch.empty(n, dtype=dtype, device=w.device)
            d, u = (None, one) if spec[0] == 1 else (one, None)
        else:
            both = torch.empty(2 * n, dtype=dtype, device=w.device)
            d, u = both[:n], both[n:]
        outs.append((d, u))
        ws.append(w.data_ptr()); pd.append(d.data_ptr() if d is not None else None); pu.append(u.data_ptr() if u is not None else None); cs.append(Cs); cl.append(Cl)
        fd.append(spec[0] if spec else 0); fo.append(spec[1].data_ptr() if spec else None); fi.append(spec[2].data_ptr() if spec else None)
        fa.append(spec[3].data_ptr() if (spec and spec[3] is not None) else None)
    k = len(ws)
    if k:
        vp = lambda v: (C.c_void_p * k)(*v)
        check(lib.cvae_conv_pack_weight_pairs(vp(ws), vp(pd), vp(pu), (C.c_int64 * k)(*cs), (C.c_int64 * k)(*cl), (C.c_int * k)(*fd), vp(fo), vp(fi), vp(fa),
                                              k, nd, L.dtype_code(dtype), stream()), "conv_pack_weight_pairs")
    return outs


SPLIT_K = True      # hand the conv data kernels their split-K scratch (tests switch it off to cover the unsplit path)


def _can_defer(weight, bias):
    """A weight gradient may be computed at the END of the backward pass only if nothing looks at it earlier: no accumulation onto an
    existing .grad (AccumulateGrad would add the still-empty tensor), no tensor hooks (pre- or post-accumulate), no double backward, and
    no second use of the same weight in this pass (the engine would add two still-empty tensors before the flush)."""
    if torch.is_grad_enabled():
        return False
    for p in (weight, bias):
        if p is None:
            continue
        if not p.is_leaf or p.grad is not None or p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None):
            return False                                     # a derived weight (ops.Conv3ToK4) hands its gradient on at once
    if _wg_task_is_current():
        if id(weight) in _WG_SHARED:
            return False
        if any(e["wid"] == id(weight) for e in _WG_PENDING):
            _wgrad_flush()                                   # the first use's gradient must exist before the engine sums the two
            _WG_SHARED.add(id(weight))
            return False
    return True


def _conv_data_workspace(device, B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, for_up):
    """Split-K scratch for the small-grid layers (cvae_conv_data_workspace_bytes; 0 bytes for the large ones)."""
    nbytes = lib.cvae_conv_data_workspace_bytes(B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, for_up) if SPLIT_K else 0
    if not nbytes:
        return None, 0
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


def image_direct_ok(x, dtype):
    """True when the first conv can read the 1-channel image `x` in ITS dtype while computing in `dtype` (cvae_conv_down_image)."""
    return x.dtype != dtype and x.is_contiguous() and bool(lib.cvae_conv_image_supported(ptr(x), x.shape[-2] if x.dim() == 5 and x.shape[-1] == 1 else x.shape[-1],
                                                                                        L.dtype_code(x.dtype), L.dtype_code(dtype)))


MASK_BITS = __import__("os").environ.get("CVAE_MASK_BITS", "1") != "0"     # (env switch: A/B runs) ReLU masks travel as bits (1/16 of the saved activation's bytes) wherever producer and consumer are this library's conv launches
BITS_STATS = {"produced": 0, "consumed": 0}      # launches that left / read a mask in bit form (tests check that the model really takes the path)


def _bits_for(t):
    """int32 tensor for the ReLU mask bits of channels-last tensor `t` (one dword per 32 consecutive elements), or None when the channel count does not allow it."""
    return torch.empty(t.numel() // 32, dtype=torch.int32, device=t.device) if (t.shape[-1] % 32 == 0 and t.numel() % 32 == 0) else None


def _conv_down(Lt, wp, bias, mask, Cs, nd, act, out_dtype=None, mask_bits=None, want_bits=None):
    """mask_bits: the ReLU mask as bits (replaces `mask`).  want_bits (True / False; None = plain return): return (S, bits) — the ReLU mask bits of the result
    when asked for and supported, else None."""
    B, ld, lh, lw, Cl = _cl_dims(Lt)
    sd, sh, sw = (ld // 2 if nd == 3 else 1), lh // 2, lw // 2
    if out_dtype is not None and out_dtype != Lt.dtype:      # single-channel image read in its own dtype, S in the compute dtype
        if Cl != 1:
            raise L.CvaeError("a mixed-dtype conv is available for the single-channel image layer only")
        S = _empty((B, sd, sh, sw, Cs), out_dtype, Lt)
        bits = _bits_for(S) if (want_bits and out_dtype == torch.bfloat16 and mask is None) else None
        if bits is not None:
            check(L.timed(f"conv_down nd{nd} B{B} L{ld}x{lh}x{lw}x{Cl} -> S{Cs}", lib.cvae_conv_down_image_f8, ptr(Lt), L.dtype_code(Lt.dtype), ptr(wp), ptr(bias), ptr(S), None, None,
                          None, ptr(bits), B, sd, sh, sw, Cs, ld, lh, lw, nd, L.act_code(act), stream()), "conv_down_image_f8")
        else:
            check(L.timed(f"conv_down nd{nd} B{B} L{ld}x{lh}x{lw}x{Cl} -> S{Cs}", lib.cvae_conv_down_image, ptr(Lt), L.dtype_code(Lt.dtype), ptr(wp), ptr(bias), ptr(mask), ptr(S),
                          B, sd, sh, sw, Cs, ld, lh, lw, nd, L.dtype_code(out_dtype), L.act_code(act), stream()), "conv_down_image")
        return (S, bits) if want_bits is not None else S
    S = _empty((B, sd, sh, sw, Cs), Lt.dtype, Lt)
    ws, nbytes = _conv_data_workspace(Lt.device, B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, 0)
    label = f"conv_down nd{nd} B{B} L{ld}x{lh}x{lw}x{Cl} -> S{Cs}"
    # the bit forms: MFMA layers in any dtype; the single-channel end (dec4's data gradient applies d3's mask) in its bf16 16-byte-row form only
    c1_ok = Cl != 1 or (Lt.dtype == torch.bfloat16 and lw % 8 == 0)
    bits = _bits_for(S) if (want_bits and Cl != 1 and Cs % 64 == 0 and Cl % 16 == 0) else None
    use_mb = mask_bits if (mask_bits is not None and c1_ok) else None      # the bit form of the mask wins over the tensor form when the launch can read it
    if use_mb is not None:
        mask = None
    elif mask is not None:
        bits = None                                          # a tensor mask: no bits (backward launches want no bits of their own anyway)
    variant = DOWN_VARIANT is not None and Cl != 1 and use_mb is None
    if variant:
        bits = None                                          # the test hook forces a kernel form: the tensor form of the mask, no bits
    check(L.timed(label, lib.cvae_conv_down, ptr(Lt), ptr(wp), ptr(bias), ptr(mask), ptr(use_mb), ptr(S), ptr(bits), B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd,
                  L.dtype_code(Lt.dtype), L.act_code(act), ptr(ws), nbytes, int(DOWN_VARIANT) if variant else -1, stream()), "conv_down")
    BITS_STATS["produced"] += bits is not None
    BITS_STATS["consumed"] += use_mb is not None
    return (S, bits) if want_bits is not None else S


_GRAD_AT_APPLY = [True]


def _backward_may_follow(ctx):
    """Inside Function.forward: was autograd recording when apply() was called, and does any input ask for a gradient?  (ctx.needs_input_grad alone ignores
    torch.no_grad(), and grad mode is always off inside forward.)  Decides whether a ReLU layer leaves its mask bits: an inference pass writes none."""
    return _GRAD_AT_APPLY[0] and any(ctx.needs_input_grad)


class _GradModeAtApply:
    """Mixin for the conv Functions: records torch.is_grad_enabled() at the call."""

    @classmethod
    def apply(cls, *args, **kwargs):
        _GRAD_AT_APPLY[0] = torch.is_grad_enabled()
        try:
            return super().apply(*args, **kwargs)
        finally:
            _GRAD_AT_APPLY[0] = True


DOWN_VARIANT = None  # test hook: xpair (0 / 1) for cvae_conv_down — two samples per tile off / on for every multi-channel `down` launch; None = automatic
UP_VARIANT = None    # test hook: (upfull, xpair, c1_walk_units) for cvae_conv_up / the xpair of cvae_conv_fp8; None = the library's automatic choice


def _conv_up(St, wp, bias, mask, Cl, nd, act, l_dims=None, mask_bits=None, want_bits=None):
    """l_dims: spatial extent (ld, lh, lw) of the result when it is not 2 s — the data gradient of a conv over an odd extent (l = 2 s + 1).
    mask_bits / want_bits: as in _conv_down."""
    B, sd, sh, sw, Cs = _cl_dims(St)
    ld, lh, lw = ((2 * sd if nd == 3 else 1), 2 * sh, 2 * sw) if l_dims is None else tuple(int(v) for v in l_dims)
    Lt = _empty((B, ld, lh, lw, Cl), St.dtype, St)
    ws, nbytes = _conv_data_workspace(St.device, B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, 1)
    label = f"conv_up nd{nd} B{B} S{sd}x{sh}x{sw}x{Cs} -> L{Cl}"
    bits_ok = UP_VARIANT is None and Cl != 1 and Cl % 32 == 0 and Cs % 16 == 0     # the test hook forces a kernel form: the tensor form of the mask, no bits
    use_mb = mask_bits if (mask_bits is not None and bits_ok) else None
    bits = _bits_for(Lt) if (want_bits and bits_ok and (mask is None or use_mb is not None)) else None
    if use_mb is not None:
        mask = None
    upfull, xpair, walk = (-1, -1, 0) if UP_VARIANT is None else (int(v) for v in UP_VARIANT)
    check(L.timed(label, lib.cvae_conv_up, ptr(St), ptr(wp), ptr(bias), ptr(mask), ptr(use_mb), ptr(Lt), ptr(bits), B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd,
                  L.dtype_code(St.dtype), L.act_code(act), ptr(ws), nbytes, upfull, xpair, walk, stream()), "conv_up")
    BITS_STATS["produced"] += bits is not None
    BITS_STATS["consumed"] += use_mb is not None
    return (Lt, bits) if want_bits is not None else Lt


_GATE_ACTS = (None, "none", "relu", "leaky001", "leaky02")


def conv_down_bwd_data(g, w_packed_up, gate, gate_act, variant=None):
    """scatter(g, w) * act'(gate): the input gradient of a 2D k4/s2/p1 `down` conv with the derivative of the activation that PRODUCED its input in the
    epilogue (cvae_conv_down_bwd_data) — one launch where _conv_up + _act_bwd are two.  g channels-last [B, 1, sh, sw, Cs] or [B, sh, sw, Cs], fp32 or bf16;
    w_packed_up = pack_weight(w, 2, True, g.dtype) of the k4 weight [Cs, Cl, 4, 4]; gate: the conv's input [B, (1,) 2 sh, 2 sw, Cl] in g's dtype, the OUTPUT of
    the activation gate_act (None / "relu" / "leaky001" / "leaky02"; LeakyReLU keeps the sign): gate > 0 ? 1 : slope, multiplied on the fp32 sum before the one
    rounding.  Returns a tensor of gate's shape (2 sh x 2 sw without a gate).  variant (tests): (upfull, xpair), the per-call kernel form of cvae_conv_up."""
    L.require_gpu(g, w_packed_up, gate)
    _forward_only("conv_down_bwd_data", g, w_packed_up, gate)
    if gate_act not in _GATE_ACTS:
        raise L.CvaeError(f"conv_down_bwd_data: gate_act must be one of {_GATE_ACTS[2:]} or None, got {gate_act!r}")
    if (gate is None) != (gate_act in (None, "none")):
        raise L.CvaeError("conv_down_bwd_data: gate and gate_act come together")
    if g.dim() not in (4, 5) or (g.dim() == 5 and g.shape[1] != 1) or not g.is_contiguous() or g.dtype not in (torch.float32, torch.bfloat16):
        raise L.CvaeError(f"conv_down_bwd_data: a contiguous channels-last [B, sh, sw, Cs] fp32 or bf16 gradient expected, got {tuple(g.shape)} {g.dtype}")
    B, sh, sw, Cs = g.shape[0], g.shape[-3], g.shape[-2], g.shape[-1]
    if w_packed_up.dtype != g.dtype or not w_packed_up.is_contiguous() or w_packed_up.numel() % (16 * Cs):
        raise L.CvaeError(f"conv_down_bwd_data: packed weight {tuple(w_packed_up.shape)} {w_packed_up.dtype} does not fit {Cs} channels in {g.dtype}")
    Cl = w_packed_up.numel() // (16 * Cs)
    oshape = tuple(g.shape[:-3]) + (2 * sh, 2 * sw, Cl) if gate is None else tuple(gate.shape)
    if gate is not None:
        if gate.dim() != g.dim() or gate.shape[0] != B or gate.shape[-1] != Cl or gate.shape[-3] // 2 != sh or gate.shape[-2] // 2 != sw:
            raise L.CvaeError(f"conv_down_bwd_data: a gate of shape {tuple(gate.shape)} does not belong to a gradient of shape {tuple(g.shape)} and {Cl} channels")
        _like_operands("conv_down_bwd_data", oshape, g.dtype, gate=gate)
    lh, lw = oshape[-3], oshape[-2]
    dx = _empty(oshape, g.dtype, g)
    ws, nbytes = _conv_data_workspace(g.device, B, 1, sh, sw, Cs, 1, lh, lw, Cl, 2, 1)
    upfull, xpair = (-1, -1) if variant is None else (int(v) for v in variant)
    check(L.timed(f"conv_down_bwd_data B{B} S{sh}x{sw}x{Cs} -> L{Cl}", lib.cvae_conv_down_bwd_data, ptr(g), ptr(w_packed_up), ptr(gate), ptr(dx), B, sh, sw, Cs, lh, lw, Cl,
                  2, L.dtype_code(g.dtype), L.act_code(gate_act), ptr(ws), nbytes, upfull, xpair, stream()), "conv_down_bwd_data")
    return dx


def conv_down_image_bwd_data(g, w_folded, alpha=1.0, out=None, accumulate=False):
    """The gradient with respect to the IMAGE of the first k4/s2/p1 conv of an encoder (cvae_conv_down_image_bwd_data): fp32 [B, 1, 2 sh, 2 sw] =
    alpha * scatter(g, w), whatever g's dtype.  g channels-last [B, 1, sh, sw, 32] or [B, sh, sw, 32], fp32 or bf16: the gradient of the layer's pre-activation;
    w_folded: the fp32 k4 weight [32, 1, 4, 4] as fold_bn_conv leaves it (never rounded: all products and sums are fp32).  out: a contiguous fp32
    [B, 1, 2 sh, 2 sw] tensor to write; with accumulate (needs out) alpha * scatter is ADDED to it (one fma per element), which is how a path integral sums
    its steps without a [steps, B, H, W] tensor.  Every element has one owner thread and a sum order that depends on the geometry alone."""
    L.require_gpu(g, w_folded, out)
    _forward_only("conv_down_image_bwd_data", g, w_folded, out)
    if (g.dim() not in (4, 5) or (g.dim() == 5 and g.shape[1] != 1) or g.shape[-1] != 32 or not g.is_contiguous() or g.dtype not in (torch.float32, torch.bfloat16)
            or g.shape[-3] < 1 or g.shape[-2] < 1):
        raise L.CvaeError(f"conv_down_image_bwd_data: a contiguous channels-last [B, sh, sw, 32] fp32 or bf16 gradient expected, got {tuple(g.shape)} {g.dtype}")
    if tuple(w_folded.shape) != (32, 1, 4, 4) or w_folded.dtype != torch.float32 or not w_folded.is_contiguous() or w_folded.device != g.device:
        raise L.CvaeError(f"conv_down_image_bwd_data: the contiguous fp32 k4 weight [32, 1, 4, 4] on {g.device} expected, got {tuple(w_folded.shape)} {w_folded.dtype}")
    B, sh, sw = g.shape[0], g.shape[-3], g.shape[-2]
    shape = (B, 1, 2 * sh, 2 * sw)
    if out is None:
        if accumulate:
            raise L.CvaeError("conv_down_image_bwd_data: accumulate adds to `out`, which was not given")
        out = _empty(shape, torch.float32, g)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != g.device:
        raise L.CvaeError(f"conv_down_image_bwd_data: out must be a contiguous float32 {shape} tensor on {g.device}, got {tuple(out.shape)} {out.dtype}")
    if B == 0:
        return out
    check(L.timed(f"conv_down_image_bwd_data B{B} S{sh}x{sw}x32", lib.cvae_conv_down_image_bwd_data, ptr(g), ptr(w_folded), ptr(out), B, sh, sw, 32, 2 * sh, 2 * sw, 2,
                  L.dtype_code(g.dtype), float(alpha), int(bool(accumulate)), stream()), "conv_down_image_bwd_data")
    return out


DEFER_WGRAD = True     # weight gradients of the MFMA conv layers are queued during a backward pass and computed by ONE grouped launch (+ one
                       # reduce launch) at its end (cvae_conv_wgrad_multi): the small layers run in the shadow of the large ones
_WG_PENDING = []
_WG_QUEUED = [False]
_WG_TASK = [-1]            # id of the autograd graph task the queue (and its end-of-backward callback) belongs to
_WG_SHARED = set()         # weights met twice in this pass (shared by two layers): their gradients are computed at once


def _graph_task_id():
    f = getattr(torch._C, "_current_graph_task_id", None)
    return f() if f is not None else -1


def _wg_task_is_current():
    return _WG_QUEUED[0] and _WG_TASK[0] == _graph_task_id()


def reset_pending_wgrads():
    """Forget queued weight gradients without computing them.  A backward pass that raised never runs its end-of-backward callback (the
    engine drops it), so its entries — and the "callback queued" flag — would otherwise outlive it; every deferral checks for that
    itself (a queue that belongs to another graph task is stale), and callers that catch a failed step / capture may call this too."""
    _WG_PENDING.clear()
    _WG_SHARED.clear()
    _WG_QUEUED[0] = False
    _WG_TASK[0] = -1


def _wgrad_flush():
    """Run every queued weight gradient (grouped by device / nd / dtype, <= 8 layers per launch).  Installed as the autograd engine's
    end-of-backward callback, so `.grad` is complete when loss.backward() / torch.autograd.grad() returns — any optimizer works.
    Every entry owns a reference to the STORAGE of its outputs (not to the tensors: a second tensor reference would make AccumulateGrad
    clone the still-empty gradient instead of adopting it), so the launch never writes to memory the allocator has handed on — also when
    nobody kept the gradient (torch.autograd.grad(loss, [x]) with trainable weights)."""
    if not _WG_PENDING:
        return
    todo = list(_WG_PENDING)
    _WG_PENDING.clear()
    groups = {}
    for e in todo:
        groups.setdefault((e["S"].device, e["nd"], e["S"].dtype), []).append(e)
    for (dev, nd, dt), es in groups.items():
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            for c0 in range(0, len(es), 8):
                ch = es[c0:c0 + 8]
                k = len(ch)
                vp = lambda key: (C_.c_void_p * k)(*[((e[key] if isinstance(e[key], int) else e[key].data_ptr()) if e[key] is not None else None) for e in ch])
                dims = (C_.c_int64 * (9 * k))(*[v for e in ch for v in e["dims"]])
                label = f"conv_wgrad_multi nd{nd} B{ch[0]['dims'][0]} " + ";".join("S{1}x{2}x{3}x{4}L{8}".format(*e["dims"]) for e in ch)
                check(L.timed(label, lib.cvae_conv_wgrad_multi, k, vp("S"), vp("L"), vp("dW"), vp("db"), (C_.c_int * k)(*[e["side"] for e in ch]), vp("ws"),
                              (C_.c_size_t * k)(*[e["nbytes"] for e in ch]), dims, nd, L.dtype_code(dt), stream()), "conv_wgrad_multi")
                for e in ch:                                 # scratch allocated on a forked side stream (FORK_BACKWARD), used here on the caller's:
                    if e["alloc_stream"] != cur.cuda_stream:  # tell the caching allocator, or the side stream's pool may hand it on too early
                        e["ws"].record_stream(cur)


def _wgrad_callback():
    _WG_QUEUED[0] = False
    _WG_TASK[0] = -1
    _WG_SHARED.clear()
    _wgrad_flush()


def flush_pending_wgrads():
    """Compute queued weight gradients now (FusedAdam.overlap_backward reads gradients before the backward pass has ended)."""
    _wgrad_flush()


def _conv_wgrad(St, Lt, nd, wshape, want_sbias=False, want_lbias=False, may_defer=False, wid=None):
    """dW and, in the same pass, the bias gradient: want_sbias = per-channel sum of S (Conv layer), want_lbias = of L (ConvTranspose).
    may_defer: the caller has checked that nothing reads the returned tensors before the backward pass ends (see _can_defer)."""
    B, sd, sh, sw, Cs = _cl_dims(St)
    _, ld, lh, lw, Cl = _cl_dims(Lt)
    dW = torch.empty(wshape, dtype=torch.float32, device=St.device)
    db = torch.empty(Cl if want_lbias else Cs, dtype=torch.float32, device=St.device) if (want_sbias or want_lbias) else None
    nbytes = lib.cvae_conv_wgrad_workspace_bytes(Cs, Cl, nd)
    ws = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=St.device)
    if Lt.dtype != St.dtype:                                 # the image layer of a bf16 model: L is the fp32 input itself
        if Cl != 1 or want_lbias:
            raise L.CvaeError("a mixed-dtype weight gradient is available for the single-channel image layer only")
        check(L.timed(f"conv_wgrad nd{nd} B{B} S{sd}x{sh}x{sw}x{Cs} L{Cl}", lib.cvae_conv_wgrad_image, ptr(St), ptr(Lt), L.dtype_code(Lt.dtype), ptr(dW), ptr(db), ptr(ws), nbytes,
                      B, sd, sh, sw, Cs, ld, lh, lw, nd, L.dtype_code(St.dtype), stream()), "conv_wgrad_image")
        return (dW, db) if want_sbias else dW
    exact2x = lh == 2 * sh and lw == 2 * sw and (nd == 2 or ld == 2 * sd)
    if (DEFER_WGRAD and may_defer and Cl != 1 and Cs % 64 == 0 and Cl % 32 == 0 and B > 0 and (exact2x or not want_lbias)):
        try:
            tid = _graph_task_id()
            if _WG_QUEUED[0] and _WG_TASK[0] != tid:         # left behind by a backward pass that raised: its callback never ran
                reset_pending_wgrads()
            if not _WG_QUEUED[0]:
                torch.autograd.Variable._execution_engine.queue_callback(_wgrad_callback)     # only legal inside a backward pass
                _WG_QUEUED[0] = True
                _WG_TASK[0] = tid
            # the outputs are queued by ADDRESS plus a reference to their STORAGE: a second reference to the tensors dW / db would make
            # AccumulateGrad clone them (still empty) instead of adopting them as .grad
            _WG_PENDING.append(dict(S=St, L=Lt, dW=dW.data_ptr(), db=(db.data_ptr() if db is not None else None), side=1 if want_lbias else 0, ws=ws,
                                    keep=(dW.untyped_storage(), db.untyped_storage() if db is not None else None), wid=wid,
                                    alloc_stream=torch.cuda.current_stream(St.device).cuda_stream,
                                    nbytes=nbytes, nd=nd, dims=(B, sd, sh, sw, Cs, ld, lh, lw, Cl)))
            return (dW, db) if (want_sbias or want_lbias) else dW
        except RuntimeError:
            pass                                             # not inside a backward pass (a direct call): compute now
    check(L.timed(f"conv_wgrad nd{nd} B{B} S{sd}x{sh}x{sw}x{Cs} L{Cl}", lib.cvae_conv_wgrad, ptr(St), ptr(Lt), ptr(dW), ptr(db), 1 if want_lbias else 0, ptr(ws), nbytes,
                  B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, L.dtype_code(St.dtype), stream()), "conv_wgrad")
    return (dW, db) if (want_sbias or want_lbias) else dW


def _channel_sum(x):
    Cc = x.shape[-1]
    out = torch.empty(Cc, dtype=torch.float32, device=x.device)
    P = x.numel() // Cc
    _t, wp, wb = _scratch(lib.cvae_channel_sum_workspace_bytes(P, Cc, L.dtype_code(x.dtype)), x)
    check(lib.cvae_channel_sum(ptr(x), ptr(out), P, Cc, L.dtype_code(x.dtype), wp, wb, stream()), "channel_sum")
    return out


def _act_bwd(g, y, act):
    out = torch.empty_like(g)
    check(lib.cvae_act_bwd(ptr(g), ptr(y), ptr(out), g.numel(), L.act_code(act), L.dtype_code(g.dtype), stream()), "act_bwd")
    return out


class ConvDown(_GradModeAtApply, torch.autograd.Function):
    """nn.Conv{2,3}d(k=4, s=2, p=1) + bias + activation on channels-last tensors.

    in_is_relu_out: the input is itself a ReLU output, so the ReLU mask of the *producer* is fused into this op's
      backward-data epilogue (the gradient it returns is already masked).
    grad_premasked: the consumer of this op's output fuses this op's ReLU mask the same way, so the incoming
      gradient needs no separate activation-backward pass.  (ReLU masking is idempotent; the flags only save traffic.)
    """

    @staticmethod
    def forward(ctx, x, weight, bias, nd, act, in_is_relu_out, grad_premasked, packed=None, out_dtype=None, f8=None):
        """out_dtype (single-channel image layer only): compute / output dtype when it differs from x's — the fp32 input batch of a bf16 model
        is read as it is, without a cast pass.
        f8 (causal_vae_amd.fp8): the forward product on fp8 operands — dict(xq = codes of x, wq = fp8 weight panels, dscale, want_out8, amax); the
        codes of the result are left in f8["y8"].  x (bf16) is still what the backward pass reads."""
        L.require_gpu(x, weight, bias)
        Cs = weight.shape[0]
        if out_dtype is not None and out_dtype == x.dtype:
            out_dtype = None
        if f8 is not None and f8.get("side"):
            # the single-channel image layer of an fp8 forward: bf16 arithmetic as always, and the result a second time as fp8 codes (+ its amax)
            # for the fp8 conv that follows (cvae_conv_down_image_f8)
            B, ld, lh, lw, Cl = _cl_dims(x)
            if Cl != 1 or (out_dtype or x.dtype) != torch.bfloat16:
                raise L.CvaeError("the fp8 side output exists for the single-channel image layer of a bf16 model only")
            sd, sh, sw = (ld // 2 if nd == 3 else 1), lh // 2, lw // 2
            y = _empty((B, sd, sh, sw, Cs), torch.bfloat16, x)
            y8 = torch.empty((B, sd, sh, sw, Cs), dtype=torch.uint8, device=x.device)
            f8["bits"] = _bits_for(y) if (MASK_BITS and act == "relu" and _backward_may_follow(ctx)) else None
            check(L.timed(f"conv_down nd{nd} B{B} L{ld}x{lh}x{lw}x{Cl} -> S{Cs}", lib.cvae_conv_down_image_f8, ptr(x), L.dtype_code(x.dtype), ptr(weight.contiguous()), ptr(bias),
                          ptr(y), ptr(y8), ptr(f8["inv_scale"]), ptr(f8.get("amax")), ptr(f8["bits"]), B, sd, sh, sw, Cs, ld, lh, lw, nd, L.act_code(act), stream()), "conv_down_image_f8")
            f8["y8"] = y8
            bits = f8.get("bits")
        elif f8 is not None:
            want_bits = MASK_BITS and act == "relu" and _backward_may_follow(ctx)
            res = conv_fp8(False, f8["xq"], f8["wq"], bias, Cs, nd, act, dscale=f8["dscale"], want_out8=f8.get("want_out8", False), amax=f8.get("amax"), want_bits=want_bits)
            y, f8["y8"], bits = res
        else:
            wp = packed[0] if packed is not None else pack_weight(weight, nd, False, out_dtype or x.dtype)
            y, bits = _conv_down(x, wp, bias, None, Cs, nd, act, out_dtype, want_bits=MASK_BITS and act == "relu" and _backward_may_follow(ctx))     # no backward to come (inference): no mask
        if bits is not None:
            y._relu_bits = bits                              # travels with the activation to the layer whose backward applies this ReLU
        ctx.x_bits = getattr(x, "_relu_bits", None) if (MASK_BITS and in_is_relu_out) else None
        ctx.save_for_backward(x, weight, y)
        ctx.bias_ref = bias
        ctx.packed_bwd = packed[1] if packed is not None else None
        ctx.cfg = (nd, act, in_is_relu_out, grad_premasked, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        nd, act, in_relu, premasked, has_bias = ctx.cfg
        g = g.contiguous()
        if act not in (None, "none") and not (premasked and act == "relu"):
            g = _act_bwd(g, y, act)
        dx = dw = db = None
        want_db = has_bias and ctx.needs_input_grad[2]
        fork = _Fork(g.device, g.shape[0] * g.shape[1] * g.shape[2] * g.shape[3])
        with fork:
            if ctx.needs_input_grad[1]:
                defer = _can_defer(weight, ctx.bias_ref if want_db else None)
                if want_db:
                    dw, db = _conv_wgrad(g, x, nd, weight.shape, want_sbias=True, may_defer=defer, wid=id(weight))
                else:
                    dw = _conv_wgrad(g, x, nd, weight.shape, may_defer=defer, wid=id(weight))
            elif want_db:
                db = _channel_sum(g)
        if ctx.needs_input_grad[0]:
            wp_up = ctx.packed_bwd if ctx.packed_bwd is not None else pack_weight(weight, nd, True, g.dtype)
            if x.dtype != g.dtype:
                raise L.CvaeError("the image read in its own dtype carries no gradient (cast it first if it needs one)")
            dx = _conv_up(g, wp_up, None, x if in_relu else None, weight.shape[1], nd, None, l_dims=x.shape[1:4], mask_bits=ctx.x_bits if in_relu else None)
        fork.join(dw, db)
        return dx, dw, db, None, None, None, None, None, None, None


class ConvUp(_GradModeAtApply, torch.autograd.Function):
    """nn.ConvTranspose{2,3}d(k=4, s=2, p=1) + bias + activation on channels-last tensors (flags as ConvDown)."""

    @staticmethod
    def forward(ctx, x, weight, bias, nd, act, in_is_relu_out, grad_premasked, packed=None, f8=None):
        L.require_gpu(x, weight, bias)
        Cl = weight.shape[1]
        if f8 is not None:                                   # forward product on fp8 operands (see ConvDown.forward)
            res = conv_fp8(True, f8["xq"], f8["wq"], bias, Cl, nd, act, dscale=f8["dscale"], want_out8=f8.get("want_out8", False), amax=f8.get("amax"),
                           want_bits=MASK_BITS and act == "relu" and _backward_may_follow(ctx))
            y, f8["y8"], bits = res
        else:
            wp = packed[1] if packed is not None else pack_weight(weight, nd, True, x.dtype)
            y, bits = _conv_up(x, wp, bias, None, Cl, nd, act, want_bits=MASK_BITS and act == "relu" and _backward_may_follow(ctx))
        if bits is not None:
            y._relu_bits = bits
        ctx.x_bits = getattr(x, "_relu_bits", None) if (MASK_BITS and in_is_relu_out) else None
        ctx.save_for_backward(x, weight, y)
        ctx.bias_ref = bias
        ctx.packed_bwd = packed[0] if packed is not None else None
        ctx.cfg = (nd, act, in_is_relu_out, grad_premasked, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        nd, act, in_relu, premasked, has_bias = ctx.cfg
        g = g.contiguous()
        if act not in (None, "none") and not (premasked and act == "relu"):
            g = _act_bwd(g, y, act)
        dx = dw = db = None
        fork = _Fork(g.device, x.shape[0] * x.shape[1] * x.shape[2] * x.shape[3])
        with fork:
            want_db = has_bias and ctx.needs_input_grad[2]
            if ctx.needs_input_grad[1]:
                defer = _can_defer(weight, ctx.bias_ref if want_db else None)
                if want_db:
                    dw, db = _conv_wgrad(x, g, nd, weight.shape, want_lbias=True, may_defer=defer, wid=id(weight))
                else:
                    dw = _conv_wgrad(x, g, nd, weight.shape, may_defer=defer, wid=id(weight))
            elif want_db:
                db = _channel_sum(g)
        if ctx.needs_input_grad[0]:
            wp_dn = ctx.packed_bwd if ctx.packed_bwd is not None else pack_weight(weight, nd, False, g.dtype)
            dx = _conv_down(g, wp_dn, None, x if in_relu else None, weight.shape[0], nd, None, mask_bits=ctx.x_bits if in_relu else None)
        fork.join(dw, db)
        return dx, dw, db, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------ fp8 inference (decode only)
FP8_MAX = 448.0      # OCP e4m3


def quantize_fp8(x, scale):
    """fp8 (e4m3) codes of x / scale as a uint8 tensor of x's shape (x: fp32 or bf16, contiguous)."""
    L.require_gpu(x)
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib.cvae_quantize_fp8(ptr(x), L.dtype_code(x.dtype), ptr(q), x.numel(), 1.0 / float(scale), None, None, stream()), "quantize_fp8")
    return q


def pack_weight_fp8(w, nd, for_up, scale):
    """fp32 [Cs][Cl][k..] -> the MFMA operand panels of pack_weight as fp8 codes of w / scale."""
    w = w.contiguous()
    out = torch.empty(w.numel(), dtype=torch.uint8, device=w.device)
    check(lib.cvae_conv_pack_weight_fp8(ptr(w), ptr(out), w.shape[0], w.shape[1], nd, int(for_up), 1.0 / float(scale), stream()), "conv_pack_weight_fp8")
    return out


def conv_up_fp8(Sq, wq, bias, Cl, nd, act, acc_scale, out_scale=None):
    """nn.ConvTranspose{2,3}d(k4, s2, p1) + bias + activation on fp8 operands (forward only).  Sq: uint8 codes [B, sd, sh, sw, Cs]; result bf16
    (out_scale None) or fp8 codes of result / out_scale."""
    return conv_fp8(True, Sq, wq, bias, Cl, nd, act, acc_scale=acc_scale, out8_scale=out_scale, codes_only=out_scale is not None)


def conv_up_c1_fp8in(Sq, weight, bias, in_scale, nd, act):
    """The single-channel nn.ConvTranspose3d(32, 1, 4, 2, 1) end of a decoder fed by fp8 codes (forward only; cvae_conv_up_c1_fp8in): Sq uint8 [B, sd, sh, sw, 32] =
    codes of activation / in_scale, weight / bias the layer's fp32 parameters.  Returns bf16 [B, 2sd, 2sh, 2sw, 1]."""
    L.require_gpu(Sq, weight)
    if Sq.dtype != torch.uint8 or nd != 3 or Sq.dim() != 5 or Sq.shape[-1] != 32 or tuple(weight.shape[:2]) != (32, 1):
        raise L.CvaeError(f"conv_up_c1_fp8in: 3D fp8 codes [B, d, h, w, 32] and a ConvTranspose3d(32, 1) weight expected, got {tuple(Sq.shape)} {Sq.dtype} / {tuple(weight.shape)}")
    Sq, weight = Sq.contiguous(), weight.contiguous().float()
    B, sd, sh, sw, Cs = Sq.shape
    out = torch.empty(B, 2 * sd, 2 * sh, 2 * sw, 1, dtype=torch.bfloat16, device=Sq.device)
    check(L.timed(f"up_c1_fp8in nd{nd} B{B} S{sd}x{sh}x{sw}x{Cs} L1", lib.cvae_conv_up_c1_fp8in, ptr(Sq), ptr(weight), ptr(bias.contiguous().float() if bias is not None else None),
                  ptr(out), float(in_scale), B, sd, sh, sw, Cs, nd, L.act_code(act), stream()), "conv_up_c1_fp8in")
    return out


AMAX_SLOTS = 4096        # CVAE_AMAX_SLOTS


def conv_fp8(up, xq, wq, bias, Cout, nd, act, acc_scale=None, out8_scale=None, codes_only=False, dscale=None, want_out8=False, amax=None, want_bits=None):
    """One fp8 (e4m3) product on the block-scaled MFMA (cvae_conv_fp8; forward only).  up False: nn.Conv (k4, s2, p1) of xq [B, ld, lh, lw, Cin];
    up True: nn.ConvTranspose of xq [B, sd, sh, sw, Cin].  xq, wq: uint8 codes (quantize_fp8 / pack_weight_fp8 panels).
    Scales by value (acc_scale = s_x * s_w; out8_scale = the scale of the fp8 copy of the result) or on the device (dscale: float32 tensor
    {acc_scale, 1 / out8_scale}, re-read by every launch — the training step's delayed scaling).
    Returns the bf16 result; with codes_only the fp8 codes instead; with want_out8 (or out8_scale and not codes_only) the pair (bf16, codes); with
    want_bits given (True / False) always the triple (bf16, codes or None, ReLU mask bits of the result or None).
    amax: optional uint32 tensor of AMAX_SLOTS words that records max |result|."""
    L.require_gpu(xq)
    if xq.dtype != torch.uint8 or wq.dtype != torch.uint8:
        raise L.CvaeError("conv_fp8: activations and weight panels must be fp8 codes (uint8 tensors from quantize_fp8 / pack_weight_fp8)")
    xq = xq.contiguous()
    B, d, h, w_, Cin = _cl_dims(xq)
    if wq.numel() != Cin * Cout * 4 ** nd:
        raise L.CvaeError(f"conv_fp8: weight panels hold {wq.numel()} codes, expected Cin * Cout * 4^nd = {Cin * Cout * 4 ** nd}")
    if up:
        sd, sh, sw, Cs, Cl = d, h, w_, Cin, Cout
        ld, lh, lw = (2 * sd if nd == 3 else 1), 2 * sh, 2 * sw
        oshape = (B, ld, lh, lw, Cl)
    else:
        ld, lh, lw, Cl, Cs = d, h, w_, Cin, Cout
        sd, sh, sw = (ld // 2 if nd == 3 else 1), lh // 2, lw // 2
        oshape = (B, sd, sh, sw, Cs)
    if dscale is None and acc_scale is None:
        raise L.CvaeError("conv_fp8: give acc_scale (by value) or dscale (device pair)")
    pair = (want_out8 or out8_scale is not None) and not codes_only
    out = torch.empty(oshape, dtype=torch.uint8 if codes_only else torch.bfloat16, device=xq.device)
    out8 = torch.empty(oshape, dtype=torch.uint8, device=xq.device) if pair else None
    ws, nbytes = (None, 0) if codes_only else _conv_data_workspace(xq.device, B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, int(bool(up)))
    label = (f"conv_up fp8 nd{nd} B{B} S{sd}x{sh}x{sw}x{Cs} -> L{Cl}" if up else f"conv_down fp8 nd{nd} B{B} L{ld}x{lh}x{lw}x{Cl} -> S{Cs}")
    bits = _bits_for(out) if (want_bits and not codes_only and Cout % 32 == 0) else None
    check(L.timed(label, lib.cvae_conv_fp8, int(bool(up)), ptr(xq), ptr(wq), ptr(bias), ptr(out), L.FP8 if codes_only else L.BF16, ptr(out8), ptr(dscale),
                  float(acc_scale if acc_scale is not None else 1.0), (1.0 / float(out8_scale)) if out8_scale is not None else 1.0, ptr(amax),
                  B, sd, sh, sw, Cs, ld, lh, lw, Cl, nd, L.act_code(act), ptr(ws), nbytes, -1 if UP_VARIANT is None else int(UP_VARIANT[1]), ptr(bits), stream()), "conv_fp8")
    if want_bits is not None:                                # the training forward's call: always the triple (result, codes or None, mask bits or None)
        return out, out8, bits
    return (out, out8) if pair else out


def absmax(x, slots):
    """Record max |x| in `slots` (AMAX_SLOTS uint32 / int32 words of float bits; atomicMax — accumulates over calls until cleared)."""
    L.require_gpu(x)
    x = x.contiguous()
    check(lib.cvae_absmax(ptr(x), L.dtype_code(x.dtype), x.numel(), ptr(slots), stream()), "absmax")


def quantize_fp8_dev(x, inv_scale_dev, amax=None):
    """quantize_fp8 with 1 / scale read from a device float (one-element tensor); optionally records max |x|."""
    L.require_gpu(x)
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib.cvae_quantize_fp8(ptr(x), L.dtype_code(x.dtype), ptr(q), x.numel(), 1.0, ptr(inv_scale_dev), ptr(amax), stream()), "quantize_fp8")
    return q


def pack_weights_fp8(weights, nd, for_up, inv_scale_devs, amaxes=None, outs=None):
    """fp8 operand panels of several conv weights in one launch (cvae_conv_pack_weights_fp8): 1 / s_w of each from device memory, max |w| recorded.
    outs: optional preallocated uint8 tensors (a captured step reuses them)."""
    k = len(weights)
    ws = [w.contiguous() for w in weights]
    if outs is None:
        outs = [torch.empty(w.numel(), dtype=torch.uint8, device=w.device) for w in ws]
    if k:
        vp = lambda ts: (C_.c_void_p * k)(*[(t.data_ptr() if t is not None else None) for t in ts])
        check(lib.cvae_conv_pack_weights_fp8(vp(ws), vp(outs), (C_.c_int64 * k)(*[w.shape[0] for w in ws]), (C_.c_int64 * k)(*[w.shape[1] for w in ws]),
                                             (C_.c_int * k)(*[int(bool(f)) for f in for_up]), vp(inv_scale_devs), vp(amaxes if amaxes is not None else [None] * k),
                                             k, nd, stream()), "conv_pack_weights_fp8")
    return outs


class Fp8Scales:
    """Device-resident delayed scaling for the fp8 forward of a training step: `n` tracked tensors (activations and weights), each with an amax
    record, a scale and its reciprocal; `layers` = [(input tensor, weight tensor, output tensor or -1)] per fp8 product, whose {s_in * s_w, 1 / s_out}
    pairs land in `dscale[l]`.  update() (one tiny launch, capturable) turns the amaxes recorded since the last call into the scales of the next
    step: scale = headroom * amax / 448 — e4m3 is a floating-point format, so headroom costs no precision until the subnormals."""

    def __init__(self, n, layers, device, headroom=2.0):
        self.n, self.layers, self.headroom = int(n), [tuple(int(v) for v in l) for l in layers], float(headroom)
        self.amax = torch.zeros(self.n, AMAX_SLOTS, dtype=torch.int32, device=device)
        self.scale = torch.ones(self.n, dtype=torch.float32, device=device)
        self.inv_scale = torch.ones(self.n, dtype=torch.float32, device=device)
        self.dscale = torch.zeros(max(len(self.layers), 1), 2, dtype=torch.float32, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)
        k = len(self.layers)
        self._li = [(C_.c_int * max(k, 1))(*([l[j] for l in self.layers] or [0])) for j in range(3)]

    def update(self):
        check(lib.cvae_fp8_scale_update(ptr(self.amax), ptr(self.scale), ptr(self.inv_scale), self.n, self.headroom, self._li[0], self._li[1], self._li[2],
                                        len(self.layers), ptr(self.dscale), ptr(self.ticket), stream()), "fp8_scale_update")

    def state(self):
        return {"scale": self.scale.detach().cpu().clone(), "amax": self.amax.detach().cpu().clone()}

    def load_state(self, st):
        self.scale.copy_(st["scale"]); self.inv_scale.copy_(1.0 / st["scale"].to(self.scale.device)); self.amax.copy_(st["amax"])


class Activation(torch.autograd.Function):
    """Stand-alone ReLU / Sigmoid / LeakyReLU(0.2) (used where no producer kernel can fuse it, e.g. after BatchNorm1d)."""

    @staticmethod
    def forward(ctx, x, act):
        L.require_gpu(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib.cvae_act_fwd(ptr(x), ptr(y), x.numel(), L.act_code(act), L.dtype_code(x.dtype), stream()), "act_fwd")
        ctx.save_for_backward(y)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return _act_bwd(g.contiguous(), y, ctx.act), None


# ------------------------------------------------------------------------------------------------ pool / resize
class AdaptiveAvgPoolFlatten(torch.autograd.Function):
    """nn.AdaptiveAvgPool{2,3}d(out) + nn.Flatten on a channels-last input -> fp32 [B, C*prod(out)] in NC(D)HW flatten order.
    relu_input: the input is a ReLU output whose mask is fused into the backward."""

    @staticmethod
    def forward(ctx, x, out_size, relu_input):
        L.require_gpu(x)
        B, D, H, W, Cc = _cl_dims(x)
        OD, OH, OW = out_size
        F = Cc * OD * OH * OW
        out = _empty((B, F), torch.float32, x)
        check(lib.cvae_adaptive_avgpool_fwd(ptr(x), ptr(out), B, D, H, W, Cc, OD, OH, OW, F, L.dtype_code(x.dtype), stream()), "avgpool_fwd")
        ctx.save_for_backward(x)
        ctx.cfg = (out_size, relu_input)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        (OD, OH, OW), relu_input = ctx.cfg
        B, D, H, W, Cc = x.shape
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(lib.cvae_adaptive_avgpool_bwd(ptr(g), ptr(x) if relu_input else None, ptr(dx), B, D, H, W, Cc, OD, OH, OW, g.shape[1],
                                            L.dtype_code(x.dtype), stream()), "avgpool_bwd")
        return dx, None, None


class FlattenCat(torch.autograd.Function):
    """cat([Flatten(AdaptiveAvgPool(x)), *extras], dim=1) written in place: the pooled / flattened features go straight into the wide matrix (row stride
    = its width) and the extras follow in one panel launch; the backward reads the feature columns of the incoming gradient where they lie."""

    @staticmethod
    def forward(ctx, x, out_size, relu_input, *extras):
        L.require_gpu(x, *extras)
        B, D, H, W, Cc = _cl_dims(x)
        OD, OH, OW = out_size
        F = Cc * OD * OH * OW
        extras = [_as_panel(e) for e in extras]
        if len(extras) > 8 or any(e.shape[0] != B for e in extras):
            raise L.CvaeError("FlattenCat: up to 8 extras with the batch of x")
        K = F + sum(e.shape[1] for e in extras)
        out = _empty((B, K), torch.float32, x)
        check(lib.cvae_adaptive_avgpool_fwd(ptr(x), ptr(out), B, D, H, W, Cc, OD, OH, OW, K, L.dtype_code(x.dtype), stream()), "avgpool_fwd")
        if extras:
            _copy_panels(extras, out, F, False)
        ctx.save_for_backward(x)
        ctx.cfg = (out_size, relu_input, F, [e.shape[1] for e in extras])
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        (OD, OH, OW), relu_input, F, widths = ctx.cfg
        B, D, H, W, Cc = x.shape
        g = g.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib.cvae_adaptive_avgpool_bwd(ptr(g), ptr(x) if relu_input else None, ptr(dx), B, D, H, W, Cc, OD, OH, OW, g.shape[1],
                                                L.dtype_code(x.dtype), stream()), "avgpool_bwd")
        outs, col = [], F
        for i, w in enumerate(widths):
            if ctx.needs_input_grad[3 + i]:
                o = _empty((B, w), torch.float32, g)
                _copy_panels([o], g, col, True)
                outs.append(o)
            else:
                outs.append(None)
            col += w
        return (dx, None, None) + tuple(outs)


class UpsampleLinear(torch.autograd.Function):
    """F.interpolate(mode='bilinear'|'trilinear', align_corners=False) on a channels-last input -> fp32 channels-last."""

    @staticmethod
    def forward(ctx, x, size):
        L.require_gpu(x)
        B, d, h, w, Cc = _cl_dims(x)
        D, H, W = size
        out = _empty((B, D, H, W, Cc), torch.float32, x)
        if Cc == 1 and lib.cvae_up2x_supported(B, d, h, w, D, H, W):          # exact 2x, one channel: the block kernel of csrc/recon_loss.hip
            check(lib.cvae_up2x_fwd(ptr(x), ptr(out), B, d, h, w, D, H, W, L.dtype_code(x.dtype), stream()), "up2x_fwd")
        else:
            check(lib.cvae_upsample_linear_fwd(ptr(x), ptr(out), B, d, h, w, D, H, W, Cc, L.dtype_code(x.dtype), stream()), "upsample_fwd")
        ctx.meta = (x.shape, x.dtype, size)
        return out

    @staticmethod
    def backward(ctx, g):
        shape, dt, (D, H, W) = ctx.meta
        B, d, h, w, Cc = shape
        g = g.contiguous()
        dx = _empty(shape, dt, g)
        check(lib.cvae_upsample_linear_bwd(ptr(g), ptr(dx), B, d, h, w, D, H, W, Cc, L.dtype_code(dt), stream()), "upsample_bwd")
        return dx, None


# ------------------------------------------------------------------------------------------------ linear / BN
LINEAR_BF16_MIN_WORK = 1 << 24      # M * K * N below which a bf16-math Linear stays on the fp32 kernels (launch-bound there, and exact)


SMALL_DENSE = __import__("os").environ.get("CVAE_SMALL_DENSE", "1") != "0"    # (env switch: A/B runs) small layers at large batch through csrc/small_dense.hip


class Linear(torch.autograd.Function):
    """nn.Linear + optional fused activation.  fp32 tensors always; math = torch.float32: exact-fp32 MFMA (default);
    math = torch.bfloat16: operands rounded to bf16 inside the GEMM kernels (fp32 accumulate) for batches > 16 and M*K*N >= LINEAR_BF16_MIN_WORK."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, math=None, in_act=None, grad_premasked=False):
        """in_act: x is the OUTPUT of that activation and this layer is its only consumer — the data gradient leaves this layer's backward already multiplied by
        the activation's derivative (cvae_linear_bwd_data's in_act); grad_premasked: the gradient arriving at this layer's output already carries act'(y) (the next
        layer was given in_act = act).  layers.MLP sets the pair for consecutive layers at batch sizes above 16: one elementwise launch fewer per layer."""
        L.require_gpu(x, weight, bias)
        if x.dtype != torch.float32:
            raise L.CvaeError("linear layers run in float32")
        x = x.contiguous()
        M, K = x.shape
        N = weight.shape[0]
        b16 = math == torch.bfloat16 and M > 16 and M * K * N >= LINEAR_BF16_MIN_WORK
        y = _empty((M, N), torch.float32, x)
        small = SMALL_DENSE and not b16 and bool(lib.cvae_small_dense_supported(M, K, N))     # small layer, large batch: the weight lives in LDS (csrc/small_dense.hip)
        if small:
            check(L.timed(f"linear_fwd M{M} K{K} N{N} small", lib.cvae_small_dense_fwd, ptr(x), ptr(weight.contiguous()), ptr(bias), ptr(y), M, K, N, K, N, L.act_code(act), stream()),
                  "small_dense_fwd")
            ctx.save_for_backward(x, weight, y)
            ctx.cfg = (act, bias is not None, b16)
            ctx.chain = (in_act if in_act not in (None, "none") else None, bool(grad_premasked))
            ctx.small = True
            return y
        ctx.small = False
        _t, wp, wb = _scratch(lib.cvae_linear_workspace_bytes(M, K, N, 0), x)
        check(L.timed(f"linear_fwd M{M} K{K} N{N}" + (" bf16" if b16 else ""), lib.cvae_linear_fwd, ptr(x), ptr(weight), ptr(bias), ptr(y), M, K, N, K, N, L.act_code(act),
                      int(b16), wp, wb, stream()), "linear_fwd")
        ctx.save_for_backward(x, weight, y)
        if (in_act not in (None, "none") or grad_premasked) and M <= 16:
            raise L.CvaeError("Linear: in_act / grad_premasked are for batches above 16 (the skinny kernels fuse the activation gradient on the consuming side)")
        ctx.cfg = (act, bias is not None, b16)
        ctx.chain = (in_act if in_act not in (None, "none") else None, bool(grad_premasked))
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        act, has_bias, b16 = ctx.cfg
        in_act, premasked = ctx.chain
        g = g.contiguous()
        M, K = x.shape
        N = weight.shape[0]
        if ctx.small:
            # this layer's activation gradient (unless the next layer already applied it) and the previous layer's (in_act) both ride in these launches
            has_act = act not in (None, "none") and not premasked
            ya, ac = (ptr(y), L.act_code(act)) if has_act else (None, L.ACT_NONE)
            dx = dw = db = None
            if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
                dw = torch.empty_like(weight)
                db = _empty((N,), torch.float32, g) if (has_bias and ctx.needs_input_grad[2]) else None
                _t, wp, wb = _scratch(lib.cvae_small_dense_workspace_bytes(M, K, N), g)
                check(L.timed(f"linear_bwd_weight M{M} K{K} N{N} small", lib.cvae_small_dense_bwd_weight, ptr(g), ptr(x), ptr(dw), ptr(db), ya, ac, M, K, N, N, K, N, wp, wb,
                              stream()), "small_dense_bwd_weight")
                if not ctx.needs_input_grad[1]:
                    dw = None
            if ctx.needs_input_grad[0]:
                dx = _empty((M, K), torch.float32, g)
                check(L.timed(f"linear_bwd_data M{M} K{K} N{N} small", lib.cvae_small_dense_bwd_data, ptr(g), ptr(weight.contiguous()), ptr(dx), ya, ac,
                              ptr(x) if in_act is not None else None, L.act_code(in_act) if in_act is not None else L.ACT_NONE, M, K, N, N, K, N, K, stream()),
                      "small_dense_bwd_data")
            return dx, dw, db, None, None, None, None
        fused = act not in (None, "none") and M <= 16          # skinny kernels apply act'(y) on the fly
        if act not in (None, "none") and not fused and not premasked:
            g = _act_bwd(g, y, act)
        ya, ac = (ptr(y), L.act_code(act)) if fused else (None, L.ACT_NONE)
        dx = dw = db = None
        fork = _Fork(g.device)
        with fork:
            if ctx.needs_input_grad[1]:
                dw = torch.empty_like(weight)
                if has_bias and ctx.needs_input_grad[2]:
                    db = _empty((N,), torch.float32, g)
                _t, wp, wb = _scratch(lib.cvae_linear_workspace_bytes(M, K, N, 2), g)
                check(L.timed(f"linear_bwd_weight M{M} K{K} N{N}" + (" bf16" if b16 else ""), lib.cvae_linear_bwd_weight, ptr(g), ptr(x), ptr(dw), ptr(db), M, K, N, N, K,
                              ya, ac, int(b16), wp, wb, stream()), "linear_bwd_weight")
            elif has_bias and ctx.needs_input_grad[2]:
                db = _channel_sum(_act_bwd(g, y, act) if fused else g)
        if ctx.needs_input_grad[0]:
            dx = _empty((M, K), torch.float32, g)
            _t2, wp2, wb2 = _scratch(lib.cvae_linear_workspace_bytes(M, K, N, 1), g)
            check(L.timed(f"linear_bwd_data M{M} K{K} N{N}" + (" bf16" if b16 else ""), lib.cvae_linear_bwd_data, ptr(g), ptr(weight), ptr(dx), M, K, N, N, K, ya, ac,
                          ptr(x) if in_act is not None else None, K, L.act_code(in_act), int(b16), wp2, wb2, stream()), "linear_bwd_data")
        fork.join(dw, db)
        return dx, dw, db, None, None, None, None


class BatchNorm1dTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps):
        L.require_gpu(x)
        x = x.contiguous()
        B, F = x.shape
        y = torch.empty_like(x)
        mean = _empty((F,), torch.float32, x)
        rstd = _empty((F,), torch.float32, x)
        check(lib.cvae_bn1d_train_fwd(ptr(x), ptr(weight), ptr(bias), ptr(y), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var),
                                      B, F, momentum, eps, stream()), "bn1d_train_fwd")
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, mean, rstd = ctx.saved_tensors
        g = g.contiguous()
        B, F = x.shape
        dx = torch.empty_like(x)
        dw = _empty((F,), torch.float32, x)
        db = _empty((F,), torch.float32, x)
        check(lib.cvae_bn1d_train_bwd(ptr(g), ptr(x), ptr(weight), ptr(mean), ptr(rstd), ptr(dx), ptr(dw), ptr(db), B, F, stream()), "bn1d_train_bwd")
        return dx, dw, db, None, None, None, None


def _group_size(group):
    import torch.distributed as dist
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


def _all_reduce_sum(t, group):
    import torch.distributed as dist
    if _group_size(group) > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


class SyncBatchNorm1dTrain(torch.autograd.Function):
    """Train-mode BatchNorm1d whose batch statistics span the data-parallel ranks of `group` (SURVEY.md §8(e) "optional tiny collectives"):
    two all-reduces of F floats forward (sum, then sum of squared deviations: the two-pass form of the single-rank kernel) and one of 2 F
    floats backward.  Every rank must hold the same per-rank batch size.  The weight / bias gradients returned are this rank's PARTIAL sums
    — the gradient all-reduce of the step adds them up, like every other parameter gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, group):
        L.require_gpu(x)
        x = x.contiguous()
        B, F = x.shape
        inv_n = 1.0 / float(B * _group_size(group))
        s1 = _empty((F,), torch.float32, x)
        check(lib.cvae_bn1d_stats(ptr(x), None, 0.0, ptr(s1), B, F, stream()), "bn1d_stats")
        _all_reduce_sum(s1, group)
        s2 = _empty((F,), torch.float32, x)
        check(lib.cvae_bn1d_stats(ptr(x), ptr(s1), inv_n, ptr(s2), B, F, stream()), "bn1d_stats")
        _all_reduce_sum(s2, group)
        y = torch.empty_like(x)
        mean, rstd = _empty((F,), torch.float32, x), _empty((F,), torch.float32, x)
        check(lib.cvae_bn1d_apply_stats(ptr(x), ptr(weight), ptr(bias), ptr(s1), ptr(s2), inv_n, ptr(y), ptr(mean), ptr(rstd), ptr(running_mean),
                                        ptr(running_var), B, F, momentum, eps, stream()), "bn1d_apply_stats")
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.cfg = (inv_n, group)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, mean, rstd = ctx.saved_tensors
        inv_n, group = ctx.cfg
        g = g.contiguous()
        B, F = x.shape
        local = _empty((2 * F,), torch.float32, x)
        check(lib.cvae_bn1d_bwd_sums(ptr(g), ptr(x), ptr(mean), ptr(rstd), ptr(local), B, F, stream()), "bn1d_bwd_sums")
        db, dw = local[:F].clone(), local[F:].clone()           # this rank's share of d beta / d gamma
        _all_reduce_sum(local, group)
        dx = torch.empty_like(x)
        check(lib.cvae_bn1d_bwd_apply(ptr(g), ptr(x), ptr(weight), ptr(mean), ptr(rstd), ptr(local), inv_n, ptr(dx), B, F, stream()), "bn1d_bwd_apply")
        return dx, dw, db, None, None, None, None, None


def bn1d_eval(x, weight, bias, running_mean, running_var, eps):
    L.require_gpu(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    check(lib.cvae_bn1d_eval_fwd(ptr(x), ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var), ptr(y), x.shape[0], x.shape[1], eps, stream()),
          "bn1d_eval_fwd")
    return y


# ------------------------------------------------------------------------------------------------ sampling + losses
def philox_normal(shape, seed, offset, device, call_counter=None, subsequence=0):
    """N(0,1) draws.  call_counter: optional device int32 tensor added (<< 24) to the offset and incremented afterwards —
    the device-side call count that keeps a captured HIP graph drawing fresh numbers on every replay.  subsequence: which of the
    2^64 independent streams of `seed` (Philox counter words 2-3)."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    fn = lib.cvae_philox_normal if call_counter is None else lib.cvae_philox_normal_advance
    check(fn(ptr(out), out.numel(), seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF, subsequence & 0xFFFFFFFFFFFFFFFF, ptr(call_counter), stream()),
          "philox_normal")
    return out


def dist_rank():
    """Rank of this process in the default process group (the torchrun RANK before the group exists, 0 for a single process)."""
    import os
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(os.environ.get("RANK", "0"))


class EpsSource:
    """Per-model device Philox stream for `reparameterize(mu, logvar)` (the reference draws torch.randn_like there).

    Key = torch.initial_seed() (the reference seeds everything with 42, causal_cascade/main.py:28); subsequence = (rank << 32) | instance,
    so the ranks of a data-parallel job — which all call torch.manual_seed(42) — and the models of one process draw independent noise;
    the call counter lives on the device (it advances under HIP-graph replay) and is part of `state()` / `load_state()` so that a resumed
    run continues the stream instead of replaying it (causal_vae_amd.checkpoint)."""
    _instances = 0

    def __init__(self):
        self.counter = None
        self.instance = EpsSource._instances
        EpsSource._instances += 1
        self._pending = None

    def subsequence(self, rank=None):
        return ((dist_rank() if rank is None else int(rank)) << 32) | (self.instance & 0xFFFFFFFF)

    def _ensure(self, device):
        if self.counter is None or self.counter.device != torch.device(device):
            start = 0 if self._pending is None else int(self._pending)
            self.counter = torch.full((), start, dtype=torch.int32, device=device)
            self._pending = None

    def draw(self, like):
        self._ensure(like.device)
        return philox_normal(like.shape, torch.initial_seed(), 0, like.device, self.counter, self.subsequence())

    def noise_args(self, device):
        """(seed, subsequence, device call counter) of the NEXT draw, for a launch that makes the draw itself (ops.BioBottleneck's `noise`): the numbers and
        the counter bump are draw()'s."""
        self._ensure(device)
        return (torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, self.subsequence() & 0xFFFFFFFFFFFFFFFF, self.counter)

    def state(self):
        """{'calls': number of draws so far (one host sync), 'instance': which of the process's streams this model draws from}."""
        return {"calls": int(self.counter.item()) if self.counter is not None else int(self._pending or 0), "instance": int(self.instance)}

    def load_state(self, st):
        calls = int(st["calls"])
        if "instance" in st:                                 # the stream id travels with the checkpoint: construction order in the resuming process
            self.instance = int(st["instance"])              # (a second model, a helper built first) must not change the noise
        if self.counter is not None:
            self.counter.fill_(calls)
        else:
            self._pending = calls


class Reparameterize(torch.autograd.Function):
    """z = mu + eps * exp(logvar / 2) (causal_cascade/models.py:65-68) with an explicit eps."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        L.require_gpu(mu, logvar, eps)
        mu, logvar, eps = mu.contiguous(), logvar.contiguous(), eps.contiguous()
        z = torch.empty_like(mu)
        check(lib.cvae_reparam_kld_fwd(ptr(mu), ptr(logvar), ptr(eps), ptr(z), None, mu.numel(), None, 0, stream()), "reparam_fwd")
        ctx.save_for_backward(mu, logvar, eps)
        return z

    @staticmethod
    def backward(ctx, g):
        mu, logvar, eps = ctx.saved_tensors
        g = g.contiguous()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(mu)
        check(lib.cvae_reparam_kld_bwd(ptr(g), None, 1.0, ptr(mu), ptr(logvar), ptr(eps), ptr(dmu), ptr(dlv), mu.numel(), stream()), "reparam_bwd")
        return dmu, dlv, None


class LatentHead(torch.autograd.Function):
    """(z1, z2, kld) from the encoder's [B, 2 Z] head h = (mu | logvar): z_k = mu + eps_k exp(logvar / 2) (eps2 / z2 optional), kld as ops.KLD — one launch,
    and one for d h in the backward (cvae_latent_head_fwd / _bwd) instead of chunk copies, three kernels, their gradient adds and a cat."""

    @staticmethod
    def forward(ctx, h, eps1, eps2, want_kld):
        L.require_gpu(h, eps1)
        if h.dtype != torch.float32 or h.dim() != 2 or h.shape[1] % 2:
            raise L.CvaeError("LatentHead: fp32 [B, 2 Z] head expected")
        h, eps1 = h.contiguous(), eps1.contiguous()
        B, Z = h.shape[0], h.shape[1] // 2
        if tuple(eps1.shape) != (B, Z) or (eps2 is not None and tuple(eps2.shape) != (B, Z)):
            raise L.CvaeError("LatentHead: eps must be [B, Z]")
        eps2 = None if eps2 is None else eps2.contiguous()
        z1 = _empty((B, Z), torch.float32, h)
        z2 = None if eps2 is None else _empty((B, Z), torch.float32, h)
        kld = torch.empty((), dtype=torch.float32, device=h.device) if want_kld else None
        check(lib.cvae_latent_head_fwd(ptr(h), ptr(eps1), ptr(eps2), ptr(z1), ptr(z2), ptr(kld), B, Z, stream()), "latent_head_fwd")
        ctx.save_for_backward(h, eps1, eps2)
        return z1, z2, kld

    @staticmethod
    def backward(ctx, g1, g2, gk):
        h, eps1, eps2 = ctx.saved_tensors
        B, Z = h.shape[0], h.shape[1] // 2
        dh = torch.empty_like(h)
        g1 = None if g1 is None else g1.contiguous()
        g2 = None if g2 is None else g2.contiguous()
        gk = None if gk is None else gk.float().contiguous()
        check(lib.cvae_latent_head_bwd(ptr(g1), ptr(g2), ptr(gk), ptr(h), ptr(eps1), ptr(eps2), ptr(dh), B, Z, stream()), "latent_head_bwd")
        return dh, None, None, None


class KLD(torch.autograd.Function):
    """-0.5 * sum(1 + logvar - mu^2 - exp(logvar))   (causal_cascade/train.py:13)."""

    @staticmethod
    def forward(ctx, mu, logvar):
        L.require_gpu(mu, logvar)
        mu, logvar = mu.contiguous(), logvar.contiguous()
        out = _scalar(mu)
        _t, wp, wb = _red_ws(mu)
        check(lib.cvae_reparam_kld_fwd(ptr(mu), ptr(logvar), None, None, ptr(out), mu.numel(), wp, wb, stream()), "kld_fwd")
        ctx.save_for_backward(mu, logvar)
        return out

    @staticmethod
    def backward(ctx, g):
        mu, logvar = ctx.saved_tensors
        g = g.contiguous()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(mu)
        check(lib.cvae_reparam_kld_bwd(None, ptr(g), 1.0, ptr(mu), ptr(logvar), None, ptr(dmu), ptr(dlv), mu.numel(), stream()), "kld_bwd")
        return dmu, dlv


class _PairLoss(torch.autograd.Function):
    """sum-reduced elementwise loss of (a, b) with gradient to a only (b is data)."""

    @staticmethod
    def forward(ctx, a, b, kind):
        L.require_gpu(a, b)
        if a.dtype != torch.float32 or b.dtype != torch.float32:
            raise L.CvaeError("loss inputs must be float32")
        a, b = a.contiguous(), b.contiguous()
        if a.shape != b.shape:
            raise RuntimeError(f"The size of tensor a {tuple(a.shape)} must match the size of tensor b {tuple(b.shape)}")
        out = _scalar(a)
        fwd = lib.cvae_sse_fwd if kind == "sse" else lib.cvae_bce_fwd
        _t, wp, wb = _red_ws(a)
        check(fwd(ptr(a), ptr(b), ptr(out), a.numel(), wp, wb, stream()), kind + "_fwd")
        ctx.save_for_backward(a, b)
        ctx.kind = kind
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = torch.empty_like(a)
        if ctx.kind == "sse":
            check(lib.cvae_sse_bwd(ptr(a), ptr(b), ptr(g), 1.0, ptr(da), a.numel(), stream()), "sse_bwd")
        else:
            check(lib.cvae_bce_bwd(ptr(a), ptr(b), ptr(g), ptr(da), a.numel(), stream()), "bce_bwd")
        db = None
        if ctx.kind == "sse" and ctx.needs_input_grad[1]:      # a target that asks (an image on the graph): the same launch with the operands swapped
            db = torch.empty_like(b)
            check(lib.cvae_sse_bwd(ptr(b), ptr(a), ptr(g), 1.0, ptr(db), a.numel(), stream()), "sse_bwd")
        return da, db, None


class Elbo(torch.autograd.Function):
    """loss = SSE(recon_x, x) + gamma * SSE(m_hat, m) + KLD(mu, logvar)   (causal_cascade/train.py:5-17) in one node:
    one zeroed 4-float buffer, three reductions, one combine; the backward scales each branch by the upstream gradient of
    `loss` on the device (no host sync, no scalar torch kernels).  Returns (loss, recon, m_loss, kld)."""

    @staticmethod
    def forward(ctx, recon_x, x, m_hat, m, mu, logvar, gamma):
        L.require_gpu(recon_x, x, m_hat, m, mu, logvar)
        ts = [t.contiguous() for t in (recon_x, x, m_hat, m, mu, logvar)]
        if any(t.dtype != torch.float32 for t in ts):
            raise L.CvaeError("loss inputs must be float32")
        recon_x, x, m_hat, m, mu, logvar = ts
        if recon_x.shape != x.shape or m_hat.shape != m.shape:
            raise RuntimeError(f"The size of tensor a {tuple(recon_x.shape)} must match the size of tensor b {tuple(x.shape)}")
        buf = torch.zeros(4, dtype=torch.float32, device=x.device)
        base = buf.data_ptr()
        _t, wp, wb = _red_ws(x)                               # one scratch block: the three reductions run in stream order
        check(lib.cvae_sse_fwd(ptr(recon_x), ptr(x), base + 4, recon_x.numel(), wp, wb, stream()), "sse_fwd")
        check(lib.cvae_sse_fwd(ptr(m_hat), ptr(m), base + 8, m.numel(), wp, wb, stream()), "sse_fwd")
        check(lib.cvae_reparam_kld_fwd(ptr(mu), ptr(logvar), None, None, base + 12, mu.numel(), wp, wb, stream()), "kld_fwd")
        check(lib.cvae_combine3(base, float(gamma), 1.0, stream()), "combine3")
        ctx.save_for_backward(*ts)
        ctx.gamma = float(gamma)
        ctx.set_materialize_grads(False)
        return buf[0], buf[1], buf[2], buf[3]

    @staticmethod
    def backward(ctx, g_loss, g_recon, g_m, g_kld):
        recon_x, x, m_hat, m, mu, logvar = ctx.saved_tensors
        gam = ctx.gamma
        if g_recon is not None or g_m is not None or g_kld is not None:      # rare: someone back-propagates a single term too
            z = torch.zeros((), dtype=torch.float32, device=x.device)
            gl = g_loss if g_loss is not None else z
            s_r = gl + (g_recon if g_recon is not None else z)
            s_m = gam * gl + (g_m if g_m is not None else z)
            s_k = gl + (g_kld if g_kld is not None else z)
            scales = ((s_r.contiguous(), 1.0), (s_m.contiguous(), 1.0), (s_k.contiguous(), 1.0))
        else:
            if g_loss is None:
                return None, None, None, None, None, None, None
            gl = g_loss.contiguous()
            scales = ((gl, 1.0), (gl, gam), (gl, 1.0))
        d_recon = d_mhat = dmu = dlv = None
        if ctx.needs_input_grad[0]:
            d_recon = torch.empty_like(recon_x)
            check(lib.cvae_sse_bwd(ptr(recon_x), ptr(x), ptr(scales[0][0]), scales[0][1], ptr(d_recon), x.numel(), stream()), "sse_bwd")
        if ctx.needs_input_grad[2]:
            d_mhat = torch.empty_like(m_hat)
            check(lib.cvae_sse_bwd(ptr(m_hat), ptr(m), ptr(scales[1][0]), scales[1][1], ptr(d_mhat), m.numel(), stream()), "sse_bwd")
        if ctx.needs_input_grad[4] or ctx.needs_input_grad[5]:
            dmu, dlv = torch.empty_like(mu), torch.empty_like(mu)
            check(lib.cvae_reparam_kld_bwd(None, ptr(scales[2][0]), scales[2][1], ptr(mu), ptr(logvar), None, ptr(dmu), ptr(dlv), mu.numel(), stream()), "kld_bwd")
        return d_recon, None, d_mhat, None, dmu, dlv, None


class ElboUp2x(torch.autograd.Function):
    """The same ELBO with the exact-2x resize of the decoder output folded in: recon = SSE(F.interpolate(src, size(x)), x) without
    ever writing the resized volume (csrc/recon_loss.hip).  src: channels-last decoder output [B, d, h, w, 1] (conv dtype);
    x: [B, 1, D, H, W] / [B, 1, H, W] fp32 with D = 2d (3D), H = 2h, W = 2w.  Returns (loss, recon, m_loss, kld)."""

    @staticmethod
    def dims(src, x):
        B, d, h, w, Cc = _cl_dims(src)
        sp = tuple(x.shape[2:])
        D, H, W = sp if len(sp) == 3 else (1,) + sp
        return B, d, h, w, Cc, D, H, W

    @staticmethod
    def supported(src, x):
        B, d, h, w, Cc, D, H, W = ElboUp2x.dims(src, x)
        return (Cc == 1 and x.shape[0] == B and x.shape[1] == 1 and x.dtype == torch.float32 and bool(lib.cvae_up2x_supported(B, d, h, w, D, H, W)))

    _tickets = {}                  # device -> the zero-initialised arrival word of the in-launch finish (the kernel leaves it zero)
    IN_LAUNCH_FINISH = __import__("os").environ.get("CVAE_ELBO_TWO_LAUNCH") != "1"        # False: the two-launch form (tests compare the two bit for bit; the env switch is for A/B runs)

    @staticmethod
    def forward(ctx, src, x, m_hat, m, mu, logvar, gamma, bump=None):
        """bump: optional device int32 tensor incremented by the launch (the optimizer's device step counter, FusedAdam.claim_step_counter)."""
        L.require_gpu(src, x, m_hat, m, mu, logvar)
        src = src.contiguous()
        x, m_hat, m, mu, logvar = (t.contiguous().float() for t in (x, m_hat, m, mu, logvar))
        if m_hat.shape != m.shape or mu.shape != logvar.shape:
            raise RuntimeError(f"The size of tensor a {tuple(m_hat.shape)} must match the size of tensor b {tuple(m.shape)}")
        B, d, h, w, Cc, D, H, W = ElboUp2x.dims(src, x)
        buf = torch.empty(4 + lib.cvae_elbo_up2x_partials(B, d, h, w), dtype=torch.float32, device=x.device)
        # a backward will follow: the forward launch also leaves t1 = U_w^T (up(src) - x), so the step reads x (33.5 MB at 128^3, B = 4) once
        t1 = torch.empty(B * D * H * w, dtype=torch.float32, device=x.device) if any(ctx.needs_input_grad[i] for i in (0, 2, 4, 5)) else None
        ticket = None
        if ElboUp2x.IN_LAUNCH_FINISH:
            ticket = ElboUp2x._tickets.get(x.device)
            if ticket is None:
                ticket = ElboUp2x._tickets[x.device] = torch.zeros(33 * 32, dtype=torch.int32, device=x.device)      # CVAE_ELBO_TICKET_WORDS
        check(lib.cvae_elbo_up2x_fwd(ptr(src), ptr(x), ptr(m_hat), ptr(m), ptr(mu), ptr(logvar), float(gamma), ptr(buf), buf.data_ptr() + 16, ptr(t1), ptr(ticket),
                                     ptr(bump) if ticket is not None else None, B, d, h, w, D, H, W, m.numel(), mu.numel(), L.dtype_code(src.dtype), stream()), "elbo_up2x_fwd")
        if bump is not None and ticket is None:
            check(lib.cvae_counter_add(ptr(bump), 1, stream()), "counter_add")
        ctx.save_for_backward(src, x, m_hat, m, mu, logvar, t1)
        ctx.gamma = float(gamma)
        ctx.set_materialize_grads(False)
        return buf[0], buf[1], buf[2], buf[3]

    @staticmethod
    def backward(ctx, g_loss, g_recon, g_m, g_kld):
        src, x, m_hat, m, mu, logvar, t1 = ctx.saved_tensors
        if g_recon is not None or g_m is not None or g_kld is not None:
            raise L.CvaeError("ElboUp2x back-propagates the total loss only; for a single term use loss_function on the model's recon_x")
        if g_loss is None:
            return None, None, None, None, None, None, None, None
        B, d, h, w, Cc, D, H, W = ElboUp2x.dims(src, x)
        dsrc, d_mhat, dmu, dlv = torch.empty_like(src), torch.empty_like(m_hat), torch.empty_like(mu), torch.empty_like(mu)
        check(lib.cvae_elbo_up2x_bwd(ptr(t1), ptr(m_hat), ptr(m), ptr(mu), ptr(logvar), ctx.gamma, ptr(g_loss.contiguous()), ptr(dsrc),
                                     ptr(d_mhat), ptr(dmu), ptr(dlv), B, d, h, w, D, H, W, m.numel(), mu.numel(), L.dtype_code(src.dtype), stream()), "elbo_up2x_bwd")
        return dsrc, None, d_mhat, None, dmu, dlv, None, None


class WeightedSum(torch.autograd.Function):
    """sum_i w_i * t_i of 0-dim device tensors as one launch (and one for all the gradients): a loss composed of several terms.
    Returns (total, weighted terms [n]); only the total carries a gradient (the weighted terms are what a training loop logs)."""

    @staticmethod
    def forward(ctx, weights, *terms):
        import ctypes as C
        L.require_gpu(*terms)
        n = len(terms)
        if not 1 <= n <= 8 or len(weights) != n:
            raise L.CvaeError("WeightedSum: 1..8 terms, one weight each")
        ts = [t.float().contiguous() for t in terms]
        if any(t.numel() != 1 for t in ts):
            raise L.CvaeError("WeightedSum: scalar (0-dim) terms expected")
        out = torch.empty(n + 1, dtype=torch.float32, device=ts[0].device)
        check(lib.cvae_weighted_sum((C.c_void_p * n)(*[t.data_ptr() for t in ts]), (C.c_float * n)(*[float(w) for w in weights]), n, None, ptr(out), 0, stream()), "weighted_sum")
        ctx.weights = [float(w) for w in weights]
        ctx.shapes = [t.shape for t in terms]
        total, parts = out[0], out[1:]
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)                     # no zeros launch for the gradient slot of `parts`
        return total, parts

    @staticmethod
    def backward(ctx, g, _gparts):
        if g is None:
            return (None,) * (1 + len(ctx.weights))
        import ctypes as C
        n = len(ctx.weights)
        out = torch.empty(n, dtype=torch.float32, device=g.device)
        check(lib.cvae_weighted_sum(None, (C.c_float * n)(*ctx.weights), n, ptr(g.float().contiguous()), ptr(out), 1, stream()), "weighted_sum_bwd")
        return (None,) + tuple(out[i].view(ctx.shapes[i]) for i in range(n))


def weighted_sum(terms, weights, return_terms=False):
    """sum_i weights[i] * terms[i]; with return_terms also the n weighted terms (a [n] tensor, no gradient)."""
    total, parts = WeightedSum.apply(tuple(weights), *terms)
    return (total, parts) if return_terms else total


def sse(a, b):
    """F.mse_loss(a, b, reduction='sum') (gradient flows to a)."""
    return _PairLoss.apply(a, b, "sse")


def bce_sum(p, x):
    """F.binary_cross_entropy(p, x, reduction='sum')."""
    return _PairLoss.apply(p, x, "bce")


class VesselRecon(torch.autograd.Function):
    """(recon_loss, sparsity_loss) of vessel_analysis/01_train/train.py:27-46 (pos-weighted MSE-sum, background L1).
    group / sync: under data parallelism pos_weight is a BATCH-GLOBAL scalar in the reference (:30-36); sync=True all-reduces (sum x) over
    `group` and uses the global element count, so every rank weights with the pos_weight of the whole batch (one 4-byte message)."""

    @staticmethod
    def forward(ctx, r, x, sync=False, group=None):
        L.require_gpu(r, x)
        r, x = r.contiguous(), x.contiguous()
        sx = _scalar(r)
        out2 = torch.zeros(2, dtype=torch.float32, device=r.device)
        _t, wp, wb = _red_ws(r)
        check(lib.cvae_sum_fwd(ptr(x), ptr(sx), x.numel(), wp, wb, stream()), "sum_fwd")
        n_pos = x.numel()
        if sync and _group_size(group) > 1:
            _all_reduce_sum(sx, group)
            n_pos *= _group_size(group)
        check(lib.cvae_wmse_sparsity_fwd(ptr(r), ptr(x), ptr(sx), ptr(out2), r.numel(), n_pos, wp, wb, stream()), "wmse_sparsity_fwd")
        ctx.save_for_backward(r, x, sx)
        ctx.n_pos = n_pos
        return out2[0], out2[1]

    @staticmethod
    def backward(ctx, g_recon, g_sp):
        r, x, sx = ctx.saved_tensors
        dr = torch.empty_like(r)
        g_recon = g_recon.contiguous() if g_recon is not None else None
        g_sp = g_sp.contiguous() if g_sp is not None else None
        check(lib.cvae_wmse_sparsity_bwd(ptr(r), ptr(x), ptr(sx), ptr(g_recon), ptr(g_sp), ptr(dr), r.numel(), ctx.n_pos, stream()), "wmse_sparsity_bwd")
        return dr, None, None, None


class GaussNLL(torch.autograd.Function):
    """0.5 * sum(logvar + (m - mu)^2 / exp(logvar))   (vessel_analysis/01_train/train.py:56-58)."""

    @staticmethod
    def forward(ctx, m, mu, logvar):
        L.require_gpu(m, mu, logvar)
        m, mu, logvar = m.contiguous(), mu.contiguous(), logvar.contiguous()
        out = _scalar(m)
        _t, wp, wb = _red_ws(m)
        check(lib.cvae_gauss_nll_fwd(ptr(m), ptr(mu), ptr(logvar), ptr(out), m.numel(), wp, wb, stream()), "gauss_nll_fwd")
        ctx.save_for_backward(m, mu, logvar)
        return out

    @staticmethod
    def backward(ctx, g):
        m, mu, logvar = ctx.saved_tensors
        g = g.contiguous()
        dmu, dlv = torch.empty_like(mu), torch.empty_like(mu)
        check(lib.cvae_gauss_nll_bwd(ptr(m), ptr(mu), ptr(logvar), ptr(g), ptr(dmu), ptr(dlv), m.numel(), stream()), "gauss_nll_bwd")
        return None, dmu, dlv


class SoftmaxCE(torch.autograd.Function):
    """F.cross_entropy(logits, target) with mean reduction (mnist_test/01_baseline_causal_vae/train.py:56)."""

    @staticmethod
    def forward(ctx, logits, target):
        L.require_gpu(logits, target)
        logits, target = logits.contiguous(), target.contiguous()
        out = _scalar(logits)
        _t, wp, wb = _red_ws(logits)
        check(lib.cvae_softmax_ce_fwd(ptr(logits), ptr(target), ptr(out), logits.shape[0], logits.shape[1], wp, wb, stream()), "softmax_ce_fwd")
        ctx.save_for_backward(logits, target)
        return out

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved_tensors
        g = g.contiguous()
        dl = torch.empty_like(logits)
        check(lib.cvae_softmax_ce_bwd(ptr(logits), ptr(target), ptr(g), ptr(dl), logits.shape[0], logits.shape[1], stream()), "softmax_ce_bwd")
        return dl, None


class UniformKL(torch.autograd.Function):
    """F.kl_div(F.log_softmax(logits, 1), full(1/C), reduction='batchmean') (mnist_test/01_baseline_causal_vae/train.py:82-85)."""

    @staticmethod
    def forward(ctx, logits):
        L.require_gpu(logits)
        logits = logits.contiguous()
        out = _scalar(logits)
        _t, wp, wb = _red_ws(logits)
        check(lib.cvae_uniform_kl_fwd(ptr(logits), ptr(out), logits.shape[0], logits.shape[1], wp, wb, stream()), "uniform_kl_fwd")
        ctx.save_for_backward(logits)
        return out

    @staticmethod
    def backward(ctx, g):
        (logits,) = ctx.saved_tensors
        g = g.contiguous()
        dl = torch.empty_like(logits)
        check(lib.cvae_uniform_kl_bwd(ptr(logits), ptr(g), ptr(dl), logits.shape[0], logits.shape[1], stream()), "uniform_kl_bwd")
        return dl


# ------------------------------------------------------------------------------------------------ fused bottleneck
class BioBottleneck(torch.autograd.Function):
    """Everything between CausalBioVAE's last encoder conv and first decoder conv as 5 + 5 launches (csrc/bottleneck.hip):
    pool + flatten + cat, enc_fc, fc_mu / fc_logvar, reparameterize, mechanism_net (train-mode BatchNorm1d), cat, dec_input.

    inputs : y_cl [B, D, H, W, C] (last encoder activation, a ReLU output), m [B, m_dim], t_onehot [B, t_dim] (or the int64 labels [B]), eps [B, Z],
             the 18 parameters in _lib.BOTTLENECK_PARAMS order, then (running_mean, running_var, num_batches_tracked, momentum,
             bn_eps, out_size).  returns (mu, logvar, m_hat, dec_cl [B, OD, OH, OW, C] in y_cl's dtype).
    Same arithmetic (fp32) as the layer-by-layer path, which stays the general fallback (eval mode, B > 16, odd pool windows).
    An optional last argument `sync` = (group, rank_stats) makes mechanism_net's BatchNorm1d a SyncBatchNorm over the ranks of `group`:
    rank_stats is bottleneck_bn_rank_stats(...) (this step's gathered per-rank statistics); the backward all-reduces 2 * HM floats and finishes
    mechanism_net.0's gradients in one extra small launch (include/cvae_hip.h, cvae_bottleneck_*_sync).  A further optional argument
    `noise` = EpsSource.noise_args(device) makes `eps` an output of the first launch (the draw of EpsSource.draw without its launch).
    """

    @staticmethod
    def supported(y_cl, out_size, training, widths=None):
        """widths (optional) = (m_dim, t_dim, N1, N2, Z, HM): also ask the library (cvae_bottleneck_sizes), which refuses widths whose level
        launches would not fit in a workgroup's LDS at this batch (include/cvae_hip.h).  Without it only the batch, channels and windows are checked."""
        B, D, H, W, C = y_cl.shape
        OD, OH, OW = out_size
        ok = training and 2 <= B <= 16 and C % 64 == 0 and D % OD == 0 and H % OH == 0 and W % OW == 0
        if ok and widths is not None:
            dims = L.BottleneckDims(B, D, H, W, C, OD, OH, OW, *widths)
            ok = lib.cvae_bottleneck_sizes(C_.byref(dims), None, None, None, None, None) == 0
        return ok

    @staticmethod
    def forward(ctx, y_cl, m, t_onehot, eps, *rest):
        params, (rm, rv, nbt, momentum, bn_eps, out_size), sync = rest[:18], rest[18:24], (rest[24] if len(rest) > 24 else None)
        noise = rest[25] if len(rest) > 25 else None
        ctx.n_extra = len(rest) - 18
        L.require_gpu(y_cl, m, t_onehot, eps, *params)
        params = [p.contiguous() for p in params]
        W1, W2, Wmu, Wm0 = params[0], params[2], params[4], params[8]
        t_labels = None
        if t_onehot.dim() == 1 and not t_onehot.is_floating_point():           # class indices: the one-hot is written by the first launch
            t_labels = t_onehot.contiguous().long()
            t_onehot = torch.empty(t_labels.shape[0], Wm0.shape[1], dtype=torch.float32, device=y_cl.device)
        y_cl, m, t_onehot, eps = y_cl.contiguous(), m.contiguous().float(), t_onehot.contiguous().float(), eps.contiguous().float()
        B, D, H, W, C = y_cl.shape
        dims = L.BottleneckDims(B, D, H, W, C, *out_size, m.shape[1], t_onehot.shape[1], W1.shape[0], W2.shape[0], Wmu.shape[0], Wm0.shape[0])
        sizes = [C_.c_int64() for _ in range(5)]
        check(lib.cvae_bottleneck_sizes(C_.byref(dims), *[C_.byref(v) for v in sizes]), "bottleneck_sizes")
        K1, K4, n_fwd, n_dzm, n_dx = (v.value for v in sizes)
        if W1.shape[1] != K1 or params[16].shape != (C * out_size[0] * out_size[1] * out_size[2], K4):
            raise L.CvaeError(f"BioBottleneck: enc_fc.0 expects {W1.shape[1]} inputs, the pooled features + m + t give {K1}")
        dev, f32 = y_cl.device, torch.float32
        new = lambda *shape: torch.empty(*shape, dtype=f32, device=dev)
        xcat, partial, dzm_acc = new(B, K1), new(n_fwd), new(n_dzm)
        N1, N2, Z, HM, DM = dims.N1, dims.N2, dims.Z, dims.HM, dims.m_dim
        saved = dict(h1=new(B, N1), h2=new(B, N2), mu=new(B, Z), logvar=new(B, Z), xhat=new(B, HM), invstd=new(HM), a1n=new(B, HM), a2=new(B, HM),
                     m_hat=new(B, DM), zm=new(B, K4))
        dec_cl = torch.empty(B, *out_size, C, dtype=y_cl.dtype, device=dev)
        pstruct = L.BottleneckPtrs18(*[ptr(p) for p in params])
        sstruct = L.BottleneckSaved(*[ptr(saved[k]) for k in L.BOTTLENECK_SAVED])
        rank_stats, ranks = None, 0
        if sync is not None:
            rank_stats = sync[1].contiguous()
            ranks = rank_stats.shape[0]
            if tuple(rank_stats.shape) != (ranks, 2, HM) or rank_stats.dtype != f32:
                raise L.CvaeError(f"BioBottleneck: sync rank_stats must be float32 [ranks, 2, {HM}], got {tuple(rank_stats.shape)}")
        nstruct = None
        if noise is not None:
            if noise[2].dtype != torch.int32 or noise[2].device != dev:
                raise L.CvaeError("BioBottleneck: the noise call counter must be an int32 tensor on the activations' device")
            nstruct = C_.byref(L.BottleneckNoise(int(noise[0]), int(noise[1]), ptr(noise[2])))
        check(lib.cvae_bottleneck_fwd(C_.byref(dims), C_.byref(pstruct), ptr(y_cl), ptr(m), ptr(t_onehot), ptr(t_labels), ptr(eps), ptr(rm), ptr(rv), ptr(nbt), float(momentum),
                                      float(bn_eps), 1, ptr(xcat), ptr(partial), ptr(dzm_acc), C_.byref(sstruct), ptr(dec_cl), L.dtype_code(y_cl.dtype), ptr(rank_stats), ranks,
                                      nstruct, stream()), "bottleneck_fwd")
        ctx.dims, ctx.scratch = dims, n_dx
        ctx.sync = None if sync is None else (sync[0], ranks)
        ctx.save_for_backward(y_cl, t_onehot, eps, xcat, *params, *[saved[k] for k in L.BOTTLENECK_SAVED], dzm_acc)
        ctx.mark_non_differentiable(*[t for t in (rm, rv, nbt) if t is not None])
        return saved["mu"], saved["logvar"], saved["m_hat"], dec_cl

    @staticmethod
    def backward(ctx, g_mu, g_logvar, g_mhat, g_dec):
        y_cl, t_onehot, eps, xcat = ctx.saved_tensors[:4]
        params, saved, dzm_part = ctx.saved_tensors[4:22], ctx.saved_tensors[22:-1], ctx.saved_tensors[-1]
        dims, n_dx = ctx.dims, ctx.scratch
        dev, f32 = y_cl.device, torch.float32
        if g_dec is None:
            g_dec = torch.zeros(dims.M, dims.OD, dims.OH, dims.OW, dims.C, dtype=y_cl.dtype, device=dev)
        fix = lambda g: None if g is None else g.contiguous().float()
        g_mu, g_logvar, g_mhat, g_dec = fix(g_mu), fix(g_logvar), fix(g_mhat), g_dec.contiguous()
        grads = [torch.empty_like(p) for p in params]
        g1, dx_part = (torch.empty(n, dtype=f32, device=dev) for n in (dims.M * (dims.N1 + dims.N2), n_dx))
        dy_cl = torch.empty_like(y_cl)
        pstruct = L.BottleneckPtrs18(*[ptr(p) for p in params])
        gstruct = L.BottleneckPtrs18(*[ptr(g) for g in grads])
        sstruct = L.BottleneckSaved(*[ptr(t) for t in saved])
        bn_dy = bn_sums = None
        if ctx.sync is not None:
            bn_dy, bn_sums = torch.empty(dims.M, dims.HM, dtype=f32, device=dev), torch.empty(2, dims.HM, dtype=f32, device=dev)
        check(lib.cvae_bottleneck_bwd(C_.byref(dims), C_.byref(pstruct), C_.byref(gstruct), C_.byref(sstruct), ptr(g_dec), ptr(g_mu), ptr(g_logvar), ptr(g_mhat),
                                      ptr(t_onehot), ptr(eps), ptr(xcat), ptr(y_cl), 1, ptr(dzm_part), ptr(g1), ptr(dx_part), ptr(dy_cl),
                                      L.dtype_code(y_cl.dtype), ptr(bn_dy), ptr(bn_sums), stream()), "bottleneck_bwd")
        if ctx.sync is not None:
            group, ranks = ctx.sync
            _all_reduce_sum(bn_sums, group)                  # 2 * HM floats: sum(dy), sum(dy * xhat) over the global batch
            check(lib.cvae_bottleneck_bn_bwd_finish(C_.byref(dims), C_.byref(pstruct), C_.byref(gstruct), C_.byref(sstruct), ptr(t_onehot), ptr(bn_dy), ptr(bn_sums), ranks,
                                                    stream()), "bottleneck_bn_bwd_finish")
        return (dy_cl, None, None, None, *grads, *([None] * ctx.n_extra))


def bottleneck_bn_rank_stats(Wm0, bm0, t, group=None):
    """Per-rank statistics of mechanism_net.0's output for the SyncBatchNorm form of BioBottleneck: float32 [ranks, 2, HM] = every rank's (sum, squared
    deviations from its own mean) over its B samples — one small launch and one all-gather of 2 * HM floats.  The layer's input is t alone, so this runs at the
    top of the step, before the encoder.  t: int64 labels [B] or the float one-hot [B, t_dim].  Every rank must hold the same B."""
    import torch.distributed as dist
    L.require_gpu(Wm0, bm0, t)
    Wm0, bm0 = Wm0.contiguous(), bm0.contiguous()
    HM, T = Wm0.shape
    labels = t.contiguous().long() if (t.dim() == 1 and not t.is_floating_point()) else None
    onehot = None if labels is not None else t.contiguous().float()
    B = t.shape[0]
    local = torch.empty(2, HM, dtype=torch.float32, device=Wm0.device)
    check(lib.cvae_bottleneck_bn_local_stats(ptr(Wm0), ptr(bm0), ptr(onehot), ptr(labels), ptr(local), B, T, HM, stream()), "bottleneck_bn_local_stats")
    world = _group_size(group)
    if world == 1:
        return local.unsqueeze(0)
    parts = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(parts, local, group=group)
    return torch.stack(parts)


# ------------------------------------------------------------------------------------------------ CausalVesselVAE extras
class BatchNorm2dAct(torch.autograd.Function):
    """nn.BatchNorm2d (+ the activation that follows it) on a channels-last tensor [B, D, H, W, C] (csrc/vessel2d.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, training, act):
        L.require_gpu(x, weight, bias)
        x = x.contiguous()
        Cc = x.shape[-1]
        P = x.numel() // Cc
        y = torch.empty_like(x)
        if training:
            mean, rstd = _empty((Cc,), torch.float32, x), _empty((Cc,), torch.float32, x)
        else:
            mean, rstd = running_mean.float().clone(), torch.rsqrt(running_var.float() + eps)
        _t, wp, wb = _scratch(lib.cvae_bn2d_workspace_bytes(P, Cc) if training else 0, x)
        check(lib.cvae_bn2d_fwd(ptr(x), ptr(weight), ptr(bias), ptr(y), ptr(mean), ptr(rstd), ptr(running_mean) if training else None,
                                ptr(running_var) if training else None, P, Cc, float(momentum), float(eps), 1 if training else 0, L.act_code(act),
                                L.dtype_code(x.dtype), wp, wb, stream()), "bn2d_fwd")
        ctx.save_for_backward(x, y, weight, mean, rstd)
        ctx.cfg = (training, act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y, weight, mean, rstd = ctx.saved_tensors
        training, act = ctx.cfg
        if not training:
            raise L.CvaeError("BatchNorm2d in eval mode is forward-only here (the reference consumers run it under no_grad)")
        Cc = x.shape[-1]
        P = x.numel() // Cc
        g = g.contiguous()
        dx = torch.empty_like(x)
        dw, db = _empty((Cc,), torch.float32, x), _empty((Cc,), torch.float32, x)
        _t, wp, wb = _scratch(lib.cvae_bn2d_workspace_bytes(P, Cc), x)
        check(lib.cvae_bn2d_bwd(ptr(x), ptr(g), ptr(y), ptr(weight), ptr(mean), ptr(rstd), ptr(dx), ptr(dw), ptr(db), P, Cc, L.act_code(act),
                                L.dtype_code(x.dtype), wp, wb, stream()), "bn2d_bwd")
        return dx, dw, db, None, None, None, None, None, None


def _bn2d_rows(what, t, **like):
    """(P, C) of the channels-last tensor t as the BatchNorm2d entries address it; every tensor of `like` has t's shape, dtype and device."""
    if t.dim() < 2 or not t.is_contiguous() or t.dtype not in (torch.float32, torch.bfloat16) or t.shape[-1] % 8 or t.numel() == 0:
        raise L.CvaeError(f"{what}: a contiguous channels-last [.., C] fp32 or bf16 tensor with C % 8 == 0 expected, got {tuple(t.shape)} {t.dtype}")
    for k, v in like.items():
        if tuple(v.shape) != tuple(t.shape) or v.dtype != t.dtype or v.device != t.device or not v.is_contiguous():
            raise L.CvaeError(f"{what}: {k} must be a contiguous {tuple(t.shape)} {t.dtype} tensor on {t.device}, got {tuple(v.shape)} {v.dtype} on {v.device}")
    return t.numel() // t.shape[-1], t.shape[-1]


def _bn2d_bwd_prepare(what, y, g, a, weight, mean, rstd, act, a_optional=False):
    """What bn2d_bwd and bn2d_batch_bwd (`what`, for the messages) share: the argument checks -> (P, C, whether `a` is read, g_y, dgamma, dbeta), the three
    outputs unwritten.  a_optional: `a` is read behind an activation only, and may be None without one."""
    reads_a = not a_optional or act not in (None, "none")
    L.require_gpu(y, g, a, weight, mean, rstd)
    _forward_only(what, y, g, a, weight, mean, rstd)
    if a_optional and reads_a and a is None:
        raise L.CvaeError(f"{what}: the activation's output `a` is needed for act={act!r}")
    P, Cc = _bn2d_rows(what, y, g=g, **({"a": a} if reads_a else {}))
    for k, v in (("weight", weight), ("mean", mean), ("rstd", rstd)):
        if tuple(v.shape) != (Cc,) or v.dtype != torch.float32 or not v.is_contiguous():
            raise L.CvaeError(f"{what}: {k} must be a contiguous fp32 [{Cc}] vector, got {tuple(v.shape)} {v.dtype}")
    return P, Cc, reads_a, torch.empty_like(y), _empty((Cc,), torch.float32, y), _empty((Cc,), torch.float32, y)


def bn2d_batch_bwd(y, g, a, weight, mean, rstd, act):
    """bn2d_bwd's function on the forward's chunking (cvae_bn2d_batch_bwd, csrc/bn2d_batch.hip): (g_y, dgamma, dbeta) of
    a = act((y - mean) rstd weight + bias) with batch statistics, in three launches that read y, g and a twice and add their partial sums in a fixed order of
    16 runs per channel.  a may be None when act is None (it is then not read): the BatchNorm that ends a ResBlock, whose output carries the residual."""
    P, Cc, gated, gy, dw, db = _bn2d_bwd_prepare("bn2d_batch_bwd", y, g, a, weight, mean, rstd, act, a_optional=True)
    _t, wp, wb = _scratch(lib.cvae_bn2d_batch_bwd_workspace_bytes(P, Cc), y)
    check(L.timed(f"bn2d_batch_bwd P{P} C{Cc}", lib.cvae_bn2d_batch_bwd, ptr(y), ptr(g), ptr(a) if gated else None, ptr(weight), ptr(mean), ptr(rstd), ptr(gy),
                  ptr(dw), ptr(db), P, Cc, L.act_code(act), L.dtype_code(y.dtype), wp, wb, stream()), "bn2d_batch_bwd")
    return gy, dw, db


def bn2d_batch_fwd(y, bn, act, resid=None):
    """(a, mean, rstd) = nn.BatchNorm2d `bn` on the statistics of THIS batch, then the activation `act` (None / "relu" / "sigmoid" / "leaky02" / "leaky001"), on
    the channels-last conv output y [.., C] (fp32 or bf16): cvae_bn2d_batch_fwd (csrc/bn2d_batch.hip), which reads y twice.  a has y's shape and dtype;
    mean and rstd (fp32 [C]: the batch mean and 1 / sqrt(biased variance + eps)) are what bn2d_bwd reads.  With bn.track_running_stats its running_mean and
    running_var are updated in place as torch does in training mode (momentum, unbiased variance) and num_batches_tracked advances by one with an in-place device
    add, so a captured step replays it.  The module's own mode is not consulted and not changed.  momentum=None (torch's cumulative average): CvaeError.
    resid (y's shape and dtype, with act None only): a = resid + bn(y), summed in fp32 and rounded once (cvae_bn2d_batch_fwd_res) — the
    BatchNorm that ends a ResBlock."""
    L.require_gpu(y, bn.weight, bn.bias)
    _forward_only("bn2d_batch_fwd", y, bn.weight, bn.bias, resid)
    P, Cc = _bn2d_rows("bn2d_batch_fwd", y) if resid is None else _bn2d_rows("bn2d_batch_fwd", y, resid=resid)
    if resid is not None and act not in (None, "none"):
        raise L.CvaeError(f"bn2d_batch_fwd: a residual goes with no activation (behind one, `a` would not carry the sign the backward reads), got act={act!r}")
    if bn.weight is None or bn.bias is None or bn.num_features != Cc or bn.weight.dtype != torch.float32:
        raise L.CvaeError(f"bn2d_batch_fwd: an affine fp32 BatchNorm2d over {Cc} channels expected, got num_features={bn.num_features}, affine={bn.weight is not None}")
    if bn.momentum is None:
        raise L.CvaeError("bn2d_batch_fwd: momentum=None (the cumulative moving average) is not implemented; give the BatchNorm2d a momentum in [0, 1]")
    track = bool(bn.track_running_stats) and bn.running_mean is not None
    if track and (bn.running_mean.dtype != torch.float32 or bn.running_var.dtype != torch.float32):
        raise L.CvaeError("bn2d_batch_fwd: fp32 running statistics expected")
    a = torch.empty_like(y)
    mean, rstd = _empty((Cc,), torch.float32, y), _empty((Cc,), torch.float32, y)
    _t, wp, wb = _scratch(lib.cvae_bn2d_batch_workspace_bytes(P, Cc), y)
    args = (ptr(y), ptr(bn.weight), ptr(bn.bias), ptr(a), ptr(mean), ptr(rstd), ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None,
            P, Cc, float(bn.momentum), float(bn.eps), L.act_code(act), L.dtype_code(y.dtype), wp, wb, stream())
    if resid is None:
        check(L.timed(f"bn2d_batch_fwd P{P} C{Cc}", lib.cvae_bn2d_batch_fwd, *args), "bn2d_batch_fwd")
    else:
        check(L.timed(f"bn2d_batch_fwd_res P{P} C{Cc}", lib.cvae_bn2d_batch_fwd_res, *args, ptr(resid)), "bn2d_batch_fwd_res")
    if track and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return a, mean, rstd


def bn2d_bwd(y, g, a, weight, mean, rstd, act):
    """(g_y, dgamma, dbeta) of a = act((y - mean) rstd weight + bias) with batch statistics (cvae_bn2d_bwd, csrc/vessel2d.hip): y the normalisation's input, g the
    gradient of a, a the forward's output (for act'), mean / rstd as bn2d_batch_fwd (or BatchNorm2dAct's training forward) left them."""
    P, Cc, _reads_a, gy, dw, db = _bn2d_bwd_prepare("bn2d_bwd", y, g, a, weight, mean, rstd, act)
    _t, wp, wb = _scratch(lib.cvae_bn2d_workspace_bytes(P, Cc), y)
    check(L.timed(f"bn2d_bwd P{P} C{Cc}", lib.cvae_bn2d_bwd, ptr(y), ptr(g), ptr(a), ptr(weight), ptr(mean), ptr(rstd), ptr(gy), ptr(dw), ptr(db), P, Cc,
                  L.act_code(act), L.dtype_code(y.dtype), wp, wb, stream()), "bn2d_bwd")
    return gy, dw, db


class Clamp(torch.autograd.Function):
    """torch.clamp(x, min, max) with its pass-through gradient mask (vessel_analysis/00_core/models.py:148-149,156)."""

    @staticmethod
    def forward(ctx, x, lo, hi):
        L.require_gpu(x)
        x = x.contiguous().float()
        y = torch.empty_like(x)
        check(lib.cvae_clamp_fwd(ptr(x), ptr(y), float(lo), float(hi), x.numel(), stream()), "clamp_fwd")
        ctx.save_for_backward(x)
        ctx.lim = (float(lo), float(hi))
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(lib.cvae_clamp_bwd(ptr(x), ptr(g), ptr(dx), ctx.lim[0], ctx.lim[1], x.numel(), stream()), "clamp_bwd")
        return dx, None, None


class Conv3ToK4(torch.autograd.Function):
    """Weight of nn.Conv2d(Cin, Cout, 3, 1, 1) applied after a nearest x2 upsample -> the equivalent transposed k4/s2/p1 weight
    [Cin][Cout][4][4] for ConvUp (K4 = A W3 A^T, csrc/vessel2d.hip); the backward maps dK4 to dW3."""

    @staticmethod
    def forward(ctx, w3):
        L.require_gpu(w3)
        w3 = w3.contiguous()
        Cout, Cin = w3.shape[0], w3.shape[1]
        if tuple(w3.shape[2:]) != (3, 3):
            raise L.CvaeError("Conv3ToK4: a [Cout, Cin, 3, 3] weight expected")
        k4 = torch.empty(Cin, Cout, 4, 4, dtype=torch.float32, device=w3.device)
        check(lib.cvae_conv3_to_k4(ptr(w3), ptr(k4), Cout, Cin, stream()), "conv3_to_k4")
        ctx.shape = (Cout, Cin)
        return k4

    @staticmethod
    def backward(ctx, g):
        Cout, Cin = ctx.shape
        g = g.contiguous()
        dw3 = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=g.device)
        check(lib.cvae_k4_to_conv3_grad(ptr(g), ptr(dw3), Cout, Cin, stream()), "k4_to_conv3_grad")
        return dw3


# ------------------------------------------------------------------------------------------------ CausalVesselVAE inference (csrc/vessel_infer.hip)
# Forward-only helpers of the eval-mode decode and the analysis sweeps: they enqueue their kernels and return plain tensors; asked for a gradient
# they raise (the reference consumers run them under no_grad).
FOLD_CONV_K4, FOLD_UPCONV_K3, FOLD_CONV_K3S2 = 0, 1, 3        # CVAE_FOLD_CONV_K4 / CVAE_FOLD_UPCONV_K3 / CVAE_FOLD_CONV_K3S2
FOLD_CONVT_K3S2, FOLD_CONV_K3S1, FOLD_CONVT_K3S2_SUBPIXEL = 4, 5, 6      # the ViT-VAE decoder's kinds (CVAE_FOLD_CONVT_K3S2 / _CONV_K3S1 / _CONVT_K3S2_SUBPIXEL)
FOLD_CONV_K3S1_GRAD, FOLD_CONVT_K3S2_SUBPIXEL_GRAD = 7, 8     # kinds 5 / 6 with the input gradient's matrix appended (CVAE_FOLD_*_GRAD)
_FOLD_GRAD = (FOLD_CONV_K3S1_GRAD, FOLD_CONVT_K3S2_SUBPIXEL_GRAD)
_FOLD_CONVT = (FOLD_CONVT_K3S2, FOLD_CONVT_K3S2_SUBPIXEL, FOLD_CONVT_K3S2_SUBPIXEL_GRAD)     # weight [Cin][Cout][3][3]: the BatchNorm's channels are dimension 1
_FOLD_GEMM = (FOLD_CONV_K3S1, FOLD_CONVT_K3S2_SUBPIXEL) + _FOLD_GRAD      # w_out is the [N][KT] matrix of conv_s1


def _forward_only(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise L.CvaeError(f"{what} is forward-only (eval-mode inference): call it under torch.no_grad()")


def fold_bn_conv(entries):
    """Fold eval-mode BatchNorm2d into the convs in front of it, for up to 16 layers in ONE launch (cvae_fold_bn_conv).
    entries: (weight, kind, bias, bn) with kind FOLD_CONV_K4 (nn.Conv2d k4 weight, layout kept), FOLD_UPCONV_K3 (the Conv2d(k3) of an Upsample x2 +
    Conv2d pair -> its transposed k4 weight [Cin][Cout][4][4]) or FOLD_CONV_K3S2 (nn.Conv2d(k3, s2, p1) weight -> the k4/s2/p1 weight [Cout][Cin][4][4]
    with a zero fourth row and column) and bn an nn.BatchNorm2d on running statistics, or None (plain transform, bias copied).
    The ViT-VAE decoder's kinds: FOLD_CONVT_K3S2 (nn.ConvTranspose2d(k3, s2, p1, output_padding 1) weight [Cin][Cout][3][3] -> the transposed k4 weight
    [Cin][Cout][4][4], zero fourth row and column, scaled per Cout), FOLD_CONV_K3S1 (nn.Conv2d(k3, s1, p1) weight -> conv_s1's matrix [Cout][KT]) and
    FOLD_CONVT_K3S2_SUBPIXEL (the ConvTranspose2d weight -> conv_s1's sub-pixel matrix [4 Cout][KT]).  FOLD_CONV_K3S1_GRAD / FOLD_CONVT_K3S2_SUBPIXEL_GRAD:
    the same forward matrix (the same bits) and, from the same launch, the matrix of the layer's input gradient for conv_s1_bwd_data ([Cin][KT] resp.
    [32][256]): these entries return (w_out, b_out, w_grad).
    Returns [(w_out, b_out)] fp32, all views of one fresh buffer."""
    import ctypes as C
    k = len(entries)
    if not 1 <= k <= 16:
        raise L.CvaeError(f"fold_bn_conv: 1 to 16 layers per launch, got {k}")
    for w, kind, bias, bn in entries:
        L.require_gpu(w, bias)
        _forward_only("fold_bn_conv", w, bias, *((bn.weight, bn.bias) if bn is not None else ()))
        if bn is not None and (bn.running_mean is None or bn.weight is None):
            raise L.CvaeError("fold_bn_conv: the BatchNorm2d needs running statistics and an affine weight (eval mode, track_running_stats, affine)")
    sizes = []
    for w, kind, _b, _bn in entries:
        if (kind not in (FOLD_CONV_K4, FOLD_UPCONV_K3, FOLD_CONV_K3S2) + _FOLD_CONVT + _FOLD_GEMM or w.dim() != 4
                or tuple(w.shape[2:]) != ((4, 4) if kind == FOLD_CONV_K4 else (3, 3))):
            raise L.CvaeError(f"fold_bn_conv: kind {kind} does not match a weight of shape {tuple(w.shape)}")
        cout = w.shape[1] if kind in _FOLD_CONVT else w.shape[0]
        if kind in _FOLD_GEMM:
            cin, taps, rows = (w.shape[0], 4, 4 * cout) if kind in _FOLD_CONVT else (w.shape[1], 9, cout)
            nbwd = 0 if kind not in _FOLD_GRAD else (32 * 256 if kind in _FOLD_CONVT else cin * ((9 * cout + 63) // 64 * 64))
            sizes.append((rows * ((taps * cin + 63) // 64 * 64), cout, nbwd))
        else:
            sizes.append((w.shape[0] * w.shape[1] * 16, cout, 0))
    pad = lambda n: (n + 3) // 4 * 4                      # every piece starts on 16 bytes
    buf = torch.empty(sum(pad(a + g) + pad(b) for a, b, g in sizes), dtype=torch.float32, device=entries[0][0].device)
    outs, off = [], 0
    for (w, kind, _b, _bn), (nw, nb, ng) in zip(entries, sizes):
        shape = tuple(w.shape[:2]) + (4, 4) if kind != FOLD_UPCONV_K3 else (w.shape[1], w.shape[0], 4, 4)
        if kind in _FOLD_GEMM:
            shape = (4 * nb if kind in _FOLD_CONVT else nb, -1)
        wo = buf[off:off + nw].view(shape)
        wg = buf[off + nw:off + nw + ng].view((32 if kind in _FOLD_CONVT else w.shape[1], -1)) if ng else None      # the forward matrix's size is a multiple of 64
        off += pad(nw + ng)
        bo = buf[off:off + nb]
        off += pad(nb)
        outs.append((wo, bo, wg) if ng else (wo, bo))
    ws = [w.contiguous() for w, _k, _b, _bn in entries]
    vp = lambda v: (C.c_void_p * k)(*v)
    dims = [d for w, (_w, kind, _b, _bn) in zip(ws, entries) for d in ((w.shape[1], w.shape[0]) if kind in _FOLD_CONVT else (w.shape[0], w.shape[1]))]
    bns = [bn for _w, _k, _b, bn in entries]
    f32 = lambda t: None if t is None else t.detach().float().contiguous()
    keep = [(f32(bn.weight), f32(bn.bias), f32(bn.running_mean), f32(bn.running_var)) if bn is not None else (None,) * 4 for bn in bns]
    biases = [f32(b) for _w, _k, b, _bn in entries]
    check(lib.cvae_fold_bn_conv(k, vp([w.data_ptr() for w in ws]), (C.c_int * k)(*[kind for _w, kind, _b, _bn in entries]), (C.c_int64 * (2 * k))(*dims),
                                vp([ptr(b) for b in biases]), vp([ptr(t[0]) for t in keep]), vp([ptr(t[1]) for t in keep]), vp([ptr(t[2]) for t in keep]),
                                vp([ptr(t[3]) for t in keep]), (C.c_float * k)(*[float(bn.eps) if bn is not None else 0.0 for bn in bns]),
                                vp([o[0].data_ptr() for o in outs]), vp([o[1].data_ptr() for o in outs]), stream()), "fold_bn_conv")
    return outs


def row_diff_norms(a, b, ref=None, want_mean_abs=False):
    """l2[r] = ||a[r] - b[ref[r]]||_2 (and mean |a[r] - b[ref[r]]| when asked) over rows = a.shape[0], each row flattened (cvae_row_diff_norms).
    a, b: fp32 or bf16 (the same), contiguous; ref: int64 [rows] indices into b's rows (None: row r of b).  Fixed-order sums: bit-reproducible.
    Returns (l2, mean_abs or None), fp32 [rows]."""
    L.require_gpu(a, b, ref)
    _forward_only("row_diff_norms", a, b)
    if a.dtype != b.dtype or a.shape[1:] != b.shape[1:]:
        raise L.CvaeError(f"row_diff_norms: a {tuple(a.shape)} {a.dtype} and b {tuple(b.shape)} {b.dtype} must share dtype and row shape")
    a, b = a.contiguous(), b.contiguous()
    rows, n = a.shape[0], a[0].numel()
    if ref is not None:
        ref = ref.to(device=a.device, dtype=torch.int64).contiguous()
        if ref.shape != (rows,):
            raise L.CvaeError(f"row_diff_norms: ref must be [{rows}], got {tuple(ref.shape)}")
    l2 = _empty((rows,), torch.float32, a)
    ma = _empty((rows,), torch.float32, a) if want_mean_abs else None
    dt = L.dtype_code(a.dtype)
    _t, wp, wb = _scratch(lib.cvae_row_diff_norms_workspace_bytes(rows, n, dt), a)
    check(lib.cvae_row_diff_norms(ptr(a), ptr(b), ptr(ref), ptr(l2), ptr(ma), rows, b.shape[0], n, dt, wp, wb, stream()), "row_diff_norms")
    return l2, ma


def stack_mean_std(tensors):
    """(torch.stack(tensors).mean(0), torch.stack(tensors).std(0)) for up to 16 equal-shape fp32 tensors, without the stacked copy
    (cvae_stack_mean_std; two-pass: mean, then squared deviations).  One tensor gives a NaN std, as torch does."""
    import ctypes as C
    k = len(tensors)
    if not 1 <= k <= 16:
        raise L.CvaeError(f"stack_mean_std: 1 to 16 tensors, got {k}")
    L.require_gpu(*tensors)
    _forward_only("stack_mean_std", *tensors)
    shape = tensors[0].shape
    if any(t.shape != shape or t.dtype != torch.float32 for t in tensors):
        raise L.CvaeError("stack_mean_std: fp32 tensors of one shape expected")
    xs = [t.contiguous() for t in tensors]
    mean, std = _empty(shape, torch.float32, xs[0]), _empty(shape, torch.float32, xs[0])
    check(lib.cvae_stack_mean_std((C.c_void_p * k)(*[t.data_ptr() for t in xs]), k, ptr(mean), ptr(std), xs[0].numel(), stream()), "stack_mean_std")
    return mean, std


# ---- ViT-VAE encoder (csrc/vit.hip): forward-only building blocks on raw tensors -------------------------------------------------
GEMM_EPI = {None: 0, "gelu": 1, "residual": 2}      # CVAE_GEMM_EPI_*


def _rows2d(t, what, cols=None):
    if t.dim() != 2 or t.stride(1) != 1 or (cols is not None and t.shape[1] != cols):
        raise L.CvaeError(f"{what}: a [rows, {cols or 'cols'}] tensor with unit column stride expected, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return t


def vit_tokens(stem_cl, cls_token, pos):
    """fp32 residual stream [B, n + 1, 256]: row 0 = cls + pos[0], row 1 + i = stem[b, i] + pos[1 + i] (cvae_vit_tokens).  stem_cl: the channels-last
    output of the last stem conv [B, 1, h, w, 256] (fp32 or bf16) — already `rearrange("b c h w -> b (h w) c")`; pos: [n + 1, 256] fp32."""
    L.require_gpu(stem_cl, cls_token, pos)
    _forward_only("vit_tokens", stem_cl, cls_token, pos)
    B, n = stem_cl.shape[0], stem_cl[0].numel() // 256
    if stem_cl.shape[-1] != 256 or not stem_cl.is_contiguous() or pos.shape != (n + 1, 256) or cls_token.numel() != 256:
        raise L.CvaeError(f"vit_tokens: stem {tuple(stem_cl.shape)}, pos {tuple(pos.shape)}, cls {tuple(cls_token.shape)} do not form [B, n + 1, 256] tokens")
    tokens = _empty((B, n + 1, 256), torch.float32, stem_cl)
    check(lib.cvae_vit_tokens(ptr(stem_cl), L.dtype_code(stem_cl.dtype), ptr(cls_token.detach().contiguous()), ptr(pos.detach().contiguous()), ptr(tokens), B, n, stream()),
          "vit_tokens")
    return tokens


def layernorm256(x, weight, bias, eps, out_dtype):
    """nn.LayerNorm(256) of the rows of x (fp32 [rows, 256], any row stride that is a multiple of 4) -> [rows, 256] in out_dtype (cvae_layernorm256)."""
    L.require_gpu(x, weight, bias)
    _forward_only("layernorm256", x, weight, bias)
    _rows2d(x, "layernorm256", 256)
    if x.dtype != torch.float32:
        raise L.CvaeError("layernorm256: fp32 input expected (the residual stream)")
    y = _empty((x.shape[0], 256), out_dtype, x)
    check(lib.cvae_layernorm256(ptr(x), x.stride(0), ptr(weight.detach()), ptr(bias.detach()), ptr(y), x.shape[0], float(eps), L.dtype_code(out_dtype), stream()), "layernorm256")
    return y


def _token_gemm(what, x, weight, bias, epilogue, resid, out, want_pre, dropout=None):
    """The one body of token_gemm, token_gemm_gelu_train and token_gemm_dropout (`what`: the caller's name, for the error text) -> (result, pre-activation or
    None).  dropout: None, or the row site (p, key) / (p, key, row0, row_step) of cvae_token_gemm_dropout[_devkey]: fp32 only, epilogue "gelu" (the
    pre-activation is always saved, resid and out are not taken) or "residual"."""
    L.require_gpu(x, weight, bias, resid, out)
    _forward_only(what, x, weight, bias, resid)
    _rows2d(x, what)
    M, K = x.shape
    N = weight.shape[0]
    epilogues = GEMM_EPI if dropout is None else ("gelu", "residual")
    if weight.shape != (N, K) or bias is None or bias.shape != (N,) or weight.dtype != torch.float32 or epilogue not in epilogues:
        raise L.CvaeError(f"{what}: x {tuple(x.shape)}, weight {tuple(weight.shape)}, epilogue {epilogue!r}" + (" ('gelu' or 'residual')" if dropout is not None else ""))
    site = None if dropout is None else _dropout_site(what, dropout, True, x)
    if epilogue == "residual":
        if resid is None or resid.dtype != torch.float32 or _rows2d(resid, f"{what} resid", N).shape[0] != M:
            raise L.CvaeError(f"{what}: the residual epilogue needs a fp32 [M, N] residual")
        out = resid if out is None else out
    elif site is not None and (resid is not None or out is not None):
        raise L.CvaeError(f"{what}: resid and out belong to the residual epilogue")
    elif out is None:
        out = _empty((M, N), x.dtype, x)
    _rows2d(out, f"{what} out", N)                        # resid and out come from token_gemm[_dropout] alone: the training form passes neither
    if site is not None and (out.shape[0] != M or out.dtype != torch.float32):
        raise L.CvaeError(f"{what}: out {tuple(out.shape)} {out.dtype}")
    w, b, dt = weight.detach().contiguous(), bias.detach(), L.dtype_code(x.dtype)
    resid_stride = resid.stride(0) if resid is not None else 0
    if site is not None:
        sfx, p, key, row0, step = site
        pre = _empty((M, N), x.dtype, x) if epilogue == "gelu" else None
        check(getattr(lib, "cvae_token_gemm_dropout" + sfx)(ptr(x), x.stride(0), ptr(w), ptr(b), ptr(resid), resid_stride, ptr(pre), N if pre is not None else 0, ptr(out),
                                                            out.stride(0), M, K, N, GEMM_EPI[epilogue], p, key, row0, step, stream()), "token_gemm_dropout" + sfx)
        return out, pre
    if not want_pre:
        check(lib.cvae_token_gemm(ptr(x), x.stride(0), ptr(w), ptr(b), ptr(resid), resid_stride, ptr(out), out.stride(0), M, K, N, GEMM_EPI[epilogue], dt, stream()),
              "token_gemm")
        return out, None
    pre = _empty((M, N), x.dtype, x)
    check(lib.cvae_token_gemm_gelu_train(ptr(x), x.stride(0), ptr(w), ptr(b), ptr(pre), N, ptr(out), out.stride(0), M, K, N, dt, stream()), "token_gemm_gelu_train")
    return out, pre


def token_gemm(x, weight, bias, epilogue=None, resid=None, out=None, dropout=None):
    """epi(x @ weight.T + bias) (cvae_token_gemm).  x [M, K] fp32 or bf16 (the arithmetic mode), weight [N, K] / bias [N] the fp32 nn.Linear tensors.
    epilogue None / "gelu": result in x's dtype; "residual": fp32 resid + (x W^T + b), written to `out` (default: resid itself, in place).
    dropout = (p, key) or (p, key, row0, row_step): token_gemm_dropout's result (its first member with "gelu"); None: exactly the path above."""
    return _token_gemm("token_gemm", x, weight, bias, epilogue, resid, out, False, dropout)[0]


def _mhsa_views(what, B, rows, *ts):
    for t, n in zip(ts, rows):
        sh = t.shape
        if len(sh) != 3 or sh[2] != 256 or t.stride(2) != 1 or t.dtype != ts[0].dtype or sh[0] != B or sh[1] < n:
            raise L.CvaeError(f"{what}: [B, tokens, 256] views with unit column stride and one dtype expected, got {tuple(t.shape)} {t.dtype}")


def _mhsa_fwd(what, q, k, v, n_query_rows, want_lse, dropout=None):
    """The one body of mhsa and mhsa_train (`what`: the caller's name, for the error text) -> (out, lse or None).  dropout (with want_lse): (p, key)."""
    L.require_gpu(q, k, v)
    _forward_only(what, q, k, v)
    B, N = k.shape[0], k.shape[1]
    nq = N if n_query_rows is None else int(n_query_rows)
    _mhsa_views(what, B, (nq, N, N), q, k, v)
    if v.shape[1] != N or not 1 <= nq <= N:
        raise L.CvaeError(f"{what}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, n_query_rows {nq}")
    out = _empty((B, nq, 256), q.dtype, q)
    tail = (q.stride(1), k.stride(1), v.stride(1), q.stride(0), k.stride(0), v.stride(0), B, N, nq, L.dtype_code(q.dtype), stream())
    if not want_lse:
        check(lib.cvae_mhsa_fwd(ptr(q), ptr(k), ptr(v), ptr(out), *tail), "mhsa_fwd")
        return out, None
    lse = _empty((B, 8, nq), torch.float32, q)
    if dropout is not None:
        sfx, p, key = _dropout_site(what, dropout, False, q)
        check(getattr(lib, "cvae_mhsa_fwd_train_dropout" + sfx)(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), *tail[:9], p, key, stream()),
              "mhsa_fwd_train_dropout" + sfx)
        return out, lse
    check(lib.cvae_mhsa_fwd_train(ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), *tail), "mhsa_fwd_train")
    return out, lse


def mhsa(q, k, v, n_query_rows=None):
    """Fused 8-head self-attention of width 256 (cvae_mhsa_fwd): q [B, >= n_query_rows, 256], k / v [B, N, 256] — views with unit column stride, e.g. the
    three column panels of the packed in-projection output [B, N, 768].  The first n_query_rows tokens are the queries (default: all N).
    Returns [B, n_query_rows, 256] in the operands' dtype."""
    return _mhsa_fwd("mhsa", q, k, v, n_query_rows, False)[0]


# ---- ViT-VAE encoder, the training forms of the two fused building blocks: the same values, plus what the backward needs --------------------------------
def token_gemm_gelu_train(x, weight, bias, dropout=None):
    """(gelu(x W^T + b), x W^T + b), both in x's dtype: token_gemm's "gelu" output, bit for bit, and the pre-activation (cvae_token_gemm_gelu_train).
    dropout = (p, key) or (p, key, row0, row_step), fp32 only: the first member is dropped with the row-site mask (cvae_token_gemm_dropout); None: exactly
    the path above."""
    return _token_gemm("token_gemm_gelu_train", x, weight, bias, "gelu", None, None, True, dropout)


def mhsa_train(q, k, v, n_query_rows=None, dropout=None):
    """mhsa (the same output, bit for bit) that also returns lse fp32 [B, 8, n_query_rows], the row statistic mhsa_bwd needs (cvae_mhsa_fwd_train).
    dropout = (p, key), fp32 only: the probabilities are dropped with the attention-site mask of include/cvae_hip.h before the P V product
    (cvae_mhsa_fwd_train_dropout); lse stays that of the undropped rows.  None: exactly the path above."""
    return _mhsa_fwd("mhsa_train", q, k, v, n_query_rows, True, dropout)


# ---- dropout when training the transformer: masks are recomputed in the kernels from (p, key); the host only hands the keys out ---------
_M64 = (1 << 64) - 1


def _splitmix64(z):
    """The splitmix64 output function: a bijection of the 64-bit integers."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class DropoutKeys:
    """The 64-bit Philox keys of the dropout sites, on the host.  key(step, block, site) = splitmix64(splitmix64(seed) + (step << 20 | block << 4 | site))
    mod 2^64, for step < 2^44, block < 2^16, site < 16: a pure function of its arguments and the seed, and — splitmix64 being a bijection and the packing
    one to one — distinct for distinct (step, block, site).  `step` is a Python int that the training forward advances once per call; seed defaults to
    torch.initial_seed().  Sites of a transformer block: ATTN, MLP_ACT (after the GELU), MLP_OUT (after the second Linear)."""
    ATTN, MLP_ACT, MLP_OUT = 0, 1, 2

    def __init__(self, seed=None):
        self.seed = int(torch.initial_seed() if seed is None else seed) & _M64
        self.step = 0

    def key(self, step, block, site):
        step, block, site = int(step), int(block), int(site)
        if not (0 <= step < 1 << 44 and 0 <= block < 1 << 16 and 0 <= site < 16):
            raise L.CvaeError(f"DropoutKeys.key: step {step} (< 2^44), block {block} (< 2^16), site {site} (< 16) expected")
        return _splitmix64((_splitmix64(self.seed) + (step << 20 | block << 4 | site)) & _M64)

    def state(self):
        return {"seed": self.seed, "step": self.step}

    def load_state(self, state):
        self.seed, self.step = int(state["seed"]) & _M64, int(state["step"])
        return self


class DeviceDropoutKeys:
    """DropoutKeys with the step counter on the device: what a captured training step needs, and usable eagerly as well.  The same seed rule,
    the same key(seed, step, block, site) integers and the same state() / load_state() dict as DropoutKeys, so checkpoints interchange.
    advance() is one launch (cvae_dropout_keys_step): it returns a NEW [n_blocks, 4] int64 table holding the keys of the counter's current step — the bit
    patterns of the unsigned 64-bit keys — and leaves the counter one higher; no value reaches the host.  A table per call keeps two forwards followed by two
    backwards correct, and under capture the table lives in the graph's pool.  key(table, block, site) is the one-element view the ops take as `key`."""
    ATTN, MLP_ACT, MLP_OUT = DropoutKeys.ATTN, DropoutKeys.MLP_ACT, DropoutKeys.MLP_OUT

    def __init__(self, n_blocks, device, seed=None, step=0):
        device = torch.device(device)
        if device.type != "cuda":
            raise L.CvaeError(f"DeviceDropoutKeys: the counter lives on the GPU, got device {device} (there is no CPU fallback; host keys: ops.DropoutKeys)")
        if not 1 <= int(n_blocks) <= 1 << 16:
            raise L.CvaeError(f"DeviceDropoutKeys: 1 <= n_blocks <= 65536 expected, got {n_blocks}")
        self.n_blocks = int(n_blocks)
        self.seed = int(torch.initial_seed() if seed is None else seed) & _M64
        self.counter = torch.full((1,), int(step), dtype=torch.int64, device=device)

    def advance(self):
        table = torch.empty((self.n_blocks, 4), dtype=torch.int64, device=self.counter.device)
        with torch.cuda.device(self.counter.device):
            check(lib.cvae_dropout_keys_step(_splitmix64(self.seed), ptr(self.counter), ptr(table), self.n_blocks, stream()), "dropout_keys_step")
        return table

    @staticmethod
    def key(table, block, site):
        return table[block, site:site + 1]

    def state(self):
        """{"seed", "step"}: reads the counter back, which synchronizes with the device — never inside a capture."""
        return {"seed": self.seed, "step": int(self.counter.item())}

    def load_state(self, state):
        """The counter is rewritten in place: a captured graph keeps reading it.  The seed is a launch argument, so a graph captured before keeps the seed
        it was captured with."""
        self.seed = int(state["seed"]) & _M64
        self.counter.fill_(int(state["step"]))
        return self


def _dropout_site(what, dropout, rows, *tensors):
    """(entry suffix, p, key) of an attention site or (entry suffix, p, key, row0, row_step) of a row site from the `dropout` argument of an op; the tensors
    must be fp32.  key: a Python int (suffix "": passed by value) or a one-element int64 tensor on the operands' device (suffix "_devkey": its address is
    passed and the kernel reads it when it runs — the value is never brought to the host)."""
    n = len(dropout) if isinstance(dropout, (tuple, list)) else 0
    if n not in ((2, 4) if rows else (2,)):
        raise L.CvaeError(f"{what}: dropout must be (p, key)" + (" or (p, key, row0, row_step)" if rows else "") + f", got {dropout!r}")
    p, key, suffix = float(dropout[0]), dropout[1], ""
    if isinstance(key, torch.Tensor):
        ref = next(t for t in tensors if t is not None)
        if key.dtype != torch.int64 or key.numel() != 1 or key.device != ref.device or key.data_ptr() % 8:
            raise L.CvaeError(f"{what}: a tensor key must be one int64 element on the operands' device ({ref.device}), got {tuple(key.shape)} {key.dtype} "
                              f"on {key.device}")
        key, suffix, key_ok = key.data_ptr(), "_devkey", True
    else:
        key = int(key)
        key_ok = 0 <= key <= _M64
    row0, step = (int(dropout[2]), int(dropout[3])) if n == 4 else (0, 1)
    if not (0.0 <= p < 1.0 and key_ok and row0 >= 0 and step >= 1):
        raise L.CvaeError(f"{what}: dropout needs 0 <= p < 1, a 64-bit key, row0 >= 0 and row_step >= 1, got {dropout!r}")
    if any(t is not None and t.dtype != torch.float32 for t in tensors):
        raise L.CvaeError(f"{what}: dropout is implemented for float32 tensors only (bfloat16 compute dtype: not yet)")
    return (suffix, p, key, row0, step) if rows else (suffix, p, key)


def token_gemm_dropout(x, weight, bias, epilogue, dropout, resid=None, out=None):
    """token_gemm on fp32 x with a row-site dropout mask over the output (cvae_token_gemm_dropout).  dropout = (p, key) or (p, key, row0, row_step).
    epilogue "gelu" -> (gelu(pre) keep s, pre): token_gemm_gelu_train's pair with the first member dropped; "residual" -> resid + (x W^T + b) keep s,
    written to `out` (default: resid itself, in place).  p = 0 gives the bits of token_gemm_gelu_train / token_gemm."""
    if not isinstance(dropout, (tuple, list)):
        raise L.CvaeError(f"token_gemm_dropout: dropout must be (p, key) or (p, key, row0, row_step), got {dropout!r}")
    res = _token_gemm("token_gemm_dropout", x, weight, bias, epilogue, resid, out, False, dropout)
    return res if epilogue == "gelu" else res[0]


def dropout_rows(x, dropout, out=None):
    """x keep s on fp32 [M, N] rows (any row stride, N % 4 == 0) with the row-site mask (cvae_dropout_rows).  dropout = (p, key) or (p, key, row0, row_step);
    out: where to write (may be x itself; default a new tensor).  On ones it is the mask."""
    L.require_gpu(x, out)
    _forward_only("dropout_rows", x)
    _rows2d(x, "dropout_rows")
    sfx, p, key, row0, step = _dropout_site("dropout_rows", dropout, True, x, out)
    M, N = x.shape
    if out is None:
        out = _empty((M, N), torch.float32, x)
    if _rows2d(out, "dropout_rows out", N).shape[0] != M:
        raise L.CvaeError(f"dropout_rows: out {tuple(out.shape)} for x {tuple(x.shape)}")
    check(getattr(lib, "cvae_dropout_rows" + sfx)(ptr(x), x.stride(0), ptr(out), out.stride(0), M, N, p, key, row0, step, stream()), "dropout_rows" + sfx)
    return out


# ---- ViT-VAE encoder, training the transformer (csrc/vit.hip): the backward building blocks, on raw tensors as the ones above ---------
def _overlap(a, b):
    """do two [B, tokens, 256] views with unit column stride share an element?  Panels of one packed buffer interleave: same storage, the same row and batch
    strides and column ranges that meet; anything else is compared by its address range."""
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return False
    if a.stride() == b.stride() and a.stride(1) >= 256:
        off = (b.storage_offset() - a.storage_offset()) % a.stride(1)
        if min(off, a.stride(1) - off) >= 256:
            return False                                                    # disjoint column panels of the same rows
    span = lambda t: (t.storage_offset(), t.storage_offset() + sum((n - 1) * st for n, st in zip(t.shape, t.stride())))
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 <= b1 and b0 <= a1


def mhsa_bwd(q, k, v, out, lse, dout, dq, dk, dv, dropout=None):
    """The gradients of mhsa_train's operands, written into dq [B, n_query_rows, 256] and dk / dv [B, N, 256] — views with unit column stride, e.g. the
    column panels of the packed in-projection cotangent [B, N, 768] (cvae_mhsa_bwd).  out / dout: contiguous [B, n_query_rows, 256].
    dropout: the (p, key) the forward ran with (cvae_mhsa_bwd_dropout: the mask is recomputed, fp32 only); None: exactly the path without."""
    L.require_gpu(q, k, v, out, lse, dout, dq, dk, dv)
    _forward_only("mhsa_bwd", q, k, v, out, dout)
    B, N, nq = k.shape[0], k.shape[1], out.shape[1]
    _mhsa_views("mhsa_bwd", B, (nq, N, N, nq, nq, nq, N, N), q, k, v, out, dout, dq, dk, dv)
    if (not out.is_contiguous() or not dout.is_contiguous() or dout.shape != out.shape or lse.shape != (B, 8, nq) or lse.dtype != torch.float32
            or not lse.is_contiguous() or v.shape[1] != N or dq.shape[1] != nq or dk.shape[1] != N or dv.shape[1] != N or not 1 <= nq <= N):
        raise L.CvaeError(f"mhsa_bwd: q {tuple(q.shape)}, k {tuple(k.shape)}, out {tuple(out.shape)}, dout {tuple(dout.shape)}, lse {tuple(lse.shape)}, "
                          f"dq {tuple(dq.shape)}, dk {tuple(dk.shape)}, dv {tuple(dv.shape)}")
    outs = (dq, dk, dv)
    if any(_overlap(a, b) for i, a in enumerate(outs) for b in outs[i + 1:] + (q, k, v, out, dout)):
        raise L.CvaeError("mhsa_bwd: dq, dk and dv must not overlap each other or an operand")
    _t, wp, wb = _scratch(lib.cvae_mhsa_bwd_workspace_bytes(B, nq), q)
    head = (ptr(q), ptr(k), ptr(v), ptr(out), ptr(lse), ptr(dout), ptr(dq), ptr(dk), ptr(dv), q.stride(1), k.stride(1), v.stride(1), q.stride(0), k.stride(0),
            v.stride(0), dq.stride(1), dk.stride(1), dv.stride(1), dq.stride(0), dk.stride(0), dv.stride(0), B, N, nq)
    if dropout is not None:
        sfx, p, key = _dropout_site("mhsa_bwd", dropout, False, q)
        check(getattr(lib, "cvae_mhsa_bwd_dropout" + sfx)(*head, p, key, wp, wb, stream()), "mhsa_bwd_dropout" + sfx)
    else:
        check(lib.cvae_mhsa_bwd(*head, L.dtype_code(q.dtype), wp, wb, stream()), "mhsa_bwd")
    return dq, dk, dv


def _gemm_mode(what, g, mode):
    """The arithmetic mode of a backward GEMM: fp32 mode takes fp32 cotangents only; bf16 mode takes bf16 ones or the fp32 stream gradient."""
    if mode not in (torch.float32, torch.bfloat16) or g.dtype not in (torch.float32, mode):
        raise L.CvaeError(f"{what}: a {g.dtype} cotangent in {mode} arithmetic")


def token_gemm_bwd_data(g, weight, mode, out_dtype=None, gate_pre=None, resid=None, out=None, dropout=None):
    """dx [M, K] = (g [M, N] @ weight [N, K]) * gelu'(gate_pre) + resid (cvae_token_gemm_bwd_data).  weight: the fp32 nn.Linear tensor or a row slice of it;
    mode: the arithmetic (torch.float32 / torch.bfloat16); g fp32 or `mode`; gate_pre [M, K] in `mode`: the saved pre-activation; resid fp32 [M, K] (any row
    stride): added, result fp32, written to `out` (default: resid itself, in place).  out_dtype (default `mode`): the result's dtype without resid.
    dropout = (p, key) or (p, key, row0, row_step): dx = (g W) keep s * gelu'(gate_pre) with the row-site mask over dx (cvae_token_gemm_bwd_data_dropout);
    fp32 throughout, no resid.  None: exactly the path above."""
    L.require_gpu(g, weight, gate_pre, resid, out)
    _forward_only("token_gemm_bwd_data", g, weight, gate_pre, resid)
    _rows2d(g, "token_gemm_bwd_data")
    _gemm_mode("token_gemm_bwd_data", g, mode)
    M, N = g.shape
    K = weight.shape[1] if weight.dim() == 2 else -1
    if weight.dim() != 2 or weight.shape[0] != N or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise L.CvaeError(f"token_gemm_bwd_data: g {tuple(g.shape)}, weight {tuple(weight.shape)} {weight.dtype} (contiguous fp32 [N, K] rows expected)")
    if gate_pre is not None and (gate_pre.dtype != mode or _rows2d(gate_pre, "token_gemm_bwd_data gate_pre", K).shape[0] != M):
        raise L.CvaeError(f"token_gemm_bwd_data: gate_pre {tuple(gate_pre.shape)} {gate_pre.dtype}")
    if resid is not None:
        if resid.dtype != torch.float32 or _rows2d(resid, "token_gemm_bwd_data resid", K).shape[0] != M or out_dtype not in (None, torch.float32):
            raise L.CvaeError("token_gemm_bwd_data: the residual needs a fp32 [M, K] tensor and a fp32 result")
        out = resid if out is None else out
    elif out is None:
        out = _empty((M, K), out_dtype or mode, g)
    if _rows2d(out, "token_gemm_bwd_data out", K).shape[0] != M or out.dtype not in (torch.float32, mode) or (resid is not None and out.dtype != torch.float32):
        raise L.CvaeError(f"token_gemm_bwd_data: out {tuple(out.shape)} {out.dtype}")
    cot, wgate, dx = (ptr(g), g.stride(0)), (ptr(weight.detach()), ptr(gate_pre), gate_pre.stride(0) if gate_pre is not None else 0), (ptr(out), out.stride(0))
    if dropout is not None:
        sfx, p, key, row0, step = _dropout_site("token_gemm_bwd_data", dropout, True, g, out)
        if mode != torch.float32 or resid is not None:
            raise L.CvaeError("token_gemm_bwd_data: dropout runs in fp32 arithmetic and takes no residual")
        check(getattr(lib, "cvae_token_gemm_bwd_data_dropout" + sfx)(*cot, *wgate, *dx, M, K, N, p, key, row0, step, stream()), "token_gemm_bwd_data_dropout" + sfx)
    else:
        check(lib.cvae_token_gemm_bwd_data(*cot, L.dtype_code(g.dtype), *wgate, ptr(resid), resid.stride(0) if resid is not None else 0, *dx, L.dtype_code(out.dtype),
                                           M, K, N, L.dtype_code(mode), stream()), "token_gemm_bwd_data")
    return out


def token_gemm_wgrad(g, x, dW=None, db=None):
    """(dW [N, K], db [N]) fp32 of token_gemm's nn.Linear from its input x [M, K] (fp32 or bf16: the arithmetic mode) and the cotangent g [M, N] of its output
    (x's dtype, or the fp32 stream gradient) (cvae_token_gemm_wgrad).  dW / db: where to write, e.g. a row slice of the packed in-projection gradient."""
    L.require_gpu(g, x, dW, db)
    _forward_only("token_gemm_wgrad", g, x)
    _rows2d(g, "token_gemm_wgrad g")
    _rows2d(x, "token_gemm_wgrad x")
    _gemm_mode("token_gemm_wgrad", g, x.dtype)
    (M, N), K = g.shape, x.shape[1]
    nbytes = lib.cvae_token_gemm_wgrad_workspace_bytes(M, K, N)
    if x.shape[0] != M or not nbytes:
        raise L.CvaeError(f"token_gemm_wgrad: g {tuple(g.shape)}, x {tuple(x.shape)}: {L.strerror(-3)}")
    dW = _empty((N, K), torch.float32, x) if dW is None else dW
    db = _empty((N,), torch.float32, x) if db is None else db
    if dW.shape != (N, K) or db.shape != (N,) or dW.dtype != torch.float32 or db.dtype != torch.float32 or not dW.is_contiguous() or not db.is_contiguous():
        raise L.CvaeError(f"token_gemm_wgrad: contiguous fp32 dW [{N}, {K}] and db [{N}] expected, got {tuple(dW.shape)} and {tuple(db.shape)}")
    _t, wp, wb = _scratch(nbytes, x)
    check(lib.cvae_token_gemm_wgrad(ptr(g), g.stride(0), L.dtype_code(g.dtype), ptr(x), x.stride(0), ptr(dW), ptr(db), M, K, N, L.dtype_code(x.dtype), wp, wb, stream()),
          "token_gemm_wgrad")
    return dW, db


def layernorm256_bwd(g, x, weight, eps, dx=None, accumulate=False):
    """(dx, dgamma, dbeta) of layernorm256 from its fp32 input x [rows, 256] (any row stride) and the cotangent g [rows, 256] of its output (fp32 or bf16)
    (cvae_layernorm256_bwd).  dx: fp32 [rows, 256] with any row stride, written — or, with accumulate, added to (the stream gradient takes the LayerNorm
    branch next to the skip); default: a fresh tensor."""
    L.require_gpu(g, x, weight, dx)
    _forward_only("layernorm256_bwd", g, x, weight)
    _rows2d(g, "layernorm256_bwd g", 256)
    _rows2d(x, "layernorm256_bwd x", 256)
    rows = x.shape[0]
    if weight.shape != (256,) or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise L.CvaeError(f"layernorm256_bwd: a contiguous fp32 [256] weight expected, got {tuple(weight.shape)} {weight.dtype}")
    if x.dtype != torch.float32 or g.shape[0] != rows or g.dtype not in (torch.float32, torch.bfloat16) or (dx is None and accumulate):
        raise L.CvaeError(f"layernorm256_bwd: x {tuple(x.shape)} {x.dtype}, g {tuple(g.shape)} {g.dtype}, accumulate {accumulate} into {None if dx is None else tuple(dx.shape)}")
    dx = _empty((rows, 256), torch.float32, x) if dx is None else dx
    if dx.dtype != torch.float32 or _rows2d(dx, "layernorm256_bwd dx", 256).shape[0] != rows:
        raise L.CvaeError(f"layernorm256_bwd: dx {tuple(dx.shape)} {dx.dtype}")
    dgamma, dbeta = _empty((256,), torch.float32, x), _empty((256,), torch.float32, x)
    _t, wp, wb = _scratch(lib.cvae_layernorm256_bwd_workspace_bytes(rows), x)
    check(lib.cvae_layernorm256_bwd(ptr(g), g.stride(0), L.dtype_code(g.dtype), ptr(x), x.stride(0), ptr(weight.detach()), ptr(dx), dx.stride(0), int(bool(accumulate)),
                                    ptr(dgamma), ptr(dbeta), rows, float(eps), wp, wb, stream()), "layernorm256_bwd")
    return dx, dgamma, dbeta


def vit_tokens_bwd(dtokens, stem_dtype, gate=None, gate_act=None):
    """(dpos [n + 1, 256], dcls [256], dstem [B, n, 256] in stem_dtype) from the fp32 residual-stream gradient [B, n + 1, 256] (cvae_vit_tokens_bwd).
    gate / gate_act (optional, together): the stem's output [B, n, 256] in stem_dtype, the output of the activation gate_act; dstem is then multiplied by
    act'(gate) = gate > 0 ? 1 : slope in fp32 before its one rounding — the gradient of the stem's last PRE-activation.  dpos and dcls are never gated."""
    L.require_gpu(dtokens, gate)
    _forward_only("vit_tokens_bwd", dtokens, gate)
    if (gate is None) != (gate_act in (None, "none")) or gate_act not in _GATE_ACTS:
        raise L.CvaeError(f"vit_tokens_bwd: gate and gate_act ({_GATE_ACTS[2:]}) come together, got gate_act={gate_act!r}")
    if dtokens.dim() != 3 or dtokens.shape[1] < 2 or dtokens.shape[2] != 256 or dtokens.dtype != torch.float32 or not dtokens.is_contiguous():
        raise L.CvaeError(f"vit_tokens_bwd: a contiguous fp32 [B, n + 1, 256] gradient expected, got {tuple(dtokens.shape)} {dtokens.dtype}")
    B, n = dtokens.shape[0], dtokens.shape[1] - 1
    dpos, dcls, dstem = _empty((n + 1, 256), torch.float32, dtokens), _empty((256,), torch.float32, dtokens), _empty((B, n, 256), stem_dtype, dtokens)
    if gate is not None:
        _like_operands("vit_tokens_bwd", (B, n, 256), stem_dtype, gate=gate)
    check(lib.cvae_vit_tokens_bwd(ptr(dtokens), ptr(dpos), ptr(dcls), ptr(dstem), L.dtype_code(stem_dtype), ptr(gate), L.act_code(gate_act), B, n, stream()),
          "vit_tokens_bwd")
    return dpos, dcls, dstem


# ---- attention weights and attention rollout (csrc/vit.hip): forward-only, recomputed from q, k and mhsa_train's lse -----------------------
def _mhsa_probe(what, q, k, lse, n_query_rows):
    """The checks mhsa_weights and mhsa_rollout_step share -> (B, N, n_query_rows, the stride / size arguments of their entries)."""
    L.require_gpu(q, k, lse)
    _forward_only(what, q, k, lse)
    B, N = k.shape[0], k.shape[1]
    nq = N if n_query_rows is None else int(n_query_rows)
    if not 1 <= nq <= N:
        raise L.CvaeError(f"{what}: 1 <= n_query_rows <= {N} expected, got {nq}")
    _mhsa_views(what, B, (nq, N), q, k)
    if lse.shape != (B, 8, nq) or lse.dtype != torch.float32 or not lse.is_contiguous():
        raise L.CvaeError(f"{what}: lse must be the contiguous float32 [{B}, 8, {nq}] row statistic of mhsa_train, got {tuple(lse.shape)} {lse.dtype}")
    return B, N, nq, (q.stride(1), k.stride(1), q.stride(0), k.stride(0))


def mhsa_weights(q, k, lse, n_query_rows=None, average_heads=True, out=None):
    """The attention probabilities mhsa never writes (cvae_mhsa_weights): P = 2^(s - lse) recomputed from q [B, >= n_query_rows, 256], k [B, N, 256] (views as
    mhsa takes them) and lse [B, 8, n_query_rows], the row statistic mhsa_train returned for the same q and k.
    average_heads=True: fp32 [B, n_query_rows, N], the head-order sum times 1/8 — what nn.MultiheadAttention(need_weights=True) returns in eval mode;
    False: fp32 [B, 8, n_query_rows, N].  Rows are dense (N floats).  Per head at N = 961 this is 29.6 MB per image: the only N x N object of the ViT path.
    out: an fp32 tensor of that shape to write into; its batch stride is free, one batch's block must be contiguous and its base 16-byte aligned."""
    B, N, nq, strides = _mhsa_probe("mhsa_weights", q, k, lse, n_query_rows)
    shape = (B, nq, N) if average_heads else (B, 8, nq, N)
    if out is None:
        out = _empty(shape, torch.float32, q)
    else:
        L.require_gpu(out)
        if (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != q.device or (B and not out[0].is_contiguous())
                or (B > 1 and out.stride(0) < out[0].numel()) or out.data_ptr() % 16):
            raise L.CvaeError(f"mhsa_weights: out must be a float32 {shape} tensor on {q.device} with contiguous batch blocks and a 16-byte-aligned base, got "
                              f"{tuple(out.shape)} {out.dtype} strides {tuple(out.stride())}")
    if B == 0:
        return out
    check(lib.cvae_mhsa_weights(ptr(q), ptr(k), ptr(lse), ptr(out), *strides, out.stride(0) if B > 1 else out[0].numel(), B, N, nq, int(bool(average_heads)),
                                L.dtype_code(q.dtype), stream()), "mhsa_weights")
    return out


def mhsa_rollout_step(q, k, lse, r, n_query_rows=None, residual=0.5, out=None):
    """One factor of attention rollout applied to a row vector, the N x N matrix never formed (cvae_mhsa_rollout_step):
    out[b, j] = residual r[b, j] + (1 - residual) / 8 sum_h sum_{i < n_query_rows} r[b, i] P[b, h, i, j], with P as in mhsa_weights.
    r: fp32 [B, N] contiguous; returns fp32 [B, N] (written to `out` if given: it must not be r or overlap it).  0 <= residual <= 1."""
    B, N, nq, strides = _mhsa_probe("mhsa_rollout_step", q, k, lse, n_query_rows)
    L.require_gpu(r, out)
    residual = float(residual)
    if not 0.0 <= residual <= 1.0:
        raise L.CvaeError(f"mhsa_rollout_step: 0 <= residual <= 1 expected, got {residual}")
    if r.shape != (B, N) or r.dtype != torch.float32 or not r.is_contiguous() or r.device != q.device:
        raise L.CvaeError(f"mhsa_rollout_step: r must be a contiguous float32 [{B}, {N}] tensor on {q.device}, got {tuple(r.shape)} {r.dtype}")
    if out is None:
        out = _empty((B, N), torch.float32, q)
    elif out.shape != r.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != r.device:
        raise L.CvaeError(f"mhsa_rollout_step: out must be a contiguous float32 [{B}, {N}] tensor on {q.device}, got {tuple(out.shape)} {out.dtype}")
    if B == 0:
        return out
    check(lib.cvae_mhsa_rollout_step(ptr(q), ptr(k), ptr(lse), ptr(r), ptr(out), *strides, B, N, nq, residual, L.dtype_code(q.dtype), stream()),
          "mhsa_rollout_step")
    return out


# ---- attention gradients and gradient-weighted relevance (csrc/vit_attention_grad_probe.inc): forward-only ---------------------------------
def _mhsa_dout(what, dout, like, B, nq):
    """dout as mhsa_bwd takes it: the contiguous [B, n_query_rows, 256] cotangent of the attention output, in the operands' dtype."""
    if tuple(dout.shape) != (B, nq, 256) or dout.dtype != like.dtype or not dout.is_contiguous() or dout.device != like.device:
        raise L.CvaeError(f"{what}: dout must be a contiguous {like.dtype} [{B}, {nq}, 256] tensor on {like.device}, got {tuple(dout.shape)} {dout.dtype}")


def mhsa_weight_grads(dout, v, n_query_rows=None, out=None):
    """The gradient with respect to the attention probabilities taken as a free variable (cvae_mhsa_weight_grads) — what a hook on the softmax output
    receives: gA[b, h, i, j] = sum_{d < 32} dout[b, i, 32 h + d] v[b, j, 32 h + d].  dout: the contiguous [B, n_query_rows, 256] cotangent of mhsa's output;
    v [B, N, 256], a view as mhsa takes it.  Returns fp32 [B, 8, n_query_rows, N] with dense rows (`out`: as in mhsa_weights)."""
    L.require_gpu(dout, v)
    _forward_only("mhsa_weight_grads", dout, v)
    B, N = v.shape[0], v.shape[1]
    nq = N if n_query_rows is None else int(n_query_rows)
    if not 1 <= nq <= N:
        raise L.CvaeError(f"mhsa_weight_grads: 1 <= n_query_rows <= {N} expected, got {nq}")
    _mhsa_views("mhsa_weight_grads", B, (N,), v)
    _mhsa_dout("mhsa_weight_grads", dout, v, B, nq)
    shape = (B, 8, nq, N)
    if out is None:
        out = _empty(shape, torch.float32, v)
    else:
        L.require_gpu(out)
        if (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != v.device or (B and not out[0].is_contiguous())
                or (B > 1 and out.stride(0) < out[0].numel()) or out.data_ptr() % 16):
            raise L.CvaeError(f"mhsa_weight_grads: out must be a float32 {shape} tensor on {v.device} with contiguous batch blocks and a 16-byte-aligned base, "
                              f"got {tuple(out.shape)} {out.dtype} strides {tuple(out.stride())}")
    if B == 0:
        return out
    check(lib.cvae_mhsa_weight_grads(ptr(dout), ptr(v), ptr(out), v.stride(1), v.stride(0), out.stride(0) if B > 1 else out[0].numel(), B, N, nq,
                                     L.dtype_code(v.dtype), stream()), "mhsa_weight_grads")
    return out


def mhsa_relevance_step(q, k, v, lse, dout, r, n_query_rows=None, out=None):
    """One step of gradient-weighted attention relevance (Chefer, Gur & Wolf 2021, the self-attention rule) applied to a row vector, no N x N matrix formed
    (cvae_mhsa_relevance_step):  out[b, j] = r[b, j] + sum_{i < n_query_rows} r[b, i] Abar[b, i, j],  Abar = 1/8 sum_h max(0, gA P),
    with P as in mhsa_weights (from q, k, lse) and gA as in mhsa_weight_grads (from dout, v).  r: fp32 [B, N] contiguous; returns fp32 [B, N] (written to `out`
    if given: it must not be r or overlap it)."""
    B, N, nq, (qs, ks, qb, kb) = _mhsa_probe("mhsa_relevance_step", q, k, lse, n_query_rows)
    L.require_gpu(v, dout, r, out)
    _forward_only("mhsa_relevance_step", v, dout)
    _mhsa_views("mhsa_relevance_step", B, (nq, N, N), q, k, v)
    if v.shape[1] != N:
        raise L.CvaeError(f"mhsa_relevance_step: k {tuple(k.shape)} and v {tuple(v.shape)} must hold the same tokens")
    _mhsa_dout("mhsa_relevance_step", dout, q, B, nq)
    if r.shape != (B, N) or r.dtype != torch.float32 or not r.is_contiguous() or r.device != q.device:
        raise L.CvaeError(f"mhsa_relevance_step: r must be a contiguous float32 [{B}, {N}] tensor on {q.device}, got {tuple(r.shape)} {r.dtype}")
    if out is None:
        out = _empty((B, N), torch.float32, q)
    elif out.shape != r.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != r.device:
        raise L.CvaeError(f"mhsa_relevance_step: out must be a contiguous float32 [{B}, {N}] tensor on {q.device}, got {tuple(out.shape)} {out.dtype}")
    if B == 0:
        return out
    _t, wp, wb = _scratch(lib.cvae_mhsa_relevance_step_workspace_bytes(B, N, nq), q)
    check(lib.cvae_mhsa_relevance_step(ptr(q), ptr(k), ptr(v), ptr(lse), ptr(dout), ptr(r), ptr(out), qs, ks, v.stride(1), qb, kb, v.stride(0), B, N, nq,
                                       L.dtype_code(q.dtype), wp, wb, stream()), "mhsa_relevance_step")
    return out


# ---- Grad-CAM on the stem output (csrc/vit_gradcam.inc): forward-only --------------------------------------------------------------------
def gradcam(A, dA, normalize=True):
    """Grad-CAM of a channels-last activation and its gradient (cvae_gradcam256): A, dA [B, n, 256] contiguous, fp32 or bf16, the same dtype (the stem output
    and `dstem`) -> fp32 [B, n]:  w[b, c] = mean_i dA[b, i, c] (rows added in index order), cam[b, i] = max(0, sum_c w[b, c] A[b, i, c]), and with normalize
    (cam - min_i cam) / (max_i cam - min_i cam + 1e-8) per image — the reference GradCAM's arithmetic without its resize.  One launch, one workgroup per image."""
    L.require_gpu(A, dA)
    _forward_only("gradcam", A, dA)
    if (A.dim() != 3 or A.shape[2] != 256 or A.shape[1] < 1 or A.dtype not in (torch.float32, torch.bfloat16) or not A.is_contiguous()
            or tuple(dA.shape) != tuple(A.shape) or dA.dtype != A.dtype or not dA.is_contiguous() or dA.device != A.device):
        raise L.CvaeError(f"gradcam: two contiguous [B, n, 256] tensors of one dtype (fp32 or bf16) expected, got A {tuple(A.shape)} {A.dtype} and dA "
                          f"{tuple(dA.shape)} {dA.dtype}")
    B, n = A.shape[0], A.shape[1]
    if n > 4096:
        raise L.CvaeError(f"gradcam: at most 4096 positions per image (the map lives in LDS), got A {tuple(A.shape)}")
    cam = _empty((B, n), torch.float32, A)
    if B == 0:
        return cam
    check(lib.cvae_gradcam256(ptr(A), ptr(dA), ptr(cam), B, n, int(bool(normalize)), L.dtype_code(A.dtype), stream()), "gradcam")
    return cam


# ---- ViT-VAE decoder (csrc/conv_s1.hip): forward-only building blocks on raw tensors -------------------------------------------------
CONV_S1_K3, CONV_S1_SUBPIXEL, CONV_S1_SUBPIXEL_T = 0, 1, 2      # CVAE_CONV_S1_* (SUBPIXEL_T: conv_s1_bwd_data only)


def conv_s1_pack_weights(mats):
    """bf16 copies of up to 16 fp32 conv_s1 matrices (fold_bn_conv's FOLD_CONV_K3S1 / FOLD_CONVT_K3S2_SUBPIXEL outputs) in ONE launch
    (cvae_conv_s1_pack_weights); views of one fresh buffer."""
    import ctypes as C
    k = len(mats)
    if not 1 <= k <= 16:
        raise L.CvaeError(f"conv_s1_pack_weights: 1 to 16 matrices per launch, got {k}")
    L.require_gpu(*mats)
    _forward_only("conv_s1_pack_weights", *mats)
    if any(m.dtype != torch.float32 or not m.is_contiguous() or m.numel() % 8 for m in mats):
        raise L.CvaeError("conv_s1_pack_weights: contiguous fp32 matrices with a multiple of 8 elements expected")
    buf = torch.empty(sum(m.numel() for m in mats), dtype=torch.bfloat16, device=mats[0].device)
    outs, off = [], 0
    for m in mats:
        outs.append(buf[off:off + m.numel()].view(m.shape))
        off += m.numel()
    vp = lambda v: (C.c_void_p * k)(*v)
    check(lib.cvae_conv_s1_pack_weights(k, vp([m.data_ptr() for m in mats]), vp([o.data_ptr() for o in outs]), (C.c_int64 * k)(*[m.numel() for m in mats]), stream()),
          "conv_s1_pack_weights")
    return outs


def _cl_operand(what, x, form, forms):
    """x must be a contiguous channels-last [B, H, W, C] tensor and form one of `forms` (shared by the forward, input-gradient and weight-gradient wrappers)"""
    if x.dim() != 4 or not x.is_contiguous() or form not in forms:
        raise L.CvaeError(f"{what}: a contiguous channels-last [B, H, W, C] tensor expected, got {tuple(x.shape)} in form {form}")


def _like_operands(what, oshape, dtype, **tensors):
    """every tensor (name = tensor or None) must be contiguous, of shape oshape and of dtype"""
    for name, t in tensors.items():
        if t is not None and (tuple(t.shape) != tuple(oshape) or t.dtype != dtype or not t.is_contiguous()):
            raise L.CvaeError(f"{what}: the {name} must be a contiguous {tuple(oshape)} {dtype} tensor")


def _conv_s1_operands(what, x, wmat, form, forms, geom, **like_out):
    """The operand checks conv_s1 and conv_s1_bwd_data share: x a contiguous channels-last [B, H, W, C] tensor and form one of `forms`; wmat the matrix of
    the layer geom(B, H, W, C) -> (Cin, Cout, output shape) in x's dtype, contiguous, cvae_conv_s1_weight_elems long; every like_out tensor (name = tensor
    or None) contiguous, of the output's shape and x's dtype.  Returns geom's triple."""
    _cl_operand(what, x, form, forms)
    cin, cout, oshape = geom(*x.shape)
    n = lib.cvae_conv_s1_weight_elems(cin, cout, form)
    if n == 0:
        raise L.CvaeError(f"{what}: {cin} -> {cout} channels in form {form}: {L.strerror(-3)}")
    if wmat.dtype != x.dtype or wmat.numel() != n or not wmat.is_contiguous():
        raise L.CvaeError(f"{what}: weight matrix {tuple(wmat.shape)} {wmat.dtype} does not fit {cin} -> {cout} channels in {x.dtype} ({n} elements)")
    _like_operands(what, oshape, x.dtype, **like_out)
    return cin, cout, oshape


def conv_s1(x, wmat, bias, form, act=None, resid=None):
    """act(conv(x) + bias + resid) on a channels-last [B, H, W, Cin] tensor (cvae_conv_s1; fp32 or bf16 = the arithmetic mode).  form CONV_S1_K3:
    nn.Conv2d(C, C, 3, 1, 1), C in {32, 64, 128} -> [B, H, W, C]; CONV_S1_SUBPIXEL: nn.ConvTranspose2d(Cin, 16, 3, 2, 1, output_padding=1), Cin in {32, 16}
    -> [B, 2H, 2W, 16].  wmat: the matrix fold_bn_conv wrote for the layer, in x's dtype (conv_s1_pack_weights for bf16); bias fp32 [Cout];
    resid (optional): the output's shape and dtype, added in fp32 before the activation."""
    L.require_gpu(x, wmat, bias, resid)
    _forward_only("conv_s1", x, wmat, bias, resid)
    up = 2 if form == CONV_S1_SUBPIXEL else 1
    Cin, Cout, oshape = _conv_s1_operands("conv_s1", x, wmat, form, (CONV_S1_K3, CONV_S1_SUBPIXEL),
                                          lambda B, H, W, C: (C, bias.numel(), (B, up * H, up * W, bias.numel())), residual=resid)
    if bias.dtype != torch.float32:
        raise L.CvaeError(f"conv_s1: an fp32 bias expected, got {bias.dtype}")
    B, H, W, _C = x.shape
    y = _empty(oshape, x.dtype, x)
    check(lib.cvae_conv_s1(ptr(x), ptr(wmat), ptr(bias.detach().contiguous()), ptr(resid), ptr(y), B, H, W, Cin, Cout, form, L.dtype_code(x.dtype), L.act_code(act),
                           stream()), "conv_s1")
    return y


def conv_s1_c1(x, weight, bias, act=None):
    """nn.Conv2d(16, 1, 3, 1, 1) of a channels-last [B, H, W, 16] tensor (fp32 or bf16) with the fp32 module weight [1, 16, 3, 3] as it is
    -> fp32 [B, 1, H, W] (cvae_conv_s1_c1)."""
    L.require_gpu(x, weight, bias)
    _forward_only("conv_s1_c1", x, weight, bias)
    if x.dim() != 4 or not x.is_contiguous() or tuple(weight.shape) != (1, x.shape[3], 3, 3) or weight.dtype != torch.float32:
        raise L.CvaeError(f"conv_s1_c1: x {tuple(x.shape)}, weight {tuple(weight.shape)} {weight.dtype}")
    B, H, W, Cin = x.shape
    y = _empty((B, 1, H, W), torch.float32, x)
    check(lib.cvae_conv_s1_c1(ptr(x), ptr(weight.detach().contiguous()), ptr(bias.detach()) if bias is not None else None, ptr(y), B, H, W, Cin,
                              L.dtype_code(x.dtype), L.act_code(act), stream()), "conv_s1_c1")
    return y


def conv_s1_bwd_data(g, wmat, form, cin=None, resid=None, gate=None, gate_act=None):
    """(conv(g, w^T) + resid) * act'(gate): the input gradient of conv_s1's layer through a frozen weight (cvae_conv_s1_bwd_data), channels-last, fp32 or bf16.
    form CONV_S1_K3: g [B, H, W, C] -> [B, H, W, C] (no cin: it is C); CONV_S1_SUBPIXEL_T (the narrow transposed convs): g [B, 2H, 2W, 16] -> [B, H, W, cin],
    cin = the layer's input channels (32 or 16: the matrix has 32 rows either way).  wmat: the third element fold_bn_conv returns for a FOLD_*_GRAD entry, in g's
    dtype.  resid / gate (optional): the result's shape and dtype; gate is the OUTPUT of the activation whose derivative is applied (LeakyReLU keeps the sign):
    gate > 0 ? 1 : slope."""
    L.require_gpu(g, wmat, resid, gate)
    _forward_only("conv_s1_bwd_data", g, wmat, resid, gate)
    sub = form == CONV_S1_SUBPIXEL_T
    if sub != (cin is not None):
        raise L.CvaeError(f"conv_s1_bwd_data: cin goes with form CONV_S1_SUBPIXEL_T and with no other, got cin={cin} in form {form}")
    C, _Cout, oshape = _conv_s1_operands("conv_s1_bwd_data", g, wmat, form, (CONV_S1_K3, CONV_S1_SUBPIXEL_T),
                                         lambda B, H, W, Cg: (int(cin), 16, (B, H // 2, W // 2, int(cin))) if sub else (Cg, Cg, (B, H, W, Cg)),
                                         residual=resid, gate=gate)
    if sub and (g.shape[3] != 16 or g.shape[1] % 2 or g.shape[2] % 2):
        raise L.CvaeError(f"conv_s1_bwd_data: the sub-pixel form takes a [B, 2H, 2W, 16] gradient, got {tuple(g.shape)}")
    if (gate is None) != (gate_act in (None, "none")):
        raise L.CvaeError("conv_s1_bwd_data: gate and gate_act come together")
    B, H, W, _C = oshape
    dx = _empty(oshape, g.dtype, g)
    check(lib.cvae_conv_s1_bwd_data(ptr(g), ptr(wmat), ptr(resid), ptr(gate), ptr(dx), B, H, W, C, form, L.dtype_code(g.dtype), L.act_code(gate_act), stream()),
          "conv_s1_bwd_data")
    return dx


def conv_s1_c1_bwd_data(g, weight, gate, gate_act, out_dtype):
    """The input gradient of nn.Conv2d(16, 1, 3, 1, 1) (cvae_conv_s1_c1_bwd_data): g fp32 [B, 1, H, W], the fp32 module weight as it is -> channels-last
    [B, H, W, 16] in out_dtype, times act'(gate) (gate: the conv's input, [B, H, W, 16] in out_dtype, or None)."""
    L.require_gpu(g, weight, gate)
    _forward_only("conv_s1_c1_bwd_data", g, weight, gate)
    if g.dim() != 4 or g.shape[1] != 1 or g.dtype != torch.float32 or tuple(weight.shape) != (1, 16, 3, 3) or weight.dtype != torch.float32:
        raise L.CvaeError(f"conv_s1_c1_bwd_data: g {tuple(g.shape)} {g.dtype}, weight {tuple(weight.shape)} {weight.dtype}")
    B, _one, H, W = g.shape
    if gate is not None and (tuple(gate.shape) != (B, H, W, 16) or gate.dtype != out_dtype or not gate.is_contiguous()):
        raise L.CvaeError(f"conv_s1_c1_bwd_data: the gate must be a contiguous {(B, H, W, 16)} {out_dtype} tensor")
    if (gate is None) != (gate_act in (None, "none")):
        raise L.CvaeError("conv_s1_c1_bwd_data: gate and gate_act come together")
    dx = _empty((B, H, W, 16), out_dtype, g)
    check(lib.cvae_conv_s1_c1_bwd_data(ptr(g.contiguous()), ptr(weight.detach().contiguous()), ptr(gate), ptr(dx), B, H, W, 16, L.dtype_code(out_dtype),
                                       L.act_code(gate_act), stream()), "conv_s1_c1_bwd_data")
    return dx


LATENT_TO_GRID_ROWS = 16     # batch rows per cvae_latent_to_grid launch


def latent_to_grid_bwd(g, weight):
    """dz [B, K] fp32 = the gradient of latent_to_grid with respect to z: sum over (p, c) of g[b][p][c] weight[c P + p][k] (cvae_latent_to_grid_bwd).
    g: channels-last [B, P, C] fp32 or bf16; weight the fp32 nn.Linear tensor [C P, K], read once per launch of up to 16 rows."""
    L.require_gpu(g, weight)
    _forward_only("latent_to_grid_bwd", g, weight)
    if g.dim() != 3 or not g.is_contiguous() or weight.dim() != 2 or weight.dtype != torch.float32 or weight.shape[0] != g.shape[1] * g.shape[2]:
        raise L.CvaeError(f"latent_to_grid_bwd: g {tuple(g.shape)}, weight {tuple(weight.shape)} {weight.dtype}")
    B, P, C = g.shape
    K = weight.shape[1]
    w = weight.detach().contiguous()
    dz = _empty((B, K), torch.float32, g)
    for b0 in range(0, B, LATENT_TO_GRID_ROWS):
        nb = min(LATENT_TO_GRID_ROWS, B - b0)
        nbytes = lib.cvae_latent_to_grid_bwd_workspace_bytes(nb, K, P, C)
        if not nbytes:
            raise L.CvaeError(f"latent_to_grid_bwd: K {K}, P {P}, C {C}: {L.strerror(-3)}")
        _t, wp, wb = _scratch(nbytes, g)
        check(lib.cvae_latent_to_grid_bwd(ptr(g[b0:]), ptr(w), ptr(dz[b0:]), nb, K, P, C, L.dtype_code(g.dtype), wp, wb, stream()), "latent_to_grid_bwd")
    return dz


def latent_to_grid(z, weight, bias, channels, out_dtype):
    """nn.Linear(K, channels * P)(z).view(B, channels, gh, gw) written channels-last: [B, P, channels] in out_dtype (cvae_latent_to_grid).  z fp32 [B, K];
    weight / bias the fp32 nn.Linear tensors, read as they are; products and sums fp32.  Batches above 16 rows run as several launches."""
    L.require_gpu(z, weight, bias)
    _forward_only("latent_to_grid", z, weight, bias)
    _rows2d(z, "latent_to_grid")
    B, K = z.shape
    if z.dtype != torch.float32 or weight.dtype != torch.float32 or weight.dim() != 2 or weight.shape[1] != K or weight.shape[0] % channels:
        raise L.CvaeError(f"latent_to_grid: z {tuple(z.shape)} {z.dtype}, weight {tuple(weight.shape)}, channels {channels}")
    P = weight.shape[0] // channels
    z, w, b = z.contiguous(), weight.detach().contiguous(), (bias.detach().contiguous() if bias is not None else None)
    out = _empty((B, P, channels), out_dtype, z)
    for b0 in range(0, max(B, 1), LATENT_TO_GRID_ROWS):
        nb = min(LATENT_TO_GRID_ROWS, B - b0)
        check(lib.cvae_latent_to_grid(ptr(z[b0:]), ptr(w), ptr(b), ptr(out[b0:]), nb, K, P, channels, L.dtype_code(out_dtype), stream()), "latent_to_grid")
    return out


# ---- the decoder's weight gradients (eval-mode BatchNorm): fp32 results, fixed-order sums, B >= 1 ------------------------------------------
def _wgrad_operands(what, x, form, forms, gshape, gdtype=None):
    """_conv_s1_operands' checks for a weight gradient (there is no weight matrix to check): x a contiguous channels-last [B, H, W, C] fp32 or bf16 tensor with
    B >= 1, form one of `forms`, and the cotangent g contiguous, of shape gshape(B, H, W, C) and of x's dtype (gdtype: another one)."""
    _cl_operand(what, x, form, forms)
    if x.shape[0] < 1 or x.dtype not in (torch.float32, torch.bfloat16):
        raise L.CvaeError(f"{what}: B >= 1 rows in float32 or bfloat16 expected, got {tuple(x.shape)} {x.dtype}")
    return lambda g: _like_operands(what, gshape(*x.shape), gdtype or x.dtype, cotangent=g)


def conv_s1_wgrad(x, g, form):
    """(dW, dbias) fp32 of conv_s1's layer from its input x [B, H, W, C] and the (already gated) cotangent g of its pre-activation (cvae_conv_s1_wgrad).
    form CONV_S1_K3: nn.Conv2d(C, C, 3, 1, 1), C in {16, 32, 64, 128}, g [B, H, W, C] -> dW [C, C, 3, 3]; CONV_S1_SUBPIXEL: nn.ConvTranspose2d(C, 16, 3, 2, 1,
    output_padding=1), C in {32, 16}, g [B, 2H, 2W, 16] -> dW [C, 16, 3, 3].  The gradient of the weight the conv ran with (the folded one), torch layout."""
    L.require_gpu(x, g)
    _forward_only("conv_s1_wgrad", x, g)
    sub = form == CONV_S1_SUBPIXEL
    _wgrad_operands("conv_s1_wgrad", x, form, (CONV_S1_K3, CONV_S1_SUBPIXEL), lambda B, H, W, Cc: (B, 2 * H, 2 * W, 16) if sub else (B, H, W, Cc))(g)
    B, H, W, Cc = x.shape
    nbytes = lib.cvae_conv_s1_wgrad_workspace_bytes(B, H, W, Cc, form)
    if not nbytes:
        raise L.CvaeError(f"conv_s1_wgrad: {Cc} channels in form {form} on {B} x {H} x {W}: {L.strerror(-3)}")
    dW = _empty((Cc, 16 if sub else Cc, 3, 3), torch.float32, x)
    db = _empty((16 if sub else Cc,), torch.float32, x)
    _t, wp, wb = _scratch(nbytes, x)
    check(lib.cvae_conv_s1_wgrad(ptr(x), ptr(g), ptr(dW), ptr(db), B, H, W, Cc, form, L.dtype_code(x.dtype), wp, wb, stream()), "conv_s1_wgrad")
    return dW, db


def conv_s1_c1_wgrad(x, g):
    """(dW [1, 16, 3, 3], dbias [1]) fp32 of nn.Conv2d(16, 1, 3, 1, 1) from its channels-last input x [B, H, W, 16] (fp32 or bf16) and the fp32 image
    cotangent g [B, 1, H, W] (cvae_conv_s1_c1_wgrad)."""
    L.require_gpu(x, g)
    _forward_only("conv_s1_c1_wgrad", x, g)
    _wgrad_operands("conv_s1_c1_wgrad", x, CONV_S1_K3, (CONV_S1_K3,), lambda B, H, W, Cc: (B, 1, H, W), torch.float32)(g)
    B, H, W, Cc = x.shape
    if Cc != 16:
        raise L.CvaeError(f"conv_s1_c1_wgrad: 16 input channels expected, got {tuple(x.shape)}: {L.strerror(-3)}")
    dW, db = _empty((1, 16, 3, 3), torch.float32, x), _empty((1,), torch.float32, x)
    _t, wp, wb = _scratch(lib.cvae_conv_s1_c1_wgrad_workspace_bytes(B, H, W), x)
    check(lib.cvae_conv_s1_c1_wgrad(ptr(x), ptr(g), ptr(dW), ptr(db), B, H, W, 16, L.dtype_code(x.dtype), wp, wb, stream()), "conv_s1_c1_wgrad")
    return dW, db


def latent_to_grid_wgrad(g, z):
    """(dW [C P, K], dbias [C P]) fp32 of latent_to_grid's nn.Linear: dW[c P + p][k] = sum_b g[b][p][c] z[b][k], rows in order (cvae_latent_to_grid_wgrad).
    g: channels-last [B, P, C] fp32 or bf16 (the grid gradient as the backward chain holds it); z fp32 [B, K].  One launch for any B >= 1."""
    L.require_gpu(g, z)
    _forward_only("latent_to_grid_wgrad", g, z)
    if (g.dim() != 3 or not g.is_contiguous() or g.shape[0] < 1 or g.dtype not in (torch.float32, torch.bfloat16) or z.dim() != 2 or z.dtype != torch.float32
            or z.shape[0] != g.shape[0]):
        raise L.CvaeError(f"latent_to_grid_wgrad: g {tuple(g.shape)} {g.dtype}, z {tuple(z.shape)} {z.dtype}")
    B, P, Cc = g.shape
    K = z.shape[1]
    if K > 512 or K % 4 or Cc % 32:                                  # cvae_latent_to_grid's limits
        raise L.CvaeError(f"latent_to_grid_wgrad: K {K}, C {Cc}: K <= 512, K % 4 == 0 and C % 32 == 0 expected: {L.strerror(-3)}")
    dW, db = _empty((Cc * P, K), torch.float32, g), _empty((Cc * P,), torch.float32, g)
    check(lib.cvae_latent_to_grid_wgrad(ptr(g), ptr(z.contiguous()), ptr(dW), ptr(db), B, K, P, Cc, L.dtype_code(g.dtype), stream()), "latent_to_grid_wgrad")
    return dW, db


def fold_bn_conv_bwd(entries):
    """The way back through fold_bn_conv for up to 16 layers in ONE launch (cvae_fold_bn_conv_bwd).  entries: (weight, kind, bias, bn, dwf, dbf) with kind
    FOLD_CONVT_K3S2 (dwf: the gradient of the k4 weight [Cin, Cout, 4, 4]), FOLD_CONV_K3S1 (dwf [Cout, Cin, 3, 3]), FOLD_CONVT_K3S2_SUBPIXEL (dwf [Cin, Cout, 3, 3])
    or FOLD_CONV_K3S2 (the ViT-VAE stem; dwf: the gradient of the k4 weight [Cout, Cin, 4, 4] as _conv_wgrad writes it, fourth row and column ignored; any Cin),
    dbf the folded bias's gradient [Cout], bn an eval-mode nn.BatchNorm2d (running statistics are constants).  Returns [(dw, db, dgamma, dbeta)] fp32, each of
    its parameter's shape: dw = s dwf, db = s dbf, dgamma = rstd (sum dwf w + dbf (bias - mean)), dbeta = dbf with s = gamma rstd."""
    import ctypes as C
    k = len(entries)
    if not 1 <= k <= 16:
        raise L.CvaeError(f"fold_bn_conv_bwd: 1 to 16 layers per launch, got {k}")
    rows, outs = [], []
    for w, kind, bias, bn, dwf, dbf in entries:
        L.require_gpu(w, bias, dwf, dbf)
        _forward_only("fold_bn_conv_bwd", w, bias, dwf, dbf, bn.weight, bn.bias)
        if kind not in (FOLD_CONVT_K3S2, FOLD_CONV_K3S1, FOLD_CONVT_K3S2_SUBPIXEL, FOLD_CONV_K3S2) or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
            raise L.CvaeError(f"fold_bn_conv_bwd: kind {kind} does not match a weight of shape {tuple(w.shape)}")
        cout, cin = (w.shape[1], w.shape[0]) if kind in _FOLD_CONVT else (w.shape[0], w.shape[1])
        want = tuple(w.shape[:2]) + ((4, 4) if kind in (FOLD_CONVT_K3S2, FOLD_CONV_K3S2) else (3, 3))
        if (tuple(dwf.shape) != want or tuple(dbf.shape) != (cout,) or dwf.dtype != torch.float32 or dbf.dtype != torch.float32 or not dwf.is_contiguous()
                or bias is None or bn.running_mean is None or bn.weight is None or bn.num_features != cout):
            raise L.CvaeError(f"fold_bn_conv_bwd: kind {kind}, weight {tuple(w.shape)}: gradients {tuple(dwf.shape)} / {tuple(dbf.shape)} (fp32 {want} / ({cout},) "
                              "expected), a conv bias and an affine BatchNorm2d with running statistics")
        f32 = lambda t: t.detach().float().contiguous()
        rows.append((f32(w), kind, cout, cin, f32(bias), f32(bn.weight), f32(bn.running_mean), f32(bn.running_var), float(bn.eps), dwf, dbf.contiguous()))
        outs.append((torch.empty_like(rows[-1][0]), _empty((cout,), torch.float32, w), _empty((cout,), torch.float32, w), _empty((cout,), torch.float32, w)))
    vp = lambda v: (C.c_void_p * k)(*[t.data_ptr() for t in v])
    col = lambda i: [r[i] for r in rows]
    check(lib.cvae_fold_bn_conv_bwd(k, vp(col(0)), (C.c_int * k)(*col(1)), (C.c_int64 * (2 * k))(*[d for r in rows for d in (r[2], r[3])]), vp(col(4)), vp(col(5)),
                                    vp(col(6)), vp(col(7)), (C.c_float * k)(*col(8)), vp(col(9)), vp(col(10)), vp([o[0] for o in outs]), vp([o[1] for o in outs]),
                                    vp([o[2] for o in outs]), vp([o[3] for o in outs]), stream()), "fold_bn_conv_bwd")
    return outs


# ---- The dense heads of CausalViTVAE (csrc/heads.hip): a whole head in one launch ----------------------------------------------------
def _heads_rows(t):
    """t [B, w] as the heads kernel addresses it (ptr + row * stride + col): unit column stride and rows that do not overlap.  A column slice of a wider
    matrix qualifies as it is; an expanded row (stride 0) or a transposed view is copied once."""
    return t if t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


class _HeadsCall:
    """The C structures of one head and the tensors that keep their pointers alive.  what: the caller's name in error messages.  Eval (train=False)
    is forward-only, reads detached fp32 contiguous copies of the parameters and needs running statistics; training reads the parameters in place
    (contiguous fp32, a float momentum), refuses a decorated last layer and batch statistics of one row, and records what may ask for a gradient."""

    __slots__ = ("B", "N", "split", "panels", "pan", "rows", "bn_rows", "params", "slots", "keep", "widths", "bn_flags", "eps", "eps_stride", "clamp0", "clamp1")

    def __init__(self, what, train, panels, layers, split, clamp0, clamp1, eps):
        import ctypes as C
        if not 1 <= len(panels) <= L.HEADS_MAX_PANELS or not 1 <= len(layers) <= L.HEADS_MAX_LAYERS:
            raise L.CvaeError(f"{what}: 1..{L.HEADS_MAX_PANELS} input panels and 1..{L.HEADS_MAX_LAYERS} layers, got {len(panels)} and {len(layers)}: {L.strerror(-3)}")
        if any(t.dim() != 2 for t in panels):
            raise L.CvaeError(f"{what}: every panel must be a [B, w] matrix, got shapes {[tuple(t.shape) for t in panels]}")
        B = self.B = panels[0].shape[0]
        for t in panels:
            if t.dtype != torch.float32 or t.shape[0] != B or t.shape[1] < 1:
                rows = f"{B} rows" if train else f"{B} rows (the first panel's)"
                raise L.CvaeError(f"{what}: every panel must be float32 with {rows} and at least one column, got {tuple(t.shape)} {t.dtype}")
        self.panels = [_heads_rows(t.detach() if train else t) for t in panels]
        K = width = sum(t.shape[1] for t in self.panels)
        self.rows = (L.HeadsLayer * len(layers))()
        self.bn_rows = (L.HeadsBnTrain * len(layers))() if train else None
        # params: the tensors that may ask for a gradient; slots: (layer, HeadsLayerGrad field) of each; keep: eval's copies, alive until the call is enqueued
        self.params, self.slots, self.keep = [], [], []
        self.widths, self.bn_flags = [], []
        if not train:
            L.require_gpu(*self.panels)
            _forward_only(what, *panels)
        for i, (lin, bn, slope) in enumerate(layers):
            pair = lin if isinstance(lin, (tuple, list)) else (lin,)
            last = i == len(layers) - 1
            if len(pair) > 2 or (len(pair) == 2 and not last):
                raise L.CvaeError(f"{what}: only the last layer may be held by two nn.Linear modules")
            if train and last and (bn is not None or slope is not None):
                raise L.CvaeError(f"{what}: the last layer is a plain Linear: {L.strerror(-3)}")
            ts = [t for p in pair for t in (p.weight, p.bias)]
            if not train:
                L.require_gpu(*ts)
                _forward_only(what, *ts)
            if any(p.weight.dtype != torch.float32 or p.weight.dim() != 2 or p.weight.shape[1] != width or p.bias is None or (train and not p.weight.is_contiguous()) for p in pair):
                raise L.CvaeError(f"{what}: layer {i} must be {'contiguous ' if train else ''}fp32 nn.Linear({width}, n) with a bias, got weights {[tuple(p.weight.shape) for p in pair]}")
            if train:
                self.params += ts
                self.slots += [(i, f) for f in ("dW", "db", "dW2", "db2")[:len(ts)]]
            else:
                ts = [t.detach().contiguous() for t in ts]
                self.keep += ts
            r, ptrs = self.rows[i], [t.data_ptr() for t in ts]
            r.W, r.b, r.out_first = ptrs[0], ptrs[1], pair[0].weight.shape[0]
            r.out = sum(p.weight.shape[0] for p in pair)
            if len(pair) == 2:
                r.W2, r.b2 = ptrs[2:]
            if bn is not None and train:
                if bn.weight is None or bn.num_features != r.out or bn.weight.dtype != torch.float32 or (bn.momentum is None and bn.track_running_stats):
                    raise L.CvaeError(f"{what}: layer {i}'s BatchNorm1d needs fp32 affine parameters, {r.out} features and a float momentum")
                if B < 2:
                    raise L.CvaeError(f"{what}: batch statistics need more than one row, got {B}: {L.strerror(-1)}")
                r.bn_weight, r.bn_bias, r.bn_eps = bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps)
                if bn.track_running_stats:
                    L.require_gpu(bn.running_mean)
                    s = self.bn_rows[i]
                    s.running_mean, s.running_var, s.num_batches_tracked = bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr()
                    s.momentum = float(bn.momentum)
                self.params += [bn.weight, bn.bias]
                self.slots += [(i, "dgamma"), (i, "dbeta")]
            elif bn is not None:
                if bn.running_var is None or bn.weight is None or bn.num_features != r.out:
                    raise L.CvaeError(f"{what}: layer {i}'s BatchNorm1d needs running statistics, an affine weight and {r.out} features")
                bts = [t.detach().float().contiguous() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)]
                L.require_gpu(*bts)
                self.keep += bts
                r.bn_weight, r.bn_bias, r.bn_mean, r.bn_var = (t.data_ptr() for t in bts)
                r.bn_eps = float(bn.eps)
            if slope is not None:
                r.leaky, r.slope = 1, float(slope)
            width = r.out
            self.widths.append(width)
            self.bn_flags.append(bn is not None)
        if train:
            L.require_gpu(*self.params, *self.panels)
        if K > L.HEADS_MAX_WIDTH or any(w > L.HEADS_MAX_WIDTH for w in self.widths):
            raise L.CvaeError(f"{what}: input width {K} / layer widths {self.widths} above {L.HEADS_MAX_WIDTH}: {L.strerror(-3)}")
        N = self.N = width
        self.split = self.rows[len(layers) - 1].out_first if split is None else split
        if not 1 <= self.split <= N:
            raise L.CvaeError(f"{what}: split {self.split} outside 1..{N}")
        self.eps = None
        if eps is not None:
            L.require_gpu(eps)
            if N != 2 * self.split or eps.dtype != torch.float32 or tuple(eps.shape) != (B, self.split):
                raise L.CvaeError(f"{what}: eps must be fp32 [{B}, {self.split}] and the head's width 2 * split, got {tuple(eps.shape)} {eps.dtype}, width {N}")
            self.eps = _heads_rows(eps.detach() if train else eps)
        self.pan = (L.HeadsPanel * len(self.panels))(*[L.HeadsPanel(t.data_ptr(), t.shape[1], max(t.stride(0), t.shape[1])) for t in self.panels])
        cl = lambda c: None if c is None else (C.c_float * 2)(float(c[0]), float(c[1]))
        self.clamp0, self.clamp1 = cl(clamp0), cl(clamp1)
        self.eps_stride = max(self.eps.stride(0), self.split) if self.eps is not None else 0

    def outputs(self):
        """first [B, split], second [B, N - split] or None, z [B, split] or None (with eps)"""
        like, B, S, N = self.panels[0], self.B, self.split, self.N
        return (_empty((B, S), torch.float32, like), _empty((B, N - S), torch.float32, like) if S < N else None,
                _empty((B, S), torch.float32, like) if self.eps is not None else None)


def mlp_heads(panels, layers, split=None, clamp0=None, clamp1=None, eps=None):
    """One fused head (cvae_mlp_heads_fwd), fp32, forward-only.
    panels  1..3 fp32 [B, w_i] matrices; the head reads torch.cat(panels, 1) without building it.  A panel with unit column stride and a row stride of
            at least its width (a column slice of a wider matrix) is read in place; any other view (an expanded row, a transpose) is copied first.
    layers  1..3 entries (linear, bn, slope): linear = an nn.Linear, or — last layer only — a pair of nn.Linear holding the first and second
            group of output columns (read from the two weight tensors, no stacked copy); bn = an nn.BatchNorm1d applied on its running
            statistics, read on every call, or None; slope = the LeakyReLU slope applied after it, or None.
    split   output columns [0, split) form the first result, [split, N) the second (default: the first linear's width of a pair, else N: one result)
    clamp0 / clamp1  (lo, hi) of torch.clamp for the two results, or None
    eps     [B, split] fp32, read in place or copied by the same rule as a panel: also returns z = first + eps * exp(0.5 * second) from the clamped values (needs N == 2 split)
    Returns (first, second or None, z or None)."""
    c = _HeadsCall("mlp_heads", False, panels, layers, split, clamp0, clamp1, eps)
    first, second, z = c.outputs()
    check(lib.cvae_mlp_heads_fwd(c.pan, len(c.panels), c.rows, len(c.rows), c.split, c.clamp0, c.clamp1, ptr(c.eps), c.eps_stride,
                                 ptr(first), c.split, ptr(second), c.N - c.split, ptr(z), c.split, c.B, stream()), "mlp_heads")
    return first, second, z


# ---- The same heads in training mode (cvae_mlp_heads_train_fwd / cvae_mlp_heads_bwd) ------------------------------------------------------
def heads_saved_layout(widths, bn_flags, B):
    """name -> (offset, shape) in floats of what cvae_mlp_heads_train_fwd leaves in its `saved` buffer (include/cvae_hip.h): per hidden layer l `mean{l}`,
    `rstd{l}`, `xhat{l}` (BatchNorm layers), `pre{l}` (the pre-LeakyReLU value), `act{l}`; then `preclamp`.  widths: every layer's `out`."""
    out, o = {}, 0
    for l, n in enumerate(widths[:-1]):
        if bn_flags[l]:
            out[f"mean{l}"], out[f"rstd{l}"], out[f"xhat{l}"] = (o, (n,)), (o + n, (n,)), (o + 2 * n, (B, n))
            o += 2 * n + B * n
        out[f"pre{l}"], out[f"act{l}"] = (o, (B, n)), (o + B * n, (B, n))
        o += 2 * B * n
    out["preclamp"] = (o, (B, widths[-1]))
    return out, o + B * widths[-1]


class _MlpHeadsTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, call, collect, *tensors):
        c, B, S, N = call, call.B, call.split, call.N
        like = c.panels[0]
        first, second, z = c.outputs()
        layout, total = heads_saved_layout(c.widths, c.bn_flags, B)
        if B and lib.cvae_mlp_heads_train_workspace_bytes(c.pan, len(c.panels), c.rows, len(c.rows), B) != 4 * total:
            raise L.CvaeError("mlp_heads_train: heads_saved_layout and cvae_mlp_heads_train_workspace_bytes disagree")
        saved = _empty((max(total, 1),), torch.float32, like)
        check(lib.cvae_mlp_heads_train_fwd(c.pan, len(c.panels), c.rows, len(c.rows), c.bn_rows, S, c.clamp0, c.clamp1, ptr(c.eps), c.eps_stride,
                                           ptr(first), S, ptr(second), N - S, ptr(z), S, B, ptr(saved), 4 * total, stream()), "mlp_heads_train")
        if collect is not None:
            for k, (o, shape) in layout.items():
                collect[k] = saved[o:o + math.prod(shape)].view(shape)
        ctx.call, ctx.saved, ctx.total = c, saved, total
        ctx.save_for_backward(*tensors)             # the kernels read panels and parameters through raw pointers: autograd's version check guards them
        ctx.set_materialize_grads(False)
        return first, second, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g0, g1, gz):
        import ctypes as C
        ctx.saved_tensors                           # raises if a panel or parameter was modified in place since the forward
        c, B, S, N = ctx.call, ctx.call.B, ctx.call.split, ctx.call.N
        like, np_ = c.panels[0], len(c.panels)
        grads = (L.HeadsLayerGrad * len(c.rows))()
        outs = []
        for p, (l, field) in zip(c.params, c.slots):
            t = torch.empty_like(p, memory_format=torch.contiguous_format)
            setattr(grads[l], field, t.data_ptr())
            outs.append(t)
        pg = [_empty(tuple(t.shape), torch.float32, like) if ctx.needs_input_grad[2 + i] else None for i, t in enumerate(c.panels)]
        pgp = (C.c_void_p * np_)(*[ptr(t) for t in pg])
        pgs = (C.c_int64 * np_)(*[t.shape[1] for t in c.panels])
        cot = [None if g is None else _heads_rows(g.float()) for g in (g0, g1, gz)]
        cs = [0 if g is None else max(g.stride(0), g.shape[1]) for g in cot]
        nbytes = lib.cvae_mlp_heads_bwd_workspace_bytes(c.pan, np_, c.rows, len(c.rows), B)
        _t, wp, wb = _scratch(nbytes, like)
        check(lib.cvae_mlp_heads_bwd(c.pan, np_, pgp, pgs, c.rows, len(c.rows), grads, S, c.clamp0, c.clamp1, ptr(c.eps), c.eps_stride, ptr(cot[0]), cs[0],
                                     ptr(cot[1]), cs[1], ptr(cot[2]), cs[2], B, ptr(ctx.saved), 4 * ctx.total, wp, wb, stream()), "mlp_heads_bwd")
        if B == 0:
            outs = [torch.zeros_like(t) for t in outs]
        need = ctx.needs_input_grad[2 + np_:]
        return (None, None, *pg, *[t if n else None for t, n in zip(outs, need)])


def mlp_heads_train(panels, layers, split=None, clamp0=None, clamp1=None, eps=None, collect=None):
    """ops.mlp_heads in TRAINING mode, differentiable (cvae_mlp_heads_train_fwd / cvae_mlp_heads_bwd; once_differentiable): a BatchNorm1d layer normalises with
    the statistics of this batch and its running_mean, running_var and num_batches_tracked are updated in place, as torch does (unbiased variance, float
    momentum).  Same arguments as mlp_heads; the last layer is a plain Linear (or pair).  Returns (first, second or None, z or None) as outputs of one
    autograd.Function: gradients go to the Linear and BatchNorm1d parameters that require grad and to the panels that require grad (eps gets none).
    collect (a dict, for tests): receives views of the saved buffer by heads_saved_layout's names: mean{l}, rstd{l}, xhat{l}, pre{l} (the pre-LeakyReLU
    values), act{l}, preclamp (the last layer's output before the clamps)."""
    call = _HeadsCall("mlp_heads_train", True, panels, layers, split, clamp0, clamp1, eps)
    return _MlpHeadsTrain.apply(call, collect, *panels, *call.params)


# ---- the latent translator (csrc/ridge.hip): float64 throughout ----
class _Result:
    """what an analysis call returns: the fields a subclass names in __slots__, every one of them given by keyword"""
    __slots__ = ()

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


class RidgeFit(_Result):
    """What ridge_fit_loo returns: coef [F, d], intercept [F], fitted [N, F], loo [N, F] (the leave-one-out predictions), leverage [N], r2 [F], corr [F]:
    float64 device tensors; info: the Cholesky's status (0: factorised)."""
    __slots__ = ("coef", "intercept", "fitted", "loo", "leverage", "r2", "corr", "info")


def _got(x):
    """what a refusal says it was handed: a tensor's shape and dtype, anything else's type"""
    return f"{tuple(x.shape)} {x.dtype}" if torch.is_tensor(x) else type(x).__name__


def _f64c(t):
    """detached, float64 (widening float32 is exact), contiguous"""
    return t.detach().double().contiguous()


def _f64_like(like):
    """new(*shape): an uninitialised float64 tensor on like's device"""
    return lambda *shape: _empty(shape, torch.float64, like)


def _f64_rows(what, name, t, cols=None):
    """a float64 matrix with contiguous rows -> its row stride in elements"""
    if t.dim() != 2 or t.dtype != torch.float64 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise L.CvaeError(f"{what}: {name} must be a float64 matrix with contiguous rows, got {tuple(t.shape)} {t.dtype} strides {tuple(t.stride())}")
    if cols is not None and t.shape[1] != cols:
        raise L.CvaeError(f"{what}: {name} must have {cols} columns, got {tuple(t.shape)}")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _f64_ws(nbytes, like):
    t = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=like.device)
    return t, t.data_ptr(), nbytes


def col_means_f64(x):
    """Column means of a float64 matrix with contiguous rows (cvae_col_means_f64): per-chunk sums in row order, the chunks added in order."""
    zs = _f64_rows("col_means_f64", "x", x)
    N, Cc = x.shape
    if N < 1 or Cc < 1:
        raise L.CvaeError(f"col_means_f64: a non-empty matrix expected, got {tuple(x.shape)}")
    L.require_gpu(x)
    mean = _empty((Cc,), torch.float64, x)
    _t, wp, wb = _f64_ws(lib.cvae_col_means_f64_workspace_bytes(N, Cc), x)
    check(lib.cvae_col_means_f64(ptr(x), N, Cc, zs, ptr(mean), wp, wb, stream()), "col_means_f64")
    return mean


def ranking_stats_f64(Y, P):
    """(r2 [F], corr [F]) of the predictions P against the truth Y, both float64 [N, F] (cvae_ranking_stats_f64): the rules of the reference's
    latent_translator/analysis.py:55-68, sklearn's r2 for a constant truth and a correlation of 0 below a standard deviation of 1e-12 included."""
    ys, ps = _f64_rows("ranking_stats_f64", "Y", Y), _f64_rows("ranking_stats_f64", "P", P, cols=Y.shape[1])
    N, F = Y.shape
    if P.shape[0] != N or N < 1 or F < 1:
        raise L.CvaeError(f"ranking_stats_f64: two non-empty matrices of one shape expected, got {tuple(Y.shape)} and {tuple(P.shape)}")
    L.require_gpu(Y, P)
    r2, corr = _empty((F,), torch.float64, Y), _empty((F,), torch.float64, Y)
    check(lib.cvae_ranking_stats_f64(ptr(Y), ys, ptr(P), ps, N, F, ptr(r2), ptr(corr), stream()), "ranking_stats_f64")
    return r2, corr


def _ridge_shapes(what, Z, M, limit):
    """the refusals of ridge_fit_loo and ridge_loo_path for the shapes and dtypes, none of which needs a device; limit: whose bound d <= 1024 is -> (N, d, F)"""
    if Z.dim() != 2 or M.dim() != 2:
        raise L.CvaeError(f"{what}: Z [N, d] and M [N, F] expected, got {tuple(Z.shape)} and {tuple(M.shape)}")
    if Z.dtype not in (torch.float32, torch.float64):
        raise L.CvaeError(f"{what}: Z must be float32 or float64, got {Z.dtype}")
    N, d = Z.shape
    F = M.shape[1]
    if M.shape[0] != N:
        raise L.CvaeError(f"{what}: Z has {N} rows, M has {M.shape[0]}")
    if N < 2:
        raise L.CvaeError(f"{what}: at least 2 samples expected (leave-one-out leaves N - 1), got N = {N}")
    if d < 1 or d > 1024:
        raise L.CvaeError(f"{what}: 1 <= d <= 1024 latent dimensions expected ({limit}), got d = {d}")
    if F < 1:
        raise L.CvaeError(f"{what}: at least one feature column expected, got M {tuple(M.shape)}")
    return N, d, F


def _ridge_alpha(what, name, a):
    """a (a Python float), or CvaeError unless it is positive and finite; name: 'alpha' or 'every alpha', how the message begins"""
    if not (a > 0.0 and math.isfinite(a)):
        raise L.CvaeError(f"{what}: {name} must be positive and finite (the centred Gram matrix is singular without it), got {a}")
    return a


def ridge_fit_loo(Z, M, alpha):
    """The Ridge translator Z [N, d] -> M [N, F] with an unpenalised intercept (sklearn's Ridge(alpha, fit_intercept=True)) and its EXACT leave-one-out
    predictions from one Cholesky factorisation (the reference refits N times, latent_translator/analysis.py:36-48), all in float64 on the device:
    column means, the centred Gram matrix A = Xc^T Xc + alpha I on the fp64 MFMA, A = L L^T, T = L^-1 Xc^T (the leverages h = 1 / N + column norms of T),
    W = A^-1 Xc^T Yc by two more solves, then fitted = mbar + Xc W, loo = M - (M - fitted) / (1 - h) and the ranking statistics of loo against M.
    Z: float32 or float64 (float32 is widened with .double(), which is exact); M is converted to float64.  Returns a RidgeFit.  The one host read is the
    Cholesky's info, at the end: non-zero (a pivot <= 0 or NaN, e.g. a NaN in Z) is a CvaeError naming the column."""
    what = "ridge_fit_loo"
    N, d, F = _ridge_shapes(what, Z, M, "the blocked Cholesky's limit")
    alpha = _ridge_alpha(what, "alpha", float(alpha))
    L.require_gpu(Z, M)
    Z, M = _f64c(Z), _f64c(M)
    zs, ms = _f64_rows(what, "Z", Z), _f64_rows(what, "M", M)
    zbar, mbar = col_means_f64(Z), col_means_f64(M)
    new = _f64_like(Z)
    A, R = new(d, d), new(d, F)
    _t, wp, wb = _f64_ws(lib.cvae_ridge_gram_f64_workspace_bytes(N, d, F), Z)
    check(L.timed(f"ridge_gram N{N} d{d} F{F}", lib.cvae_ridge_gram_f64, ptr(Z), zs, ptr(zbar), ptr(M), ms, ptr(mbar), N, d, F, alpha, ptr(A), ptr(R), wp, wb,
                  stream()), "ridge_gram_f64")
    info = _empty((1,), torch.int32, Z)
    check(L.timed(f"chol d{d}", lib.cvae_chol_f64, ptr(A), d, ptr(info), stream()), "chol_f64")
    T = new(d, N)
    check(lib.cvae_trsm_f64(ptr(A), d, ptr(Z), 1, zs, ptr(zbar), ptr(T), N, d, N, 0, stream()), "trsm_f64")          # T = L^-1 Xc^T
    check(lib.cvae_trsm_f64(ptr(A), d, ptr(R), F, 1, None, ptr(R), F, d, F, 0, stream()), "trsm_f64")                 # R <- L^-1 R
    check(lib.cvae_trsm_f64(ptr(A), d, ptr(R), F, 1, None, ptr(R), F, d, F, 1, stream()), "trsm_f64")                 # R <- L^-T R = W
    out = dict(leverage=new(N), fitted=new(N, F), loo=new(N, F), coef=new(F, d), intercept=new(F))
    check(lib.cvae_ridge_loo_f64(ptr(Z), zs, ptr(zbar), ptr(M), ms, ptr(mbar), ptr(R), ptr(T), N, d, F, ptr(out["leverage"]), ptr(out["fitted"]), ptr(out["loo"]),
                                 ptr(out["coef"]), ptr(out["intercept"]), stream()), "ridge_loo_f64")
    out["r2"], out["corr"] = ranking_stats_f64(M, out["loo"])
    code = int(info.item())
    if code != 0:
        raise L.CvaeError(f"{what}: the Cholesky factorisation of Xc^T Xc + alpha I failed at column {code - 1} (info = {code}): a pivot that is <= 0 or NaN "
                          "(a NaN or an infinity in Z?)")
    return RidgeFit(info=code, **out)


def ridge_predict(Z, coef, intercept):
    """intercept + Z coef^T in float64 (cvae_ridge_predict_f64): Z [N, d] float32 or float64, coef [F, d], intercept [F] float64 -> [N, F] float64."""
    what = "ridge_predict"
    if Z.dim() != 2 or coef.dim() != 2 or intercept.dim() != 1 or coef.shape[1] != Z.shape[1] or intercept.shape[0] != coef.shape[0]:
        raise L.CvaeError(f"{what}: Z [N, d], coef [F, d] and intercept [F] expected, got {tuple(Z.shape)}, {tuple(coef.shape)}, {tuple(intercept.shape)}")
    if Z.dtype not in (torch.float32, torch.float64) or coef.dtype != torch.float64 or intercept.dtype != torch.float64:
        raise L.CvaeError(f"{what}: Z float32 or float64 and float64 coefficients expected, got {Z.dtype}, {coef.dtype}, {intercept.dtype}")
    N, d = Z.shape
    F = coef.shape[0]
    if d < 1 or d > 1024 or F < 1:
        raise L.CvaeError(f"{what}: 1 <= d <= 1024 and F >= 1 expected, got d = {d}, F = {F}")
    L.require_gpu(Z, coef, intercept)
    Z, coef, intercept = _f64c(Z), coef.contiguous(), intercept.contiguous()
    out = _empty((N, F), torch.float64, Z)
    check(lib.cvae_ridge_predict_f64(ptr(Z), d, ptr(coef), ptr(intercept), N, d, F, ptr(out), stream()), "ridge_predict_f64")
    return out


def group_means_resampled(Z, codes, idx, G):
    """(means [n_boot, G, d] float64, counts [n_boot, G] int32): for every bootstrap b and group g the mean, in index order, of the rows Z[idx[b, i]] whose
    codes[idx[b, i]] == g (cvae_group_means_resampled_f64; the reference's compute_group_means(Z[idx], groups[idx]) for every draw at once,
    latent_translator/analysis.py:139-142).  Z [N, d] float32 or float64, codes [N] and idx [n_boot, N] integer tensors.  An empty group: a zero row, count 0."""
    what = "group_means_resampled"
    if Z.dim() != 2 or codes.dim() != 1 or idx.dim() != 2 or codes.shape[0] != Z.shape[0] or idx.shape[1] != Z.shape[0]:
        raise L.CvaeError(f"{what}: Z [N, d], codes [N] and idx [n_boot, N] expected, got {tuple(Z.shape)}, {tuple(codes.shape)}, {tuple(idx.shape)}")
    if Z.dtype not in (torch.float32, torch.float64) or codes.dtype.is_floating_point or idx.dtype.is_floating_point:
        raise L.CvaeError(f"{what}: Z float32 or float64, integer codes and indices expected, got {Z.dtype}, {codes.dtype}, {idx.dtype}")
    N, d = Z.shape
    n_boot, G = idx.shape[0], int(G)
    if N < 1 or d < 1 or d > 65536 or G < 1 or G > 65535 or n_boot > 65535:
        raise L.CvaeError(f"{what}: N >= 1, 1 <= d <= 65536, 1 <= G <= 65535 and n_boot <= 65535 expected, got N = {N}, d = {d}, G = {G}, n_boot = {n_boot}")
    L.require_gpu(Z, codes, idx)
    Z, codes, idx = _f64c(Z), codes.to(torch.int32).contiguous(), idx.to(torch.int32).contiguous()
    out, counts = _empty((n_boot, G, d), torch.float64, Z), _empty((n_boot, G), torch.int32, Z)
    check(lib.cvae_group_means_resampled_f64(ptr(Z), d, ptr(codes), ptr(idx), N, d, G, n_boot, ptr(out), ptr(counts), stream()), "group_means_resampled_f64")
    return out, counts


# ---- the symmetric eigensolver, the ridge alpha path and the latent PCA (csrc/eigh.hip, csrc/ridge.hip): float64 throughout ----
EIGH_MAX_N = 1024
RIDGE_PATH_MAX_ALPHAS = 64


def eigh_f64(A):
    """(w [n] ascending, V [n, n] with column k the eigenvector of w[k], sweeps) of a symmetric float64 matrix on the device, 1 <= n <= 1024
    (cvae_eigh_f64: a two-sided Jacobi method in round-robin order; the lower triangle of A is read; numpy.linalg.eigh's convention).  Not enqueue-only: the
    entry synchronises the stream once per sweep.  The status is read once, here: CvaeError if the sweep cap was reached (info 1) or a non-finite entry was met
    (info 2)."""
    what = "eigh_f64"
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float64:
        raise L.CvaeError(f"{what}: a square float64 matrix expected, got {tuple(A.shape)} {A.dtype}")
    n = A.shape[0]
    if n < 1 or n > EIGH_MAX_N:
        raise L.CvaeError(f"{what}: 1 <= n <= {EIGH_MAX_N} expected, got n = {n}")
    L.require_gpu(A)
    A = A.detach().contiguous()
    w, V, info = _empty((n,), torch.float64, A), _empty((n, n), torch.float64, A), _empty((2,), torch.int32, A)
    _t, wp, wb = _f64_ws(lib.cvae_eigh_f64_workspace_bytes(n), A)
    check(L.timed(f"eigh n{n}", lib.cvae_eigh_f64, ptr(A), n, n, ptr(w), ptr(V), n, ptr(info), wp, wb, stream()), "eigh_f64")
    code, sweeps = (int(v) for v in info.cpu().tolist())
    if code == 1:
        raise L.CvaeError(f"{what}: no convergence within the cap of {lib.cvae_eigh_max_sweeps()} sweeps (info = 1)")
    if code != 0:
        raise L.CvaeError(f"{what}: a non-finite entry was met (info = {code}): a NaN or an infinity in the matrix?")
    return w, V, sweeps


def centered_gram_f64(Z, zbar, M=None, mbar=None):
    """(G [d, d] = Xc^T Xc, R [d, F] = Xc^T Yc or None without M) with Xc = Z - zbar, Yc = M - mbar (cvae_centered_gram_f64: the kernels of the ridge's Gram
    matrix without the shift).  Float64 device tensors with contiguous rows."""
    what = "centered_gram_f64"
    zs = _f64_rows(what, "Z", Z)
    N, d = Z.shape
    F = 0 if M is None else M.shape[1]
    ms = 0 if M is None else _f64_rows(what, "M", M)
    if N < 1 or d < 1 or d > 1024 or (M is not None and (M.shape[0] != N or mbar is None or mbar.shape != (F,))) or zbar.shape != (d,):
        raise L.CvaeError(f"{what}: Z [N, d] with 1 <= d <= 1024, zbar [d] and optionally M [N, F], mbar [F] expected, got {tuple(Z.shape)}, {tuple(zbar.shape)}")
    L.require_gpu(Z, zbar)
    G = _empty((d, d), torch.float64, Z)
    R = _empty((d, F), torch.float64, Z) if F > 0 else None
    _t, wp, wb = _f64_ws(lib.cvae_centered_gram_f64_workspace_bytes(N, d, F), Z)
    check(L.timed(f"centered_gram N{N} d{d} F{F}", lib.cvae_centered_gram_f64, ptr(Z), zs, ptr(zbar), ptr(M) if F > 0 else None, ms, ptr(mbar) if F > 0 else None,
                  N, d, F, ptr(G), ptr(R) if F > 0 else None, wp, wb, stream()), "centered_gram_f64")
    return G, R


def centered_matmul_f64(x, mean, b, x_t=False, b_t=False):
    """(X - mean) B in float64 on the fp64 MFMA (cvae_centered_matmul_f64), the mean (a vector over X's columns, or None) subtracted on load.  X = x, or x^T with
    x_t; B = b, or b^T with b_t: a transpose is read in place through the strides.  x and b: contiguous float64 device matrices."""
    what = "centered_matmul_f64"
    for name, t in (("x", x), ("b", b)):
        if t.dim() != 2 or t.dtype != torch.float64 or not t.is_contiguous():
            raise L.CvaeError(f"{what}: {name} must be a contiguous float64 matrix, got {tuple(t.shape)} {t.dtype}")
    (R, K), (xrs, xcs) = ((x.shape[1], x.shape[0]), (1, x.shape[1])) if x_t else (tuple(x.shape), (x.shape[1], 1))
    (Kb, Cc), (brs, bcs) = ((b.shape[1], b.shape[0]), (1, b.shape[1])) if b_t else (tuple(b.shape), (b.shape[1], 1))
    if Kb != K or K < 1 or K > 1024 or R < 1 or Cc < 1 or (mean is not None and (mean.dtype != torch.float64 or mean.shape != (K,))):
        raise L.CvaeError(f"{what}: [R, K] times [K, C] with 1 <= K <= 1024 and a float64 mean [K] expected, got [{R}, {K}] times [{Kb}, {Cc}]")
    L.require_gpu(x, b)
    out = _empty((R, Cc), torch.float64, x)
    check(lib.cvae_centered_matmul_f64(ptr(x), max(xrs, 1), max(xcs, 1), None if mean is None else ptr(mean.contiguous()), ptr(b), max(brs, 1), max(bcs, 1), R, K, Cc,
                                       ptr(out), Cc, stream()), "centered_matmul_f64")
    return out


class RidgePath(_Result):
    """What ridge_loo_path returns, float64 device tensors: alphas [G], eigenvalues [d] (of the centred Gram matrix, ascending, clamped at 0), leverage [G, N],
    loo [G, N, F] (the leave-one-out predictions), sse [G, F] (sum over the rows of (M - loo)^2), r2 [G, F] and corr [G, F] (cvae_ranking_stats_f64's);
    sweeps: how many Jacobi sweeps the eigensolver used."""
    __slots__ = ("alphas", "eigenvalues", "leverage", "loo", "sse", "r2", "corr", "sweeps")


def ridge_path_alphas(what, alphas):
    """the grid as a list of Python floats, or CvaeError: empty, more than 64, or an alpha that is not positive and finite"""
    try:
        grid = [float(a) for a in alphas]
    except TypeError:
        raise L.CvaeError(f"{what}: alphas must be a sequence of numbers, got {alphas!r}") from None
    if not grid:
        raise L.CvaeError(f"{what}: alphas is empty")
    if len(grid) > RIDGE_PATH_MAX_ALPHAS:
        raise L.CvaeError(f"{what}: at most {RIDGE_PATH_MAX_ALPHAS} alphas expected, got {len(grid)}")
    return [_ridge_alpha(what, "every alpha", a) for a in grid]


def ridge_loo_path(Z, M, alphas):
    """The exact leave-one-out predictions of the Ridge translator Z [N, d] -> M [N, F] (ridge_fit_loo's model) for a whole grid of alphas from ONE
    eigendecomposition (what sklearn's RidgeCV does): column means, the centred Gram matrix G = Xc^T Xc = V diag(lambda) V^T (cvae_eigh_f64, lambda
    clamped at 0), P = Xc V, Q = V^T Xc^T Yc, then per alpha h = 1 / N + sum_k P_k^2 / (lambda_k + alpha), Yhat = mbar + P diag(1 / (lambda + alpha)) Q,
    loo = M - (M - Yhat) / (1 - h), and the ranking statistics of every loo against M.  Z: float32 or float64; M is converted to float64.  Every refusal
    (ridge_fit_loo's for the shapes and dtypes; an empty grid, more than 64 alphas, an alpha that is not positive and finite) comes before the first launch.
    Returns a RidgePath.  The one host read is the eigensolver's status."""
    what = "ridge_loo_path"
    grid = ridge_path_args(what, Z, M, alphas)
    (N, d), F = Z.shape, M.shape[1]
    L.require_gpu(Z, M)
    Z, M = _f64c(Z), _f64c(M)
    ms = _f64_rows(what, "M", M)
    Gn = len(grid)
    zbar, mbar = col_means_f64(Z), col_means_f64(M)
    gram, R = centered_gram_f64(Z, zbar, M, mbar)
    w, V, sweeps = eigh_f64(gram)
    P = centered_matmul_f64(Z, zbar, V)                  # Xc V
    Q = centered_matmul_f64(V, None, R, x_t=True)        # V^T (Xc^T Yc)
    new = _f64_like(Z)
    a_dev = torch.tensor(grid, dtype=torch.float64, device=Z.device)
    out = dict(eigenvalues=new(d), leverage=new(Gn, N), loo=new(Gn, N, F), sse=new(Gn, F), r2=new(Gn, F), corr=new(Gn, F))
    check(L.timed(f"ridge_path N{N} d{d} F{F} G{Gn}", lib.cvae_ridge_path_f64, ptr(P), ptr(Q), ptr(w), ptr(a_dev), ptr(M), ms, ptr(mbar), N, d, F, Gn,
                  ptr(out["eigenvalues"]), ptr(out["leverage"]), ptr(out["loo"]), ptr(out["sse"]), stream()), "ridge_path_f64")
    for g in range(Gn):
        check(lib.cvae_ranking_stats_f64(ptr(M), ms, ptr(out["loo"][g]), F, N, F, ptr(out["r2"][g]), ptr(out["corr"][g]), stream()), "ranking_stats_f64")
    return RidgePath(alphas=a_dev, sweeps=sweeps, **out)


def ridge_path_args(what, Z, M, alphas):
    """every refusal of ridge_loo_path, none of which needs a device: ridge_fit_loo's for the shapes and dtypes, then the grid's -> the grid as Python floats"""
    _ridge_shapes(what, Z, M, "the eigensolver's limit")
    return ridge_path_alphas(what, alphas)


def pca_args(what, Z, n_components):
    """every refusal of pca_fit_f64, none of which needs a device -> n_components as an int"""
    if Z.dim() != 2 or Z.dtype not in (torch.float32, torch.float64):
        raise L.CvaeError(f"{what}: a float32 or float64 matrix Z [N, d] expected, got {tuple(Z.shape)} {Z.dtype}")
    N, d = Z.shape
    if d < 1 or d > 1024:
        raise L.CvaeError(f"{what}: 1 <= d <= 1024 latent dimensions expected (the eigensolver's limit), got d = {d}")
    if int(n_components) != n_components or n_components < 1 or n_components > min(N - 1, d):
        raise L.CvaeError(f"{what}: 1 <= n_components <= min(N - 1, d) = {min(N - 1, d)} expected, got {n_components}")
    return int(n_components)


def pca_fit_f64(Z, n_components):
    """sklearn's PCA(n_components).fit on the device in float64: column means, the centred Gram matrix, cvae_eigh_f64, then
    cvae_pca_components_f64 (the top components in descending order, each signed so that its entry of largest |value| is positive).  Z [N, d] float32 or
    float64, 1 <= n_components <= min(N - 1, d), d <= 1024.  Returns a dict of float64 device tensors: mean [d], components [k, d], explained_variance [k],
    explained_variance_ratio [k], singular_values [k]."""
    k = pca_args("pca_fit_f64", Z, n_components)
    N, d = Z.shape
    L.require_gpu(Z)
    Z = _f64c(Z)
    mean = col_means_f64(Z)
    gram, _r = centered_gram_f64(Z, mean)
    w, V, _sweeps = eigh_f64(gram)
    new = _f64_like(Z)
    out = dict(components=new(k, d), explained_variance=new(k), explained_variance_ratio=new(k), singular_values=new(k))
    check(lib.cvae_pca_components_f64(ptr(w), ptr(V), d, d, k, N, ptr(out["components"]), ptr(out["explained_variance"]), ptr(out["explained_variance_ratio"]),
                                      ptr(out["singular_values"]), stream()), "pca_components_f64")
    return dict(mean=mean, **out)


def pca_transform_f64(Z, mean, components):
    """(Z - mean) components^T in float64 (cvae_centered_matmul_f64): Z [N, d] float32 or float64, mean [d], components [k, d] -> [N, k]"""
    what = "pca_transform_f64"
    if Z.dim() != 2 or Z.dtype not in (torch.float32, torch.float64) or components.dim() != 2 or Z.shape[1] != components.shape[1] or Z.shape[0] < 1:
        raise L.CvaeError(f"{what}: Z [N >= 1, d] float32 or float64 and components [k, d] expected, got {tuple(Z.shape)} {Z.dtype}, {tuple(components.shape)}")
    L.require_gpu(Z, mean, components)
    return centered_matmul_f64(_f64c(Z), mean, components.contiguous(), b_t=True)


# ---- the exact t-SNE of the latents (csrc/tsne.hip): float64 throughout ----
TSNE_MIN_N, TSNE_MAX_N = 3, 4096
TSNE_STOP_REASONS = ("max_iter iterations ran", "the gradient norm fell to min_grad_norm", "no progress within n_iter_without_progress iterations")


class TsneFit(_Result):
    """What tsne_fit_f64 returns: Y [N, 2] (float64, on the device), kl (a float: the KL divergence of P from the embedding's Q), n_iter (the index of the last
    iteration run, sklearn's n_iter_), reason (an index into TSNE_STOP_REASONS), checks (how many times the host read the device's record)."""
    __slots__ = ("Y", "kl", "n_iter", "reason", "checks")


def tsne_args(what, Z, perplexity=30.0, n_components=2, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, init="pca", tol=1e-5,
              n_iter_without_progress=300, distances=False):
    """Every refusal of the t-SNE entries, none of which needs a device.  Z: the tensor to embed, [N, d] float32 / float64, or with distances=True the squared
    distances [N, N].  Returns (N, the learning rate as a float)."""
    if not torch.is_tensor(Z) or Z.dim() != 2 or Z.dtype not in (torch.float32, torch.float64):
        raise L.CvaeError(f"{what}: a float32 or float64 matrix expected, got {_got(Z)}")
    N, d = Z.shape
    if N < TSNE_MIN_N or N > TSNE_MAX_N:
        raise L.CvaeError(f"{what}: {TSNE_MIN_N} <= N <= {TSNE_MAX_N} points expected (the exact method holds the N x N affinities), got N = {N}")
    if d < 1 or (distances and d != N):
        raise L.CvaeError(f"{what}: {'a square matrix of squared distances' if distances else 'at least one column'} expected, got {tuple(Z.shape)}")
    if n_components != 2:
        raise L.CvaeError(f"{what}: n_components must be 2, got {n_components}")
    if not (0.0 < float(perplexity) < N):
        raise L.CvaeError(f"{what}: perplexity must be in (0, N) = (0, {N}), got {perplexity}")
    if not (float(early_exaggeration) > 0.0 and math.isfinite(float(early_exaggeration))):
        raise L.CvaeError(f"{what}: early_exaggeration must be positive and finite, got {early_exaggeration}")
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise L.CvaeError(f"{what}: learning_rate must be a positive number or 'auto', got {learning_rate!r}")
        lr = max(N / float(early_exaggeration) / 4.0, 50.0)
    else:
        lr = float(learning_rate)
    if not (lr > 0.0 and math.isfinite(lr)):
        raise L.CvaeError(f"{what}: learning_rate must be positive and finite, got {learning_rate}")
    if int(max_iter) != max_iter or max_iter < 0:
        raise L.CvaeError(f"{what}: max_iter must be a non-negative integer, got {max_iter}")
    if int(n_iter_without_progress) != n_iter_without_progress or n_iter_without_progress < 0:
        raise L.CvaeError(f"{what}: n_iter_without_progress must be a non-negative integer, got {n_iter_without_progress}")
    if not (float(tol) >= 0.0):
        raise L.CvaeError(f"{what}: tol must be >= 0, got {tol}")
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise L.CvaeError(f"{what}: init must be 'pca', 'random' or an array [N, 2], got {init!r}")
        if init == "pca" and distances:
            raise L.CvaeError(f"{what}: init='pca' cannot be used with precomputed distances (there are no coordinates to project); use 'random' or an array")
    elif init is not None and tuple(getattr(init, "shape", ())) != (N, 2):
        raise L.CvaeError(f"{what}: an init array must have shape [N, 2] = [{N}, 2], got {tuple(getattr(init, 'shape', ()))}")
    return N, lr


def _tsne_f64(what, name, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != tuple(shape):
        raise L.CvaeError(f"{what}: {name} must be a float64 tensor {list(shape)}, got {_got(t)}")
    return t.detach().contiguous()


def tsne_sqdist_f64(Z):
    """D [N, N] float64 = the squared distances between the rows of Z [N, d] (float32 or float64, read as it is) from differences (cvae_tsne_sqdist_f64):
    bitwise symmetric, a zero diagonal."""
    what = "tsne_sqdist_f64"
    N, _lr = tsne_args(what, Z, perplexity=1.0)
    L.require_gpu(Z)
    Z = Z.detach()
    if Z.stride(1) != 1 or Z.stride(0) < Z.shape[1]:
        Z = Z.contiguous()
    D = _empty((N, N), torch.float64, Z)
    check(L.timed(f"tsne_sqdist N{N} d{Z.shape[1]}", lib.cvae_tsne_sqdist_f64, ptr(Z), int(Z.dtype == torch.float32), Z.stride(0), N, Z.shape[1], ptr(D), stream()),
          what)
    return D


def tsne_affinities_f64(D, perplexity, tol=1e-5):
    """(P, Pc, beta, steps) from squared distances D [N, N] float64: per row sklearn's search for the beta whose conditional distribution Pc[i] has the
    perplexity (cvae_tsne_affinities_f64; at most 100 steps, the first with |H - log perplexity| <= tol the last), then P = max((Pc + Pc^T) / sum, 2^-52)
    (cvae_tsne_joint_f64).  One host read, the status: a non-finite entry of D, Pc or the sum is a CvaeError (info = 2)."""
    what = "tsne_affinities_f64"
    N, _lr = tsne_args(what, D, perplexity=perplexity, tol=tol, init=None, distances=True)
    D = _tsne_f64(what, "D", D, (N, N))
    L.require_gpu(D)
    Pc, P = _empty((N, N), torch.float64, D), _empty((N, N), torch.float64, D)
    beta, steps, info = _empty((N,), torch.float64, D), _empty((N,), torch.int32, D), _empty((1,), torch.int32, D)
    check(L.timed(f"tsne_affinities N{N}", lib.cvae_tsne_affinities_f64, ptr(D), N, float(perplexity), float(tol), ptr(Pc), ptr(beta), ptr(steps), stream()),
          "tsne_affinities_f64")
    _t, wp, wb = _f64_ws(lib.cvae_tsne_joint_f64_workspace_bytes(N), D)
    check(L.timed(f"tsne_joint N{N}", lib.cvae_tsne_joint_f64, ptr(D), ptr(Pc), N, ptr(P), ptr(info), wp, wb, stream()), "tsne_joint_f64")
    code = int(info.item())
    if code != 0:
        raise L.CvaeError(f"cvae_tsne_joint_f64: a non-finite entry in the distances or the affinities (info = {code}): a NaN or an infinity in the input?")
    return P, Pc, beta, steps


def _tsne_pair_pass(what, Y, P, want_kl):
    N = Y.shape[0]
    new = _f64_like(Y)
    A, R, S = new(N, 2), new(N, 2), new(N)
    klp = new(3, N) if want_kl else None
    check(L.timed(f"tsne_forces N{N}", lib.cvae_tsne_forces_f64, ptr(Y), ptr(P), N, ptr(A), ptr(R), ptr(S), ptr(klp), stream()), "tsne_forces_f64")
    return A, R, S, klp


def _tsne_state(what, P, **mats):
    if not torch.is_tensor(P) or P.dim() != 2 or P.shape[0] != P.shape[1]:
        raise L.CvaeError(f"{what}: P must be a square float64 tensor, got {tuple(P.shape) if torch.is_tensor(P) else type(P).__name__}")
    N = P.shape[0]
    if N < TSNE_MIN_N or N > TSNE_MAX_N:
        raise L.CvaeError(f"{what}: {TSNE_MIN_N} <= N <= {TSNE_MAX_N} points expected, got N = {N}")
    out = [_tsne_f64(what, "P", P, (N, N))] + [_tsne_f64(what, k, v, (N, 2)) for k, v in mats.items()]
    L.require_gpu(*out)
    return N, out


def tsne_forces_f64(Y, P, exaggeration=1.0):
    """(kl, grad): the KL divergence of exaggeration * P from the embedding's Q (a float64 tensor [1]) and its gradient [N, 2], sklearn's _kl_divergence without
    the clamp of Q (cvae_tsne_forces_f64, the pair pass, then cvae_tsne_grad_f64).  Y [N, 2] and P [N, N] float64; P positive off the diagonal."""
    what = "tsne_forces_f64"
    if not (float(exaggeration) > 0.0):
        raise L.CvaeError(f"{what}: exaggeration must be positive, got {exaggeration}")
    N, (P, Y) = _tsne_state(what, P, Y=Y)
    A, R, S, klp = _tsne_pair_pass(what, Y, P, True)
    grad, kl = _empty((N, 2), torch.float64, Y), _empty((1,), torch.float64, Y)
    check(lib.cvae_tsne_grad_f64(ptr(A), ptr(R), ptr(S), ptr(klp), N, float(exaggeration), ptr(grad), ptr(kl), stream()), "tsne_grad_f64")
    return kl, grad


def tsne_step_f64(Y, update, gains, P, exaggeration, momentum, learning_rate):
    """One iteration of sklearn's _gradient_descent from a given state: (Y, update, gains) after it, as new tensors, and (kl, grad_norm), float64 tensors [1]:
    the KL of exaggeration * P at the Y handed in and |gains grad| (cvae_tsne_forces_f64, then cvae_tsne_update_f64 with a record)."""
    what = "tsne_step_f64"
    if not (float(exaggeration) > 0.0 and float(learning_rate) > 0.0):
        raise L.CvaeError(f"{what}: exaggeration and learning_rate must be positive, got {exaggeration}, {learning_rate}")
    N, (P, Y, update, gains) = _tsne_state(what, P, Y=Y, update=update, gains=gains)
    A, R, S, klp = _tsne_pair_pass(what, Y, P, True)
    Yn, un, gn = _empty((N, 2), torch.float64, Y), _empty((N, 2), torch.float64, Y), _empty((N, 2), torch.float64, Y)
    rec = _empty((4,), torch.float64, Y)
    check(lib.cvae_tsne_update_f64(ptr(Y), ptr(update), ptr(gains), ptr(A), ptr(R), ptr(S), ptr(klp), N, float(exaggeration), float(momentum), float(learning_rate),
                                   ptr(Yn), ptr(un), ptr(gn), ptr(rec), stream()), "tsne_update_f64")
    return Yn, un, gn, (rec[0:1], rec[1:2].sqrt())


def tsne_fit_f64(P, Y0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, n_iter_without_progress=300, min_grad_norm=1e-7):
    """sklearn's TSNE._tsne with method="exact" from the joint affinities P [N, N] and the start Y0 [N, 2] (float64, on the device; neither is written):
    min(250, max_iter) iterations at early_exaggeration and momentum 0.5, then to max_iter at 1 and 0.8; every 50 iterations the host reads the device's
    record and stops on sklearn's two tests (cvae_tsne_fit_f64; NOT enqueue-only).  Two differences from sklearn, both stated in DESIGN §27: a gradient norm at
    or below min_grad_norm ends the fit, and the KL returned is that of P at the returned Y.  A non-finite embedding is a CvaeError (info = 2)."""
    what = "tsne_fit_f64"
    N, (P, Y0) = _tsne_state(what, P, Y0=Y0)
    _n, lr = tsne_args(what, P, perplexity=1.0, early_exaggeration=early_exaggeration, learning_rate=learning_rate, max_iter=max_iter, init=None,
                       n_iter_without_progress=n_iter_without_progress, distances=True)
    Y = Y0.clone()
    kl, info = _empty((1,), torch.float64, Y), _empty((4,), torch.int32, Y)
    _t, wp, wb = _f64_ws(lib.cvae_tsne_fit_f64_workspace_bytes(N), Y)
    check(L.timed(f"tsne_fit N{N}", lib.cvae_tsne_fit_f64, ptr(P), ptr(Y), N, float(early_exaggeration), lr, int(max_iter), int(n_iter_without_progress),
                  float(min_grad_norm), ptr(kl), ptr(info), wp, wb, stream()), "tsne_fit_f64")
    code, n_iter, reason, checks = (int(v) for v in info.cpu().tolist())
    if code != 0:
        raise L.CvaeError(f"cvae_tsne_fit_f64: the embedding or its KL divergence stopped being finite by iteration {n_iter} (info = {code}): a NaN in P or Y0, "
                          "or a learning rate that is too large?")
    return TsneFit(Y=Y, kl=float(kl.item()), n_iter=n_iter, reason=reason, checks=checks)


# ---- the 12 morphology features of small grey images (csrc/morphology.hip) ----
MORPH_MAX_SIDE, MORPH_RAW_WORDS = 64, 32
MORPH_NORMS = (784.0, 100.0, 5.0, 28.0)          # area, perimeter, thickness, major axis: the reference's divisors for 28 x 28 digits
MORPH_EMPTY, MORPH_NO_BACKGROUND = 1, 2          # bits of raw[:, 0]


def morph_args(what, x, threshold=0.2, norms=MORPH_NORMS):
    """Every refusal of morph_features12, raised before any launch; the device is asked about last, so that the others can be met without one.  Returns (B, H, W)."""
    if not torch.is_tensor(x) or x.dim() not in (3, 4):
        raise L.CvaeError(f"{what}: images [B, H, W] or [B, 1, H, W] expected, got {_got(x)}")
    if x.dim() == 4 and x.shape[1] != 1:
        raise L.CvaeError(f"{what}: one channel expected (grey images [B, 1, H, W]), got {x.shape[1]} in {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise L.CvaeError(f"{what}: float32, bfloat16 or float16 images expected (uint8 images: divide by 255 first, as ToTensor does), got {x.dtype}")
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    if B < 1 or H < 1 or W < 1:
        raise L.CvaeError(f"{what}: at least one image of at least one pixel expected, got {tuple(x.shape)}")
    if H > MORPH_MAX_SIDE or W > MORPH_MAX_SIDE:
        raise L.CvaeError(f"{what}: H, W <= {MORPH_MAX_SIDE} expected (an image and its working arrays stay in one workgroup's LDS), got {H} x {W}")
    try:
        norms = tuple(float(v) for v in norms)
    except (TypeError, ValueError):
        norms = ()
    if len(norms) != 4 or not all(v > 0.0 and math.isfinite(v) for v in norms):
        raise L.CvaeError(f"{what}: norms must be four positive finite numbers (area, perimeter, thickness, axis), got {norms!r}")
    if not math.isfinite(float(threshold)):
        raise L.CvaeError(f"{what}: threshold must be finite, got {threshold}")
    L.require_gpu(x)
    return B, H, W


def morph_features12(x, threshold=0.2, norms=MORPH_NORMS, return_raw=False):
    """feats [B, 12] float32: the reference's extract_refined_features of every image of x ([B, H, W] or [B, 1, H, W] on the device, H, W <= 64; float32 as
    it is, bfloat16 / float16 converted first), in its order (Area, Perimeter, Thickness, MajorAxis, Eccentricity, Orientation, Solidity, Extent, AspectRatio,
    Euler, H_Symmetry, V_Symmetry); cvae_morph12_f32: one launch, one workgroup per image, enqueue-only.  threshold is compared in float32.  An empty mask
    gives twelve zeros; a mask without a background pixel a NaN thickness.  return_raw: (feats, raw), raw int32 [B, 32] = the integers behind the features
    (include/cvae_hip.h, CVAE_MORPH_RAW_*)."""
    what = "morph_features12"
    B, H, W = morph_args(what, x, threshold, norms)
    xx = x.detach().reshape(B, H, W)
    if xx.dtype != torch.float32:
        xx = xx.float()
    xx = xx.contiguous()
    feats = _empty((B, 12), torch.float32, xx)
    raw = _empty((B, MORPH_RAW_WORDS), torch.int32, xx) if return_raw else None
    check(L.timed(f"morph12 B{B} {H}x{W}", lib.cvae_morph12_f32, ptr(xx), B, H, W, float(threshold), *(float(v) for v in norms), ptr(feats), ptr(raw), stream()), what)
    return (feats, raw) if return_raw else feats


# ---- vessel image preparation (csrc/image_prep.hip) ----
PREP_CONSTANT, PREP_NONFINITE = 1, 2          # CVAE_PREP_*: bits of a record's flag word
PREP_MAX_BATCH, PREP_MAX_PIXELS = 65535, 2 ** 31 - 1


def _prep_images(what, x, dims, dtypes, names):
    """the refusals the four image_prep ops share: a tensor of `dims` axes, one of `dtypes`, no empty axis, at most PREP_MAX_BATCH images of less than 2^31 pixels"""
    if not torch.is_tensor(x) or x.dim() != dims:
        raise L.CvaeError(f"{what}: a tensor {names} expected, got {_got(x)}")
    if x.dtype not in dtypes:
        raise L.CvaeError(f"{what}: {' or '.join(str(d).replace('torch.', '') for d in dtypes)} expected, got {x.dtype}")
    if min(x.shape) < 1:
        raise L.CvaeError(f"{what}: no axis of {names} may be empty, got {tuple(x.shape)}")
    if x.shape[0] > PREP_MAX_BATCH or x.shape[-2] * x.shape[-1] > PREP_MAX_PIXELS:
        raise L.CvaeError(f"{what}: at most {PREP_MAX_BATCH} images of less than 2^31 pixels per call, got {tuple(x.shape)}")


def _prep_size(what, size):
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise L.CvaeError(f"{what}: size must be (H, W), got {size!r}") from None
    if H < 1 or W < 1 or H * W > PREP_MAX_PIXELS:
        raise L.CvaeError(f"{what}: size must be (H, W) with H, W >= 1 and less than 2^31 pixels, got {size!r}")
    return H, W


def mip_args(what, x):
    """Every refusal of mip_max, raised before any launch; the device is asked about last.  Returns (B, D, Hs, Ws)."""
    _prep_images(what, x, 4, (torch.uint16, torch.float32), "[B, D, Hs, Ws]")
    L.require_gpu(x)
    return tuple(x.shape)


def mip_max(x):
    """[B, D, Hs, Ws] uint16 or float32 on the device -> float32 [B, Hs, Ws], the maximum over D (np.max(axis=0) of each stack: a NaN propagates);
    cvae_mip_max, one launch, enqueue-only."""
    what = "mip_max"
    B, D, Hs, Ws = mip_args(what, x)
    xx = x.detach().contiguous()
    out = _empty((B, Hs, Ws), torch.float32, xx)
    check(L.timed(f"mip_max B{B} D{D} {Hs}x{Ws}", lib.cvae_mip_max, ptr(xx), ptr(out), B, D, Hs, Ws, L.U16 if xx.dtype == torch.uint16 else L.F32, stream()), what)
    return out


# the antialiased resize stages a tile's source rows in LDS: AA_TILE_H rows of output need about (AA_TILE_H + 2) * max(Hs / H, 1) + 2 of them, AA_TILE_W floats each
AA_TILE_W, AA_TILE_H, AA_LDS_BYTES = 64, 8, 160 * 1024


def _aa_window(i, n_in, n_out):
    scale = n_in / n_out
    support = max(scale, 1.0)
    c = scale * (i + 0.5)
    return max(0, int(c - support + 0.5)), min(int(c + support + 0.5), n_in)


@functools.lru_cache(maxsize=64)
def aa_lds_bytes(Hs, Ws, H, W):
    """the LDS one workgroup of cvae_resize_bilinear_aa_f32 needs for this shape (the entry point's own arithmetic; remembered per shape: the walk over
    the outputs costs half a millisecond of host time at 768 x 1280, several times the kernel)"""
    kw = max(b - a for a, b in (_aa_window(i, Ws, W) for i in range(W)))
    kh = max(b - a for a, b in (_aa_window(i, Hs, H) for i in range(H)))
    rows = max(_aa_window(min(o + AA_TILE_H, H) - 1, Hs, H)[1] - _aa_window(o, Hs, H)[0] for o in range(0, H, AA_TILE_H))
    return 4 * (rows * AA_TILE_W + kw * AA_TILE_W + kh * AA_TILE_H + 2 * AA_TILE_W + 2 * AA_TILE_H)


def resize_aa_args(what, x, size):
    """Every refusal of resize_bilinear_aa, raised before any launch; the device is asked about last.  Returns (B, Hs, Ws, H, W)."""
    _prep_images(what, x, 3, (torch.float32,), "[B, Hs, Ws]")
    H, W = _prep_size(what, size)
    B, Hs, Ws = x.shape
    need = aa_lds_bytes(Hs, Ws, H, W)
    if need > AA_LDS_BYTES or -(-H // AA_TILE_H) > 65535:
        raise L.CvaeError(f"{what}: {Hs} x {Ws} -> {H} x {W} needs {need} bytes of LDS for the source rows of one output tile, above the {AA_LDS_BYTES} of a "
                          "workgroup (a height ratio above about 50): reduce in two steps")
    L.require_gpu(x)
    return B, Hs, Ws, H, W


def resize_bilinear_aa(x, size):
    """F.interpolate(x[:, None], size, mode="bilinear", antialias=True, align_corners=False)[:, 0] (torchvision's Resize(antialias=True)) of float32
    [B, Hs, Ws] on the device -> float32 [B, H, W]; cvae_resize_bilinear_aa_f32: one launch, both passes, enqueue-only.  Weights are formed in float64 and
    rounded once, the sums run in float32.  Equal sizes copy."""
    what = "resize_bilinear_aa"
    B, Hs, Ws, H, W = resize_aa_args(what, x, size)
    xx = x.detach().contiguous()
    out = _empty((B, H, W), torch.float32, xx)
    check(L.timed(f"resize_aa B{B} {Hs}x{Ws}->{H}x{W}", lib.cvae_resize_bilinear_aa_f32, ptr(xx), ptr(out), B, Hs, Ws, H, W, stream()), what)
    return out


class BinariseStats:
    """cvae_binarise_record per source image, as device tensors [B]: mn, mx float32, thr float64, ones int64 (of the unflipped variant), flags int32"""

    def __init__(self, rec):
        self.thr, self.ones = rec.view(torch.float64)[:, 0], rec.view(torch.int64)[:, 1]
        f = rec.view(torch.float32)
        self.mn, self.mx, self.flags = f[:, 4], f[:, 5], rec.view(torch.int32)[:, 6]


def binarise_args(what, y, augment=False, dtype=torch.float32):
    """Every refusal of minmax_binarise, raised before any launch; the device is asked about last.  Returns (B, H, W)."""
    _prep_images(what, y, 3, (torch.float32,), "[B, H, W]")
    if dtype not in (torch.float32, torch.bfloat16):
        raise L.CvaeError(f"{what}: the masks are written as float32 or bfloat16, got dtype={dtype}")
    L.require_gpu(y)
    return tuple(y.shape)


def minmax_binarise(y, augment=False, dtype=torch.float32):
    """The tail of the reference's VesselDataset.__getitem__ for float32 [B, H, W] on the device: per image v = (y - min) / (max - min) in float32, the mask
    v > mean(v) (the mean: a float64 sum in a fixed order), as [B * A, 1, H, W] of 0 / 1 in `dtype`; augment: A = 4, image b's variants at 4 b + a, a = 0 as it
    is, 1 flipped horizontally, 2 vertically, 3 both (the dataset's index real_idx * 4 + aug_mode).  A constant image gives zeros (flag PREP_CONSTANT), and so
    does one with a NaN or an infinity (PREP_NONFINITE).  Returns (masks, BinariseStats).  cvae_minmax_binarise: three launches, enqueue-only."""
    what = "minmax_binarise"
    B, H, W = binarise_args(what, y, augment, dtype)
    yy = y.detach().contiguous()
    A = 4 if augment else 1
    out = _empty((B * A, 1, H, W), dtype, yy)
    rec = _empty((B, 32), torch.uint8, yy)
    _t, wp, wb = _f64_ws(lib.cvae_minmax_binarise_workspace_bytes(B, H, W), yy)
    check(L.timed(f"minmax_binarise B{B} {H}x{W} A{A}", lib.cvae_minmax_binarise, ptr(yy), ptr(out), ptr(rec), B, H, W, int(bool(augment)), L.dtype_code(dtype),
                  wp, wb, stream()), what)
    return out, BinariseStats(rec)


def percentile_ranks(n, p):
    """numpy's "linear" percentile pair [100 - p, p] of n values as 0-based order statistics: ((lo, lo', hi, hi'), (t_lo, t_hi)) with the value of a percentile
    = lerp(x[k], x[k'], t).  The virtual index is (n - 1) q with q = percent / 100, the expression numpy 2.x uses for this method (its _QuantileMethods table;
    the general form n q + (alpha + q (1 - alpha - beta)) - 1 at alpha = beta = 1 differs from it in the last bits and does NOT reproduce np.percentile:
    tests/test_image_prep_cpu.py).  Beyond the ends both neighbours are the end (numpy's _get_indexes), and t is taken against the neighbour as numpy indexes
    it (-1 for the last)."""
    ranks, ts = [], []
    for pct in (100 - p, p):
        q = pct / 100
        vi = (n - 1) * q
        if vi >= n - 1:
            prev, k0, k1 = -1, n - 1, n - 1
        elif vi < 0:
            prev, k0, k1 = 0, 0, 0
        else:
            prev = k0 = math.floor(vi)
            k1 = k0 + 1
        ranks += [k0, k1]
        ts.append(vi - prev)
    return tuple(ranks), tuple(ts)


def percentile_args(what, x, p=99.5):
    """Every refusal of percentile_clip_scale, raised before any launch; the device is asked about last.  Returns (B, N)."""
    if not torch.is_tensor(x) or x.dim() not in (2, 3):
        raise L.CvaeError(f"{what}: a tensor [B, N] or [B, H, W] expected, got {_got(x)}")
    _prep_images(what, x if x.dim() == 3 else x[:, None, :], 3, (torch.float32,), "[B, N] or [B, H, W]")
    try:
        ok = 50.0 <= float(p) <= 100.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise L.CvaeError(f"{what}: a clip percentile in [50, 100] expected, got {p!r}")
    L.require_gpu(x)
    return x.shape[0], x.numel() // x.shape[0]


class ClipStats:
    """cvae_clip_record per image, as device tensors [B]: vmin, vmax float64, flags int32"""

    def __init__(self, rec):
        d = rec.view(torch.float64)
        self.vmin, self.vmax, self.flags = d[:, 0], d[:, 1], rec.view(torch.int32)[:, 4]


def percentile_clip_scale(x, p=99.5, check_finite=True):
    """The reference's normalize_image for float32 [B, N] (or [B, H, W]) on the device: vmin, vmax = np.percentile(x_b, [100 - p, p]) found EXACTLY (a radix
    select of the four order statistics, numpy's interpolation in float64), then (clip(x, vmin, vmax) - vmin) / (vmax - vmin, or 1e-5 when that is 0) in
    float64, rounded once to float32.  Returns (out of x's shape, ClipStats).  cvae_percentile_clip_scale: nine launches, enqueue-only; check_finite reads the
    flag words back afterwards (one host read) and raises for an image with a NaN or an infinity, which the reference would silently turn into NaNs; with
    check_finite=False the caller looks at ClipStats.flags when it suits."""
    what = "percentile_clip_scale"
    B, N = percentile_args(what, x, p)
    xx = x.detach().contiguous()
    out = torch.empty_like(xx)
    rec = _empty((B, 24), torch.uint8, xx)
    ranks, ts = percentile_ranks(N, float(p))
    _t, wp, wb = _f64_ws(lib.cvae_percentile_clip_scale_workspace_bytes(B, N), xx)
    check(L.timed(f"percentile_clip_scale B{B} N{N}", lib.cvae_percentile_clip_scale, ptr(xx), ptr(out), ptr(rec), B, N, (C_.c_int64 * 4)(*ranks),
                  (C_.c_double * 2)(*ts), wp, wb, stream()), what)
    stats = ClipStats(rec)
    if check_finite:
        raise_nonfinite(what, stats.flags)
    return out, stats


def raise_nonfinite(what, flags):
    bad = torch.nonzero(flags.cpu() & PREP_NONFINITE).flatten().tolist()
    if bad:
        raise L.CvaeError(f"{what}: image(s) {bad} of the batch hold a NaN or an infinity; the percentiles of such an image are not defined")
