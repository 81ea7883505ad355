"""Known answers for the sampler (csrc/common.h philox_normal4, cvae_philox_normal / _advance in csrc/losses.hip).

CPU: an independent numpy Philox4x32-10 reproduces the published Random123 vectors, and a numpy float32 Box-Muller stays inside the bound below.
GPU: the kernels against that generator, the kernel's own uniform construction mirrored in float32 — u = ((c >> 8) + 0.5f) * 2^-24, where the addition
ROUNDS for c >> 8 >= 2^23 (to even: u can be exactly 1, giving radius 0) — and Box-Muller in float64 with the kernel's float32 constant 6.2831855f.
Counter layout: words 0-1 = offset + i for output quadruple i (+ call_counter << 24), words 2-3 = subsequence, key = seed.

Bound per element, v = r t with r = sqrtf(-2 logf(u_r)), t = cos / sin(theta), theta = fl(6.2831855f * u_a):
  theta     one fp32 multiplication: |d theta| <= theta 2^-24; cos and sin are 1-Lipschitz, and sincosf is documented at 1 ulp: |dt| <= theta 2^-24 + 2^-23 |t|
  r         logf is documented at 1 ulp (relative 2^-23), -2 x is exact, sqrt halves a relative error and sqrtf adds 1 ulp: |dr| <= 1.5 * 2^-23 r
  product   one fp32 multiplication: 2^-24 |v|
  |dv| <= r (theta 2^-24 + 2^-23 |t|) + |v| (1.5 * 2^-23 + 2^-24), times 1.001 for the second-order terms."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TWO_PI_F32 = float(np.float32(6.283185307179586))


def philox4x32_10(ctr, key):
    """ctr: uint32 [n, 4], key: (k0, k1) -> uint32 [n, 4]"""
    c = [ctr[:, j].astype(np.uint64) for j in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(0xFFFFFFFF), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(0xFFFFFFFF)]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, 1).astype(np.uint32)


def uniforms(words):
    """the kernel's construction in float32, rounding included"""
    return ((words >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def reference(n, seed, offset, subseq, calls=0):
    """(ref, err) float64 [n]: what cvae_philox_normal(out, n, seed, offset, subseq, call_counter -> calls) must write, and the bound"""
    n4 = (n + 3) // 4
    pos = (np.arange(n4, dtype=np.uint64) + np.uint64((offset + (calls << 24)) & 0xFFFFFFFFFFFFFFFF))          # wraps modulo 2^64 like the kernel
    ctr = np.stack([pos & np.uint64(0xFFFFFFFF), pos >> np.uint64(32), np.full(n4, subseq & 0xFFFFFFFF, np.uint64), np.full(n4, subseq >> 32, np.uint64)], 1).astype(np.uint32)
    u = uniforms(philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))).astype(np.float64)
    ref, err = np.empty((n4, 4)), np.empty((n4, 4))
    for ur, ua, j in ((u[:, 0], u[:, 1], 0), (u[:, 2], u[:, 3], 2)):
        r = np.sqrt(-2.0 * np.log(ur))
        theta = TWO_PI_F32 * ua
        for k, t in ((j, np.cos(theta)), (j + 1, np.sin(theta))):
            ref[:, k] = r * t
            err[:, k] = 1.001 * (r * (theta * 2.0 ** -24 + 2.0 ** -23 * np.abs(t)) + np.abs(r * t) * (1.5 * 2.0 ** -23 + 2.0 ** -24))
    return ref.reshape(-1)[:n], err.reshape(-1)[:n], u


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox4x32_10_reproduces_the_random123_vectors(ctr, key, out):
    got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
    assert tuple(int(v) for v in got) == out


def test_uniform_construction_rounds_above_2_to_the_23():
    w = np.array([0, 0x7fffff00, 0x80000000, 0x80000100, 0xffffffff], dtype=np.uint32)
    u = uniforms(w)
    assert u[0] == np.float32(2.0 ** -25) and u[1] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)
    assert u[2] == np.float32(0.5) and u[3] == np.float32((2 ** 23 + 2) * 2.0 ** -24) and u[4] == np.float32(1.0)      # ties to even; the top word gives u = 1


def test_a_float32_box_muller_stays_inside_the_bound():
    n = 1 << 18
    ref, err, u = reference(n, 0x1234567890ABCDEF, 77, (5 << 32) | 3)
    u = u.astype(np.float32)
    got = np.empty((n // 4, 4), np.float32)
    for ur, ua, j in ((u[:, 0], u[:, 1], 0), (u[:, 2], u[:, 3], 2)):
        r = np.sqrt(np.float32(-2.0) * np.log(ur))
        theta = np.float32(TWO_PI_F32) * ua
        got[:, j], got[:, j + 1] = r * np.cos(theta), r * np.sin(theta)
    ratio = np.abs(got.reshape(-1).astype(np.float64) - ref) / err
    print("float32 Box-Muller: max |got - ref| / err =", float(ratio.max()))
    assert ratio.max() <= 1.0
    assert abs(ref.mean()) < 0.01 and abs(ref.std() - 1) < 0.01
    wrong = reference(n, 0x1234567890ABCDEF, 78, (5 << 32) | 3)[0]                  # one counter step off: nothing matches
    assert (np.abs(wrong - ref) > err).mean() > 0.99


def _draw(n, seed, offset, subseq, counter=None, advance=False):
    from causal_vae_amd import _lib as L
    from causal_vae_amd import ops
    out = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    fn = L.lib.cvae_philox_normal_advance if advance else L.lib.cvae_philox_normal
    rc = fn(C.c_void_p(out.data_ptr()), n, seed, offset, subseq, None if counter is None else C.c_void_p(counter.data_ptr()), ops.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all()), "wrote past n"
    return out[:n].double().cpu().numpy()


GPU_CASES = [  # n, seed, offset, subsequence, call counter (None: no pointer), advance
    (4096, 0, 0, 0, None, False), (1001, 42, 0, 0, None, False), (4099, 0xDEADBEEF12345678, 0xFFFFFFF0, (7 << 32) | 9, None, False),
    (1 << 16, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFC00, 0xFFFFFFFF00000001, None, False), (513, 42, 5, 1 << 32, 3, False), (16384, 7, 0, 2, 255, True), (16385, 7, 0, 2, 256, True),
    (16387, 7, 1 << 40, 2, 0, True), (2, 99, 11, 0, 1, True), (300, 1 << 63, (1 << 32) - 3, 0, 1000, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,offset,subseq,calls,advance", GPU_CASES)
def test_kernels_draw_the_documented_stream(n, seed, offset, subseq, calls, advance):
    counter = None if calls is None else torch.tensor([calls], dtype=torch.int32, device="cuda")
    got = _draw(n, seed, offset, subseq, counter, advance)
    ref, err, _ = reference(n, seed, offset, subseq, calls or 0)
    ratio = np.abs(got - ref) / err
    print(f"RATIO philox n={n} {float(ratio.max()):.3f}")
    bad = np.nonzero(~(ratio <= 1.0))[0]
    assert bad.size == 0, f"{bad.size} of {n} outside the bound; first at {bad[0]}: got {got[bad[0]]} ref {ref[bad[0]]} bound {err[bad[0]]}"
    if counter is not None:
        assert int(counter.item()) == calls + (1 if advance else 0)
