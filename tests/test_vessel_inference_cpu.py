"""CPU-side checks of the CausalVesselVAE inference layer: the argument checks of the three C entries (cvae_fold_bn_conv, cvae_row_diff_norms,
cvae_stack_mean_std) answer malformed calls with their documented codes before anything is enqueued, and batched_counterfactual reaches a
decode(z, m) model through its declared signature (a swapped call would return a wrong image of the right shape)."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADSHAPE, DTYPE, UNSUPPORTED, WORKSPACE, NULLPTR = -1, -2, -3, -4, -6


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "causal_vae_amd", "libcvae_hip.so")):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    from causal_vae_amd import _lib
    return _lib.lib


def _fold_call(lib, count=1, kind=0, dims=(8, 4), w=0x10000, w_out=0x20000, b_out=0x30000, gamma=None, beta=None, mean=None, var=None):
    """cvae_fold_bn_conv with `count` copies of one entry; the addresses are never dereferenced (every call here carries a defect the host-side
    checks reject before the launch)."""
    n = max(count, 1)
    vp = lambda v: (C.c_void_p * n)(*([v] * n))
    return lib.cvae_fold_bn_conv(count, vp(w), (C.c_int * n)(*([kind] * n)), (C.c_int64 * (2 * n))(*(list(dims) * n)), None,
                                 vp(gamma) if gamma is not None else None, vp(beta), vp(mean), vp(var), (C.c_float * n)(*([1e-5] * n)),
                                 vp(w_out), vp(b_out), None)


def test_fold_bn_conv_rejects_malformed_tables(lib):
    assert _fold_call(lib, count=0) == BADSHAPE
    assert _fold_call(lib, count=17) == UNSUPPORTED                  # more than 16 layers per launch
    assert _fold_call(lib, count=-3) == BADSHAPE
    assert _fold_call(lib, kind=2) == UNSUPPORTED                    # neither CVAE_FOLD_CONV_K4 nor CVAE_FOLD_UPCONV_K3
    assert _fold_call(lib, dims=(0, 4)) == BADSHAPE
    assert _fold_call(lib, dims=(8, -1)) == BADSHAPE
    assert _fold_call(lib, w=None) == NULLPTR
    assert _fold_call(lib, w_out=None) == NULLPTR
    assert _fold_call(lib, b_out=None) == NULLPTR
    assert _fold_call(lib, gamma=0x40000, beta=0x50000, mean=0x60000, var=None) == NULLPTR    # BatchNorm without its variance
    assert _fold_call(lib, w_out=0x20004) == UNSUPPORTED             # not 16-byte aligned
    assert _fold_call(lib, kind=0, w=0x10008) == UNSUPPORTED
    assert _fold_call(lib, count=16, dims=(1 << 15, 1 << 14)) == BADSHAPE    # Cout * Cin above 2^28
    assert lib.cvae_fold_bn_conv(1, None, None, None, None, None, None, None, None, None, None, None, None) == NULLPTR


def test_row_diff_norms_and_stack_mean_std_reject_malformed_calls(lib):
    p = 0x10000
    ws = lib.cvae_row_diff_norms_workspace_bytes(3, 1000, 0)
    assert ws > 0 and lib.cvae_row_diff_norms_workspace_bytes(0, 1000, 0) == 0 and lib.cvae_row_diff_norms_workspace_bytes(3, 1000, 9) == 0
    assert lib.cvae_row_diff_norms(p, p, None, p, None, 0, 3, 1000, 0, p, ws, None) == BADSHAPE
    assert lib.cvae_row_diff_norms(p, p, None, p, None, 3, 3, 0, 0, p, ws, None) == BADSHAPE
    assert lib.cvae_row_diff_norms(p, p, None, p, None, 3, 2, 1000, 0, p, ws, None) == BADSHAPE      # no ref: b needs a row per row of a
    assert lib.cvae_row_diff_norms(p, p, None, p, None, 3, 3, 1000, 7, p, ws, None) == DTYPE
    assert lib.cvae_row_diff_norms(None, p, None, p, None, 3, 3, 1000, 0, p, ws, None) == NULLPTR
    assert lib.cvae_row_diff_norms(p, p, None, None, None, 3, 3, 1000, 0, p, ws, None) == NULLPTR
    assert lib.cvae_row_diff_norms(p, p, None, p, None, 3, 3, 1000, 0, None, ws, None) == NULLPTR
    assert lib.cvae_row_diff_norms(p, p, None, p, None, 3, 3, 1000, 0, p, ws - 4, None) == WORKSPACE
    xs = (C.c_void_p * 17)(*([p] * 17))
    assert lib.cvae_stack_mean_std(xs, 0, p, p, 10, None) == BADSHAPE
    assert lib.cvae_stack_mean_std(xs, 17, p, p, 10, None) == UNSUPPORTED
    assert lib.cvae_stack_mean_std(xs, 2, p, p, 0, None) == BADSHAPE
    assert lib.cvae_stack_mean_std(xs, 2, None, p, 10, None) == NULLPTR
    assert lib.cvae_stack_mean_std((C.c_void_p * 2)(p, None), 2, p, p, 10, None) == NULLPTR


class _ZMDecoder:
    """A decode(z, m) model that records how it was called and returns its input rows as [rows, 1, 1, Z + M] images."""
    decode_signature = "z_m"

    def __init__(self):
        self.calls = []

    def decode(self, z, m):
        self.calls.append((z.shape[1], m.shape[1], z.shape[0]))
        return torch.cat([z, m], 1)[:, None, None, :]


class _MZDecoder(_ZMDecoder):
    """The MNIST models' decode(m, z) (no decode_signature, no dec_input)."""
    decode_signature = None

    def decode(self, m, z):
        return super().decode(z, m)


def test_batched_counterfactual_dispatches_on_the_declared_signature():
    from causal_vae_amd.counterfactual import batched_counterfactual, sweep_inputs
    from causal_vae_amd.vessel import CausalVesselVAE
    assert CausalVesselVAE.decode_signature == "z_m"
    g = torch.Generator().manual_seed(0)
    z, m = torch.randn(2, 128, generator=g), torch.randn(2, 12, generator=g)
    feats, vals = [0, 7, 11], [-1.0, 0.5]
    z_rep, m_cf = sweep_inputs(z, m, feats, vals)
    want = torch.cat([z_rep, m_cf], 1).view(2, 3, 2, 1, 1, 140)
    zm = _ZMDecoder()
    out = batched_counterfactual(zm, z, m, feats, vals)
    assert zm.calls == [(128, 12, 12)] and torch.equal(out, want)      # decode(z, m), not decode(m, z)
    zm = _ZMDecoder()
    out = batched_counterfactual(zm, z, m, feats, vals, chunk_rows=5)
    assert zm.calls == [(128, 12, 5), (128, 12, 5), (128, 12, 2)] and torch.equal(out, want)
    with pytest.raises(ValueError):
        batched_counterfactual(_ZMDecoder(), z, m, feats, vals, chunk_rows=0)
    with pytest.raises(ValueError):
        batched_counterfactual(_ZMDecoder(), z, m, feats, vals, size=(64, 64))
    mz = _MZDecoder()
    assert torch.equal(batched_counterfactual(mz, z, m, feats, vals), want)     # decode(m, z) models: as before
