"""CPU-side checks of the attention-weights / attention-rollout feature: the float64 helper of the GPU tests (tests/vit_attention_reference.py)
is tied to the module the reference uses (nn.MultiheadAttention with need_weights=True), its vector recursion to the explicit matrix product, the public
names exist, and the two C entries answer bad arguments with the documented codes before anything is launched (no GPU is touched)."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_attention_reference as ar  # noqa: E402

F64 = torch.float64


@pytest.mark.parametrize("N", [7, 65])
@pytest.mark.parametrize("average", [True, False])
def test_helper_weights_equal_torch_multihead_attention(N, average):
    torch.manual_seed(3)
    mha = torch.nn.MultiheadAttention(256, 8, batch_first=True).double().eval()
    with torch.no_grad():
        mha.in_proj_bias.normal_()                                            # torch initialises it to zero
        x = torch.randn(2, N, 256, dtype=F64)
        _out, w = mha(x, x, x, need_weights=True, average_attn_weights=average)
        q, k = ar.in_projection(x, mha.in_proj_weight, mha.in_proj_bias)
        p = ar.head_weights(q, k)
    got = p.mean(1) if average else p
    assert got.shape == w.shape
    assert float((got - w).abs().max()) <= 1e-12
    # the kernels' form, 2^(s log2(e) / sqrt(32) - lse) with lse the row's log2-sum, is the same softmax
    s = (ar.split_heads(q, N) @ ar.split_heads(k, N).transpose(-1, -2)) * ar.C_LOG2
    lse = torch.log2(torch.exp2(s - s.amax(-1, keepdim=True)).sum(-1)) + s.amax(-1)
    p2, e_p = ar.weights_from_lse(q, k, lse)
    assert float((p2 - p).abs().max()) <= 1e-12 and bool((e_p >= 0).all())
    # the CLS row alone is row 0 of the full matrix
    assert float((ar.head_weights(q, k, 1) - p[:, :, :1]).abs().max()) <= 1e-15


@pytest.mark.parametrize("residual", [0.5, 0.2, 1.0, 0.0])
def test_vector_recursion_is_the_cls_row_of_the_matrix_product(residual):
    g = torch.Generator().manual_seed(5)
    B, N, L = 2, 9, 3
    mats = [torch.softmax(2 * torch.randn(B, N, N, generator=g, dtype=F64), dim=-1) for _ in range(L)]
    R = ar.rollout_matrix(mats, residual)
    r = ar.rollout_vector(mats, residual)
    assert float((R[:, 0] - r).abs().max()) <= 1e-14
    assert float((r.sum(-1) - 1).abs().max()) <= 1e-14 and bool((r >= 0).all())
    # a last block that holds only its CLS row (the CLS-only form) gives the same row
    r1 = ar.rollout_vector(mats[:-1] + [mats[-1][:, :1]], residual)
    assert float((r1 - r).abs().max()) <= 1e-15
    if residual == 1.0:
        e = torch.zeros(B, N, dtype=F64)
        e[:, 0] = 1
        assert torch.equal(r, e)
    # one factor at a time: rollout_step_ref on per-head matrices whose mean is the block's matrix
    heads = mats[0][:, None].expand(B, 8, N, N)
    v = torch.randn(B, N, generator=g, dtype=F64)
    out, e = ar.rollout_step_ref(heads, torch.zeros_like(heads), v, residual)
    assert float((out - (residual * v + (1 - residual) * (v[:, None] @ mats[0])[:, 0])).abs().max()) <= 1e-14 and bool((e >= 0).all())


def test_names_exist():
    from causal_vae_amd import ops, vit
    for name in ("attention_weights", "attention_rollout"):
        assert callable(getattr(vit.ViTVAEEncoder, name)) and callable(getattr(vit.ViTVAE, name))
    assert callable(vit.CausalViTVAE.attention_rollout)
    assert "extract_vit_attention" in vit.__all__ and callable(vit.extract_vit_attention)
    assert all(hasattr(vit, n) for n in vit.__all__)
    assert callable(ops.mhsa_weights) and callable(ops.mhsa_rollout_step)


def test_entries_check_their_arguments_before_any_launch():
    """Every call here is refused (or has B == 0), so nothing is enqueued: the pointers are never read."""
    from causal_vae_amd import _lib as L
    lib = L.lib
    OK, BADSHAPE, DTYPE, UNSUPPORTED, NULLPTR = 0, -1, -2, -3, -6
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    q, k, lse, w, r, out = base, base + 256, base + 512, base + 1024, base + 2048, base + 3072

    def weights(q=q, k=k, lse=lse, w=w, qs=768, ks=768, qb=7 * 768, kb=7 * 768, wb=7 * 7, B=2, N=7, nq=7, avg=1, dt=L.F32):
        return lib.cvae_mhsa_weights(q, k, lse, w, qs, ks, qb, kb, wb, B, N, nq, avg, dt, None)

    def step(q=q, k=k, lse=lse, r=r, out=out, qs=768, ks=768, qb=7 * 768, kb=7 * 768, B=2, N=7, nq=7, residual=0.5, dt=L.F32):
        return lib.cvae_mhsa_rollout_step(q, k, lse, r, out, qs, ks, qb, kb, B, N, nq, residual, dt, None)

    assert weights(B=0) == OK and step(B=0) == OK and weights(B=0, q=None, w=None) == OK
    for f in (weights, step):
        assert f(nq=0) == BADSHAPE and f(nq=8) == BADSHAPE and f(N=0) == BADSHAPE and f(B=-1) == BADSHAPE and f(B=65536) == BADSHAPE
        assert f(dt=L.FP8) == DTYPE and f(dt=7) == DTYPE and f(dt=-1) == DTYPE       # an unknown dtype code, the arguments otherwise valid
        assert f(q=None) == NULLPTR and f(k=None) == NULLPTR and f(lse=None) == NULLPTR
        assert f(qs=255) == BADSHAPE and f(kb=-768) == BADSHAPE
        assert f(qs=770) == UNSUPPORTED and f(q=q + 4) == UNSUPPORTED and f(dt=L.BF16, ks=772) == UNSUPPORTED
    assert weights(w=None) == NULLPTR and weights(w=w + 4) == UNSUPPORTED
    assert weights(wb=7 * 7 - 1) == BADSHAPE and weights(avg=0, wb=8 * 7 * 7 - 1) == BADSHAPE and weights(avg=0, wb=7 * 7) == BADSHAPE
    assert step(residual=-0.01) == BADSHAPE and step(residual=1.5) == BADSHAPE and step(residual=float("nan")) == BADSHAPE
    assert step(r=None) == NULLPTR and step(out=None) == NULLPTR
    assert step(out=r) == UNSUPPORTED and step(out=r + 4 * 13) == UNSUPPORTED      # out == r, and an out that overlaps r's [2][7] floats
