"""CPU-side checks of the attention-gradient / attention-relevance feature: the float64 helper of the GPU tests
(tests/vit_attention_grad_reference.py) is tied to torch autograd's retain_grad() on the probabilities of a float64 restatement of the encoder, its row
recursion to the explicit matrix product, the public names exist, the model methods refuse what they document, and the new C entries answer bad arguments with
the documented codes before anything is launched (no GPU is touched)."""
import ctypes
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_attention_grad_reference as gr  # noqa: E402
import vit_reference as vr  # noqa: E402

F64 = torch.float64
H, W, DEPTH, MB = 64, 96, 2, 2


@functools.lru_cache(maxsize=None)
def cpu_model():
    from causal_vae_amd.vit import ViTVAEEncoder
    torch.manual_seed(H + W)
    m = ViTVAEEncoder(img_size=(H, W), depth=DEPTH, latent_dim=16)
    vr.randomize_stem_bn(m.stem, H)
    return m.requires_grad_(False).eval(), {k: v.detach().double() for k, v in m.state_dict().items()}, vr.vit_inputs(MB, H, W, W)


@pytest.mark.parametrize("target,index", [("mu", 3), ("cls", 5)])
def test_weight_grads_equal_autograd_retain_grad(target, index):
    _m, sd, x = cpu_model()
    res = gr.encoder_attention_grads(sd, x, DEPTH, target, index)
    N = 7
    for l in range(DEPTH):
        want = res["gA"][l]
        assert want.shape == (MB, 8, N, N) and float(want.abs().max()) > 1e-3
        got, e_g, mag = gr.weight_grads_ref(res["datt"][l], res["v"][l])
        print(f"block {l} {target}: max |dO V^T - P.grad| = {float((got - want).abs().max()):.2e}, max |P.grad| = {float(want.abs().max()):.2e}")
        assert float((got - want).abs().max()) <= 1e-12
        assert bool((e_g >= 0).all()) and bool((got.abs() <= mag).all())
    # only the CLS output of the last block reaches a target: its other rows are zero, exactly
    assert float(res["gA"][-1][:, :, 1:].abs().max()) == 0.0 and float(res["datt"][-1][:, 1:].abs().max()) == 0.0
    assert float(gr.weight_grads_ref(res["datt"][-1], res["v"][-1])[0][:, :, 1:].abs().max()) == 0.0
    # one query row is row 0 of all rows
    one = gr.weight_grads_ref(res["datt"][0][:, :1], res["v"][0])[0]
    assert float((one - gr.weight_grads_ref(res["datt"][0], res["v"][0])[0][:, :, :1]).abs().max()) <= 1e-15


def test_row_recursion_is_the_cls_row_of_the_matrix_product():
    g = torch.Generator().manual_seed(5)
    B, N, L = 2, 9, 3
    mats = [torch.relu(torch.randn(B, N, N, generator=g, dtype=F64)) for _ in range(L)]
    mats[-1][:, 1:] = 0                                                       # the last block has only its CLS row
    R = gr.relevance_matrix(mats)
    r = gr.relevance_vector(mats)
    assert float((R[:, 0] - r).abs().max()) <= 1e-13 * float(r.abs().max())
    # the CLS-only form of the last block gives the same row, bit for bit
    assert torch.equal(gr.relevance_vector(mats[:-1] + [mats[-1][:, :1]]), r)
    assert torch.equal(gr.relevance_matrix(mats[:-1] + [mats[-1][:, :1]]), R)
    # zero matrices leave e_cls
    e = torch.zeros(B, N, dtype=F64)
    e[:, 0] = 1
    assert torch.equal(gr.relevance_vector([torch.zeros(B, N, N, dtype=F64)] * 2), e)
    # one step at a time: relevance_step_ref on heads whose relu-mean is the block's matrix; the composed bound is non-negative
    heads = mats[0][:, None].expand(B, 8, N, N)
    abar, e_abar, magp = gr.relevance_matrix_ref(torch.ones_like(heads), torch.zeros_like(heads), heads, torch.zeros_like(heads), heads.abs())
    v = torch.randn(B, N, generator=g, dtype=F64)
    out, err = gr.relevance_step_ref(abar, e_abar, magp, v)
    assert float((out - (v + (v[:, None] @ mats[0])[:, 0])).abs().max()) <= 1e-13 and bool((err >= 0).all())
    _r, bound = gr.relevance_vector(mats, bounds=[1e-9 * m for m in mats])
    assert bool((bound >= 0).all())


def test_model_relevance_of_the_restatement_is_target_dependent():
    """What the feature is for: the float64 relevance rows of two targets differ, where attention rollout is the same for both."""
    _m, sd, x = cpu_model()
    rows = [gr.relevance_from_grads(gr.encoder_attention_grads(sd, x, DEPTH, "mu", k))[0] for k in (3, 7)]
    assert rows[0].shape == (MB, 7) and bool((rows[0] >= 0).all()) and float(rows[0][:, 0].min()) >= 1.0
    assert float((rows[0] - rows[1]).abs().max()) > 1e-6 * float(rows[0].abs().max())


def test_names_exist():
    from causal_vae_amd import ops, vit
    for name in ("attention_gradients", "attention_relevance"):
        assert callable(getattr(vit.ViTVAEEncoder, name)) and callable(getattr(vit.ViTVAE, name)) and callable(getattr(vit.CausalViTVAE, name))
    assert "extract_vit_relevance" in vit.__all__ and callable(vit.extract_vit_relevance)
    assert all(hasattr(vit, n) for n in vit.__all__)
    assert callable(ops.mhsa_weight_grads) and callable(ops.mhsa_relevance_step)


def test_model_methods_refuse():
    from causal_vae_amd._lib import CvaeError
    m, _sd, x = cpu_model()
    for f in (m.attention_gradients, m.attention_relevance):
        for kw, text in (({"target": "z"}, "target must be"), ({"target": "mu", "index": 16}, "index must be"), ({"index": [1, 1]}, "index must be"),
                         ({"index": True}, "index must be"), ({"target": "cls", "index": 256}, "index must be"), ({"index": []}, "index must be")):
            with pytest.raises(CvaeError, match=text):
                f(x, **kw)
        with pytest.raises(CvaeError, match="CPU tensor"):
            f(x)
        with pytest.raises(CvaeError, match="float32"):
            f(x[:, :, :32])
    for kw, text in (({"query": "patches"}, "query must be"), ({"blocks": [2]}, "blocks must name"), ({"blocks": []}, "blocks must name"),
                     ({"blocks": [-1]}, "blocks must name")):
        with pytest.raises(CvaeError, match=text):
            m.attention_gradients(x, **kw)
    try:
        m.train()
        for f in (m.attention_gradients, m.attention_relevance):
            with pytest.raises(RuntimeError, match="eval mode"):
                f(x)
    finally:
        m.eval()


def test_entries_check_their_arguments_before_any_launch():
    """Every call here is refused (or has B == 0), so nothing is enqueued: the pointers are never read."""
    from causal_vae_amd import _lib as L
    lib = L.lib
    OK, BADSHAPE, DTYPE, UNSUPPORTED, WORKSPACE, NULLPTR = 0, -1, -2, -3, -4, -6
    buf = (ctypes.c_char * 16384)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    q, k, v, lse, dout, w, r, out, ws = (base + 1024 * i for i in range(9))

    def grads(dout=dout, v=v, w=w, vs=768, vb=7 * 768, wb=8 * 7 * 7, B=2, N=7, nq=7, dt=L.F32):
        return lib.cvae_mhsa_weight_grads(dout, v, w, vs, vb, wb, B, N, nq, dt, None)

    def step(q=q, k=k, v=v, lse=lse, dout=dout, r=r, out=out, qs=768, ks=768, vs=768, qb=7 * 768, kb=7 * 768, vb=7 * 768, B=2, N=7, nq=7, dt=L.F32, ws=ws,
             wsb=4096):
        return lib.cvae_mhsa_relevance_step(q, k, v, lse, dout, r, out, qs, ks, vs, qb, kb, vb, B, N, nq, dt, ws, wsb, None)

    assert grads(B=0) == OK and step(B=0) == OK and grads(B=0, dout=None, v=None, w=None) == OK and step(B=0, q=None, r=None, out=None, ws=None) == OK
    for f in (grads, step):
        assert f(nq=0) == BADSHAPE and f(nq=8) == BADSHAPE and f(N=0) == BADSHAPE and f(B=-1) == BADSHAPE and f(B=65536) == BADSHAPE
        assert f(N=(1 << 24) + 1, nq=1) == BADSHAPE
        assert f(dt=L.FP8) == DTYPE and f(dt=7) == DTYPE and f(dt=-1) == DTYPE
        assert f(dout=None) == NULLPTR and f(v=None) == NULLPTR
        assert f(vs=255) == BADSHAPE and f(vb=-768) == BADSHAPE
        assert f(vs=770) == UNSUPPORTED and f(v=v + 4) == UNSUPPORTED and f(dout=dout + 8) == UNSUPPORTED and f(dt=L.BF16, vs=772) == UNSUPPORTED
    assert grads(w=None) == NULLPTR and grads(w=w + 4) == UNSUPPORTED
    assert grads(wb=8 * 7 * 7 - 1) == BADSHAPE and grads(nq=1, wb=8 * 7 - 1) == BADSHAPE and grads(wb=7 * 7) == BADSHAPE
    assert step(q=None) == NULLPTR and step(k=None) == NULLPTR and step(lse=None) == NULLPTR and step(r=None) == NULLPTR and step(out=None) == NULLPTR
    assert step(qs=255) == BADSHAPE and step(kb=-768) == BADSHAPE and step(qs=770) == UNSUPPORTED and step(q=q + 4) == UNSUPPORTED and step(lse=lse + 2) == UNSUPPORTED
    assert step(r=r + 2) == UNSUPPORTED and step(out=out + 1) == UNSUPPORTED
    assert step(out=r) == UNSUPPORTED and step(out=r + 4 * 13) == UNSUPPORTED      # out == r, and an out that overlaps r's [2][7] floats
    # the workspace: none is needed while the query rows fit one chunk; beyond that it is [B][chunks][N] floats, and one byte less is refused
    need = lib.cvae_mhsa_relevance_step_workspace_bytes
    assert need(2, 7, 7) == 0 and need(3, 130, 1) == 0 and need(2, 64, 64) == 0
    assert need(2, 65, 65) == 2 * 2 * 65 * 4 and need(3, 130, 130) == 3 * 3 * 130 * 4 and need(8, 961, 961) == 8 * 16 * 961 * 4
    assert need(0, 7, 7) == 0 and need(2, 7, 8) == 0 and need(2, 0, 0) == 0
    big = dict(N=65, nq=65, qb=65 * 768, kb=65 * 768, vb=65 * 768)
    assert step(**big, wsb=need(2, 65, 65) - 1) == WORKSPACE and step(**big, wsb=0) == WORKSPACE
    assert step(**big, ws=None, wsb=need(2, 65, 65)) == NULLPTR and step(**big, ws=ws + 2, wsb=need(2, 65, 65)) == UNSUPPORTED
    assert step(N=(1 << 24), nq=(1 << 24), B=1) == UNSUPPORTED                     # more chunks than a grid dimension holds
