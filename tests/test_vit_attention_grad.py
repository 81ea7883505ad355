"""GPU tests of the attention gradients and the gradient-weighted attention relevance (csrc/vit_attention_grad_probe.inc, ops.mhsa_weight_grads /
mhsa_relevance_step, ViTVAEEncoder.attention_gradients / attention_relevance).  Every comparison is against float64 with the bounds derived in
tests/vit_attention_grad_reference.py's docstring (u = 2^-24; nothing is fitted), by the project's 4 x rule (model level, fp32), or is exact (torch.equal).

Shapes: tests/test_vit_attention.py's — N = 7 (one ragged tile; a 64 x 96 image), 65 (a full 64-row tile plus one: two chunks of the relevance split), 130 (two key
workgroups, a ragged third query tile, three chunks), n_query_rows = N and 1, B = 3, fp32 and bf16 operands (bf16-exact values, float64 on the same values), q, k,
v as panels of a packed [B, N, 768] buffer and, for one query row, q as its own [B, 1, 256] tensor; operand scales 1 and 3 (flat and peaked rows).

Measured on the MI355X (largest |got - float64| / bound over all cases): mhsa_weight_grads 0.15, mhsa_relevance_step 0.24 (0.24 against the two storing
kernels' own outputs); model level, rel-L2 over the fp32 CPU evaluation's (4 allowed): attention_gradients 1.23 to 1.36, attention_relevance 1.00 to 1.07."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_attention_grad_reference as gr  # noqa: E402
import vit_attention_reference as ar  # noqa: E402
import vit_reference as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
B = 3
SHAPES = [(7, 7), (7, 1), (65, 65), (65, 1), (130, 130), (130, 1)]


def ops():
    from causal_vae_amd import ops as o
    return o


def within(got, ref, err, what):
    ratio = float(((got.detach().cpu().double() - ref).abs() / err).max())
    print(f"{what}: max |got - float64| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)


@functools.lru_cache(maxsize=None)
def case(dtype, N, nq, scale):
    """One set of operands, computed once and left unchanged: the packed buffer and the attention output's cotangent on the device, mhsa_train's lse for these
    queries, and the float64 values of the kernels' expressions on exactly these inputs (P and gA per head, Abar, each with its bound)."""
    g = torch.Generator().manual_seed(1000 * N + int(10 * scale))
    qkv = (scale * torch.randn(B, N, 768, generator=g)).to(dtype)
    dout = torch.randn(B, nq, 256, generator=g).to(dtype)
    d = qkv.to(DEV)
    q, k, v = d[:, :, :256], d[:, :, 256:512], d[:, :, 512:]
    _out, lse = ops().mhsa_train(q, k, v, n_query_rows=nq)
    p, e_p = ar.weights_from_lse(qkv[:, :, :256], qkv[:, :, 256:512], lse.cpu(), nq)
    ga, e_g, mag = gr.weight_grads_ref(dout, qkv[:, :, 512:])
    abar, e_abar, magp = gr.relevance_matrix_ref(p, e_p, ga, e_g, mag)
    return {"qkv": qkv, "q": q, "k": k, "v": v, "lse": lse, "dout": dout.to(DEV), "p": p, "e_p": e_p, "ga": ga, "e_g": e_g, "abar": abar, "e_abar": e_abar,
            "magp": magp}


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("N,nq", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_weight_grads_against_float64(dtype, N, nq, scale):
    c = case(dtype, N, nq, scale)
    got = ops().mhsa_weight_grads(c["dout"], c["v"], nq)
    assert got.shape == (B, 8, nq, N) and got.dtype == F32
    within(got, c["ga"], c["e_g"], f"weight_grads {dtype} N{N} nq{nq} scale{scale}")


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("N,nq", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_relevance_step_against_float64(dtype, N, nq, scale):
    c = case(dtype, N, nq, scale)
    o = ops()
    g = torch.Generator().manual_seed(N + nq)
    r_rand = torch.randn(B, N, generator=g) * torch.exp(2 * torch.randn(B, N, generator=g))       # random signs and magnitudes
    e_cls = torch.zeros(B, N)
    e_cls[:, 0] = 1.0
    # Abar from the two storing kernels' own outputs, in float64: they and the step round independently, hence twice the matrix bound
    own = torch.relu(o.mhsa_weight_grads(c["dout"], c["v"], nq).cpu().double() * o.mhsa_weights(c["q"], c["k"], c["lse"], nq, average_heads=False).cpu().double()).mean(1)
    for name, r in (("random", r_rand), ("e_cls", e_cls)):
        got = o.mhsa_relevance_step(c["q"], c["k"], c["v"], c["lse"], c["dout"], r.to(DEV), nq)
        assert got.shape == (B, N) and got.dtype == F32
        ref, err = gr.relevance_step_ref(c["abar"], c["e_abar"], c["magp"], r)
        within(got, ref, err, f"relevance_step {name} {dtype} N{N} nq{nq} scale{scale}")
        ref2, err2 = gr.relevance_step_ref(own, 2 * c["e_abar"], c["magp"], r)
        within(got, ref2, err2, f"relevance_step vs the stored gA and P {name} {dtype} N{N} nq{nq} scale{scale}")


@pytest.mark.parametrize("N", [7, 65, 130])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_exact_properties(dtype, N):
    from causal_vae_amd import _lib as L
    o = ops()
    full, one = case(dtype, N, N, 3.0), case(dtype, N, 1, 3.0)
    q, k, v, lse, dout = full["q"], full["k"], full["v"], full["lse"], full["dout"]
    r = torch.randn(B, N, generator=torch.Generator().manual_seed(N)).to(DEV)
    w = o.mhsa_weight_grads(dout, v)
    assert torch.equal(w, o.mhsa_weight_grads(dout, v))                                                      # two runs
    for b in range(B):                                                                                      # a batch row alone
        assert torch.equal(w[b:b + 1], o.mhsa_weight_grads(dout[b:b + 1], v[b:b + 1]))
    dout1 = dout[:, :1].contiguous()
    assert torch.equal(o.mhsa_weight_grads(dout1, v, 1), w[:, :, :1])                                        # one query row is row 0 of all rows
    big = torch.full((B, 2) + tuple(w.shape[1:]), -1.0, device=DEV)                                         # `out`: a strided batch of a larger buffer
    assert o.mhsa_weight_grads(dout, v, out=big[:, 0]) is not None and torch.equal(big[:, 0], w) and bool((big[:, 1] == -1).all())
    assert torch.equal(one["lse"], lse[:, :, :1])
    for nq, c in ((N, full), (1, one)):
        args = (c["q"], k, v, c["lse"], c["dout"])
        s = o.mhsa_relevance_step(*args, r, nq)
        assert torch.equal(s, o.mhsa_relevance_step(*args, r, nq))                                           # two runs
        for b in range(B):
            assert torch.equal(s[b:b + 1], o.mhsa_relevance_step(c["q"][b:b + 1], k[b:b + 1], v[b:b + 1], c["lse"][b:b + 1].contiguous(), c["dout"][b:b + 1],
                                                                 r[b:b + 1].contiguous(), nq))
        assert torch.equal(o.mhsa_relevance_step(c["q"], k, v, c["lse"], torch.zeros_like(c["dout"]), r, nq), r)     # dout = 0 returns r
        out = torch.empty_like(r)
        assert o.mhsa_relevance_step(*args, r, nq, out=out) is out and torch.equal(out, s)
        # a workspace one byte short is refused before anything is launched (the entry itself; ops sizes its own)
        need = L.lib.cvae_mhsa_relevance_step_workspace_bytes(B, N, nq)
        assert need == (0 if nq <= 64 else B * ((nq + 63) // 64) * N * 4)
        if need:
            ws = torch.empty(need // 4, device=DEV)
            call = lambda nbytes: L.lib.cvae_mhsa_relevance_step(
                c["q"].data_ptr(), k.data_ptr(), v.data_ptr(), c["lse"].data_ptr(), c["dout"].data_ptr(), r.data_ptr(), out.data_ptr(), c["q"].stride(1),
                k.stride(1), v.stride(1), c["q"].stride(0), k.stride(0), v.stride(0), B, N, nq, L.dtype_code(dtype), ws.data_ptr(), nbytes, None)
            assert call(need - 1) == -4
            out.fill_(-1.0)
            assert call(need) == 0 and torch.equal(out, s)
    # only r[0] non-zero: only the first row of the matrix matters, so one query row gives the bits of all rows — q as a panel, and as its own tensor
    e = torch.zeros(B, N, device=DEV)
    e[:, 0] = torch.tensor([1.0, -2.5, 0.3], device=DEV)
    row0 = o.mhsa_relevance_step(q, k, v, lse, dout, e, N)
    assert torch.equal(row0, o.mhsa_relevance_step(q, k, v, one["lse"], dout1, e, 1))
    assert torch.equal(row0, o.mhsa_relevance_step(q[:, :1].contiguous(), k, v, one["lse"], dout1, e, 1))


def test_refusals():
    from causal_vae_amd._lib import CvaeError
    o = ops()
    c = case(F32, 7, 7, 1.0)
    q, k, v, lse, dout = c["q"], c["k"], c["v"], c["lse"], c["dout"]
    r = torch.zeros(B, 7, device=DEV)
    bad = [lambda: o.mhsa_weight_grads(dout[:, :6], v),                                     # dout: not contiguous / the wrong rows
           lambda: o.mhsa_weight_grads(dout, v, 6),
           lambda: o.mhsa_weight_grads(dout.bfloat16(), v),                                 # mixed dtypes
           lambda: o.mhsa_weight_grads(dout, v, 0), lambda: o.mhsa_weight_grads(dout, v, 8),
           lambda: o.mhsa_weight_grads(dout, v, out=torch.empty(B, 8, 7, 8, device=DEV)),
           lambda: o.mhsa_weight_grads(dout.cpu(), v.cpu()),
           lambda: o.mhsa_relevance_step(q, k, v, lse[:, :, :6].contiguous(), dout, r),
           lambda: o.mhsa_relevance_step(q, k, v, lse.double(), dout, r),
           lambda: o.mhsa_relevance_step(q, k, v.bfloat16(), lse, dout, r),
           lambda: o.mhsa_relevance_step(q, k, v[:, :6], lse, dout, r),
           lambda: o.mhsa_relevance_step(q, k, v, lse, dout.transpose(1, 2).contiguous().transpose(1, 2), r),
           lambda: o.mhsa_relevance_step(q, k, v, lse, dout, r, out=r),                      # out is r
           lambda: o.mhsa_relevance_step(q, k, v, lse, dout, r.double()),
           lambda: o.mhsa_relevance_step(q, k, v, lse, dout, r[:, :6]),
           lambda: o.mhsa_relevance_step(q, k, v, lse, dout, r, 0), lambda: o.mhsa_relevance_step(q, k, v, lse, dout, r, 8)]
    for f in bad:
        with pytest.raises(CvaeError):
            f()
    with pytest.raises(CvaeError):
        o.mhsa_weight_grads(dout.clone().requires_grad_(True), v)                            # forward-only
    assert o.mhsa_weight_grads(dout[:0], v[:0]).shape == (0, 8, 7, 7) and o.mhsa_relevance_step(q[:0], k[:0], v[:0], lse[:0], dout[:0], r[:0]).shape == (0, 7)


# ---- model level ----------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 96), (128, 160)]            # N = 7 and 21
DEPTH, MB = 2, 2
TARGETS = [("mu", 3), ("cls", 5)]            # one coordinate each: the sum of all 256 LayerNorm outputs has a gradient of zero up to rounding


@functools.lru_cache(maxsize=None)
def built(H, W, dtype):
    from causal_vae_amd.vit import ViTVAEEncoder
    torch.manual_seed(H + W)
    m = ViTVAEEncoder(img_size=(H, W), depth=DEPTH, latent_dim=16)
    vr.randomize_stem_bn(m.stem, H)
    return m.requires_grad_(False).to(DEV).eval().set_compute_dtype(dtype), vr.vit_inputs(MB, H, W, W).to(DEV)


def hooked(m, x, target, index, cls_only_last):
    """What the backward's hook hands out, per block from the last to the first: (i, q, k, v, lse, datt, n_query_rows)."""
    g = m._target_cotangent("test", x.shape[0], target, index, x.device)
    seen = []
    m._data_backward(x, m._head_cotangent(target, g), stem=False, attention_grad=lambda *a: seen.append(a), cls_only_last=cls_only_last)
    assert [a[0] for a in seen] == list(reversed(range(DEPTH)))
    return seen


@pytest.mark.parametrize("target,index", TARGETS)
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_model_is_the_ops_on_the_hooks_tensors(H, W, dtype, target, index):
    m, x = built(H, W, dtype)
    N = m.num_patches + 1
    o = ops()
    for full_last in (False, True):
        seen = hooked(m, x, target, index, not full_last)
        assert all(a[1].dtype == dtype and a[5].dtype == dtype for a in seen) and seen[0][6] == 1 and seen[1][6] == N
        # attention_gradients: the CLS form is row 0 of every block; the full form has the last block's rows >= 1 zero
        want = {i: (v, datt, nq) for i, _q, _k, v, _lse, datt, nq in seen}
        got = m.attention_gradients(x, target, index, query="all" if full_last else "cls")
        assert got.shape == (MB, DEPTH, 8, N if full_last else 1, N) and got.dtype == F32
        for i in range(DEPTH):
            v, datt, nq = want[i]
            if full_last and nq == N:
                assert torch.equal(got[:, i], o.mhsa_weight_grads(datt, v, N))
            else:
                assert torch.equal(got[:, i, :, :1], o.mhsa_weight_grads(datt[:, :1].contiguous(), v, 1))
                assert not full_last or float(got[:, i, :, 1:].abs().max()) == 0.0
        assert torch.equal(m.attention_gradients(x, target, index, blocks=(1, 0)), m.attention_gradients(x, target, index)[:, [1, 0]])
        # attention_relevance: one step per block, the last block first; the model's flag decides the last block's forward, the bits are the same
        r = torch.zeros(MB, N, device=DEV)
        r[:, 0] = 1.0
        for _i, q, k, v, lse, datt, nq in seen:
            r = o.mhsa_relevance_step(q, k, v, lse, datt, r, nq)
        try:
            m._cls_only_last_block = not full_last
            row = m.attention_relevance(x, target, index, as_grid=False)
            assert row.shape == (MB, N) and row.dtype == F32 and torch.equal(row, r)
            grid = m.attention_relevance(x, target, index)
            assert grid.shape == (MB, m.grid_h, m.grid_w) and torch.equal(grid, row[:, 1:].reshape(MB, m.grid_h, m.grid_w))
        finally:
            del m._cls_only_last_block                                       # back to the class's default
    # row 0 of the full form is the CLS form, and both last-block forms gave the same relevance
    assert torch.equal(m.attention_gradients(x, target, index, query="all")[:, :, :, :1], m.attention_gradients(x, target, index))
    assert torch.equal(m.attention_relevance(x, target, index, as_grid=False), r)
    assert m.attention_gradients(x[:0], target, index).shape == (0, DEPTH, 8, 1, N) and m.attention_relevance(x[:0], target, index).shape == (0, m.grid_h, m.grid_w)


@functools.lru_cache(maxsize=None)
def references(H, W, target, index):
    m, x = built(H, W, F32)
    sd = {k_: v.detach().cpu() for k_, v in m.state_dict().items()}
    r64 = gr.encoder_attention_grads({k_: v.double() for k_, v in sd.items()}, x.cpu(), DEPTH, target, index, F64)
    r32 = gr.encoder_attention_grads(sd, x.cpu(), DEPTH, target, index, F32)
    return r64, r32


@pytest.mark.parametrize("target,index", TARGETS)
@pytest.mark.parametrize("H,W", SIZES)
def test_model_against_float64_autograd(H, W, target, index):
    """fp32 against torch autograd (retain_grad on the probabilities) of the float64 restatement, by the 4 x rule: rel-L2 at most four times the gap of an fp32
    CPU evaluation of the same restatement.  Measured on the MI355X: see DESIGN §22."""
    m, x = built(H, W, F32)
    r64, r32 = references(H, W, target, index)
    got = m.attention_gradients(x, target, index, query="all").cpu()
    ref64, ref32 = torch.stack(r64["gA"], dim=1), torch.stack(r32["gA"], dim=1)
    mine, yard = vr.rel_l2(got, ref64), vr.rel_l2(ref32, ref64)
    print(f"attention_gradients {H}x{W} {target}: rel-L2 {mine:.3e}, fp32 CPU evaluation {yard:.3e}, ratio {mine / yard:.3f} (allowed 4)")
    assert mine <= 4 * yard
    row = m.attention_relevance(x, target, index, as_grid=False).cpu()
    rel64, rel32 = gr.relevance_from_grads(r64)[0], gr.relevance_from_grads(r32)[0]
    mine, yard = vr.rel_l2(row, rel64), vr.rel_l2(rel32, rel64)
    print(f"attention_relevance {H}x{W} {target}: rel-L2 {mine:.3e}, fp32 CPU evaluation {yard:.3e}, ratio {mine / yard:.3f} (allowed 4)")
    assert mine <= 4 * yard
    assert bool((row >= 0).all()) and float(row[:, 0].min()) >= 1.0           # R = I + non-negative terms


@pytest.mark.parametrize("H,W", SIZES)
def test_no_side_effects(H, W):
    m, x = built(H, W, F32)
    g = torch.ones(MB, 16, device=DEV)

    def state():
        return (m.cls_features(x), m.dropout_keys.step, m._cls_only_last_block, "_cls_only_last_block" in vars(m) and vars(m)["_cls_only_last_block"],
                {k_: v.clone() for k_, v in m.state_dict().items()}, m.training, [p.requires_grad for p in m.parameters()], m.encode_vjp(x, g),
                [p.grad is None for p in m.parameters()])

    def same(a, b):
        assert torch.equal(a[0], b[0]) and a[1:4] == b[1:4] and a[5:7] == b[5:7] and torch.equal(a[7], b[7]) and a[8] == b[8]
        assert a[4].keys() == b[4].keys() and all(torch.equal(a[4][k_], b[4][k_]) for k_ in a[4])

    def calls():
        m.attention_gradients(x)
        m.attention_gradients(x, "log_var", [0, 5], query="all", blocks=[1])
        m.attention_relevance(x)
        m.attention_relevance(x, "cls", 7, as_grid=False)

    before = state()
    calls()
    same(before, state())
    ref = m.attention_relevance(x)
    try:
        m.train_transformer(dropout=True)                                     # the training forward would drop; these never do, and take no key
        before = state()
        calls()
        same(before, state())
        assert torch.equal(m.attention_relevance(x), ref)
    finally:
        m.freeze_transformer()


def test_delegates():
    from causal_vae_amd.vit import CausalViTVAE, extract_vit_relevance
    torch.manual_seed(2)
    c = CausalViTVAE(img_size=(64, 96), depth=2).to(DEV).eval()
    vr.randomize_stem_bn(c.backbone.stem, 3)
    xs = [vr.vit_inputs(2, 64, 96, 5), vr.vit_inputs(1, 64, 96, 6)]
    maps = [c.backbone.attention_relevance(x.to(DEV)) for x in xs]
    assert torch.equal(c.attention_relevance(xs[0].to(DEV)), maps[0])
    assert torch.equal(c.attention_relevance(xs[0].to(DEV), target="log_var", index=2, as_grid=False),
                       c.backbone.attention_relevance(xs[0].to(DEV), target="log_var", index=2, as_grid=False))
    assert torch.equal(c.attention_gradients(xs[0].to(DEV), target="cls", query="all"), c.backbone.attention_gradients(xs[0].to(DEV), target="cls", query="all"))
    loader = [{"x": x} for x in xs]
    want = torch.cat(maps).cpu().numpy()
    for model in (c, c.backbone):
        got = extract_vit_relevance(model, loader, DEV)
        assert got.shape == (3, 2, 3) and got.dtype == want.dtype and (got == want).all()
    assert extract_vit_relevance(c, [], DEV).shape == (0, 2, 3) and extract_vit_relevance(c, [], DEV, as_grid=False).shape == (0, 7)
    got = extract_vit_relevance(c, loader, DEV, target="cls", index=[1, 2], as_grid=False)
    assert (got == torch.cat([c.attention_relevance(x.to(DEV), target="cls", index=[1, 2], as_grid=False) for x in xs]).cpu().numpy()).all()
    # the map depends on the target, which attention rollout cannot
    assert not torch.equal(c.attention_relevance(xs[0].to(DEV), index=0), c.attention_relevance(xs[0].to(DEV), index=1))
