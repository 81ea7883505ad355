"""GPU tests of the ViT training step as one HIP graph: the device-resident dropout keys (cvae_dropout_keys_step, ops.DeviceDropoutKeys), the
*_devkey forms of the five dropout entries, vit_vae_train_step / causal_vit_train_step and GraphedViTTrainStep.

Everything here is an exact comparison.  The key table is compared with ops.DropoutKeys.key as integers; a device-key launch with the by-value launch of
the same key, and a captured run with the eager run of the same recipe, with torch.equal: the captured graph holds the launches the eager step issues
(plus one key-table launch per walk), in the same order on the same operands, and no kernel here uses atomics, so there is no rounding to allow for.  Each
run comparison first asserts its premise — two eager runs from one state agree bit for bit — so that a failure points at the captured side."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as vd  # noqa: E402
import vit_dropout_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
KEY_A, KEY_B = 0x1234567890ABCDEF, 0x0FEDCBA987654321
IMG, DEPTH, B = (64, 96), 2, 2
P = 0.1


def ops():
    from causal_vae_amd import ops as o
    return o


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


def dev_key(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


# ---- the key table -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [1, 6, 65536])
@pytest.mark.parametrize("step", [0, 1, 2 ** 20 + 3, 2 ** 43 + 1])
@pytest.mark.parametrize("seed", [5, 0xFEDCBA9876543210])
def test_key_table_is_dropout_keys_key(seed, step, n_blocks):
    o = ops()
    host = o.DropoutKeys(seed)
    keys = o.DeviceDropoutKeys(n_blocks, DEV, seed=seed, step=step)
    assert keys.state() == {"seed": seed, "step": step}
    table = keys.advance()
    assert table.shape == (n_blocks, 4) and table.dtype == torch.int64
    got = table.cpu().numpy().view(np.uint64)
    want = np.array([[host.key(step, b, site) for site in range(3)] for b in range(n_blocks)], dtype=np.uint64)
    assert np.array_equal(got[:, :3], want)
    assert keys.state()["step"] == step + 1
    view = keys.key(table, n_blocks - 1, host.MLP_OUT)
    assert view.shape == (1,) and view.data_ptr() == table.data_ptr() + 8 * (4 * (n_blocks - 1) + 2)


def test_two_advances_give_two_tables_and_the_state_interchanges():
    o = ops()
    keys = o.DeviceDropoutKeys(DEPTH, DEV, seed=5, step=7)
    first, second = keys.advance(), keys.advance()
    torch.cuda.synchronize()
    assert first.data_ptr() != second.data_ptr()
    host = o.DropoutKeys(5)
    as_int = lambda t, b, s: int(t[b, s].item()) & ((1 << 64) - 1)
    for b in range(DEPTH):
        for site in range(3):
            assert as_int(first, b, site) == host.key(7, b, site) and as_int(second, b, site) == host.key(8, b, site)
    assert keys.state() == {"seed": 5, "step": 9}
    moved = o.DropoutKeys(1).load_state(keys.state())                       # device -> host -> device
    assert moved.state() == {"seed": 5, "step": 9}
    back = o.DeviceDropoutKeys(DEPTH, DEV, seed=1).load_state(moved.state())
    assert back.state() == {"seed": 5, "step": 9} and torch.equal(back.advance(), o.DeviceDropoutKeys(DEPTH, DEV, seed=5, step=9).advance())


# ---- the device-key forms equal the by-value forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,rows", [((3, 256), (5, 3)), ((70, 512), ())])
def test_dropout_rows_devkey(shape, rows):
    o = ops()
    x, t = rand(*shape, seed=1), dev_key(KEY_A)
    assert torch.equal(o.dropout_rows(x, (P, t) + rows), o.dropout_rows(x, (P, KEY_A) + rows))
    assert not torch.equal(o.dropout_rows(x, (P, dev_key(KEY_B)) + rows), o.dropout_rows(x, (P, KEY_A) + rows))


def test_token_gemm_devkey():
    o = ops()
    M = 129
    y2, hid = rand(M, 256, seed=1), rand(M, 512, seed=2)
    W1, b1, W2, b2 = rand(512, 256, seed=3, scale=0.1), rand(512, seed=4), rand(256, 512, seed=5, scale=0.1), rand(256, seed=6)
    resid, g = rand(M, 256, seed=7), rand(M, 256, seed=8)
    t = dev_key(KEY_A)
    for a, b in zip(o.token_gemm_dropout(y2, W1, b1, "gelu", (P, t)), o.token_gemm_dropout(y2, W1, b1, "gelu", (P, KEY_A))):
        assert torch.equal(a, b)
    res = lambda key: o.token_gemm_dropout(hid, W2, b2, "residual", (P, key, 0, 7), resid=resid, out=torch.empty_like(resid))
    assert torch.equal(res(t), res(KEY_A))
    pre = o.token_gemm_dropout(y2, W1, b1, "gelu", (P, KEY_A))[1]
    for gate in (pre, None):
        assert torch.equal(o.token_gemm_bwd_data(g, W2, F32, gate_pre=gate, dropout=(P, t)), o.token_gemm_bwd_data(g, W2, F32, gate_pre=gate, dropout=(P, KEY_A)))


@pytest.mark.parametrize("one", [False, True])
@pytest.mark.parametrize("N", [7, 65, 130])
def test_attention_devkey(N, one):
    o = ops()
    nq = 1 if one else N
    qkv = rand(B, N, 768, seed=N)
    q, k, v = qkv[:, :, :256], qkv[:, :, 256:512], qkv[:, :, 512:]
    t = dev_key(KEY_A)
    out_t, lse_t = o.mhsa_train(q, k, v, n_query_rows=nq, dropout=(P, t))
    out_v, lse_v = o.mhsa_train(q, k, v, n_query_rows=nq, dropout=(P, KEY_A))
    assert torch.equal(out_t, out_v) and torch.equal(lse_t, lse_v)
    dout = rand(B, nq, 256, seed=N + 1)

    def bwd(key):
        d = torch.full_like(qkv, 7.0)
        o.mhsa_bwd(q, k, v, out_v, lse_v, dout, d[:, :nq, :256], d[:, :, 256:512], d[:, :, 512:], dropout=(P, key))
        return d
    assert torch.equal(bwd(t), bwd(KEY_A))


def test_tensor_key_refusals():
    o = ops()
    x = rand(3, 256)
    from causal_vae_amd._lib import CvaeError
    for bad in (torch.tensor([KEY_A]), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)):
        with pytest.raises(CvaeError, match="tensor key"):
            o.dropout_rows(x, (P, bad))


def test_the_key_is_read_when_the_graph_runs():
    o = ops()
    M, N = 3, 256
    ones, t, out = torch.ones(M, N, device=DEV), dev_key(KEY_A), torch.empty(M, N, device=DEV)
    o.dropout_rows(ones, (P, t), out=out)                                   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o.dropout_rows(ones, (P, t), out=out)
    s = np.float32(1.0) / (np.float32(1.0) - np.float32(P))
    for key in (KEY_A, KEY_B):
        t.fill_(key)
        out.zero_()
        graph.replay()
        assert np.array_equal(out.cpu().numpy(), dr.keep_rows(M, N, P, key).astype(np.float32) * s), hex(key)


# ---- models and runs -----------------------------------------------------------------------------------------------------------------------------
def vitvae(dropout, dtype=F32, seed=0):
    from causal_vae_amd.vit.models import ViTVAE
    torch.manual_seed(seed)
    model = ViTVAE(img_size=IMG, depth=DEPTH, latent_dim=128)
    vr.randomize_stem_bn(model.stem, seed + 1)
    vd.randomize_decoder_bn(model.decoder, seed + 2)
    model = model.to(DEV).eval().set_compute_dtype(dtype)
    model.dropout_keys = ops().DropoutKeys(seed=77)
    model.train_all(dropout=dropout)
    return model


def causal_vitvae(seed=5):
    from causal_vae_amd.vit.causal import CausalViTVAE
    torch.manual_seed(seed)
    model = CausalViTVAE(img_size=IMG, depth=DEPTH)
    vd.randomize_decoder_bn(model.backbone.decoder, seed + 1)
    vr.randomize_stem_bn(model.backbone.stem, seed + 2)
    model = model.to(DEV)
    model.backbone.dropout_keys = ops().DropoutKeys(seed=78)
    return model, model.train_adapters(decoder=True, transformer=True, stem=True, dropout=True)


def vit_batches(n=3):
    return [(vr.vit_inputs(B, *IMG, seed=11 + i).to(DEV),) for i in range(n)], [rand(B, 128, seed=40 + i) for i in range(n)]


def causal_batches(model, n=3):
    gen = torch.Generator().manual_seed(8)
    batches = [(torch.rand(B, 1, *IMG, generator=gen).to(DEV), torch.randn(B, model.m_dim, generator=gen).to(DEV),
                torch.randn(B, model.t_dim, generator=gen).to(DEV)) for _ in range(n)]
    return batches, [rand(B, model.my_z_dim, seed=50 + i) for i in range(n)]


def adam(params):
    from causal_vae_amd import FusedAdam
    return FusedAdam(params, lr=1e-3, device_step=True)


def adam_state(opt):
    """[(step, exp_avg, exp_avg_sq)] in parameter order; state_dict() reads the device step count back"""
    st = opt.state_dict()["state"]
    return [(int(st[i]["step"]), st[i]["exp_avg"].clone(), st[i]["exp_avg_sq"].clone()) for i in sorted(st)]


def drop_step(model):
    enc = getattr(model, "backbone", model)
    return enc.dropout_keys.state()["step"]


def same_tensors(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def assert_same_training_state(m1, o1, m2, o2, what):
    assert same_tensors(m1.parameters(), m2.parameters()), f"{what}: parameters"
    assert same_tensors(m1.buffers(), m2.buffers()), f"{what}: buffers (BatchNorm statistics and counters)"
    s1, s2 = adam_state(o1), adam_state(o2)
    assert len(s1) == len(s2) > 0
    for (t1, a1, v1), (t2, a2, v2) in zip(s1, s2):
        assert t1 == t2 and torch.equal(a1, a2) and torch.equal(v1, v2), f"{what}: Adam state"


def eager_run(model, params, step_fn, batches, noises, **recipe):
    opt = adam(params)
    outs = [step_fn(model, opt, *b, eps=e, **recipe) for b, e in zip(batches, noises)]
    return opt, [tuple(t.clone() for t in (o if isinstance(o, tuple) else (o,))) for o in outs]


def captured_run(model, params, batches, noises, **recipe):
    from causal_vae_amd.vit import GraphedViTTrainStep
    opt = adam(params)
    step = GraphedViTTrainStep(model, opt, batches[0], eps=noises[0], **recipe)
    outs = []
    for b, e in zip(batches, noises):
        o = step(*b, eps=e)
        outs.append(tuple(t.clone() for t in (o if isinstance(o, tuple) else (o,))))
    return opt, outs


# ---- constructing the captured step does not train -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepped", [False, True])
def test_construction_does_not_train(stepped):
    from causal_vae_amd.vit import GraphedViTTrainStep, causal_vit_train_step
    model, params = causal_vitvae()
    batches, noises = causal_batches(model, 2)
    opt = adam(params)
    if stepped:                                                             # moments, step count, BatchNorm1d counters and the dropout step are past zero
        causal_vit_train_step(model, opt, *batches[1], eps=noises[1])
    keys_before = sorted(model.state_dict())
    ref_model = copy.deepcopy(model)
    ref_adam = adam_state(opt) if stepped else None
    ref_drop = drop_step(model)
    assert ref_drop == (1 if stepped else 0)
    step = GraphedViTTrainStep(model, opt, batches[0], eps=noises[0], warmup=2)
    assert isinstance(model.backbone.dropout_keys, ops().DeviceDropoutKeys) and sorted(model.state_dict()) == keys_before
    assert same_tensors(model.parameters(), ref_model.parameters()) and same_tensors(model.buffers(), ref_model.buffers())
    assert any(k.endswith("num_batches_tracked") for k in keys_before)
    assert drop_step(model) == ref_drop
    got = adam_state(opt)
    if stepped:
        for (t1, a1, v1), (t2, a2, v2) in zip(got, ref_adam):
            assert t1 == t2 == 1 and torch.equal(a1, a2) and torch.equal(v1, v2)
    else:
        assert all(t == 0 and not a.any() and not v.any() for t, a, v in got)
    assert step.eps is not noises[0] and torch.equal(step.eps, noises[0])


# ---- captured equals eager -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dropout", [(F32, False), (torch.bfloat16, False), (F32, True)], ids=["fp32", "bf16", "fp32-dropout"])
def test_captured_equals_eager_vitvae(dtype, dropout):
    from causal_vae_amd.vit import vit_vae_train_step
    start = vitvae(dropout, dtype)
    batches, noises = vit_batches()
    runs = []
    for _ in range(2):
        m = copy.deepcopy(start)
        runs.append((m,) + eager_run(m, m.parameters(), vit_vae_train_step, batches, noises, beta=0.7))
    (m1, o1, l1), (m2, o2, l2) = runs
    assert all(torch.equal(a[0], b[0]) for a, b in zip(l1, l2))
    assert_same_training_state(m1, o1, m2, o2, "premise: two eager runs")
    assert not same_tensors(m1.parameters(), start.parameters())            # it trained

    mc = copy.deepcopy(start)
    oc, lc = captured_run(mc, mc.parameters(), batches, noises, beta=0.7)
    assert isinstance(mc.dropout_keys, ops().DeviceDropoutKeys) == dropout and isinstance(m1.dropout_keys, ops().DropoutKeys)
    for i, (a, b) in enumerate(zip(l1, lc)):
        print(f"step {i}: eager loss {float(a[0])!r}, captured loss {float(b[0])!r}")
    for i, (a, b) in enumerate(zip(l1, lc)):
        assert torch.equal(a[0], b[0]), f"loss of step {i}"
    assert_same_training_state(m1, o1, mc, oc, "captured against eager")
    assert drop_step(m1) == drop_step(mc) == (3 if dropout else 0)


def test_captured_equals_eager_causal_vitvae():
    from causal_vae_amd.vit import causal_vit_train_step
    start, _params = causal_vitvae()
    batches, noises = causal_batches(start)
    trainable = lambda m: [p for p in m.parameters() if p.requires_grad]
    runs = []
    for _ in range(2):
        m = copy.deepcopy(start)
        runs.append((m,) + eager_run(m, trainable(m), causal_vit_train_step, batches, noises))
    (m1, o1, l1), (m2, o2, l2) = runs
    assert all(same_tensors(a, b) for a, b in zip(l1, l2))
    assert_same_training_state(m1, o1, m2, o2, "premise: two eager runs")
    assert not same_tensors(m1.parameters(), start.parameters())

    mc = copy.deepcopy(start)
    oc, lc = captured_run(mc, trainable(mc), batches, noises)
    for i, (a, b) in enumerate(zip(l1, lc)):
        print(f"step {i}: eager (loss, recon, kld, morph) {[float(v) for v in a]!r}, captured {[float(v) for v in b]!r}")
    for i, (a, b) in enumerate(zip(l1, lc)):
        assert len(a) == len(b) == 4 and same_tensors(a, b), f"(loss, recon, kld, morph) of step {i}"
    assert_same_training_state(m1, o1, mc, oc, "captured against eager")
    heads = {k: v for k, v in mc.state_dict().items() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked") and "backbone" not in k}
    assert heads and all(torch.equal(v, m1.state_dict()[k]) for k, v in heads.items())
    assert any(k.endswith("num_batches_tracked") and int(v) == 3 for k, v in heads.items())
    assert drop_step(m1) == drop_step(mc) == 3


def test_noise_is_drawn_inside_the_graph():
    from causal_vae_amd.vit import GraphedViTTrainStep
    model = vitvae(False)
    (x,), = vit_batches(1)[0]
    step = GraphedViTTrainStep(model, adam(model.parameters()), (x,), warmup=1)
    step()
    first = step.eps.clone()
    loss = step(x).clone()
    assert not torch.equal(first, step.eps) and bool(first.any()) and bool(torch.isfinite(loss))
    from causal_vae_amd._lib import CvaeError
    with pytest.raises(CvaeError, match="draws its own noise"):
        step(x, eps=first)


def test_train_vit_vae_with_a_graph():
    from causal_vae_amd.vit import train_vit_vae
    model = vitvae(False)
    start = [p.detach().clone() for p in model.parameters()]
    loader = [{"x": vr.vit_inputs(b, *IMG, seed=60 + i)} for i, b in enumerate((B, B, B, 1))]
    losses = train_vit_vae(model, loader, adam(model.parameters()), DEV, epochs=1, dropout=True, graph=True)
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert isinstance(model.dropout_keys, ops().DeviceDropoutKeys) and drop_step(model) == 4      # three replays and the eager ragged batch
    changed = [not torch.equal(a, b) for a, b in zip(start, model.parameters())]
    print(f"{sum(changed)} of {len(changed)} parameter tensors moved")
    assert sum(changed) > len(changed) // 2                                 # it trained (a tensor whose gradient is exactly zero stays where it was)
    assert sorted(model.use_device_dropout_keys(False).state_dict()) == sorted(vitvae(False).state_dict()) and model.dropout_keys.step == 4
