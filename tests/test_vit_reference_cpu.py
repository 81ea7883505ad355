"""CPU checks of the ViT-VAE encoder's yardsticks (no GPU): tests/vit_reference.py against the goldens captured from the reference ViTVAE, the k3 -> k4
zero embedding and BatchNorm fold restated in float64, the position-embedding resize, and the C ABI's new entries.

The goldens are fp32 (torch on the CPU); the restatement is float64; the bound is vit_reference.composed_bound: the per-layer fp32 bounds (accumulation
lengths, u = 2^-24) composed over depth through the actual Jacobian action, rounding errors at their worst-case magnitudes with independent signs, three
sigma.  The reference's own rounding must lie inside it — that pins the restatement to every stored array of both goldens — and the bound must stay a
small fraction of the values it guards, else it would be useless for the kernels.
Printed by test_float64_restatement_matches_golden (CPU): bound / ||value|| 2e-4 .. 1e-3 for token streams, CLS rows, cls_out, mu, log_var and 6.5e-3 for the
stem (K = 16 x 256 + 5 at worst-case magnitude) in both cases; ||golden - float64|| / bound 1.7e-5 (stem) .. 4.3e-4: fp32 arithmetic does about
sqrt(K) x better than the worst-case magnitudes the model is fed with."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402

CASES = {"vitvae_enc_256x320": True, "vitvae_enc_768x1280": False}


def reference_state(g):
    """The encoder state_dict of a golden: the seed's draws + the seeded BatchNorm statistics, checked against the stored digests."""
    from causal_vae_amd.vit import ViTVAEEncoder
    B, H, W, depth, seed_model, seed_bn, seed_data = (int(v) for v in g.z["in/seed"])
    torch.manual_seed(seed_model)
    model = ViTVAEEncoder(img_size=(H, W), depth=depth)
    vr.randomize_stem_bn(model.stem, seed_bn)
    sd = model.state_dict()
    assert sorted(sd) == g.keys("sd0")
    for k, v in sd.items():
        g.check("sd0", k, v, rtol=0, atol=0)
    x = vr.vit_inputs(B, H, W, seed_data)
    g.check("in", "x", x, rtol=0, atol=0)
    return model, sd, x, depth


@pytest.mark.parametrize("name", list(CASES))
def test_float64_restatement_matches_golden(golden, name):
    g = golden(name)
    _model, sd, x, depth = reference_state(g)
    if CASES[name]:
        assert np.array_equal(np.unpackbits(g.z["in/x_bits"])[:x.numel()], x.numpy().astype(np.uint8).reshape(-1))
    bound, ref = vr.composed_bound(sd, x, depth, key=name)
    stored = [k for k in ref if g.has("out/" + k)]
    assert {"mu", "log_var", "cls_out"} | {f"cls_row{i}" for i in range(depth)} <= set(stored)
    if CASES[name]:
        assert {"stem"} | {f"tokens{i}" for i in range(depth - 1)} <= set(stored)
    for key in ref:
        rel = bound[key] / float(ref[key].norm())
        assert 0.0 < rel < 1e-2, (key, rel, "the bound must be finite and a small fraction of the values it guards")
        if key in stored:
            ratio = vr.fro_ratio(g.t("out/" + key), ref[key], bound[key])
            print(f"{name} {key}: ||golden - float64|| / bound = {ratio:.2e}; bound / ||value|| = {rel:.2e}")
            assert ratio <= 1.0, (key, ratio)
    if CASES[name]:
        # the last token stream is stored as a digest: sums of n elements move by at most sqrt(n) ||diff||_F <= sqrt(n) bound, an element by at most the bound
        k = f"tokens{depth - 1}"
        g.check("out", k, ref[k].float(), rtol=bound[k] / float(ref[k].norm()), atol=bound[k] / 20)


def test_what_the_bound_refuses(golden):
    """What the composed bound can tell apart, so that nobody reads more into it: a result off by a factor 1 + 2^-9 (a quarter of a bf16 ulp) leaves the
    bound at every stage but the stem (there 1 + 2^-7: K = 4101 at worst-case magnitude makes the stem bound 6.5e-3 of the value); the bf16 rounding
    oracle leaves it at the CLS rows, cls_out, mu and log_var.  On the full token streams bf16 operand rounding sits AT the bound (0.9 - 1.2 of it):
    the bound guards fp32 arithmetic against errors of 1e-3 and up, not against a few ulp."""
    name = "vitvae_enc_256x320"
    g = golden(name)
    _model, sd, x, depth = reference_state(g)
    bound, ref = vr.composed_bound(sd, x, depth, key=name)
    for key in ref:
        f = 1 + 2.0 ** (-7 if key == "stem" else -9)
        assert vr.fro_ratio(ref[key] * f, ref[key], bound[key]) > 1.0, key
    rounded = vr.flat(vr.encode_ref(sd, x, depth, rnd=vr.round_bf16), depth)
    for key in ("mu", "log_var", "cls_out", "cls_row0", "cls_row1"):
        assert vr.fro_ratio(rounded[key], ref[key], bound[key]) > 1.0, key


def test_rounding_oracle_gap_is_what_the_gpu_test_uses(golden):
    """The bf16 whole-model tolerance of tests/test_vit_encoder.py is 2 x this gap; it is computed there again — here it is printed for DESIGN §10."""
    g = golden("vitvae_enc_768x1280")
    _model, sd, x, depth = reference_state(g)
    plain = vr.flat(vr.encode_ref(sd, x, depth), depth)
    orac = vr.flat(vr.encode_ref(sd, x, depth, rnd=vr.round_bf16), depth)
    gaps = {k: vr.rel_l2(orac[k], plain[k]) for k in ("mu", "cls_out", "log_var")}
    print("rounding oracle vs float64, rel-L2:", gaps)
    assert all(1e-4 < v < 5e-2 for v in gaps.values()), gaps        # bf16 rounding is there (not 0) and the model does not blow it up


def test_k3_zero_embedding_and_fold_equal_conv_bn_in_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 12, 20, generator=gen, dtype=torch.float64)
    w3 = torch.randn(16, 8, 3, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(16, generator=gen, dtype=torch.float64)
    gam, bet, mean = (torch.randn(16, generator=gen, dtype=torch.float64) for _ in range(3))
    var = 0.5 + torch.rand(16, generator=gen, dtype=torch.float64)
    w4 = torch.zeros(16, 8, 4, 4, dtype=torch.float64)
    w4[:, :, :3, :3] = w3
    y3, y4 = F.conv2d(x, w3, b, stride=2, padding=1), F.conv2d(x, w4, b, stride=2, padding=1)
    assert y3.shape == y4.shape and float((y3 - y4).abs().max()) == 0.0
    want = F.batch_norm(y3, mean, var, gam, bet, training=False, eps=1e-5)
    s = gam / torch.sqrt(var + 1e-5)
    got = F.conv2d(x, w4 * s[:, None, None, None], (b - mean) * s + bet, stride=2, padding=1)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_pos_embedding_resize(golden):
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import resize_pos_embedding
    gen = torch.Generator().manual_seed(3)
    pos = torch.randn(1, 1 + 8 * 10, 256, generator=gen)
    assert resize_pos_embedding(pos, (8, 10), (8, 10)) is pos
    out = resize_pos_embedding(pos, (8, 10), (4, 5))
    assert out.shape == (1, 21, 256) and torch.equal(out[:, 0], pos[:, 0])
    grid = pos[:, 1:].transpose(1, 2).reshape(1, 256, 8, 10)
    want = F.interpolate(grid, size=(4, 5), mode="bicubic", align_corners=False)
    assert torch.equal(out[:, 1:].transpose(1, 2).reshape(1, 256, 4, 5), want)
    const = torch.cat([pos[:, :1], torch.full((1, 80, 256), 0.25)], dim=1)        # a constant grid stays constant at any size
    up = resize_pos_embedding(const, (8, 10), (24, 40))
    assert up.shape == (1, 961, 256) and torch.allclose(up[:, 1:], torch.full((1, 960, 256), 0.25), atol=1e-6)
    with pytest.raises(CvaeError):
        resize_pos_embedding(pos, (9, 9), (4, 5))


def test_header_exports_and_ctypes_table_hold_the_vit_entries():
    import ctypes
    from causal_vae_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvae_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "causal_vae_amd", "libcvae_hip.so"))
    for n in ("cvae_vit_tokens", "cvae_layernorm256", "cvae_token_gemm", "cvae_mhsa_fwd"):
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert re.search(r"#define\s+CVAE_ACT_LEAKY001\s+4\b", src) and _lib.act_code("leaky001") == 4
    assert re.search(r"#define\s+CVAE_FOLD_CONV_K3S2\s+3\b", src) and ops.FOLD_CONV_K3S2 == 3
    # argument checks that need no GPU: refused before any launch
    lib = _lib.lib                                                      # with the argument types of the ctypes table
    assert lib.cvae_token_gemm(None, 256, None, None, None, 0, None, 256, 4, 256, 100, 0, 0, None) == -3          # N = 100: unsupported
    assert lib.cvae_mhsa_fwd(None, None, None, None, 768, 768, 768, 0, 0, 0, 1, 81, 82, 0, None) == -1            # more query rows than tokens
    assert lib.cvae_layernorm256(None, 255, None, None, None, 4, 1e-5, 0, None) == -1


def test_encoder_refuses_unsupported_configurations_and_cpu_tensors():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAEEncoder
    for kw in (dict(embed_dim=128), dict(heads=4), dict(mlp_dim=1024), dict(img_size=(250, 320)), dict(patch_size=16), dict(in_channels=3)):
        with pytest.raises(CvaeError):
            ViTVAEEncoder(**{**dict(img_size=(64, 64), depth=1), **kw})
    m = ViTVAEEncoder(img_size=(64, 64), depth=1, latent_dim=8)
    assert not hasattr(m, "decode")
    with pytest.raises(RuntimeError, match="eval mode"):
        m.encode(torch.zeros(1, 1, 64, 64))
    with pytest.raises(CvaeError, match="no CPU fallback"):
        m.eval().encode(torch.zeros(1, 1, 64, 64))
