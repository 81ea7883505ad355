"""CPU checks of the ViT-VAE decoder's yardsticks (no GPU): the ViTVAE constructor against the goldens captured from the reference ViTVAE, the float64
restatement tests/vit_decoder_reference.py against those goldens, the loader contract, the two identities the kernels rest on (zero embedding of the
k3 transposed conv into k4; its sub-pixel form) against F.conv_transpose2d in float64, what the composed bound refuses, and the C ABI's new entries.

Printed by test_float64_restatement_matches_golden: bound / ||value|| 1.1e-2 (stage0: K = 16 x 256 at worst-case magnitude) falling to 2e-4 .. 5e-4 at the
last stage and the image; ||golden - float64|| / bound 1e-4 .. 1e-3.  Rounding oracle (bf16) vs float64 on the 768 x 1280 image: printed by
test_rounding_oracle_gap_is_what_the_gpu_test_uses."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_reference as vr  # noqa: E402
import vit_decoder_reference as dr  # noqa: E402

CASES = ("vitvae_dec_64x96", "vitvae_dec_256x320", "vitvae_dec_768x1280")
NAMES = ["grid"] + [f"stage{i}" for i in range(8)] + ["image"]


def reference_state(g):
    """The full state_dict of a decoder golden: the seed's draws + the seeded BatchNorm statistics, checked against the stored digests."""
    from causal_vae_amd.vit import ViTVAE
    B, H, W, depth, seed_model, seed_bn, seed_dec_bn, seed_z = (int(v) for v in g.z["in/seed"])
    torch.manual_seed(seed_model)
    model = ViTVAE(img_size=(H, W), depth=depth)
    vr.randomize_stem_bn(model.stem, seed_bn)
    dr.randomize_decoder_bn(model.decoder, seed_dec_bn)
    sd = model.state_dict()
    assert sorted(sd) == g.keys("sd0")
    for k, v in sd.items():
        g.check("sd0", k, v, rtol=0, atol=0)
    z = dr.dec_inputs(B, 128, seed_z)
    g.check("in", "z", z, rtol=0, atol=0)
    return model, sd, z, (H // 32, W // 32)


@pytest.mark.parametrize("name", CASES)
def test_constructor_reproduces_the_reference_state_dict(golden, name):
    model, sd, _z, grid = reference_state(golden(name))
    assert [k for k in sd if k.startswith("decoder")][:3] == ["decoder_input.weight", "decoder_input.bias", "decoder.0.weight"]
    assert "decoder.3.conv.4.running_var" in sd and "decoder.18.bias" in sd and len(dr.decoder_batchnorms(model.decoder)) == 11
    assert sd["decoder_input.weight"].shape == (256 * grid[0] * grid[1], 128)


def check_against_golden(g, name, got, bound, ref, factor=1.0):
    for k in NAMES:
        if g.has("out/" + k):
            ratio = vr.fro_ratio(g.t("out/" + k), ref[k], bound[k])
            print(f"{name} {k}: ||golden - float64|| / bound = {ratio:.2e}; bound / ||value|| = {bound[k] / float(ref[k].norm()):.2e}")
            assert ratio <= 1.0, (k, ratio)
        # digest: sums of n elements move by at most sqrt(n) ||diff||_F <= sqrt(n) bound, an element by at most the bound (as tests/test_vit_reference_cpu.py)
        g.check("out", k, got[k].float(), rtol=factor * bound[k] / float(ref[k].norm()), atol=factor * bound[k] / 20)


@pytest.mark.parametrize("name", CASES[:2])
def test_float64_restatement_matches_golden(golden, name):
    g = golden(name)
    _model, sd, z, grid = reference_state(g)
    bound, ref = dr.composed_bound(sd, z, grid, key=name)
    assert g.has("out/image") and (name != CASES[0] or all(g.has(f"out/stage{i}") for i in range(6)))
    for k in NAMES:
        rel = bound[k] / float(ref[k].norm())
        assert 0.0 < rel < 2e-2, (k, rel, "the bound must be finite and a small fraction of the values it guards")
    check_against_golden(g, name, ref, bound, ref)


def test_what_the_bound_refuses(golden):
    """The whole-decoder bound must reject every structural mistake a decoder port can make: a ResBlock without its residual add, LeakyReLU slope 0.01
    where the ResBlocks' 0.2 belongs, a one-pixel shift of the transposed convs' output (output_padding on the wrong side), running means left out of the
    BatchNorm fold — and a result off by a factor 1 + 2^-9 on the image."""
    name = CASES[0]
    _model, sd, z, grid = reference_state(golden(name))
    bound, ref = dr.composed_bound(sd, z, grid, key=name)
    for mutate in ("no_residual", "slope", "shift", "bn_mean"):
        wrong = dr.decode_ref(sd, z, grid, mutate=mutate)
        ratio = vr.fro_ratio(wrong["image"], ref["image"], bound["image"])
        print(f"{mutate}: ||wrong - float64|| / bound = {ratio:.1f}")
        assert ratio > 1.0, mutate
        assert vr.fro_ratio(wrong["stage7"], ref["stage7"], bound["stage7"]) > 1.0, mutate
    assert vr.fro_ratio(ref["image"] * (1 + 2.0 ** -9), ref["image"], bound["image"]) > 1.0
    rounded = dr.decode_ref(sd, z, grid, rnd=vr.round_bf16)
    assert vr.fro_ratio(rounded["image"], ref["image"], bound["image"]) > 1.0                  # bf16 operand rounding is outside the fp32 bound


def test_rounding_oracle_gap_is_what_the_gpu_test_uses(golden):
    """The bf16 whole-decoder tolerance of tests/test_vit_decoder.py is 2 x this gap; it is computed there again — here it is printed for DESIGN §11."""
    _model, sd, z, grid = reference_state(golden(CASES[2]))
    plain = dr.decode_ref(sd, z, grid)
    orac = dr.decode_ref(sd, z, grid, rnd=vr.round_bf16)
    gap = vr.rel_l2(orac["image"], plain["image"])
    print("decoder rounding oracle vs float64, rel-L2 of the 768 x 1280 image:", gap)
    assert 1e-4 < gap < 5e-2, gap


def test_loader_contract():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAE, ViTVAEEncoder, load_vitvae_state_dict
    torch.manual_seed(11)
    src = ViTVAE(img_size=(64, 96), depth=1, latent_dim=32)
    dr.randomize_decoder_bn(src.decoder, 3)
    full = src.state_dict()
    dst = ViTVAE(img_size=(64, 96), depth=1, latent_dim=32)
    assert load_vitvae_state_dict(dst, full) == []
    for k, v in full.items():
        assert torch.equal(v, dst.state_dict()[k]), k
    enc = ViTVAEEncoder(img_size=(64, 96), depth=1, latent_dim=32)
    dropped = load_vitvae_state_dict(enc, full)
    assert dropped == sorted(k for k in full if k.startswith(("decoder_input.", "decoder."))) and len(dropped) > 60
    assert not hasattr(enc, "decode")
    with pytest.raises(CvaeError, match="shape mismatch"):
        load_vitvae_state_dict(dst, {**full, "decoder.3.conv.0.weight": torch.zeros(128, 128, 3, 4)})
    with pytest.raises(CvaeError, match="missing"):
        load_vitvae_state_dict(dst, {k: v for k, v in full.items() if k != "decoder.18.bias"})
    with pytest.raises(CvaeError):
        load_vitvae_state_dict(dst, {**full, "decoder.19.weight": torch.zeros(1)})


def test_zero_embedding_equals_conv_transpose_in_float64():
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 5, 7, generator=gen, dtype=torch.float64)
    w3 = torch.randn(8, 6, 3, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(6, generator=gen, dtype=torch.float64)
    w4 = torch.zeros(8, 6, 4, 4, dtype=torch.float64)
    w4[:, :, :3, :3] = w3
    y3 = F.conv_transpose2d(x, w3, b, stride=2, padding=1, output_padding=1)
    y4 = F.conv_transpose2d(x, w4, b, stride=2, padding=1)
    assert y3.shape == y4.shape == (2, 6, 10, 14) and float((y3 - y4).abs().max()) == 0.0


def subpixel_matrix(w3):
    """[Cin][Cout][3][3] -> [4 Cout][4 Cin] (row (py 2 + px) Cout + co, column (dy 2 + dx) Cin + ci), the layout of CVAE_FOLD_CONVT_K3S2_SUBPIXEL"""
    cin, cout = w3.shape[:2]
    kmap = {(0, 0): 1, (1, 0): 2, (1, 1): 0}
    m = torch.zeros(4 * cout, 4 * cin, dtype=w3.dtype)
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    if (py, dy) in kmap and (px, dx) in kmap:
                        q, t = py * 2 + px, dy * 2 + dx
                        m[q * cout:(q + 1) * cout, t * cin:(t + 1) * cin] = w3[:, :, kmap[(py, dy)], kmap[(px, dx)]].T
    return m


def test_subpixel_form_equals_conv_transpose_in_float64():
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(2, 8, 5, 7, generator=gen, dtype=torch.float64)
    w3 = torch.randn(8, 6, 3, 3, generator=gen, dtype=torch.float64)
    b = torch.randn(6, generator=gen, dtype=torch.float64)
    want = F.conv_transpose2d(x, w3, b, stride=2, padding=1, output_padding=1)
    m = subpixel_matrix(w3)                                                        # a stride-1 conv with a 2 x 2 forward window, input padded right / bottom
    wconv = m.view(24, 2, 2, 8).permute(0, 3, 1, 2)                                # [4 Cout][Cin][dy][dx]
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), wconv)                                    # [B, 4 Cout, H, W]
    got = F.pixel_shuffle(y.view(2, 2, 2, 6, 5, 7).permute(0, 3, 1, 2, 4, 5).reshape(2, 24, 5, 7), 2) + b[None, :, None, None]
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_header_exports_and_ctypes_table_hold_the_decoder_entries():
    import ctypes
    from causal_vae_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvae_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "causal_vae_amd", "libcvae_hip.so"))
    for n in ("cvae_conv_s1", "cvae_conv_s1_c1", "cvae_conv_s1_pack_weights", "cvae_conv_s1_weight_elems", "cvae_latent_to_grid"):
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    for n, v in (("CONVT_K3S2", 4), ("CONV_K3S1", 5), ("CONVT_K3S2_SUBPIXEL", 6)):
        assert re.search(r"#define\s+CVAE_FOLD_" + n + r"\s+" + str(v) + r"\b", src) and getattr(ops, "FOLD_" + n) == v
    assert re.search(r"#define\s+CVAE_FOLD_CONV_K3S2\s+3\b", src)                   # the existing kinds keep their values; 2 stays unassigned
    lib = _lib.lib
    # argument checks that need no GPU: refused (or accepted as empty) before any launch
    assert lib.cvae_conv_s1(None, None, None, None, None, 1, 8, 8, 48, 48, 0, 0, 0, None) == -3             # channel count outside the list
    assert lib.cvae_conv_s1(None, None, None, None, None, 1, 8, 8, 64, 16, 1, 0, 0, None) == -3
    assert lib.cvae_conv_s1(None, None, None, None, None, 0, 8, 8, 64, 64, 0, 0, 0, None) == 0              # B == 0
    assert lib.cvae_conv_s1(None, None, None, None, None, 1, 8, 8, 64, 64, 0, 0, 0, None) == -6
    assert lib.cvae_conv_s1_c1(None, None, None, None, 1, 8, 8, 32, 0, 0, None) == -3
    assert lib.cvae_conv_s1_c1(None, None, None, None, 0, 8, 8, 16, 0, 0, None) == 0
    assert lib.cvae_latent_to_grid(None, None, None, None, 17, 128, 6, 256, 0, None) == -3                  # more rows than one launch takes
    assert lib.cvae_latent_to_grid(None, None, None, None, 0, 128, 6, 256, 0, None) == 0
    assert lib.cvae_conv_s1_weight_elems(32, 32, 0) == 32 * 320 and lib.cvae_conv_s1_weight_elems(16, 16, 1) == 64 * 64
    assert lib.cvae_conv_s1_weight_elems(128, 128, 0) == 128 * 1152 and lib.cvae_conv_s1_weight_elems(32, 16, 1) == 64 * 128


def test_decoder_refuses_train_mode_and_cpu_tensors():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAE
    m = ViTVAE(img_size=(64, 64), depth=1, latent_dim=8)
    with pytest.raises(RuntimeError, match="eval mode"):
        m.decode(torch.zeros(1, 8))
    with pytest.raises(CvaeError, match="no CPU fallback"):
        m.eval().decode(torch.zeros(1, 8))
    with pytest.raises(CvaeError):
        m.decode(torch.zeros(1, 9))
    z = m.reparameterize(torch.zeros(2, 8), torch.zeros(2, 8))
    assert z.shape == (2, 8)
