"""CPU checks of the ViT-VAE decoder's latent-gradient yardsticks (no GPU): the fixed-mask float64 restatement tests/vit_decoder_grad_reference.py against
torch.autograd through decode_ref, the two float64 identities the new kernel forms rest on (flipped / transposed K3; SUBPIXEL_T with its top / left zero
border), the C ABI's new entries, and what decode_with_grad refuses."""
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
import vit_decoder_grad_reference as gr  # noqa: E402
from test_vit_decoder_cpu import CASES, reference_state  # noqa: E402


def cotangent(B, H, W, seed):
    return torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(seed))


def test_restatement_equals_autograd_through_decode_ref(golden):
    """float64's own masks: the fixed-mask linear map IS the derivative wherever no pre-activation is exactly zero"""
    _model, sd, z, grid = reference_state(golden(CASES[0]))
    zz = z.double().requires_grad_(True)
    out = dr.decode_ref(sd, zz, grid)
    g = cotangent(z.shape[0], 64, 96, 5)
    want, = torch.autograd.grad(out["image"], zz, g.double())
    stages = {k: v.detach() for k, v in out.items()}
    masks = gr.masks_of(stages, gr.res_inner_ref(sd, stages))
    got = gr.decode_vjp_ref(sd, g, grid, masks)
    rel = vr.rel_l2(got, want)
    print(f"fixed-mask restatement vs autograd through decode_ref: rel-L2 {rel:.3e}")
    assert got.shape == z.shape and rel < 1e-12, rel
    for mutate in ("slope", "no_residual", "shift"):
        assert vr.rel_l2(gr.decode_vjp_ref(sd, g, grid, masks, mutate=mutate), want) > 1e-3, mutate


def k3_grad_matrix(w):
    """[Cout][Cin][3][3] -> [Cin][9 Cout] (row ci, column (ky 3 + kx) Cout + co = w[co][ci][2 - ky][2 - kx]), the layout of CVAE_FOLD_CONV_K3S1_GRAD"""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], 9 * w.shape[0])


def subpixel_t_matrix(w3):
    """[Cin][16][3][3] -> [32][256] (row ci, column (dy 2 + dx) 64 + (py 2 + px) 16 + co = w[ci][co][2 dy + py - 1][2 dx + px - 1], zero where an index is
    negative and in rows ci >= Cin), the layout of CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD"""
    cin, cout = w3.shape[:2]
    m = torch.zeros(32, 4, 4, cout, dtype=w3.dtype)
    for dy in range(2):
        for dx in range(2):
            for py in range(2):
                for px in range(2):
                    ky, kx = 2 * dy + py - 1, 2 * dx + px - 1
                    if ky >= 0 and kx >= 0:
                        m[:cin, dy * 2 + dx, py * 2 + px] = w3[:, :, ky, kx]
    return m.reshape(32, 16 * cout)


def test_flipped_transposed_k3_is_the_conv2d_input_gradient_in_float64():
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 8, 5, 7, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(8, 8, 3, 3, generator=gen, dtype=torch.float64)
    g = torch.randn(2, 8, 5, 7, generator=gen, dtype=torch.float64)
    want, = torch.autograd.grad(F.conv2d(x, w, padding=1), x, g)
    wb = k3_grad_matrix(w).view(8, 3, 3, 8).permute(0, 3, 1, 2)                     # [Cin][Cout][ky][kx]: a plain K3 conv of g
    got = F.conv2d(g, wb, padding=1)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float((F.conv_transpose2d(g, w, padding=1) - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_subpixel_t_is_the_conv_transpose_input_gradient_in_float64():
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(2, 8, 5, 7, generator=gen, dtype=torch.float64, requires_grad=True)
    w3 = torch.randn(8, 16, 3, 3, generator=gen, dtype=torch.float64)
    g = torch.randn(2, 16, 10, 14, generator=gen, dtype=torch.float64)
    want, = torch.autograd.grad(F.conv_transpose2d(x, w3, stride=2, padding=1, output_padding=1), x, g)
    assert float((F.conv2d(g, w3, stride=2, padding=1) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # space-to-depth view [B][64 = (py, px, co)][H][W], a 2 x 2 window over positions (y - 1, y) x (x - 1, x): one zero row on top, one zero column left
    s2d = g.view(2, 16, 5, 2, 7, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 64, 5, 7)
    wconv = subpixel_t_matrix(w3).view(32, 2, 2, 64).permute(0, 3, 1, 2)            # [32][64][dy][dx]
    got = F.conv2d(F.pad(s2d, (1, 0, 1, 0)), wconv)
    assert got.shape == (2, 32, 5, 7) and float(got[:, 8:].abs().max()) == 0.0
    assert float((got[:, :8] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    wrong = F.conv2d(F.pad(s2d, (0, 1, 0, 1)), wconv)                               # the border on the forward form's side: refused
    assert float((wrong[:, :8] - want).abs().max()) > 1e-2 * float(want.abs().max())


def test_header_exports_and_ctypes_table_hold_the_grad_entries():
    import ctypes
    from causal_vae_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvae_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "causal_vae_amd", "libcvae_hip.so"))
    for n in ("cvae_conv_s1_bwd_data", "cvae_conv_s1_c1_bwd_data", "cvae_latent_to_grid_bwd", "cvae_latent_to_grid_bwd_workspace_bytes"):
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    for n, v in (("CONV_K3S1_GRAD", 7), ("CONVT_K3S2_SUBPIXEL_GRAD", 8)):
        assert re.search(r"#define\s+CVAE_FOLD_" + n + r"\s+" + str(v) + r"\b", src) and getattr(ops, "FOLD_" + n) == v
    assert re.search(r"#define\s+CVAE_CONV_S1_SUBPIXEL_T\s+2\b", src) and ops.CONV_S1_SUBPIXEL_T == 2
    assert re.search(r"#define\s+CVAE_FOLD_CONVT_K3S2_SUBPIXEL\s+6\b", src)          # the existing kinds keep their values
    lib = _lib.lib
    # argument checks that need no GPU: refused (or accepted as empty) before any launch
    assert lib.cvae_conv_s1_bwd_data(None, None, None, None, None, 1, 8, 8, 48, 0, 0, 0, None) == -3        # channel count outside the list
    assert lib.cvae_conv_s1_bwd_data(None, None, None, None, None, 1, 8, 8, 64, 2, 0, 0, None) == -3        # SUBPIXEL_T: 32 or 16
    assert lib.cvae_conv_s1_bwd_data(None, None, None, None, None, 1, 8, 8, 64, 1, 0, 0, None) == -3        # the forward's form is not a backward form
    assert lib.cvae_conv_s1_bwd_data(None, None, None, None, None, 0, 8, 8, 64, 0, 0, 0, None) == 0
    assert lib.cvae_conv_s1_bwd_data(None, None, None, None, None, 1, 8, 8, 64, 0, 0, 0, None) == -6
    assert lib.cvae_conv_s1_c1_bwd_data(None, None, None, None, 1, 8, 8, 32, 0, 0, None) == -3
    assert lib.cvae_conv_s1_c1_bwd_data(None, None, None, None, 0, 8, 8, 16, 0, 0, None) == 0
    assert lib.cvae_latent_to_grid_bwd(None, None, None, 17, 128, 6, 256, 0, None, 0, None) == -3           # more rows than one launch takes
    assert lib.cvae_latent_to_grid_bwd(None, None, None, 0, 128, 6, 256, 0, None, 0, None) == 0
    assert lib.cvae_latent_to_grid_bwd_workspace_bytes(17, 128, 6, 256) == 0
    # slabs of 32 channels x 8 positions, a split that does not depend on B: 8 x ceil(6 / 8) slabs of B x K floats
    assert lib.cvae_latent_to_grid_bwd_workspace_bytes(3, 128, 6, 256) == 8 * 3 * 128 * 4
    assert lib.cvae_latent_to_grid_bwd_workspace_bytes(1, 512, 960, 256) == 8 * 120 * 512 * 4
    assert lib.cvae_conv_s1_weight_elems(32, 16, 2) == 32 * 256 and lib.cvae_conv_s1_weight_elems(16, 16, 2) == 32 * 256
    assert lib.cvae_conv_s1_weight_elems(64, 16, 2) == 0


def test_decode_with_grad_refuses_cpu_tensors_train_mode_and_unfrozen_parameters():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit import ViTVAE
    m = ViTVAE(img_size=(64, 64), depth=1, latent_dim=8)
    z = torch.zeros(1, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="eval mode"):
        m.decode_with_grad(z)
    m.eval()
    with pytest.raises(CvaeError, match="no CPU fallback"):
        m.freeze_decoder().decode_with_grad(z)
    with pytest.raises(CvaeError, match="no CPU fallback"):
        m.decode_vjp(z.detach(), torch.zeros(1, 1, 64, 64))
    assert not any(p.requires_grad for p in m.decoder.parameters()) and not m.decoder_input.weight.requires_grad
    assert all(p.requires_grad for p in m.stem.parameters())                                     # the encoder is not touched
    m.decoder[3].conv[0].weight.requires_grad_(True)
    m.decoder_input.bias.requires_grad_(True)
    with pytest.raises(CvaeError, match=r"decoder\.3\.conv\.0\.weight.*decoder_input\.bias"):
        m.decode_with_grad(z)
    with pytest.raises(CvaeError):
        m.freeze_decoder().decode_with_grad(torch.zeros(1, 9))
