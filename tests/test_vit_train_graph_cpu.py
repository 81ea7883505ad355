"""CPU checks of the captured ViT training step's plumbing: the six new C entries in the ctypes table, their argument refusals, and the
switches that must refuse before they touch a device.

The refusals call cvae_dropout_keys_step and cvae_dropout_rows_devkey with 16-byte-aligned host buffers standing in for device memory, in the manner of
tests/test_launch_layer_cpu.py: otherwise-valid arguments get past every check and end as CVAE_E_LAUNCH on a machine without a device.  The whole file is
skipped where a device exists, so that a missed check can only end as CVAE_E_LAUNCH, never as a launch on host pointers."""
import ctypes as C

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host pointers stand in for device memory: only where no launch can succeed", allow_module_level=True)

from causal_vae_amd import _lib  # noqa: E402
from causal_vae_amd._lib import CvaeError  # noqa: E402

lib = _lib.lib
OK, E_BADSHAPE, E_UNSUPPORTED, E_LAUNCH, E_NULLPTR = 0, -1, -3, -5, -6
IMG = (64, 96)

_buf = (C.c_char * (1 << 16))()                     # never read or written through: no launch succeeds here
P = (C.addressof(_buf) + 15) & ~15

# entry -> number of parameters: the sibling's list with `uint64_t key` replaced by `const uint64_t* key` (the count stays), and the key-table step
NEW_ENTRIES = {"cvae_dropout_keys_step": 5, "cvae_mhsa_fwd_train_dropout_devkey": 17, "cvae_mhsa_bwd_dropout_devkey": 29,
               "cvae_token_gemm_dropout_devkey": 19, "cvae_token_gemm_bwd_data_dropout_devkey": 15, "cvae_dropout_rows_devkey": 11}


def test_the_ctypes_table_holds_the_six_entries():
    for name, n in NEW_ENTRIES.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n, name
        assert hasattr(lib, name)
        if name.endswith("_devkey"):
            sibling = _lib.SIGNATURES[name[:-len("_devkey")]]
            assert len(sibling) == n
            diff = [i for i in range(n) if sibling[i] is not _lib.SIGNATURES[name][i]]
            assert len(diff) == 1 and sibling[diff[0]] is C.c_uint64 and _lib.SIGNATURES[name][diff[0]] is C.c_void_p, name      # the key, and only the key


def test_dropout_keys_step_refusals():
    step = lib.cvae_dropout_keys_step
    base = 0x0123456789ABCDEF
    assert step(base, P, P + 64, 6, None) == E_LAUNCH, "the arguments are not otherwise valid"
    assert step(base, P, P + 64, 1, None) == E_LAUNCH and step(base, P, P + 64, 65536, None) == E_LAUNCH
    for bad in (0, -1, 65537):
        assert step(base, P, P + 64, bad, None) == E_BADSHAPE, bad
    assert step(base, None, P + 64, 6, None) == E_NULLPTR
    assert step(base, P, None, 6, None) == E_NULLPTR
    assert step(base, None, None, 0, None) == E_BADSHAPE                     # the shape is judged first, as everywhere


def test_dropout_rows_devkey_refusals():
    rows = lib.cvae_dropout_rows_devkey
    good = (P, 256, P, 256, 1, 256, 0.1, P + 4096, 0, 1, None)
    assert len(good) == len(_lib.SIGNATURES["cvae_dropout_rows_devkey"])
    assert rows(*good) == E_LAUNCH, "the arguments are not otherwise valid"
    at = lambda i, v: good[:i] + (v,) + good[i + 1:]
    assert rows(*at(7, None)) == E_NULLPTR                                    # the key pointer
    assert rows(*at(0, None)) == E_NULLPTR and rows(*at(2, None)) == E_NULLPTR
    assert rows(*at(7, P + 4096 + 4)) == E_UNSUPPORTED                        # 8-byte alignment of the key
    for p in (-0.1, 1.0, float("nan")):
        assert rows(*at(6, p)) == E_BADSHAPE
    assert rows(*at(5, 254)) == E_BADSHAPE and rows(*at(9, 0)) == E_BADSHAPE
    # the by-value sibling takes the same arguments with the key as a number and answers alike
    assert lib.cvae_dropout_rows(*at(7, 1)) == E_LAUNCH


def vitvae():
    from causal_vae_amd.vit.models import ViTVAE
    torch.manual_seed(0)
    return ViTVAE(img_size=IMG, depth=2, latent_dim=128).eval()


def test_device_keys_are_refused_on_a_cpu_model_and_the_host_keys_stay():
    from causal_vae_amd import ops
    model = vitvae()
    keys = model.dropout_keys
    keys.step = 5
    before = sorted(model.state_dict())
    with pytest.raises(CvaeError, match="no CPU fallback"):
        model.use_device_dropout_keys()
    assert model.dropout_keys is keys and isinstance(keys, ops.DropoutKeys) and keys.step == 5
    assert model.use_device_dropout_keys(False) is model and model.dropout_keys is keys       # already host keys: nothing to do
    assert sorted(model.state_dict()) == before
    with pytest.raises(CvaeError, match="no CPU fallback"):
        ops.DeviceDropoutKeys(2, "cpu", seed=1)
    for bad in (0, 65537):
        with pytest.raises(CvaeError, match="n_blocks"):
            ops.DeviceDropoutKeys(bad, "cuda", seed=1)                       # refused before any device call


@pytest.mark.parametrize("device_step", [None, False])
def test_capture_needs_fused_adam_with_a_device_step(device_step):
    from causal_vae_amd import FusedAdam
    from causal_vae_amd.vit import CausalViTVAE, GraphedViTTrainStep, train_vit_vae
    model = vitvae()
    make = (lambda ps: torch.optim.Adam(ps, lr=1e-3)) if device_step is None else (lambda ps: FusedAdam(ps, lr=1e-3, device_step=False))
    x = torch.zeros(2, 1, *IMG)
    start = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(CvaeError, match="device_step=True"):
        train_vit_vae(model, [{"x": x}], make(model.parameters()), "cpu", epochs=1, graph=True)
    with pytest.raises(CvaeError, match="device_step=True"):
        GraphedViTTrainStep(model, make(model.parameters()), (x,))
    causal = CausalViTVAE(img_size=IMG, depth=1)
    with pytest.raises(CvaeError, match="device_step=True"):
        GraphedViTTrainStep(causal, make(causal.parameters()), (x, torch.zeros(2, causal.m_dim), torch.zeros(2, causal.t_dim)))
    assert all(torch.equal(a, b) for a, b in zip(start, model.parameters())) and not model._transformer_grads      # refused before anything was switched


def test_the_new_names_are_exported():
    from causal_vae_amd import ops, vit
    for name in ("vit_vae_train_step", "causal_vit_train_step", "GraphedViTTrainStep"):
        assert callable(getattr(vit, name)), name
    assert ops.DeviceDropoutKeys.ATTN == ops.DropoutKeys.ATTN == 0 and ops.DeviceDropoutKeys.MLP_OUT == 2
