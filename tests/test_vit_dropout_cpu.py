"""CPU checks of the transformer's dropout: the numpy restatement of the mask (tests/vit_dropout_reference.py) against the Random123
vectors and its own statistics, the five new C entries in the header and the ctypes table, ops.DropoutKeys, and the Python switches on a CPU model."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_dropout_reference as dr  # noqa: E402

KEY_A, KEY_B = 0x1234567890ABCDEF, 0x0FEDCBA987654321
NEW_ENTRIES = {"cvae_mhsa_fwd_train_dropout": 17, "cvae_mhsa_bwd_dropout": 29, "cvae_token_gemm_dropout": 19, "cvae_token_gemm_bwd_data_dropout": 15,
               "cvae_dropout_rows": 11}


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_numpy_philox_reproduces_random123(ctr, key, want):
    got = dr.philox4x32_10(*ctr, key[0] | (key[1] << 32))
    assert tuple(int(w) for w in got) == want


def test_threshold_and_scale():
    assert dr.threshold(0.1) == 1677721 and dr.threshold(0.0) == 0 and dr.threshold(0.5) == 1 << 23
    assert dr.scale(0.0) == np.float32(1.0) and dr.scale(0.5) == np.float32(2.0)
    assert dr.scale(0.1).dtype == np.float32 and dr.scale(0.1) == np.float32(1.0) / np.float32(0.9)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("key", [KEY_A, KEY_B])
def test_keep_fraction(p, key):
    """the measured keep fraction of a [4096][256] row site and of a B = 2, N = 200 attention site lies within 5 standard deviations of 1 - T / 2^24"""
    want = 1.0 - dr.threshold(p) / 2.0 ** 24
    for what, keep in (("rows", dr.keep_rows(4096, 256, p, key)), ("attention", dr.keep_attn(2, 200, p, key))):
        n = keep.size
        dev = abs(float(keep.mean()) - want) / np.sqrt(want * (1.0 - want) / n)
        print(f"{what} p={p} key={key:#x}: keep fraction {keep.mean():.6f}, expected {want:.6f}, {dev:.2f} standard deviations")
        assert dev <= 5.0, (what, p, dev)


def test_masks_of_different_keys_differ_and_p0_keeps_all():
    a, b = dr.keep_rows(64, 256, 0.1, KEY_A), dr.keep_rows(64, 256, 0.1, KEY_B)
    assert a.shape == (64, 256) and (a != b).any() and 0.05 < float((a != b).mean()) < 0.4
    a, b = dr.keep_attn(2, 33, 0.1, KEY_A), dr.keep_attn(2, 33, 0.1, KEY_B)
    assert a.shape == (2, 8, 33, 33) and (a != b).any()
    assert dr.keep_rows(8, 256, 0.0, KEY_A).all() and dr.keep_attn(1, 9, 0.0, KEY_A).all()


def test_row_site_with_a_row_step_is_the_strided_rows_of_the_full_mask():
    N, B = 7, 5
    full = dr.keep_rows(B * N, 256, 0.1, KEY_A)
    assert np.array_equal(dr.keep_rows(B, 256, 0.1, KEY_A, 0, N), full[::N])
    assert np.array_equal(dr.keep_rows(3, 256, 0.1, KEY_A, 2, N), full[2::N][:3])
    big = dr.keep_rows(2, 256, 0.1, KEY_A, (1 << 32) + 5, 1)                # the row's high word is a counter word of its own
    assert not np.array_equal(big, dr.keep_rows(2, 256, 0.1, KEY_A, 5, 1))


def test_attention_mask_does_not_depend_on_the_query_count():
    assert np.array_equal(dr.keep_attn(2, 65, 0.1, KEY_A, 1), dr.keep_attn(2, 65, 0.1, KEY_A)[:, :, :1])


def test_header_and_ctypes_table_hold_the_new_entries():
    from causal_vae_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvae_hip.h")).read(), flags=re.S)
    for name, n in NEW_ENTRIES.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == n, name
        m = re.search(r"\bint " + name + r"\((.*?)\);", src, flags=re.S)
        assert m and len(m.group(1).split(",")) == n, name
        assert hasattr(_lib.lib, name)
        assert "dtype" not in m.group(1), name                              # fp32 only: no dtype code


def test_bad_rate_is_refused_before_any_launch():
    import ctypes as C
    from causal_vae_amd import _lib
    buf = (C.c_char * 8192)()
    P = (C.addressof(buf) + 15) & ~15
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert _lib.lib.cvae_dropout_rows(P, 256, P, 256, 1, 256, p, 1, 0, 1, None) == -1


def test_dropout_keys():
    from causal_vae_amd import ops
    a, b = ops.DropoutKeys(seed=5), ops.DropoutKeys(seed=5)
    assert a.key(3, 2, 1) == b.key(3, 2, 1) == a.key(3, 2, 1) and 0 <= a.key(3, 2, 1) < 1 << 64      # pure in its arguments
    assert a.key(3, 2, 1) != ops.DropoutKeys(seed=6).key(3, 2, 1)
    keys = {a.key(s, blk, site) for s in range(200) for blk in range(10) for site in range(5)}
    assert len(keys) == 10000
    assert a.step == 0
    a.step = 17
    c = ops.DropoutKeys(seed=1).load_state(a.state())
    assert c.state() == a.state() == {"seed": 5, "step": 17} and c.key(17, 0, 0) == a.key(17, 0, 0)
    torch.manual_seed(1234)
    assert ops.DropoutKeys().seed == 1234


def test_switches_on_a_cpu_model():
    from causal_vae_amd._lib import CvaeError
    from causal_vae_amd.vit.causal import CausalViTVAE
    from causal_vae_amd.vit.models import ViTVAE
    model = ViTVAE(img_size=(64, 96), depth=1).eval()
    model.requires_grad_(False)
    assert model._dropout is False
    model.train_transformer(dropout=True)
    assert model._dropout is True and model._transformer_grads
    model.train_transformer()
    assert model._dropout is False
    model.train_all(dropout=True)
    assert model._dropout is True
    model.freeze_transformer()
    assert model._dropout is False and not model._transformer_grads
    drops = model._block_dropout(model.transformer[0], 0, 4)
    assert [d[0] for d in drops] == [0.1, 0.1, 0.1] and len({d[1] for d in drops}) == 3
    model.transformer[0].mlp[2].p = 0.0
    assert model._block_dropout(model.transformer[0], 0, 4)[1] is None         # a rate of 0: the plain launch
    model.set_compute_dtype(torch.bfloat16)
    with pytest.raises(CvaeError, match="float32"):
        model.train_transformer(dropout=True)
    model.set_compute_dtype(torch.float32).train_transformer(dropout=True)
    model.set_compute_dtype(torch.bfloat16)                                     # changed afterwards: refused at the walk
    with pytest.raises(CvaeError, match="float32"):
        model._check_dropout_dtype()
    model.set_compute_dtype(torch.float32)
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        model.encode(torch.zeros(1, 1, 64, 96))
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train_transformer(dropout=True)
    cm = CausalViTVAE(img_size=(64, 96), depth=1)
    with pytest.raises(CvaeError, match="transformer=True"):
        cm.train_adapters(dropout=True)
    cm.train_adapters(transformer=True, dropout=True)
    assert cm.backbone._dropout is True and not cm.backbone.training
    cm.train_adapters(transformer=True)
    assert cm.backbone._dropout is False
