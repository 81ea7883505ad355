"""The weight gradient of a layer whose sum is a single slab, against the float64 reference and bounds of tests/test_conv_reference.py (oracle/conv64.py:
C sqrt(K) U (|S| . |L|) elementwise for dW, the pairwise-sum bound for a bias gradient).

A layer whose (kd, channel block) groups get ONE slab each (n_split == 1; here a single tile of 4x4x8 / 8x16 positions) has its dW stored by
conv_wgrad_kernel itself (csrc/conv_mfma.hip); wgrad_reduce_kernel keeps only the layer's bias blocks.  Outputs are pre-filled with NaN: a NaN left behind
is an element nobody wrote.  Every launch runs twice and must repeat its bits.  In a grouped launch such a layer rides next to one that still goes
through the slabs (the same channels at B = 2: two tiles, n_split == 2), and each must give the bits of its own launch.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conv_reference import DEV, DT, F32, L, c64, dev, ops, ptr, run_multi  # noqa: E402

pytestmark = pytest.mark.gpu


def own_launch(c, side, dtype):
    """cvae_conv_wgrad into NaN-filled outputs"""
    nd, Cs, Cl = c["nd"], c["Cs"], c["Cl"]
    S, Lt = dev(c["S"], dtype), dev(c["L"], dtype)
    dW = torch.full((Cs, Cl, *([4] * nd)), float("nan"), device=DEV)
    db = None if side is None else torch.full((Cl if side else Cs,), float("nan"), device=DEV)
    nb = L.lib.cvae_conv_wgrad_workspace_bytes(Cs, Cl, nd)
    ws = torch.empty(nb // 4, dtype=F32, device=DEV)
    dims = (c["B"], *c["s_dims"], Cs, *c["l_dims"])
    rc = L.lib.cvae_conv_wgrad(ptr(S), ptr(Lt), ptr(dW), ptr(db), int(side or 0), ptr(ws), nb, *dims, Cl, nd, L.dtype_code(dtype), ops.stream())
    assert rc == 0, L.lib.cvae_strerror(rc)
    torch.cuda.synchronize()
    return {"dW": dW} if side is None else {"dW": dW, "dbias": db}


def same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def check_launch(family, c, side, dtype):
    ref, err = c64.reference(c, dbias_side=side)
    got, again = own_launch(c, side, dtype), own_launch(c, side, dtype)
    for k in got:
        assert not torch.isnan(got[k]).any(), f"{family}: {int(torch.isnan(got[k]).sum())} elements of {k} were never written"
        print(f"RATIO {family}-{k} {c64.max_ratio(got[k], ref[k], err[k]):.3f}")
    bad = c64.compare(got, ref, err)
    assert not bad, family + ": " + "\n".join(bad)
    assert same_bits(got, again), family + ": two runs differ"


# ------------------------------------------------------------------------------------------------ one slab per group: dW straight from the main kernel
ONE_TILE = {3: (4, 4, 8), 2: (8, 16)}
CHANNELS = [(64, 32), (128, 64)]


@pytest.mark.parametrize("side", [0, 1, None], ids=["sbias", "lbias", "nobias"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("ch", CHANNELS, ids=["64x32", "128x64"])
@pytest.mark.parametrize("nd", [3, 2])
def test_one_slab_direct_store(nd, ch, dt, side):
    Cs, Cl = ch
    c = c64.make_case("wgrad", 2000 + 10 * nd + Cs, nd, 1, Cl, Cs, ONE_TILE[nd], DT[dt])
    check_launch(f"wgrad-direct{nd}d-{dt}", c, side, DT[dt])


@pytest.mark.parametrize("side", [1, None], ids=["lbias", "nobias"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("ch", CHANNELS, ids=["64x32", "128x64"])
@pytest.mark.parametrize("nd", [3, 2])
def test_one_slab_layer_next_to_a_two_slab_layer(nd, ch, dt, side):
    """one cvae_conv_wgrad_multi call: B = 1 (one slab, direct; with the L-side bias sum, or with nothing left for the reduce pass) and B = 2 (two
    slabs, reduce pass, S-side bias sum)"""
    Cs, Cl = ch
    cases = [c64.make_case("wgrad", 2100 + 10 * nd + Cs + B, nd, B, Cl, Cs, ONE_TILE[nd], DT[dt]) for B in (1, 2)]
    sides = [side, 0]
    grouped = run_multi(nd, cases, sides, dt)
    for j, c in enumerate(cases):
        assert not any(torch.isnan(v).any() for v in grouped[j].values()), f"layer {j}: elements never written"
        alone = own_launch(c, sides[j], DT[dt])
        assert same_bits(grouped[j], alone), f"layer {j} (B = {c['B']}): the grouped launch and the layer's own launch differ"
    assert same_bits(grouped[0], run_multi(nd, cases, sides, dt)[0]), "two grouped runs differ"
