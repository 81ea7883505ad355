"""conv_wgrad_kernel's tile staging (csrc/conv_mfma.hip): which thread loads which 16-byte piece of the S and L tiles, from where, whether it is zeroed, and
where it lands in LDS — through cvae_conv_wgrad (per layer) and cvae_conv_wgrad_multi (the same layers in one launch).

Two checks per case:
 (a) exact: S and L hold integers of {-2, -1, 1, 2} (exact in bf16).  Every product and partial sum is an integer below 2^24 (at most 8192 positions x 4),
     exact in fp32 in any order, so dW and dbias must EQUAL the float64 reference.  A piece that is misplaced, dropped, duplicated or wrongly zeroed
     cannot hide behind a tolerance; out-of-range pieces are loaded from clamped addresses that hold non-zero data, so a wrong in-range bit shows.
 (b) bounded: normal operands against float64 with the bound of the conv-family tests (oracle/conv64.py: C sqrt(K) U (|S| . |L|) for dW, the
     pairwise-sum bound for a bias gradient), through the same helpers as tests/test_conv_reference.py.
The grouped launch must give each layer the bits of its own launch.  Outputs are pre-filled with NaN: a NaN left behind is an element nobody wrote.

Shapes (Tile<3,128> = 4x4x8 positions, Tile<2,128> = 8x16; slab counts from plan_wgrad for these channel counts):
  3D  4x4x8 B=2         one tile per sample, every face a border (lz = -1 and lz = ld), 2 slabs
      4x4x8 B=1         one slab: the workgroup stores dW itself
      5x6x9 B=1, B=3    ragged last tiles on all three axes; B=3: 24 tiles on 16 slabs, so a workgroup's second tile lies two samples on
      5x6x17 B=3        36 tiles (2x2x3 per sample) on 16 slabs: the walk's step has non-zero w, h and sample digits and carries in w and h
      8x8x16 B=1        interior tile faces
      4x4x8 B=2, Cs=128, Cl=64   channel-block offsets, with the bias sum of either side (only the first channel block of the OTHER side sums)
  2D  7x7 B=4, B=3      two samples side by side in one tile, with and without a partner for the last sample
      7x7 B=1           the same map unpaired, one slab
      9x20 B=2          ragged
      17x33 B=8         72 tiles on 64 slabs: a second tile per workgroup, step digits (1, 0, 7)
  fp32: 3D 5x6x9 B=3 and 4x4x8 B=2, 2D 7x7 B=3 and 9x20 B=2.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conv_reference import DT, F32, c64, exact, run_multi  # noqa: E402
from test_wgrad_roundtrips import own_launch, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

# group -> (nd, dtype, [(B, Cs, Cl, small extent, dbias side)]); a group is one cvae_conv_wgrad_multi launch (at most 8 layers)
GROUPS = {
    "3d-bf16": (3, "bf16", [(2, 64, 32, (4, 4, 8), 0), (1, 64, 32, (4, 4, 8), 1), (1, 64, 32, (5, 6, 9), 1), (3, 64, 32, (5, 6, 9), 0), (3, 64, 32, (5, 6, 17), 1),
                            (1, 64, 32, (8, 8, 16), 0), (2, 128, 64, (4, 4, 8), 0), (2, 128, 64, (4, 4, 8), 1)]),
    "2d-bf16": (2, "bf16", [(4, 64, 32, (7, 7), 1), (3, 64, 32, (7, 7), 0), (1, 64, 32, (7, 7), 1), (2, 64, 32, (9, 20), 0), (8, 64, 32, (17, 33), 1)]),
    "3d-f32": (3, "f32", [(3, 64, 32, (5, 6, 9), 1), (2, 64, 32, (4, 4, 8), 0)]),
    "2d-f32": (2, "f32", [(3, 64, 32, (7, 7), 1), (2, 64, 32, (9, 20), 0)]),
}
ARMS = [(g, j) for g, (_, _, layers) in GROUPS.items() for j in range(len(layers))]
ARM_IDS = [f"{g}-{'x'.join(map(str, GROUPS[g][2][j][3]))}-B{GROUPS[g][2][j][0]}-Cs{GROUPS[g][2][j][1]}-side{GROUPS[g][2][j][4]}" for g, j in ARMS]


def make(group, kind):
    nd, dt, layers = GROUPS[group]
    cases = []
    for j, (B, Cs, Cl, size, _) in enumerate(layers):
        c = c64.make_case("wgrad", 3000 + 10 * len(cases) + nd, nd, B, Cl, Cs, size, DT[dt])
        if kind == "int":
            g = torch.Generator().manual_seed(3100 + j)
            vals = torch.tensor([-2.0, -1.0, 1.0, 2.0])
            for key in ("S", "L"):
                c[key] = vals[torch.randint(0, 4, c[key].shape, generator=g)]
        cases.append(c)
    return cases


@functools.lru_cache(maxsize=None)
def results(group, kind):
    """every layer of the group through its own launch and all of them through one grouped launch, with the float64 reference: computed once per session"""
    nd, dt, layers = GROUPS[group]
    cases, sides = make(group, kind), [l[4] for l in layers]
    own = [own_launch(c, s, DT[dt]) for c, s in zip(cases, sides)]
    grouped = run_multi(nd, cases, sides, dt)
    refs = [c64.reference(c, dbias_side=s) for c, s in zip(cases, sides)]
    return own, grouped, refs


@pytest.mark.parametrize("group,j", ARMS, ids=ARM_IDS)
def test_exact_on_small_integers(group, j):
    own, grouped, refs = results(group, "int")
    ref, _ = refs[j]
    for key in ("dW", "dbias"):
        exact(f"{group} layer {j} own launch {key}", own[j][key], ref[key], "(cs, cl, k..)" if key == "dW" else "(c)")
        exact(f"{group} layer {j} grouped launch {key}", grouped[j][key], ref[key], "(cs, cl, k..)" if key == "dW" else "(c)")


@pytest.mark.parametrize("group,j", ARMS, ids=ARM_IDS)
def test_within_the_float64_bound(group, j):
    own, grouped, refs = results(group, "rand")
    ref, err = refs[j]
    for name, got in (("own", own[j]), ("grouped", grouped[j])):
        for key in got:
            print(f"RATIO wgrad-tile-{group}-{j}-{name}-{key} {c64.max_ratio(got[key], ref[key], err[key]):.3f}")
        bad = c64.compare(got, ref, err)
        assert not bad, f"{group} layer {j}, {name} launch: " + "\n".join(bad)


@pytest.mark.parametrize("kind", ["int", "rand"])
@pytest.mark.parametrize("group,j", ARMS, ids=ARM_IDS)
def test_grouped_launch_has_the_bits_of_the_own_launch(group, j, kind):
    own, grouped, _ = results(group, kind)
    assert not any(torch.isnan(v).any() for v in grouped[j].values()), "elements never written"
    assert same_bits(grouped[j], own[j]), f"{group} layer {j}: the grouped launch and the layer's own launch differ"
