"""GPU: the carried staging stream of the hand-written trunk convolution (algo 1, elf_amd/csrc/net_conv3x3.hip).  A full item with
a full item behind it on its workgroup stages that item's first seven half-tiles from its own last two K tiles, from rows it decoded
during its own first K tile, and the next item starts in the LDS buffer the chain's K-tile parity gives it; its first K tile counts
the stores of the item before into its waits.  What that newly puts at risk:

A. Chains and parity: five full items on one workgroup (width 1) at Cin = 64 and 192 (9 and 27 K tiles: the parity flips at every
   transition) and at Cin = 128 and 256 (even counts).
B. A partial tile in mid-chain: K = 512, width 1, M = 513 (1 x 1 x 513): t0, t1, t2 (one valid row) of column 0, then the three of
   column 1: the first K tile behind a tile that issued fewer stores, and a bias column that changes inside a chain.
C. The drained ends behind carried transitions: full, full, full, half on two workgroups; chains of a single item; fewer items than
   workgroups.
D. Rows carried early must not leak: a NaN in x in the first rows of item i + 1 leaves every output of item i a number, and a NaN
   in the last rows of item i every output of item i + 1; the same for a NaN row of res; all-ones operands on 5 x 37 and 37 x 5
   boards give Cin x (taps on the board), so a mask or an offset taken from the wrong item is a wrong integer.
E. 20 launches of two of the cases, bit-equal launch to launch.

Every comparison is exact: against algo 0, and against algo 1 with one item per workgroup (width 2^30), which has no transition at
all.  y is prefilled with NaN and has a NaN guard row behind it.  Each case runs with and without skip and ReLU."""
import ctypes as C

import numpy as np
import pytest

import conv_cases as cc
from conv_cases import ALONE, RES_RELU, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 4099 + rows + 31 * h + 977 * wd + c + 7 * k


def _launch(elf, t, use_res, relu, how, width=0):
    """one launch into a fresh NaN-filled, guarded y (cc.run_guarded; how: 'algo0', or 'linear' at `width`)"""
    return cc.run_guarded(elf.lib(), how, t["x"], t["w"], t["b"], t["r"] if use_res else None, relu, width)


_cases = {}


def _case(elf, rows, h, wd, c, k):
    """random operands of one shape and, per (skip, ReLU), algo 0's output and algo 1's with one item per workgroup: made once"""
    import torch
    key = (rows, h, wd, c, k)
    if key not in _cases:
        x, w, b, r = cc.rand_case(_seed(*key), *key)
        t = {"x": x, "w": w, "b": b, "r": r, "ref": {}}
        for use_res, relu in RES_RELU:
            y0 = cc.algo0_ref(elf.lib(), _seed(*key), key, use_res, relu)
            ya = cc.cached_ref(elf.lib(), "linear", _seed(*key), key, use_res, relu, ALONE)
            assert not bool(torch.isnan(y0).any())
            assert torch.equal(cc.bits(ya), cc.bits(y0)), "algo 1 with one item per workgroup differs from algo 0"
            t["ref"][(use_res, relu)] = (y0, ya)
        _cases[key] = t
    return _cases[key]


def _check(elf, shape, width, use_res, relu):
    import torch
    t = _case(elf, *shape)
    y0, ya = t["ref"][(use_res, relu)]
    y = _launch(elf, t, use_res, relu, "linear", width)
    print("%s width %d res %d relu %d: %d of %d elements differ from algo 0, %d from one item per workgroup"
          % (shape, width, use_res, relu, int((cc.bits(y) != cc.bits(y0)).sum().item()), y.numel(),
             int((cc.bits(y) != cc.bits(ya)).sum().item())))
    assert torch.equal(cc.bits(y), cc.bits(y0))
    assert torch.equal(cc.bits(y), cc.bits(ya))


# ------------------------------------------------------------------------------------------------ A. chains and K-tile parity

@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("c", [64, 192, 128, 256])
def test_five_full_items_on_one_workgroup(elf, c, use_res, relu):
    """20 boards of 8 x 8: M = 1280, five full tiles, K = 256: one workgroup runs four carried transitions and a drained end"""
    assert int(elf.lib().elfnet_conv3x3_f16_grid(5, 1, 1)) == 1
    _check(elf, (20, 8, 8, c, 256), 1, use_res, relu)


# ------------------------------------------------------------------------------------------------ B. a partial tile in mid-chain

@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("c", [64, 128])
def test_partial_tile_followed_by_full_items(elf, c, use_res, relu):
    """M = 513: the third tile has one valid row, and the chain goes on into column 1 behind it"""
    L = elf.lib()
    tile, col, half = C.c_int(), C.c_int(), C.c_int()
    assert int(L.elfnet_conv3x3_f16_plan(3, 2, 1, 2, C.byref(tile), C.byref(col), C.byref(half))) == 6
    assert (tile.value, col.value, half.value) == (2, 0, -1)
    assert int(L.elfnet_conv3x3_f16_plan(3, 2, 1, 3, C.byref(tile), C.byref(col), C.byref(half))) == 6
    assert (tile.value, col.value, half.value) == (0, 1, -1)
    _check(elf, (1, 1, 513, c, 512), 1, use_res, relu)


# ------------------------------------------------------------------------------------------------ C. the drained ends

@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("c", [64, 128])
def test_full_full_full_half_on_two_workgroups(elf, c, use_res, relu):
    """seven tiles at width 2: six full items and the seventh as two half items: both workgroups run full, full, full, half"""
    L = elf.lib()
    half = C.c_int()
    assert int(L.elfnet_conv3x3_f16_plan(7, 1, 2, 5, None, None, C.byref(half))) == 8 and half.value == -1
    assert int(L.elfnet_conv3x3_f16_plan(7, 1, 2, 6, None, None, C.byref(half))) == 8 and half.value == 0
    assert int(L.elfnet_conv3x3_f16_grid(7, 1, 2)) == 2
    _check(elf, (7, 16, 16, c, 256), 2, use_res, relu)


@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("width", [5, 8, 3])
def test_short_chains_and_fewer_items_than_workgroups(elf, width, use_res, relu):
    """five items: at width 5 every chain is a single item, at width 8 there are fewer items than workgroups, at width 3 two
    workgroups run two items and one runs one"""
    assert int(elf.lib().elfnet_conv3x3_f16_grid(5, 1, width)) == min(width, 5)
    _check(elf, (20, 8, 8, 64, 256), width, use_res, relu)


# ------------------------------------------------------------------------------------------------ D. carried rows do not leak

# 20 boards of 8 x 8 are four boards per tile: no tap crosses a tile, so a NaN in one tile's x reaches no other tile's outputs
@pytest.mark.parametrize("use_res,relu", [(False, 0), (True, 0)])
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("item,first", [(1, True), (3, True), (1, False), (2, False)])
def test_a_nan_in_x_stays_in_its_item(elf, c, item, first, use_res, relu):
    """first: x[first position of the item, channel 0], the first row the item before it stages early; else x[last position of
    the item, last channel], among the last rows staged while the next item's are already in flight"""
    import torch
    t = dict(_case(elf, 20, 8, 8, c, 256))
    x = t["x"].clone()
    xf = x.view(1280, c)
    if first:
        xf[256 * item, 0] = float("nan")
    else:
        xf[256 * item + 255, c - 1] = float("nan")
    t["x"] = x
    y = _launch(elf, t, use_res, relu, "linear", 1).view(5, 256, 256)
    y0 = _launch(elf, t, use_res, relu, "algo0").view(5, 256, 256)
    nan_tiles = [bool(torch.isnan(y[i]).any()) for i in range(5)]
    print("c %d item %d first %d res %d: tiles with a NaN %s" % (c, item, first, use_res, nan_tiles))
    assert nan_tiles == [i == item for i in range(5)]
    assert torch.equal(cc.bits(y), cc.bits(y0))
    clean = t["ref"][(use_res, relu)][0].view(5, 256, 256)
    for i in range(5):
        if i != item:
            assert torch.equal(cc.bits(y[i]), cc.bits(clean[i])), "tile %d changed" % i


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("p", [256, 511, 512, 1279])
def test_a_nan_row_of_res_stays_in_its_row(elf, c, p):
    import torch
    t = dict(_case(elf, 20, 8, 8, c, 256))
    r = t["r"].clone()
    r.view(1280, 256)[p, :] = float("nan")
    t["r"] = r
    y = _launch(elf, t, True, 0, "linear", 1).view(1280, 256)
    clean = t["ref"][(True, 0)][0].view(1280, 256)
    assert bool(torch.isnan(y[p]).all())
    keep = torch.ones(1280, dtype=torch.bool, device="cuda")
    keep[p] = False
    assert not bool(torch.isnan(y[keep]).any())
    assert torch.equal(cc.bits(y[keep]), cc.bits(clean[keep]))


@pytest.mark.parametrize("c", [64, 192])
@pytest.mark.parametrize("rows,h,wd", [(7, 5, 37), (7, 37, 5)])
def test_all_ones_count_the_taps_of_their_own_item(elf, rows, h, wd, c):
    """M = 1295: six tiles on one workgroup, boards that straddle the tiles.  At most 9 x 192 = 1728: exact in fp16"""
    import torch
    k = 256
    t = {"x": torch.ones((rows, h, wd, c), device="cuda", dtype=torch.float16),
         "w": torch.ones((k, 3, 3, c), device="cuda", dtype=torch.float16),
         "b": torch.zeros((k,), device="cuda", dtype=torch.float16), "r": None}
    rowc = np.array([(i > 0) + 1 + (i < h - 1) for i in range(h)])
    colc = np.array([(j > 0) + 1 + (j < wd - 1) for j in range(wd)])
    taps = torch.from_numpy((c * rowc[:, None] * colc[None, :]).astype(np.float32)).cuda()[None, :, :, None].expand(rows, h, wd, k)
    y = _launch(elf, t, False, 0, "linear", 1)
    y0 = _launch(elf, t, False, 0, "algo0")
    bad = int((y.float() != taps).sum().item())
    print("%s c %d: %d of %d differ from the nine-tap integers" % ((rows, h, wd), c, bad, y.numel()))
    assert bad == 0
    assert torch.equal(cc.bits(y), cc.bits(y0))


# ------------------------------------------------------------------------------------------------ E. launch against launch

@pytest.mark.parametrize("shape,width", [((20, 8, 8, 64, 256), 1), ((1, 1, 513, 64, 512), 1)])
def test_twenty_launches_are_bit_equal(elf, shape, width):
    import torch
    t = _case(elf, *shape)
    y0 = t["ref"][(True, 1)][0]
    for i in range(20):
        y = _launch(elf, t, True, 1, "linear", width)
        assert torch.equal(cc.bits(y), cc.bits(y0)), "launch %d differs from algo 0" % i
