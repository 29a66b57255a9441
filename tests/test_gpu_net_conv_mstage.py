"""GPU: the hand-written trunk convolution (algo 1, elf_amd/csrc/net_conv3x3.hip) with its LDS-DMA staging issued from the MFMA
segments.  Every staged half-tile is issued one segment later than before, so the counted waits of the load segments have new
counts (6 and 2 loads in flight for the full tile, 4 and 2 for the half tile, 0 in the last K tile) and a half-tile has three
slots to land in instead of four.  What that can break is a half-tile read before it has landed or restaged before it was read:
wrong tiles, or tiles that come and go from launch to launch.  So: the shortest loop (Cin = 64: nine K tiles, of which the prologue
and the two countdown tiles are most) and the odd K-tile counts, partial tiles, chains of items with the half tile at their end,
and a race screen.  Every comparison is exact: bit for bit against algo 0, against integers, and launch against launch; y is
prefilled with NaN and has a NaN guard row behind it."""
import ctypes as C

import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

F, H0, H1 = -1, 0, 1


def _seed(rows, h, wd, c, k):
    return 6262 + rows + 31 * h + 977 * wd + c + 7 * k


def _launch(L, x, w, b, r, y, relu, width=None):
    """algo 1; width None: elfnet_conv3x3_f16 (the device's own round width); otherwise elfnet_conv3x3_f16_width"""
    if width is None:
        return cc.launch(L, "plain", x, w, b, r, y, relu)
    return cc.launch(L, "linear", x, w, b, r, y, relu, width)


def _kinds(L, rows, h, wd, k, width):
    """the kinds (half) of every workgroup's items, by the library's own host arithmetic"""
    tiles, cols = (rows * h * wd + 255) // 256, k // 256
    ids = L.elfnet_conv3x3_f16_plan(tiles, cols, width, 0, None, None, None)
    G = L.elfnet_conv3x3_f16_grid(tiles, cols, width)
    hf = C.c_int()
    out = []
    for g in range(G):
        ch = []
        for i in range(g, ids, G):
            assert L.elfnet_conv3x3_f16_plan(tiles, cols, width, i, None, None, C.byref(hf)) == ids
            ch.append(hf.value)
        out.append(ch)
    return out


def _check_against_algo0(elf, rows, h, wd, c, k, use_res, relu, width):
    import torch
    shape = (rows, h, wd, c, k)
    x, w, b, res = cc.rand_case(_seed(*shape), *shape)
    want = cc.algo0_ref(elf.lib(), _seed(*shape), shape, use_res, relu)
    buf, y = cc.guarded(rows, h, wd, k)
    assert _launch(elf.lib(), x, w, b, res if use_res else None, y, relu, width) == 0
    torch.cuda.synchronize()
    print("%s width %s res %d relu %d: %d of %d elements differ from algo 0"
          % ((rows, h, wd, c, k), width, use_res, relu, int((y != want).sum().item()), y.numel()))
    assert torch.equal(y, want)
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("k", [256, 512])
@pytest.mark.parametrize("c", [64, 128, 192])
def test_short_and_odd_loops_are_bit_equal_with_algo_0(elf, c, k, use_res, relu):
    """9, 18 and 27 K tiles; four 9 x 9 boards are M = 324: one full tile and one of 68 rows, per channel column"""
    _check_against_algo0(elf, 4, 9, 9, c, k, use_res, relu, None)


@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("rows,h,wd", [(1, 9, 9), (1, 1, 257)])
def test_partial_tiles_are_bit_equal_with_algo_0(elf, rows, h, wd, c, use_res):
    """M = 81: one tile, and every row of its late half-tiles Xb is beyond M; M = 257: a second tile with one valid row"""
    _check_against_algo0(elf, rows, h, wd, c, 256, use_res, 1, None)


# rows, h, w, Cin, K, round width, the kinds of every workgroup's items
CHAINS = [(3, 19, 19, 64, 256, 1, [[F] * 5]),                      # five tiles (the last of 59 rows) in one workgroup
          (3, 19, 19, 64, 256, 2, [[F, F, H0], [F, F, H1]]),       # the last round split: full, full, half on both workgroups
          (3, 19, 19, 64, 256, 3, [[F, F], [F, F], [F]]),          # a fuller last round is left alone: full after full
          (3, 19, 19, 192, 256, 1, [[F] * 5]),                     # the same three at 27 K tiles
          (3, 19, 19, 192, 256, 2, [[F, F, H0], [F, F, H1]]),
          (3, 19, 19, 192, 256, 3, [[F, F], [F, F], [F]]),
          (7, 19, 19, 64, 256, 3, [[F, F, F, H0], [F, F, F, H1], [F, F, F]])]   # ten tiles at width 3: r = 1, split


@pytest.mark.parametrize("use_res,relu", [(False, 0), (True, 1)])
@pytest.mark.parametrize("rows,h,wd,c,k,width,kinds", CHAINS)
def test_chained_items_and_half_tiles_are_bit_equal_with_algo_0(elf, rows, h, wd, c, k, width, kinds, use_res, relu):
    """several items per workgroup: the first wait of an item that follows another counts the epilogue's stores, the half tile has
    its own counts, and a full item hands over to a half one"""
    assert _kinds(elf.lib(), rows, h, wd, k, width) == kinds
    _check_against_algo0(elf, rows, h, wd, c, k, use_res, relu, width)


@pytest.mark.parametrize("width", [None, 1, 2])
def test_repeated_launches(elf, width):
    """four 9 x 9 boards at Cin = 64: two tiles, nine K tiles, with the skip; one item per workgroup, both in one workgroup, and
    (width 2 of 2 items: no split) again one each through the explicit entry.  20 launches into fresh NaN-filled outputs: the first is
    algo 0's, every later one the first's.  A half-tile read before it has landed gives tiles that come and go."""
    import torch
    shape = rows, h, wd, c, k = 4, 9, 9, 64, 256
    x, w, b, r = cc.rand_case(_seed(*shape), *shape)
    want = cc.algo0_ref(elf.lib(), _seed(*shape), shape, True, 1)
    first = None
    for i in range(20):
        y = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert _launch(elf.lib(), x, w, b, r, y, 1, width) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert torch.equal(y, want), "the first launch differs from algo 0"
        else:
            assert torch.equal(y, first), "launch %d differs from the first" % i


def test_non_square_board_exact_integers(elf):
    """7 boards of 5 x 37 (M = 1295: six tiles whose rows straddle boards, the last with 15 rows) at width 2, Cin = 128, against the
    nine-tap form in integers: x in {-1,0,1}, w in {-1,0,1} with about 3/4 zeros and asymmetric in (ky,kx), integer bias and res;
    every partial sum is an integer below 2048 in magnitude, exact in fp32 and in fp16"""
    import torch
    rows, h, wd, c, k, width = 7, 5, 37, 128, 256, 2
    assert _kinds(elf.lib(), rows, h, wd, k, width) == [[F] * 3] * 2
    d = cc.int_case(4711, rows, h, wd, c, k)      # this one case has a seed of its own
    x, w, b, r, conv = d["x"], d["w"], d["b"], d["r"], d["conv"]
    assert not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(2))
    assert conv.abs().max().item() < 1024
    ref = torch.relu(conv + b.float() + r.float())
    buf, y = cc.guarded(rows, h, wd, k)
    assert _launch(elf.lib(), x, w, b, r, y, 1, width) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("5 x 37: %d of %d differ" % (bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())
