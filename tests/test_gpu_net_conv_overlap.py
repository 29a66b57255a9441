"""GPU: several work items per workgroup in the hand-written trunk convolution (elfnet_conv3x3_f16_width with algo 1,
elf_amd/csrc/net_conv3x3.hip): workgroup g of G = min(width, ids) runs the work ids g, g + G, ... one after the other, and behind an
item's main loop it decodes the next item's rows and issues that item's prologue before its own wave-private epilogue.  The round
width is given explicitly, so a few tiles make chains of every kind: full after full, half after full, a partial tile in the
middle, a column change, the shortest and an odd K-tile count.  What is carried from item to item (accumulators, tap masks, row
offsets, the bias column, the skip rows) is what can go wrong.  Every comparison is exact: bit for bit against algo 0, against algo
1 with one item per workgroup, against integers, and launch against launch; y is prefilled with NaN and has a NaN guard row."""
import ctypes as C

import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 99 + rows + 1000 * h + 31 * wd + c + 7 * k


def _rseed(rows, h, wd, c, k):
    return 5151 + rows + 31 * h + 977 * wd + c + 7 * k


def _chains(L, rows, h, wd, k, width):
    """the work ids of every workgroup as (tile, column, half), by the library's own host arithmetic"""
    tiles, cols = (rows * h * wd + 255) // 256, k // 256
    ids = L.elfnet_conv3x3_f16_plan(tiles, cols, width, 0, None, None, None)
    G = L.elfnet_conv3x3_f16_grid(tiles, cols, width)
    t, c, hf = C.c_int(), C.c_int(), C.c_int()
    out = []
    for g in range(G):
        ch = []
        for i in range(g, ids, G):
            assert L.elfnet_conv3x3_f16_plan(tiles, cols, width, i, C.byref(t), C.byref(c), C.byref(hf)) == ids
            ch.append((t.value, c.value, hf.value))
        out.append(ch)
    return out


def _reference(elf, rows, h, wd, c, k, use_res, relu, algo):
    """algo 0's output, or algo 1's with one item per workgroup (cc.ALONE); computed once per case"""
    shape = (rows, h, wd, c, k)
    if algo == 0:
        return cc.algo0_ref(elf.lib(), _rseed(*shape), shape, use_res, relu)
    return cc.cached_ref(elf.lib(), "linear", _rseed(*shape), shape, use_res, relu, cc.ALONE)


F, H0, H1 = -1, 0, 1
# rows, h, w, Cin, K, round width, the kinds (half) of every workgroup's items
CASES = [(3, 19, 19, 256, 256, 1, [[F] * 5]),                      # one workgroup runs all five items, the last one partial (59 rows)
         (4, 19, 19, 256, 256, 2, [[F] * 3] * 2),                  # three full items each
         (3, 19, 19, 256, 256, 2, [[F, F, H0], [F, F, H1]]),       # two full items, then a half item, on both workgroups
         (21, 9, 9, 256, 256, 5, [[F, H0], [F, H1], [F, H0], [F, H1], [F]]),   # seven tiles, r = 2: full then half, and one full only
         (3, 19, 19, 256, 512, 3, [[F, F, F, H0], [F, F, F, H1], [F] * 3]),    # ten items: a partial tile and a column change mid-chain
         (8, 9, 9, 64, 768, 2, [[F] * 4 + [H0], [F] * 4 + [H1]]),   # Cin = 64: nine K tiles, the prologue's whole depth; three columns
         (3, 19, 19, 192, 256, 2, [[F, F, H0], [F, F, H1]]),       # 27 K tiles, an odd count
         (1, 1, 513, 256, 256, 1, [[F] * 3])]                      # the last item has one valid row


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("rows,h,wd,c,k,width,kinds", CASES)
def test_chains_are_bit_equal_with_algo_0_and_with_one_item_per_workgroup(elf, rows, h, wd, c, k, width, kinds, use_res, relu):
    import torch
    L = elf.lib()
    chains = _chains(L, rows, h, wd, k, width)
    assert [[hf for _, _, hf in ch] for ch in chains] == kinds, chains
    if (rows, k, width) == (3, 512, 3):
        # workgroup 1: ids 1, 4, 7 (and the half id 10); id 4 is the partial tile of column 0, id 7 a full tile of column 1
        assert chains[1][:3] == [(1, 0, F), (4, 0, F), (2, 1, F)]
    x, w, b, res = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(L, "linear", x, w, b, res if use_res else None, y, relu, width) == 0
    torch.cuda.synchronize()
    for name, algo in (("algo 0", 0), ("algo 1, one item per workgroup", 1)):
        want = _reference(elf, rows, h, wd, c, k, use_res, relu, algo)
        print("%s width %d res %d relu %d: %d of %d elements differ from %s"
              % ((rows, h, wd, c, k), width, use_res, relu, int((y != want).sum().item()), y.numel(), name))
        assert torch.equal(y, want), name
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("h,wd", [(5, 37), (37, 5)])
def test_non_square_boards_exact_integers(elf, h, wd, c, use_res, relu):
    """7 boards of 5 x 37 or 37 x 5 (M = 1295: six tiles whose rows straddle boards, the last with 15 rows) at width 2: three
    items per workgroup; against the nine-tap fp32 form"""
    import torch
    rows, k, width = 7, 256, 2
    assert [[hf for _, _, hf in ch] for ch in _chains(elf.lib(), rows, h, wd, k, width)] == [[F] * 3] * 2
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    ref = d["conv"] + d["b"].float()
    if use_res:
        ref = ref + d["r"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", d["x"], d["w"], d["b"], d["r"] if use_res else None, y, relu, width) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("h %d w %d c %d res %d relu %d: %d of %d differ" % (h, wd, c, use_res, relu, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("width", [1, 2])
def test_tap_masks_are_the_items_own(elf, width):
    """all-ones x and w, zero bias, no ReLU, three 19 x 19 boards: every output is Cin x (the on-board taps of its position), exact
    in fp16 for Cin = 64 (at most 576).  Consecutive items of a workgroup have different mask patterns (a tile is 256 positions, a
    board 361), so a mask or a row offset left over from the item before shows as a wrong integer."""
    import torch
    rows, n, c, k = 3, 19, 64, 256
    x = torch.ones((rows, n, n, c), device="cuda", dtype=torch.float16)
    w = torch.ones((k, 3, 3, c), device="cuda", dtype=torch.float16)
    b = torch.zeros((k,), device="cuda", dtype=torch.float16)
    i = torch.arange(n, device="cuda")
    cnt = 3 - (i == 0).int() - (i == n - 1).int()
    want = (c * cnt[:, None] * cnt[None, :]).float()[None, :, :, None].expand(rows, n, n, k)
    buf, y = cc.guarded(rows, n, n, k)
    assert cc.launch(elf.lib(), "linear", x, w, b, None, y, 0, width) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != want).sum().item())
    print("width %d: %d of %d differ" % (width, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())


POISON = (3, 19, 19, 64, 256, 2)   # workgroup 0 runs tiles 0, 2 and half 0 of tile 4, workgroup 1 tiles 1, 3 and half 1 of tile 4


@pytest.mark.parametrize("ch", [127, 128])
def test_a_nan_weight_row_reaches_its_own_channel_only(elf, ch):
    """with that weight row NaN (no ReLU) the channel is NaN at every position, in every item of both chains, and every other
    channel is what it was"""
    import torch
    rows, h, wd, c, k, width = POISON
    x, w, b, r = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    want = _reference(elf, rows, h, wd, c, k, True, 0, 0)
    wn = w.clone()
    wn[ch] = float("nan")
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", x, wn, b, r, y, 0, width) == 0
    torch.cuda.synchronize()
    nan = torch.isnan(y)
    print("channel %d: %d NaN in it of %d, %d NaN elsewhere" % (ch, int(nan[..., ch].sum().item()), rows * h * wd,
                                                                int(nan.sum().item() - nan[..., ch].sum().item())))
    assert bool(nan[..., ch].all())
    keep = [i for i in range(k) if i != ch]
    assert torch.equal(y[..., keep], want[..., keep])
    assert bool(torch.isnan(buf[-1]).all())


def test_a_nan_in_x_stays_in_its_own_item(elf):
    """position 600 (board 1, row 12, column 11) lies in tile 2, the second item of workgroup 0: with one element of x NaN there,
    y is NaN at its nine neighbours on that board, in every channel, and nowhere else"""
    import torch
    rows, h, wd, c, k, width = POISON
    assert _chains(elf.lib(), rows, h, wd, k, width)[0][1] == (2, 0, F)
    x, w, b, r = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    want = _reference(elf, rows, h, wd, c, k, True, 0, 0)
    xn = x.clone()
    xn[1, 12, 11, 5] = float("nan")
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", xn, w, b, r, y, 0, width) == 0
    torch.cuda.synchronize()
    hit = torch.zeros((rows, h, wd), device="cuda", dtype=torch.bool)
    hit[1, 11:14, 10:13] = True
    nan = torch.isnan(y)
    print("%d NaN elements, %d expected" % (int(nan.sum().item()), 9 * k))
    assert torch.equal(nan, hit[..., None].expand_as(nan))
    assert torch.equal(y[~hit], want[~hit])
    assert bool(torch.isnan(buf[-1]).all())


def test_a_nan_row_of_res_reaches_its_own_row_only(elf):
    import torch
    rows, h, wd, c, k, width = POISON
    x, w, b, r = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    want = _reference(elf, rows, h, wd, c, k, True, 0, 0)
    rn = r.clone()
    rn[1, 12, 11] = float("nan")
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", x, w, b, rn, y, 0, width) == 0
    torch.cuda.synchronize()
    hit = torch.zeros((rows, h, wd), device="cuda", dtype=torch.bool)
    hit[1, 12, 11] = True
    nan = torch.isnan(y)
    print("%d NaN elements, %d expected" % (int(nan.sum().item()), k))
    assert torch.equal(nan, hit[..., None].expand_as(nan))
    assert torch.equal(y[~hit], want[~hit])
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("rows,h,wd,c,k,width", [(3, 19, 19, 256, 512, 3), (21, 9, 9, 256, 256, 5)])
def test_repeated_launches(elf, rows, h, wd, c, k, width):
    """the first wait of an item that follows another is placed by a count that includes the epilogue's stores: 20 launches into
    fresh NaN-filled outputs all return the bits of the first, and the first is algo 0's.  A first K tile read before it has
    landed gives wrong tiles that come and go from launch to launch."""
    import torch
    x, w, b, r = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    want = _reference(elf, rows, h, wd, c, k, True, 1, 0)
    first = None
    for i in range(20):
        y = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.launch(elf.lib(), "linear", x, w, b, r, y, 1, width) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert torch.equal(y, want), "the first launch differs from algo 0"
        else:
            assert torch.equal(y, first), "launch %d differs from the first" % i
