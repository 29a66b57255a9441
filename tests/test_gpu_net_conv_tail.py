"""GPU: the split last round of the hand-written trunk convolution (elfnet_conv3x3_f16_width with algo 1,
elf_amd/csrc/net_conv3x3.hip): where the last round of work items is at most half full, each of its items runs as two workgroups
of 256 positions x 128 channels.  The round width is given explicitly, so a few tiles reach every branch of the rule.  Every
comparison is exact: bit for bit against algo 0, against algo 1 with a width that never splits, against the integer nine-tap
form, and launch against launch; y is prefilled with NaN and has a NaN guard row behind it."""
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 99 + rows + 1000 * h + 31 * wd + c + 7 * k


def _rseed(rows, h, wd, c, k):
    return 5151 + rows + 31 * h + 977 * wd + c + 7 * k


def _groups(L, rows, h, wd, k, width):
    """(work items, workgroups of the launch) by the library's own host arithmetic"""
    tiles = (rows * h * wd + 255) // 256
    return tiles * (k // 256), L.elfnet_conv3x3_f16_plan(tiles, k // 256, width, 0, None, None, None)


def _reference(elf, rows, h, wd, c, k, use_res, relu, algo):
    """algo 0's output, or algo 1's with a width that never splits (cc.ALONE); computed once per case"""
    shape = (rows, h, wd, c, k)
    if algo == 0:
        return cc.algo0_ref(elf.lib(), _rseed(*shape), shape, use_res, relu)
    return cc.cached_ref(elf.lib(), "linear", _rseed(*shape), shape, use_res, relu, cc.ALONE)


# rows, h, w, Cin, K, round width, whether the rule splits
CASES = [(3, 19, 19, 256, 256, 4, True),     # 5 tiles, r = 1: the split item is the partial tile (59 rows)
         (4, 19, 19, 256, 256, 4, True),     # 6 tiles, 2 r == width
         (21, 9, 9, 256, 256, 4, False),     # 7 tiles, 2 r > width
         (25, 9, 9, 256, 256, 4, False),     # 8 tiles, r == 0
         (3, 19, 19, 256, 256, 8, False),    # 5 tiles, total < width
         (12, 9, 9, 256, 256, 3, True),      # an odd width: 4 tiles, r = 1
         (21, 9, 9, 256, 256, 3, True),      # ... 7 tiles, r = 1
         (1, 1, 513, 256, 256, 2, True),     # 3 tiles, the split one has one valid row
         (3, 19, 19, 256, 512, 4, True),     # K = 512: 5 tiles x 2 columns (an even total whatever the tiles), r = 2: both in column 1
         (8, 9, 9, 64, 768, 4, True),        # K = 768: 3 tiles x 3 columns, an odd total, r = 1: the last tile of column 2
         (3, 19, 19, 64, 256, 4, True),      # Cin = 64: 9 K tiles, the prologue's depth
         (3, 19, 19, 192, 256, 4, True)]     # Cin = 192: 27 K tiles, an odd count


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("rows,h,wd,c,k,width,split", CASES)
def test_split_launch_is_bit_equal_with_algo_0_and_with_the_unsplit_launch(elf, rows, h, wd, c, k, width, split, use_res, relu):
    import torch
    L = elf.lib()
    total, groups = _groups(L, rows, h, wd, k, width)
    r = total % width
    assert groups == (total + r if split else total), (total, groups)
    x, w, b, res = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(L, "linear", x, w, b, res if use_res else None, y, relu, width) == 0
    torch.cuda.synchronize()
    for name, algo in (("algo 0", 0), ("algo 1 unsplit", 1)):
        want = _reference(elf, rows, h, wd, c, k, use_res, relu, algo)
        print("%s width %d res %d relu %d: %d of %d elements differ from %s"
              % ((rows, h, wd, c, k), width, use_res, relu, int((y != want).sum().item()), y.numel(), name))
        assert torch.equal(y, want), name
    assert bool(torch.isnan(buf[-1]).all())


def test_a_negative_width_launches_nothing(elf):
    import torch
    rows, h, wd, c, k = 3, 19, 19, 64, 256
    x, w, b, _ = cc.rand_case(_rseed(rows, h, wd, c, k), rows, h, wd, c, k)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", x, w, b, None, y, 1, -1) == -1
    assert cc.launch(elf.lib(), "linear", x, w, b, None, y, 1, 4, algo=2) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("h,wd", [(5, 7), (7, 5)])
def test_non_square_boards_exact_integers(elf, h, wd, c, use_res, relu):
    """20 boards of 5 x 7 or 7 x 5 (M = 700: three tiles whose rows straddle boards) at width 2: the third tile, 188 rows, is the
    split one; against the nine-tap fp32 form"""
    import torch
    rows, k, width = 20, 256, 2
    assert _groups(elf.lib(), rows, h, wd, k, width) == (3, 4)
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


@pytest.mark.parametrize("ch", [127, 128])
def test_a_nan_weight_row_reaches_its_own_channel_only(elf, ch):
    """channel 127 is the last of half 0 and 128 the first of half 1: with that weight row NaN (no ReLU) the channel is NaN at
    every position, in the full tiles and in the split one, and every other channel is what it was"""
    import torch
    rows, h, wd, c, k, width = 3, 19, 19, 64, 256, 4
    assert _groups(elf.lib(), rows, h, wd, k, width) == (5, 6)
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


@pytest.mark.parametrize("c", [64, 192])
def test_repeated_split_launches(elf, c):
    """the half tile's waits are placed by a count of their own (three half-tiles in flight, vmcnt(6)): 20 launches of a split case
    into fresh NaN-filled outputs all return the bits of the first, and the first is algo 0's.  A half-tile read before it has
    landed, or restaged before its last read, gives wrong tiles that come and go from launch to launch."""
    import torch
    rows, h, wd, k, width = 4, 19, 19, 256, 4
    assert _groups(elf.lib(), rows, h, wd, k, width) == (6, 8)
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
