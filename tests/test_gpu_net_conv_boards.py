"""GPU: board order of the hand-written trunk convolution (algo 1, elf_amd/csrc/net_conv3x3.hip): a work item is one board
position (h, w) of 256 consecutive boards and runs only the taps that are on the board there, so items have 4, 6 or 9 taps (2 or 3
on a board one position wide), a chain of items on a workgroup has K-tile counts that change from item to item, and rows of one
item lie H W positions apart.  Everything goes through elfnet_conv3x3_f16_boards, which forces that order at any size.

A. Random operands: boards 19 x 19, 9 x 9, 5 x 7, 2 x 2, 1 x 5, 3 x 1 (and 2 x 5, whose row-major ranks run a 6-tap item behind a
   4-tap one); 256, 257, 300 and 513 rows (one exact block; a block with one valid board; partial blocks); C = 64 (one K tile per
   tap: a corner item is 4 K tiles, an end of a 1 x 5 board is 2, and 9 flips the buffer parity), 128, 192; K = 256 and 512;
   widths 1, 2, 3 and one above the item count; with and without skip and ReLU.
B. The chains those launches run, read from the plan: which tap counts follow which, in which LDS buffer parity.  With the deal
   longest-first a chain of a board with inner positions never runs a longer item behind a shorter one; the boards below 3 wide do.
C. Exact integers: all-ones x and w = 2^tap / C give every output the 9-bit mask of its own position, so a missing, doubled or
   wrong tap is a wrong integer.
D. A NaN in x reaches exactly its 3 x 3 neighbourhood on its own board; a NaN row of res its own row.
E. Twenty launches, bit-equal.
F. The plain entry takes the order elfnet_conv3x3_f16_order names and gives the same bits.

Every comparison is exact, against algo 0 and against algo 1 in linear order with one item per workgroup.  y is prefilled with NaN
and has a NaN guard row behind it."""
import ctypes as C

import pytest

import conv_cases as cc
from conv_cases import ALONE, RES_RELU, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu

# (rows, h, w, c, k)
SHAPES = [(256, 19, 19, 64, 256), (257, 19, 19, 128, 256),
          (256, 9, 9, 192, 256), (300, 9, 9, 64, 512), (513, 9, 9, 128, 256),
          (257, 5, 7, 64, 256), (513, 5, 7, 192, 512),
          (256, 2, 2, 64, 256), (300, 2, 2, 128, 512), (513, 2, 2, 192, 256),
          (257, 1, 5, 64, 256), (300, 1, 5, 192, 256), (513, 1, 5, 64, 512),
          (256, 3, 1, 64, 512), (300, 3, 1, 128, 256), (513, 3, 1, 64, 256),
          (300, 2, 5, 64, 256)]
WIDTHS = [1, 2, 3, ALONE]


def _seed(rows, h, wd, c, k):
    return 8191 + rows + 31 * h + 977 * wd + c + 7 * k


def _launch(elf, t, use_res, relu, how, width=0):
    """one launch into a fresh NaN-filled, guarded y (cc.run_guarded; how: cc.launch's)"""
    return cc.run_guarded(elf.lib(), how, t["x"], t["w"], t["b"], t["r"] if use_res else None, relu, width)


_cases = {}


def _case(elf, rows, h, wd, c, k):
    """random operands of one shape and, per (skip, ReLU), algo 0's output, which linear algo 1 with one item per workgroup must
    equal: made once and not changed"""
    import torch
    key = (rows, h, wd, c, k)
    if key not in _cases:
        x, w, b, r = cc.rand_case(_seed(*key), *key)
        t = {"x": x, "w": w, "b": b, "r": r, "ref": {}}
        for use_res, relu in RES_RELU:
            y0 = cc.algo0_ref(elf.lib(), _seed(*key), key, use_res, relu)
            ya = _launch(elf, t, use_res, relu, "linear", ALONE)
            assert not bool(torch.isnan(y0).any())
            assert torch.equal(cc.bits(ya), cc.bits(y0)), "linear algo 1 with one item per workgroup differs from algo 0"
            t["ref"][(use_res, relu)] = y0
        _cases[key] = t
    return _cases[key]


def _chains(L, rows, h, wd, c, k, width):
    """per workgroup, the K-tile counts of its items in the order it runs them"""
    G = L.elfnet_conv3x3_f16_boards_deal(rows, h, wd, k, width, -1, 0)
    m = C.c_int()
    out = []
    for g in range(G):
        ch, j = [], 0
        while True:
            i = L.elfnet_conv3x3_f16_boards_deal(rows, h, wd, k, width, g, j)
            if i < 0:
                break
            assert L.elfnet_conv3x3_f16_boards_plan(rows, h, wd, k, width, i, None, None, None, C.byref(m)) > 0
            ch.append(bin(m.value).count("1") * (c // 64))
            j += 1
        assert sum(ch) == L.elfnet_conv3x3_f16_boards_load(rows, h, wd, c, k, width, g)
        out.append(ch)
    return out


def _transitions(chains):
    """(K tiles of an item, K tiles of the item behind it, the LDS buffer parity that item starts in)"""
    seen = set()
    for ch in chains:
        par = 0
        for a, b in zip(ch, ch[1:]):
            par = (par + a) & 1
            seen.add((a, b, par))
    return seen


# ------------------------------------------------------------------------------------------------ A. random operands

@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_board_order_equals_algo0(elf, shape, width, use_res, relu):
    import torch
    t = _case(elf, *shape)
    y0 = t["ref"][(use_res, relu)]
    y = _launch(elf, t, use_res, relu, "board", width)
    print("%s width %d res %d relu %d: %d of %d elements differ from algo 0"
          % (shape, width, use_res, relu, int((cc.bits(y) != cc.bits(y0)).sum().item()), y.numel()))
    assert torch.equal(cc.bits(y), cc.bits(y0))


# ------------------------------------------------------------------------------------------------ B. the chains of those launches

def test_the_chains_have_the_wanted_transitions(elf):
    L = elf.lib()
    seen = {}
    for shape in SHAPES:
        for width in WIDTHS:
            seen[(shape, width)] = _transitions(_chains(L, *shape, width))
    assert not seen[((256, 19, 19, 64, 256), ALONE)]                                  # no chain at all
    one = seen[((256, 19, 19, 64, 256), 1)]                                          # C = 64: 9, 6 and 4 K tiles
    assert {(9, 9, 0), (9, 9, 1), (9, 6, 0), (6, 6, 0), (6, 4, 0), (4, 4, 0)} <= one | seen[((256, 19, 19, 64, 256), 2)]
    assert {(9, 6, 1), (6, 6, 1), (6, 4, 1), (4, 4, 1)} <= seen[((257, 5, 7, 64, 256), 1)] | seen[((257, 5, 7, 64, 256), 2)] | \
        seen[((257, 5, 7, 64, 256), 3)] | seen[((300, 9, 9, 64, 512), 1)] | seen[((300, 9, 9, 64, 512), 3)]
    # a board one position wide: ends of 2 K tiles (the first K tile is the last but one) between middles of 3, both parities
    ends = seen[((257, 1, 5, 64, 256), 1)] | seen[((513, 1, 5, 64, 512), 1)] | seen[((513, 3, 1, 64, 256), 1)] | \
        seen[((513, 3, 1, 64, 256), 2)] | seen[((256, 3, 1, 64, 512), 1)]
    # (only 2-tile items can stand in front of the first 3-tile item of a chain, so that one always starts in buffer 0)
    assert {(2, 3, 0), (3, 3, 1), (3, 3, 0), (3, 2, 1), (3, 2, 0), (2, 2, 0), (2, 2, 1)} <= ends, ends
    # a longer item behind a shorter one: row-major ranks on a board two positions high
    assert {(4, 6), (6, 4), (6, 6)} <= {(a, b) for a, b, _ in seen[((300, 2, 5, 64, 256), 1)]}
    # several chunks per tap
    assert {(18, 12, 0), (27, 18, 1), (12, 12, 0)} <= seen[((257, 19, 19, 128, 256), 1)] | seen[((256, 9, 9, 192, 256), 1)]


# ------------------------------------------------------------------------------------------------ C. exact integers

@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("rows,h,wd,c", [(257, 19, 19, 64), (300, 5, 7, 128), (257, 2, 2, 64), (300, 1, 5, 64), (257, 3, 1, 128)])
def test_every_output_is_the_mask_of_its_position(elf, rows, h, wd, c, width):
    """x = 1, w[k, ky, kx, :] = 2^(3 ky + kx) / C: the sum over the taps on the board is the position's 9-bit mask, at most 511"""
    import torch
    k = 256
    w = torch.empty((k, 3, 3, c), device="cuda", dtype=torch.float16)
    for tap in range(9):
        w[:, tap // 3, tap % 3, :] = float(1 << tap) / c
    t = {"x": torch.ones((rows, h, wd, c), device="cuda", dtype=torch.float16), "w": w,
         "b": torch.zeros((k,), device="cuda", dtype=torch.float16), "r": None}
    want = torch.zeros((h, wd), dtype=torch.float32)
    for hh in range(h):
        for ww in range(wd):
            want[hh, ww] = sum(1 << (3 * ky + kx) for ky in range(3) for kx in range(3)
                               if 0 <= hh + ky - 1 < h and 0 <= ww + kx - 1 < wd)
    want = want.cuda()[None, :, :, None].expand(rows, h, wd, k)
    y = _launch(elf, t, False, 0, "board", width)
    bad = int((y.float() != want).sum().item())
    print("%s c %d width %d: %d of %d differ from the mask integers" % ((rows, h, wd), c, width, bad, y.numel()))
    assert bad == 0
    assert torch.equal(cc.bits(y), cc.bits(_launch(elf, t, False, 0, "algo0")))


# ------------------------------------------------------------------------------------------------ D. NaNs stay where they belong

@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("shape,board,hh,ww", [((257, 5, 7, 64, 256), 3, 0, 0), ((257, 5, 7, 64, 256), 255, 2, 3),
                                               ((257, 5, 7, 64, 256), 256, 4, 6), ((300, 1, 5, 192, 256), 299, 0, 4),
                                               ((513, 9, 9, 128, 256), 256, 8, 4)])
def test_a_nan_in_x_reaches_its_neighbourhood_on_its_board(elf, shape, board, hh, ww, width):
    import torch
    t = dict(_case(elf, *shape))
    rows, h, wd, c, k = shape
    x = t["x"].clone()
    x[board, hh, ww, c - 1] = float("nan")
    t["x"] = x
    y = _launch(elf, t, True, 0, "board", width)
    want = torch.zeros((rows, h, wd), dtype=torch.bool, device="cuda")
    want[board, max(hh - 1, 0):hh + 2, max(ww - 1, 0):ww + 2] = True
    isn = torch.isnan(y)
    assert torch.equal(isn.all(dim=3), want) and torch.equal(isn.any(dim=3), want)
    clean = t["ref"][(True, 0)]
    assert torch.equal(cc.bits(y[~want]), cc.bits(clean[~want]))


@pytest.mark.parametrize("shape,p", [((257, 5, 7, 64, 256), 0), ((257, 5, 7, 64, 256), 256 * 35 + 34), ((513, 9, 9, 128, 256), 255 * 81 + 80),
                                     ((300, 2, 2, 128, 512), 299 * 4 + 3)])
def test_a_nan_row_of_res_stays_in_its_row(elf, shape, p):
    import torch
    t = dict(_case(elf, *shape))
    rows, h, wd, c, k = shape
    r = t["r"].clone()
    r.view(-1, k)[p, :] = float("nan")
    t["r"] = r
    y = _launch(elf, t, True, 0, "board", 2).view(-1, k)
    clean = t["ref"][(True, 0)].view(-1, k)
    assert bool(torch.isnan(y[p]).all())
    keep = torch.ones(y.shape[0], dtype=torch.bool, device="cuda")
    keep[p] = False
    assert not bool(torch.isnan(y[keep]).any())
    assert torch.equal(cc.bits(y[keep]), cc.bits(clean[keep]))


# ------------------------------------------------------------------------------------------------ E. launch against launch

@pytest.mark.parametrize("shape,width", [((257, 5, 7, 64, 256), 3), ((513, 1, 5, 64, 512), 1)])
def test_twenty_launches_are_bit_equal(elf, shape, width):
    import torch
    t = _case(elf, *shape)
    y0 = t["ref"][(True, 1)]
    for i in range(20):
        y = _launch(elf, t, True, 1, "board", width)
        assert torch.equal(cc.bits(y), cc.bits(y0)), "launch %d differs from algo 0" % i


# ------------------------------------------------------------------------------------------------ F. the plain entry

@pytest.mark.parametrize("shape", [(256, 9, 9, 192, 256), (1024, 9, 9, 64, 256)])
def test_the_plain_entry_takes_the_order_the_rule_names(elf, shape):
    """256 x 9 x 9 is one round in either order on any device of at least 81 CUs: linear.  1024 x 9 x 9 at C = 64 is 324 items: on
    256 CUs a split last round in linear order (15.75 K tiles) against 13 in board order.  Whatever the device, the order is the one
    the rule names at its CU count, and the bits are algo 0's."""
    import torch
    L = elf.lib()
    rows, h, wd, c, k = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    order = L.elfnet_conv3x3_f16_order(rows, h, wd, c, k, 0)
    assert order in (0, 1) and order == L.elfnet_conv3x3_f16_order(rows, h, wd, c, k, cus)
    if cus == 256:
        assert order == (1 if rows == 1024 else 0)
    t = _case(elf, *shape)
    for use_res, relu in RES_RELU:
        y = _launch(elf, t, use_res, relu, "plain")
        assert torch.equal(cc.bits(y), cc.bits(t["ref"][(use_res, relu)]))
        yb = _launch(elf, t, use_res, relu, "board", 0)
        assert torch.equal(cc.bits(yb), cc.bits(y))
