"""CPU: the host arithmetic of algo 1's board order (elf_amd/csrc/net_conv3x3.hip): elfnet_conv3x3_f16_boards_plan, _deal and
_load, and elfnet_conv3x3_f16_order, the rule by which the plain entry picks an order.  The kernel decodes its work ids with the
same functions, so a wrong plan here is a wrong or missing output tile there."""
import ctypes as C

import pytest

BADARG = -1
BOARDS = [(19, 19), (9, 9), (5, 7), (2, 2), (1, 5), (3, 1)]


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _plan(L, rows, h, w, k, width):
    """[(block, position, column, mask)] by work id"""
    ids = L.elfnet_conv3x3_f16_boards_plan(rows, h, w, k, width, -1, None, None, None, None)
    assert ids > 0
    out = []
    b, p, c, m = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7)
    for i in range(ids):
        assert L.elfnet_conv3x3_f16_boards_plan(rows, h, w, k, width, i, C.byref(b), C.byref(p), C.byref(c), C.byref(m)) == ids
        out.append((b.value, p.value, c.value, m.value))
    return out


def _chains(L, rows, h, w, k, width):
    G = L.elfnet_conv3x3_f16_boards_deal(rows, h, w, k, width, -1, 0)
    chains = []
    for g in range(G):
        ch, j = [], 0
        while True:
            i = L.elfnet_conv3x3_f16_boards_deal(rows, h, w, k, width, g, j)
            if i < 0:
                break
            ch.append(i)
            j += 1
        chains.append(ch)
    return chains


def _brute_mask(h, w, hh, ww):
    m = 0
    for ky in range(3):
        for kx in range(3):
            if 0 <= hh + ky - 1 < h and 0 <= ww + kx - 1 < w:
                m |= 1 << (3 * ky + kx)
    return m


@pytest.mark.parametrize("h,w", BOARDS)
@pytest.mark.parametrize("rows,k,width", [(256, 256, 3), (257, 512, 7), (513, 256, 256), (300, 512, 1000000)])
def test_every_item_once_with_its_mask(L, h, w, rows, k, width):
    plan = _plan(L, rows, h, w, k, width)
    blocks, cols = (rows + 255) // 256, k // 256
    assert len(plan) == blocks * h * w * cols
    assert sorted((b, p, c) for b, p, c, _ in plan) == [(b, p, c) for b in range(blocks) for p in range(h * w) for c in range(cols)]
    for b, p, c, m in plan:
        assert m == _brute_mask(h, w, p // w, p % w), (p, m)
    # every work id runs on exactly one workgroup, and a workgroup's load is its items' taps x C / 64
    chains = _chains(L, rows, h, w, k, width)
    assert len(chains) == min(width, len(plan))
    assert sorted(i for ch in chains for i in ch) == list(range(len(plan)))
    for ch_in in (64, 192):
        for g, ch in enumerate(chains):
            want = sum(bin(plan[i][3]).count("1") * (ch_in // 64) for i in ch)
            assert L.elfnet_conv3x3_f16_boards_load(rows, h, w, ch_in, k, width, g) == want


def test_long_items_first_block_fastest(L):
    """19 x 19, two blocks: the ids run over inner positions, edges, corners, each row-major, the block fastest"""
    plan = _plan(L, 512, 19, 19, 256, 256)
    taps = [bin(m).count("1") for _, _, _, m in plan]
    assert taps == sorted(taps, reverse=True)
    assert [b for b, _, _, _ in plan] == [0, 1] * 361
    for n in (9, 6, 4):
        pos = [p for (b, p, _, m) in plan if b == 0 and bin(m).count("1") == n]
        assert pos == sorted(pos)


def test_headline_shape(L):
    rows, n, ch = 2048, 19, 256
    ids = L.elfnet_conv3x3_f16_boards_plan(rows, n, n, ch, 256, -1, None, None, None, None)
    assert ids == 8 * 361
    loads = [L.elfnet_conv3x3_f16_boards_load(rows, n, n, ch, ch, 256, g) for g in range(256)]
    assert sum(loads) == 96800
    assert max(loads) <= 396
    assert loads[:8] == [384] * 8 and loads[8:184] == [372] * 176 and set(loads[184:]) == {388, 396}
    # the linear plan: 2888 items on 256 workgroups are eleven full rounds and 72 items, split into 144 half tiles: 11 x 36 + 27
    tiles = (rows * n * n + 255) // 256
    assert L.elfnet_conv3x3_f16_plan(tiles, 1, 256, 0, None, None, None) == tiles + 72
    assert 11 * 36 + 27 == 423 > max(loads)
    assert L.elfnet_conv3x3_f16_order(rows, n, n, ch, ch, 256) == 1


def test_order_rule(L):
    # fewer than 256 rows: linear, whatever the loads
    for rows in (1, 5, 91, 255):
        for h, w in BOARDS:
            assert L.elfnet_conv3x3_f16_order(rows, h, w, 256, 256, 256) == 0
            assert L.elfnet_conv3x3_f16_order(rows, h, w, 64, 256, 2) == 0
    # the shapes of the poisoned-weight tests and of a 91-row call
    assert L.elfnet_conv3x3_f16_order(5, 9, 9, 256, 256, 256) == 0
    assert L.elfnet_conv3x3_f16_order(91, 19, 19, 256, 256, 256) == 0
    # 256 x 9 x 9 on 256 workgroups is one round either way (81 items, the longest 36 K tiles in both): not strictly fewer
    assert L.elfnet_conv3x3_f16_order(256, 9, 9, 256, 256, 256) == 0
    # the rule itself, from the two plans, at widths with full, split and unsplit last rounds
    for rows, h, w, ch, k, width in [(2048, 19, 19, 256, 256, 256), (256, 9, 9, 64, 256, 8), (512, 9, 9, 128, 512, 60),
                                     (300, 5, 7, 64, 256, 4), (1024, 19, 19, 256, 256, 304), (256, 2, 2, 64, 256, 1)]:
        total = (rows * h * w + 255) // 256 * (k // 256)
        full, r = divmod(total, width)
        split = total >= width and 0 < 2 * r <= width
        lin4 = (4 * full + (0 if r == 0 else 3 if split else 4)) * 9 * (ch // 64)
        G = L.elfnet_conv3x3_f16_boards_deal(rows, h, w, k, width, -1, 0)
        most = max(L.elfnet_conv3x3_f16_boards_load(rows, h, w, ch, k, width, g) for g in range(G))
        assert L.elfnet_conv3x3_f16_order(rows, h, w, ch, k, width) == (1 if 4 * most < lin4 else 0), (rows, h, w, ch, k, width)


def test_refusals(L):
    assert L.elfnet_conv3x3_f16_boards_plan(0, 9, 9, 256, 4, -1, None, None, None, None) == BADARG
    assert L.elfnet_conv3x3_f16_boards_plan(256, 9, 9, 128, 4, -1, None, None, None, None) == BADARG     # k % 256
    assert L.elfnet_conv3x3_f16_boards_plan(256, 9, 9, 256, 0, -1, None, None, None, None) == BADARG     # host arithmetic needs a width
    assert L.elfnet_conv3x3_f16_boards_plan(256, 9, 9, 256, 4, 81, None, None, None, None) == BADARG     # one past the last id
    assert L.elfnet_conv3x3_f16_boards_deal(256, 9, 9, 256, 4, 4, 0) == BADARG
    assert L.elfnet_conv3x3_f16_boards_load(256, 9, 9, 96, 256, 4, 0) == BADARG                         # c % 64
    assert L.elfnet_conv3x3_f16_boards_load(256, 1, 1, 64, 256, 4, 0) == BADARG                         # an item of one K tile
    assert L.elfnet_conv3x3_f16_boards_load(256, 1, 1, 128, 256, 1, 0) == 2
    assert L.elfnet_conv3x3_f16_order(256, 9, 9, 96, 256, 4) == BADARG
