"""CPU: elfnet_conv3x3_f16_width (elf_amd/csrc/net_conv.hip, net_conv3x3.hip) refuses bad arguments with ELFGO_E_BADARG before it
touches the GPU runtime -- the pointers here are made-up addresses that are never read -- and elfnet_conv3x3_f16_plan, the host
arithmetic of its launch, hands every (tile, column, half) out exactly once."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
X, W, B, R, Y = (C.c_void_p(A * i) for i in range(1, 6))


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _conv(L, x=X, w=W, b=B, r=R, y=Y, rows=2, n=9, c=64, k=256, algo=1, width=0):
    return L.elfnet_conv3x3_f16_width(x, w, b, r, y, rows, n, n, c, k, 1, algo, width, None)


def test_accepts_no_rows_before_the_runtime(L):
    """rows = 0 is accepted after every argument check and before the first call into the GPU runtime"""
    for algo in (0, 1):
        for width in (0, 1, 4, 1 << 30):
            assert _conv(L, rows=0, algo=algo, width=width) == 0


@pytest.mark.parametrize("algo", [0, 1])
def test_refuses_a_negative_width_and_an_unknown_algo(L, algo):
    assert _conv(L, algo=algo, width=-1) == BADARG
    assert _conv(L, rows=0, algo=algo, width=-1) == BADARG
    assert _conv(L, rows=0, algo=algo, width=-(1 << 31)) == BADARG
    for width in (0, 4):
        assert _conv(L, algo=2, width=width) == BADARG
        assert _conv(L, rows=0, algo=2, width=width) == BADARG
        assert _conv(L, rows=0, algo=-1, width=width) == BADARG


@pytest.mark.parametrize("width", [0, 4])
def test_refuses_what_elfnet_conv3x3_f16_refuses(L, width):
    for null in ("x", "w", "b", "y"):
        assert _conv(L, width=width, **{null: None}) == BADARG, null
    for name in ("x", "w", "b", "r", "y"):
        assert _conv(L, width=width, **{name: C.c_void_p(A * 9 + 8)}) == BADARG, name   # 8-B aligned only
    assert _conv(L, width=width, c=12) == BADARG and _conv(L, width=width, k=12) == BADARG            # c % 8, k % 8
    assert _conv(L, width=width, c=0) == BADARG and _conv(L, width=width, k=0) == BADARG
    assert _conv(L, width=width, y=X) == BADARG and _conv(L, width=width, y=R) == BADARG              # y == x, y == res
    assert _conv(L, width=width, rows=-1) == BADARG and _conv(L, width=width, n=0) == BADARG
    assert _conv(L, width=width, rows=1 << 22, n=19) == BADARG                                        # y of 2^22 * 361 * 256 * 2 B
    assert L.elfnet_conv3x3_f16(X, W, B, R, Y, 0, 9, 9, 64, 256, 1, 1, None) == 0                     # the old entry: width 0


def _plan(L, tiles, cols, width):
    t, c, h = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    groups = L.elfnet_conv3x3_f16_plan(tiles, cols, width, 0, None, None, None)
    out = []
    for i in range(groups):
        assert L.elfnet_conv3x3_f16_plan(tiles, cols, width, i, C.byref(t), C.byref(c), C.byref(h)) == groups
        out.append((t.value, c.value, h.value))
    return out


@pytest.mark.parametrize("cols", [1, 2, 3])
def test_every_tile_column_and_half_is_handed_out_exactly_once(L, cols):
    """total 1 .. 40 x width 1 .. 9 (and the totals that are multiples of 2 and 3 as two and three channel columns): the tail is
    split iff total >= width and 0 < 2 r <= width; ids below total - r are full items in the unsplit order, tiles fastest, then
    the column; each of the last r items is two consecutive ids, half 0, then half 1"""
    for total in range(cols, 41, cols):
        tiles = total // cols
        order = [(i % tiles, i // tiles) for i in range(total)]
        for width in range(1, 10):
            r = total % width
            split = total >= width and 0 < 2 * r <= width
            got = _plan(L, tiles, cols, width)
            if not split:
                assert got == [(t, c, -1) for t, c in order], (total, width)
                continue
            assert len(got) == total + r
            assert got[:total - r] == [(t, c, -1) for t, c in order[:total - r]], (total, width)
            want = [(t, c, h) for t, c in order[total - r:] for h in (0, 1)]
            assert got[total - r:] == want, (total, width)
            assert len(set(got)) == len(got)
            assert {(t, c) for t, c, _ in got} == set(order)


def test_plan_refuses_bad_arguments(L):
    t = C.c_int(-7)
    assert L.elfnet_conv3x3_f16_plan(0, 1, 4, 0, None, None, None) == BADARG
    assert L.elfnet_conv3x3_f16_plan(5, 0, 4, 0, None, None, None) == BADARG
    assert L.elfnet_conv3x3_f16_plan(5, 1, 0, 0, None, None, None) == BADARG
    assert L.elfnet_conv3x3_f16_plan(5, 1, -1, 0, None, None, None) == BADARG
    assert L.elfnet_conv3x3_f16_plan(1 << 29, 2, 4, 0, None, None, None) == BADARG
    assert L.elfnet_conv3x3_f16_plan(5, 1, 4, 6, C.byref(t), None, None) == BADARG and t.value == -7   # 5 + 1 workgroups: ids 0 .. 5
    assert L.elfnet_conv3x3_f16_plan(5, 1, 4, -1, C.byref(t), None, None) == BADARG
    assert L.elfnet_conv3x3_f16_plan(5, 1, 4, 5, C.byref(t), None, None) == 6 and t.value == 4
    # the headline: 2888 tiles on 256 CUs, r = 72
    assert L.elfnet_conv3x3_f16_plan(2888, 1, 256, 0, None, None, None) == 2888 + 72
    assert L.elfnet_conv3x3_f16_plan(2888, 1, 1 << 30, 0, None, None, None) == 2888
