"""CPU: elfnet_conv3x3_f16_grid (elf_amd/csrc/net_conv3x3.hip), the host arithmetic of how many workgroups algo 1 launches.
Workgroup g of G runs the work ids g, g + G, g + 2 G, ... of elfnet_conv3x3_f16_plan one after the other: together they cover every
id exactly once, and a half id is always the last item of its workgroup (the kernel relies on both)."""
import ctypes as C

import pytest

BADARG = -1


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _ids(L, tiles, cols, width):
    return L.elfnet_conv3x3_f16_plan(tiles, cols, width, 0, None, None, None)


def _half(L, tiles, cols, width, i):
    h = C.c_int(-7)
    assert L.elfnet_conv3x3_f16_plan(tiles, cols, width, i, None, None, C.byref(h)) > 0
    return h.value


def test_grid_refuses_what_the_plan_refuses(L):
    for tiles, cols, width in ((0, 1, 4), (5, 0, 4), (5, 1, 0), (5, 1, -1), (1 << 29, 2, 4), (-3, 1, 4), (5, -1, 4)):
        assert _ids(L, tiles, cols, width) == BADARG, (tiles, cols, width)
        assert L.elfnet_conv3x3_f16_grid(tiles, cols, width) == BADARG, (tiles, cols, width)
    assert L.elfnet_conv3x3_f16_grid((1 << 29) - 1, 2, 4) == 4


@pytest.mark.parametrize("cols", [1, 2, 3])
def test_the_chains_cover_every_id_once_and_a_half_id_ends_its_chain(L, cols):
    for total in range(cols, 41, cols):
        tiles = total // cols
        for width in list(range(1, 10)) + [1 << 30]:
            ids = _ids(L, tiles, cols, width)
            G = L.elfnet_conv3x3_f16_grid(tiles, cols, width)
            assert G == min(width, ids), (total, width)
            chains = [list(range(g, ids, G)) for g in range(G)]
            assert sorted(i for ch in chains for i in ch) == list(range(ids)), (total, width)
            assert all(ch for ch in chains)
            for ch in chains:
                halves = [_half(L, tiles, cols, width, i) >= 0 for i in ch]
                assert not any(halves[:-1]), (total, width, ch)          # a half id only as the last item
            if total < width:
                assert all(len(ch) == 1 for ch in chains)
            # a chain never starts with a half id: the split needs one whole round of full items in front of it
            assert all(_half(L, tiles, cols, width, ch[0]) < 0 for ch in chains), (total, width)


def test_the_headline_launch(L):
    """2888 tiles x 1 column on 256 CUs: 2816 full ids and 144 half ids on 256 workgroups; the first 144 run eleven full items and
    a half item, the others eleven full items"""
    tiles, cols, width = 2888, 1, 256
    ids = _ids(L, tiles, cols, width)
    assert ids == 2888 + 72
    G = L.elfnet_conv3x3_f16_grid(tiles, cols, width)
    assert G == 256
    for g in range(G):
        ch = list(range(g, ids, G))
        kinds = [_half(L, tiles, cols, width, i) for i in ch]
        if g < 144:
            assert len(ch) == 12 and all(k < 0 for k in kinds[:11]) and kinds[11] in (0, 1), g
        else:
            assert len(ch) == 11 and all(k < 0 for k in kinds), g
    assert L.elfnet_conv3x3_f16_grid(tiles, cols, 1 << 30) == 2888
