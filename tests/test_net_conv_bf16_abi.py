"""CPU: the bf16 trunk convolution's entries (elf_amd/csrc/net_conv3x3_bf16.hip) are exported and refuse bad arguments with
ELFGO_E_BADARG before they touch the GPU runtime -- the pointers here are made-up addresses that are never read --, the tile rule
elfnet_conv3x3_bf16_pick is the header's arithmetic, and FusedInferenceNet._fusable_bf16 names the convolutions it takes."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
X, W, B, R, Y = (C.c_void_p(A * i) for i in range(1, 6))


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _conv(L, x=X, w=W, b=B, r=R, y=Y, rows=2, h=9, wd=9, c=64, k=64, tile=None):
    if tile is None:
        return L.elfnet_conv3x3_bf16(x, w, b, r, y, rows, h, wd, c, k, 1, None)
    return L.elfnet_conv3x3_bf16_tile(x, w, b, r, y, rows, h, wd, c, k, 1, tile, None)


def test_the_symbols_are_exported_and_declared(L):
    import elf_amd._lib as lib
    for name, nargs in (("elfnet_conv3x3_bf16", 12), ("elfnet_conv3x3_bf16_tile", 13), ("elfnet_conv3x3_bf16_pick", 3)):
        assert name in lib.SIGNATURES
        assert getattr(L, name).restype is C.c_int and len(getattr(L, name).argtypes) == nargs


@pytest.mark.parametrize("tile", [None, 0, 64, 128])
def test_no_rows_pointers_and_sizes(L, tile):
    """rows = 0 is accepted after every argument check and before the first call into the GPU runtime; the checks are conv_args'"""
    assert _conv(L, rows=0, k=128, tile=tile) == 0 and _conv(L, rows=0, k=128, r=None, tile=tile) == 0
    assert _conv(L, rows=0, c=192, k=256, h=19, wd=7, tile=tile) == 0
    for null in ("x", "w", "b", "y"):
        assert _conv(L, k=128, tile=tile, **{null: None}) == BADARG and _conv(L, rows=0, k=128, tile=tile, **{null: None}) == BADARG, null
    for name in ("x", "w", "b", "r", "y"):
        assert _conv(L, rows=0, k=128, tile=tile, **{name: C.c_void_p(A * 9 + 8)}) == BADARG, name   # 8-B aligned only
    assert _conv(L, rows=0, k=128, y=X, tile=tile) == BADARG and _conv(L, rows=0, k=128, y=R, tile=tile) == BADARG   # y == x, y == res
    assert _conv(L, rows=-1, k=128, tile=tile) == BADARG and _conv(L, h=0, k=128, tile=tile) == BADARG
    assert _conv(L, rows=1 << 22, h=19, wd=19, c=256, k=256, tile=tile) == BADARG        # y of 2^22 * 361 * 256 * 2 B
    assert _conv(L, rows=1 << 22, h=19, wd=19, c=256, k=128, tile=tile) == BADARG        # x of that size
    assert _conv(L, rows=0, c=1 << 14, k=1 << 13, tile=tile) == BADARG                   # w of 2^27 * 9 elements
    assert _conv(L, rows=0, c=1 << 13, k=1 << 13, tile=tile) == 0                        # 2^26 * 9: below 2^30


@pytest.mark.parametrize("bad", [72, 32, 8, 96, 0, -64])
def test_refuses_channel_counts_that_are_no_multiple_of_64(L, bad):
    for rows in (0, 2):
        assert _conv(L, rows=rows, c=bad) == BADARG and _conv(L, rows=rows, k=bad) == BADARG


def test_refuses_tiles_that_do_not_exist(L):
    for tile in (1, 32, 96, 192, 256, -64, -1):
        assert _conv(L, rows=0, k=256, tile=tile) == BADARG, tile
    for k in (64, 192):   # the wide tile needs K in multiples of 128
        assert _conv(L, rows=0, k=k, tile=128) == BADARG
        assert _conv(L, rows=0, k=k, tile=64) == 0 and _conv(L, rows=0, k=k, tile=0) == 0


@pytest.mark.parametrize("positions,k,tile", [(5776, 256, 64), (128 * 128, 256, 128), (128 * 128 - 128, 256, 64),
                                              (2048 * 361, 256, 128), (2048 * 361, 192, 64)])
def test_the_tile_rule(L, positions, k, tile):
    """128 iff K is a multiple of 128 and the wide tiles alone give each of the 256 CUs a workgroup"""
    assert L.elfnet_conv3x3_bf16_pick(positions, k, 256) == tile


def test_fusable_bf16_names_the_convolutions_the_entry_takes():
    """bf16 only, C and K multiples of 64, and a weight that lies in memory as [K,3,3,C]"""
    import torch
    from elf_amd.net import FusedInferenceNet

    def fusable(dtype, cin, k, channels_last=True):
        f = object.__new__(FusedInferenceNet)
        f.dtype = dtype
        c = torch.nn.Conv2d(cin, k, 3, padding=1).to(dtype)
        c = c.to(memory_format=torch.channels_last) if channels_last else c
        return f._fusable_bf16(torch.zeros((1, cin, 5, 5), dtype=dtype), c)

    assert FusedInferenceNet.bf16_conv in (True, False)
    assert fusable(torch.bfloat16, 64, 64) and fusable(torch.bfloat16, 192, 128)
    assert not fusable(torch.float16, 64, 64) and not fusable(torch.bfloat16, 64, 64, channels_last=False)
    assert not fusable(torch.bfloat16, 32, 64) and not fusable(torch.bfloat16, 64, 96) and not fusable(torch.bfloat16, 72, 64)
