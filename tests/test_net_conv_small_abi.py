"""CPU: elfnet_conv3x3_small_f16 (elf_amd/csrc/net_conv3x3_small.hip) is exported and refuses bad arguments with ELFGO_E_BADARG
before it touches the GPU runtime -- the pointers here are made-up addresses that are never read -- and elfnet_conv3x3_f16 still
has two algos: the small kernel is an entry of its own, not algo 2."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
X, W, B, R, Y = (C.c_void_p(A * i) for i in range(1, 6))


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _conv(L, x=X, w=W, b=B, r=R, y=Y, rows=2, h=9, wd=9, c=64, k=64):
    return L.elfnet_conv3x3_small_f16(x, w, b, r, y, rows, h, wd, c, k, 1, None)


def test_the_symbol_is_exported_and_declared(L):
    import elf_amd._lib as lib
    assert "elfnet_conv3x3_small_f16" in lib.SIGNATURES
    f = L.elfnet_conv3x3_small_f16
    assert f.restype is C.c_int and len(f.argtypes) == 12


def test_accepts_no_rows_before_the_runtime(L):
    """rows = 0 is accepted after every argument check and before the first call into the GPU runtime"""
    assert _conv(L, rows=0) == 0
    assert _conv(L, rows=0, r=None) == 0
    assert _conv(L, rows=0, c=256, k=192, h=19, wd=7) == 0


def test_refuses_null_and_misaligned_pointers(L):
    for null in ("x", "w", "b", "y"):
        assert _conv(L, **{null: None}) == BADARG, null
        assert _conv(L, rows=0, **{null: None}) == BADARG, null
    for name in ("x", "w", "b", "r", "y"):
        assert _conv(L, **{name: C.c_void_p(A * 9 + 8)}) == BADARG, name   # 8-B aligned only
    assert _conv(L, y=X) == BADARG and _conv(L, y=R) == BADARG              # y == x, y == res


@pytest.mark.parametrize("bad", [72, 32, 8, 96, 0, -64])
def test_refuses_channel_counts_that_are_no_multiple_of_64(L, bad):
    for rows in (0, 2):
        assert _conv(L, rows=rows, c=bad) == BADARG
        assert _conv(L, rows=rows, k=bad) == BADARG


def test_refuses_bad_sizes(L):
    assert _conv(L, rows=-1) == BADARG and _conv(L, h=0) == BADARG and _conv(L, wd=0) == BADARG and _conv(L, h=-1) == BADARG
    assert _conv(L, rows=1 << 22, h=19, wd=19, c=256, k=256) == BADARG        # y of 2^22 * 361 * 256 * 2 B
    assert _conv(L, rows=1 << 22, h=19, wd=19, c=256, k=64) == BADARG         # x of that size
    assert _conv(L, rows=0, c=1 << 14, k=1 << 13) == BADARG                   # w of 2^27 * 9 elements
    assert _conv(L, rows=0, c=1 << 13, k=1 << 13) == 0                        # 2^26 * 9: below 2^30


def test_elfnet_conv3x3_f16_still_has_two_algos(L):
    for rows in (0, 2):
        assert L.elfnet_conv3x3_f16(X, W, B, R, Y, rows, 9, 9, 64, 256, 1, 2, None) == BADARG
        assert L.elfnet_conv3x3_f16_width(X, W, B, R, Y, rows, 9, 9, 64, 256, 1, 2, 0, None) == BADARG
    assert L.elfnet_conv3x3_f16(X, W, B, R, Y, 0, 9, 9, 64, 256, 1, 1, None) == 0
