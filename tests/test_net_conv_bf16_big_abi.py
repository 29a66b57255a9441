"""CPU: the big-tile bf16 trunk convolution's entry (elfnet_conv3x3_bf16_big, elf_amd/csrc/net_conv3x3_bf16_big.hip) is exported
and refuses bad arguments with ELFGO_E_BADARG before it touches the GPU runtime -- the pointers here are made-up addresses that are
never read --, and FusedInferenceNet carries the size it is routed in from."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
X, W, B, R, Y = (C.c_void_p(A * i) for i in range(1, 6))


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _conv(L, x=X, w=W, b=B, r=R, y=Y, rows=0, h=9, wd=9, c=64, k=256):
    return L.elfnet_conv3x3_bf16_big(x, w, b, r, y, rows, h, wd, c, k, 1, None)


def test_the_symbol_is_exported_and_declared(L):
    import elf_amd._lib as lib
    assert "elfnet_conv3x3_bf16_big" in lib.SIGNATURES
    assert L.elfnet_conv3x3_bf16_big.restype is C.c_int and len(L.elfnet_conv3x3_bf16_big.argtypes) == 12


@pytest.mark.parametrize("c,k", [(64, 256), (192, 512)])
def test_no_rows_is_accepted_behind_the_checks(L, c, k):
    assert _conv(L, c=c, k=k) == 0 and _conv(L, c=c, k=k, r=None) == 0


@pytest.mark.parametrize("bad", [dict(k=64), dict(k=128), dict(k=384), dict(c=32), dict(c=96), dict(x=None), dict(w=None),
                                 dict(b=None), dict(y=None), dict(x=C.c_void_p(A * 9 + 8)), dict(r=C.c_void_p(A * 9 + 8)),
                                 dict(y=X), dict(y=R), dict(rows=-1)], ids=str)
def test_refusals(L, bad):
    """K a multiple of 256 and C of 64; conv_args' checks of pointers, alignment, aliasing and rows -- with and without rows"""
    assert _conv(L, **bad) == BADARG
    if "rows" not in bad:
        assert _conv(L, rows=2, **bad) == BADARG


def test_the_routed_size_is_a_class_attribute():
    from elf_amd.net import FusedInferenceNet, NativeBf16InferenceNet
    v = FusedInferenceNet.bf16_big_min_positions
    assert isinstance(v, int) and not isinstance(v, bool) and v >= 0
    assert NativeBf16InferenceNet.bf16_big_min_positions == v
