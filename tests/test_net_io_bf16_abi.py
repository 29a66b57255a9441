"""CPU: elfnet_conv3x3_in_bf16 and elfnet_heads_bf16 (elf_amd/csrc/net_io.hip) are exported with the documented signatures and
refuse bad arguments with ELFGO_E_BADARG before they touch the GPU runtime -- the pointers here are made-up addresses that are never
read --, and rows == 0 returns 0 without a GPU."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
X, W, B, Y, WS, PI, V, LG = (C.c_void_p(A * i) for i in range(1, 9))
ODD = C.c_void_p(A * 9 + 8)   # 8-B aligned only


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _conv(L, x=X, f16=1, w=W, b=B, y=Y, rows=0, n=9, c=18, k=64):
    return L.elfnet_conv3x3_in_bf16(x, f16, w, b, y, rows, n, n, c, k, 1, None)


def _heads(L, ch=64, vh=256, null=None, act=X, rows=0, n=9, pi=PI, stride=None, value=V, ws=WS, ws_bytes=None):
    from elf_amd._lib import ElfNetHeads
    names = [f[0] for f in ElfNetHeads._fields_[:10]]
    hd = ElfNetHeads(*[None if nm == null else A * (16 + i) for i, nm in enumerate(names)], ch, vh)
    ws_bytes = L.elfnet_heads_workspace(rows, n, n) if ws_bytes is None else ws_bytes
    return L.elfnet_heads_bf16(act, C.byref(hd), rows, n, n, pi, n * n + 1 if stride is None else stride, value, LG, ws, ws_bytes, None)


def test_the_symbols_are_exported_and_declared(L):
    import elf_amd._lib as lib
    for name, nargs, second in (("elfnet_conv3x3_in_bf16", 12, C.c_int), ("elfnet_heads_bf16", 12, C.c_void_p)):
        assert name in lib.SIGNATURES
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs and fn.argtypes[1] is second


def test_no_rows_is_accepted_without_a_gpu(L):
    """behind every check and in front of the first call into the GPU runtime"""
    for f16 in (0, 1):
        assert _conv(L, f16=f16) == 0 and _conv(L, f16=f16, c=2, k=32) == 0 and _conv(L, f16=f16, c=32, k=288, n=19) == 0
        assert _conv(L, f16=f16, x=C.c_void_p(A + 4)) == 0     # x of either type is read in channel pairs: 4-B aligned is enough
    assert _heads(L) == 0 and _heads(L, ch=8, n=19) == 0


@pytest.mark.parametrize("rows", [0, 2])
@pytest.mark.parametrize("bad", [dict(x=None), dict(w=None), dict(b=None), dict(y=None),      # null pointers
                                 dict(c=17), dict(c=34), dict(k=48), dict(f16=2), dict(f16=-1),
                                 dict(y=X),                                                    # y == x
                                 dict(w=ODD), dict(b=ODD), dict(y=ODD), dict(x=C.c_void_p(A + 2))])
def test_input_conv_refuses(L, bad, rows):
    assert _conv(L, rows=rows, **bad) == BADARG


@pytest.mark.parametrize("rows", [0, 2])
@pytest.mark.parametrize("bad", [dict(act=None), dict(pi=None), dict(value=None), dict(ws=None),
                                 dict(null="pconv_w"), dict(null="pi_b"), dict(null="v2_w"),
                                 dict(stride=81),                                               # pi_stride < d + 1
                                 dict(ch=60), dict(ch=0), dict(vh=0),                           # channels % 8 != 0
                                 dict(act=ODD), dict(pi=C.c_void_p(A * 6 + 2)), dict(n=64)])    # alignment; a row beyond the LDS
def test_heads_refuse(L, bad, rows):
    assert _heads(L, rows=rows, **bad) == BADARG


def test_heads_refuse_a_short_workspace(L):
    need = 2 * 3 * 81 * 4   # rows x (2 + 1) head values x d positions, fp32
    assert _heads(L, rows=2, ws_bytes=need - 1) == BADARG and _heads(L, rows=2, ws_bytes=0) == BADARG
