"""CPU: elfnet_conv3x3_in_f16 and elfnet_heads_f16 (elf_amd/csrc/net_io.hip) refuse bad arguments with ELFGO_E_BADARG before
they touch the GPU runtime -- the pointers here are made-up addresses that are never read -- and elfnet_heads_workspace is host
arithmetic."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
X, W, B, Y, WS, PI, V, LG = (C.c_void_p(A * i) for i in range(1, 9))


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _conv(L, x=X, w=W, b=B, y=Y, rows=2, n=9, c=18, k=64):
    return L.elfnet_conv3x3_in_f16(x, w, b, y, rows, n, n, c, k, 1, None)


def _heads(ch=64, vh=256, null=None):
    from elf_amd._lib import ElfNetHeads
    names = [f[0] for f in ElfNetHeads._fields_[:10]]
    vals = [None if n == null else A * (16 + i) for i, n in enumerate(names)]
    return ElfNetHeads(*vals, ch, vh)


def _run_heads(L, hd, act=X, rows=2, n=9, pi=PI, stride=None, value=V, logits=LG, ws=WS, ws_bytes=None):
    d = n * n
    if ws_bytes is None:
        ws_bytes = L.elfnet_heads_workspace(rows, n, n)
    return L.elfnet_heads_f16(act, C.byref(hd) if hd is not None else None, rows, n, n, pi, d + 1 if stride is None else stride, value,
                              logits, ws, ws_bytes, None)


@pytest.mark.parametrize("null", ["x", "w", "b", "y"])
def test_input_conv_refuses_null_pointers(L, null):
    assert _conv(L, **{null: None}) == BADARG


@pytest.mark.parametrize("c,k", [(17, 64), (34, 64), (0, 64), (18, 48), (18, 0)])
def test_input_conv_refuses_other_channel_counts(L, c, k):
    assert _conv(L, c=c, k=k) == BADARG


def test_input_conv_refuses_aliasing_size_and_alignment(L):
    assert _conv(L, y=X) == BADARG
    assert _conv(L, rows=1 << 22, n=19, k=256) == BADARG                  # y of 2^22 * 361 * 256 * 2 B
    for name in ("w", "b", "y"):
        assert _conv(L, **{name: C.c_void_p(A * 9 + 8)}) == BADARG, name   # 8-B aligned only
    assert _conv(L, x=C.c_void_p(A + 2)) == BADARG                         # a position is 36 B: x needs its 4-B alignment, no more
    assert _conv(L, rows=-1) == BADARG and _conv(L, n=0) == BADARG


@pytest.mark.parametrize("null", ["act", "pi", "value", "ws"])
def test_heads_refuse_null_pointers(L, null):
    assert _run_heads(L, _heads(), **{null: None}) == BADARG


def test_heads_refuse_a_null_struct_and_null_weights(L):
    from elf_amd._lib import ElfNetHeads
    assert _run_heads(L, None) == BADARG
    for f in ElfNetHeads._fields_[:10]:
        assert _run_heads(L, _heads(null=f[0])) == BADARG, f[0]


def test_heads_refuse_channels_workspace_and_stride(L):
    assert _run_heads(L, _heads(ch=60)) == BADARG                     # C % 8 != 0
    assert _run_heads(L, _heads(ch=0)) == BADARG
    assert _run_heads(L, _heads(vh=0)) == BADARG
    need = 2 * 3 * 81 * 4                                             # rows x (2 + 1) head values x d positions, fp32
    assert L.elfnet_heads_workspace(2, 9, 9) >= need
    assert _run_heads(L, _heads(), ws_bytes=need - 1) == BADARG       # a short workspace
    assert _run_heads(L, _heads(), ws_bytes=0) == BADARG
    assert _run_heads(L, _heads(), stride=81) == BADARG               # pi_stride = d
    assert _run_heads(L, _heads(), rows=-1) == BADARG


def test_heads_workspace_is_positive_and_monotone_in_rows(L):
    for n in (9, 19):
        prev = 0
        for rows in (1, 2, 3, 16, 17, 2048, 16384):
            b = L.elfnet_heads_workspace(rows, n, n)
            assert b >= rows * 3 * n * n * 4 and b > prev, (n, rows, b)
            prev = b
    assert L.elfnet_heads_workspace(0, 19, 19) > 0
    assert L.elfnet_heads_workspace(-1, 19, 19) == 0 and L.elfnet_heads_workspace(4, 0, 19) == 0


def test_heads_refuse_a_row_beyond_the_lds(L):
    """k_head_fc holds 4 d + 1 + value_hidden floats of a row in LDS and a workgroup has 64 KiB: a 64 x 64 board with 256 value
    neurons is 66 564 B and refused, 63 x 63 (64 532 B) is not -- with rows = 0, which is accepted after every check and before
    the first call into the GPU runtime"""
    assert (4 * 64 * 64 + 1 + 256) * 4 > 65536 >= (4 * 63 * 63 + 1 + 256) * 4
    assert _run_heads(L, _heads(), n=64) == BADARG
    assert _run_heads(L, _heads(), rows=0, n=64) == BADARG
    assert _run_heads(L, _heads(), rows=0, n=63) == 0
    # value_hidden counts too: 9 x 9 takes 16 059 value neurons and not one more
    assert (4 * 81 + 1 + 16059) * 4 == 65536
    assert _run_heads(L, _heads(vh=16059), rows=0) == 0
    assert _run_heads(L, _heads(vh=16060), rows=0) == BADARG


def test_heads_refuse_sizes_beyond_their_index_range(L):
    """rows * d at or above 2^31 (positions are indexed with an int), d or value_hidden above 2^20; the workspace size is passed
    as a number that would be large enough"""
    rows = 1 << 26
    assert rows * 81 >= 1 << 31
    assert _run_heads(L, _heads(), rows=rows, ws_bytes=rows * 3 * 81 * 4) == BADARG
    rows = (1 << 31) // 81 + 1                                             # the first refused row count at 9 x 9
    assert (rows - 1) * 81 < 1 << 31 <= rows * 81
    assert _run_heads(L, _heads(), rows=rows, ws_bytes=rows * 3 * 81 * 4) == BADARG
    assert _run_heads(L, _heads(), rows=0, n=1025, stride=1025 * 1025 + 1, ws_bytes=1 << 40) == BADARG     # d = 1 050 625 > 2^20
    assert _run_heads(L, _heads(vh=(1 << 20) + 1), rows=0) == BADARG
