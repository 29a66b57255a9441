"""CPU: elfnet_conv3x3_f16_bufstage (elf_amd/csrc/net_conv3x3.hip), the arithmetic algo 1's kernel addresses its staging loads by:
a raw buffer descriptor per operand, a 32-bit vector offset per lane (the row) and a wave-uniform scalar offset per K tile
(tap, 64 channels), both unsigned, the descriptor of x moved back by `bias` bytes so that a tap above or left of a position has a
scalar offset that is not negative, and a sentinel vector offset that the descriptor's range check turns into zeros.  The kernel
calls the same functions, so a wrong offset here is a wrong or out-of-tensor read there.

Boards 19 x 19, 9 x 9, 2 x 2, 1 x 5, 3 x 1, 5 x 37, 37 x 5 and 1 x 1281, C = 64 and 256, every position of the first and last board
of a few rows and every tap that is on the board there."""
import ctypes as C

import pytest

BADARG = -1
BOARDS = [(19, 19), (9, 9), (2, 2), (1, 5), (3, 1), (5, 37), (37, 5), (1, 1281)]
CHANNELS = [64, 256]
U32 = C.c_uint32


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _shape(L, rows, h, w, c, k=256):
    bias, xr, wr, sen = U32(7), U32(7), U32(7), U32(7)
    assert L.elfnet_conv3x3_f16_bufstage(rows, h, w, c, k, -1, 0, C.byref(bias), C.byref(xr), C.byref(wr), C.byref(sen), None, None) == 0
    return bias.value, xr.value, wr.value, sen.value


def _soff(L, rows, h, w, c, tap, kc, k=256):
    xs, ws = U32(7), U32(7)
    assert L.elfnet_conv3x3_f16_bufstage(rows, h, w, c, k, tap, kc, None, None, None, None, C.byref(xs), C.byref(ws)) == 0
    return xs.value, ws.value


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("h,w", BOARDS)
def test_every_tap_on_the_board_addresses_its_neighbour(L, h, w, c):
    rows = 3
    bias, xrec, wrec, sen = _shape(L, rows, h, w, c)
    xbytes = rows * h * w * c * 2
    assert bias == (w + 1) * c * 2 and xrec == xbytes + bias and wrec == 256 * 9 * c * 2
    assert sen % 16 == 0 and sen >= xrec and sen >= wrec
    soff = {(tap, kc): _soff(L, rows, h, w, c, tap, kc) for tap in range(9) for kc in range(c // 64)}
    for (tap, kc), (xs, ws) in soff.items():
        assert 0 <= xs < 1 << 30, "soffset >= 0 for all nine taps, and small"
        assert ws == tap * c * 2 + kc * 128 and ws + 128 <= 9 * c * 2
        assert sen + xs < 1 << 32 and sen + ws < 1 << 32, "the sentinel's sums do not wrap"
    checked = 0
    for n in (0, rows - 1):
        for hh in range(h):
            for ww in range(w):
                p = (n * h + hh) * w + ww
                for tap in range(9):
                    ky, kx = divmod(tap, 3)
                    if not (0 <= hh + ky - 1 < h and 0 <= ww + kx - 1 < w):
                        continue
                    q = ((n * h + hh + ky - 1) * w + ww + kx - 1)
                    for kc in range(c // 64):
                        xs = soff[(tap, kc)][0]
                        for chunk in (0, 7):
                            voff = p * c * 2 + chunk * 16
                            assert voff < xrec and voff + xs < xrec, "in range under either reading of the range check"
                            assert voff + xs < 1 << 32
                            at = voff + xs - bias
                            assert at == q * c * 2 + kc * 128 + chunk * 16
                            assert 0 <= at and at + 16 <= xbytes
                            checked += 1
    assert checked > 0


def test_the_largest_tensors_the_entry_accepts(L):
    """just below 2^30 elements: 11 618 rows of 19 x 19 x 256; a single row of a very wide board; the widest board at all"""
    for rows, h, w, c in [(11618, 19, 19, 256), (1, 1, (1 << 30) // 256 // 16 - 1, 256), (4194303, 1, 1, 256),
                          (1, 1, (1 << 22) - 2, 64), (1, 1, (1 << 20) - 2, 256)]:
        bias, xrec, wrec, sen = _shape(L, rows, h, w, c)
        xbytes = rows * h * w * c * 2
        assert xbytes < 1 << 31 and xrec == xbytes + bias, "no wrap in num_records"
        assert sen >= xrec and sen >= wrec and sen % 16 == 0
        assert sen == _shape(L, 1, 19, 19, 64)[3], "the sentinel does not depend on the tensor"
        top = max(_soff(L, rows, h, w, c, tap, kc)[0] for tap in range(9) for kc in range(c // 64))
        assert top < 1 << 30
        assert xbytes - 16 + top < 1 << 32 and sen + top < 1 << 32
    # the largest weight tensor
    bias, xrec, wrec, sen = _shape(L, 1, 1, 1, 64, k=1863936)
    assert wrec == 1863936 * 9 * 64 * 2 < 1 << 31 and sen >= wrec


def test_refusals(L):
    a = [None] * 6
    assert L.elfnet_conv3x3_f16_bufstage(2, 19, 19, 64, 256, -1, 0, *a) == 0
    for args in [(0, 19, 19, 64, 256, -1, 0), (2, 0, 19, 64, 256, -1, 0), (2, 19, 19, 96, 256, -1, 0), (2, 19, 19, 64, 128, -1, 0),
                 (2, 19, 19, 64, 256, 9, 0), (2, 19, 19, 64, 256, 0, 1), (2, 19, 19, 64, 256, 0, -1),
                 (11619, 19, 19, 256, 256, -1, 0),               # 2^30 elements or more
                 (1, 1, (1 << 22) - 1, 64, 256, -1, 0)]:          # (2 wd + 3) c 2 >= 2^30
        assert L.elfnet_conv3x3_f16_bufstage(*args, *a) == BADARG, args
