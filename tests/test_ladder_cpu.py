"""CPU: the reference's ladder reader on the inputs of the ladder tests (ladder_expected over oracle/_ref's unshimmed board
library), the conditions those inputs must meet before the GPU tests mean anything, and the library surface of elfgo_ladder_map
without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ladder_expected as LE
import setup_expected as SE
from pyoracle import RefBoard

ELFGO_E_BADARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# counts of the committed inputs, from a run of LE.statistics on them
WANT_19 = dict(positions=12522, with_ladder=836, searches=2432, nonzero=882, backtracked=336, ko_with_ladder=4, max_calls=77,
               hist={3: 233, 5: 231, 7: 22, 9: 56, 11: 30, 13: 23, 15: 33, 17: 21, 19: 19, 21: 9, 23: 6, 25: 6, 27: 14, 29: 7, 31: 4,
                     33: 4, 35: 59, 37: 7, 39: 24, 41: 14, 43: 1, 45: 22, 47: 13, 49: 17, 51: 5, 55: 2})
WANT_9 = dict(positions=7055, with_ladder=153, searches=312, nonzero=157, backtracked=38, ko_with_ladder=0, max_calls=10,
              hist={3: 128, 5: 23, 7: 6})


def _need(n):
    assert RefBoard.available(n), "build() must have produced oracle/_ref/libelfboard%d.so" % n


def test_reference_statistics_19(built):
    """all plies of the 115 ladder-suite games: the expected maps are computed without a crash (the reference's error() is a
    deliberate segfault), the direct search returns checkLadder's depth wherever checkLadder's own test passes (asserted inside
    Ladder.expected), and the counts are those of the committed inputs"""
    _need(19)
    gs, exp = LE.all_expected(19)
    assert len(gs) == 115
    st = LE.statistics(exp)
    print("ladder statistics 19x19:", st)
    assert st == WANT_19


def test_reference_statistics_9(built):
    _need(9)
    gs, exp = LE.all_expected(9)
    assert len(gs) == 64
    st = LE.statistics(exp)
    print("ladder statistics 9x9:", st)
    assert st == WANT_9


def test_conditions_on_the_19_inputs(built):
    """conditions, not measurements: deep ladders, backtracking searches and a ladder next to a pending ko are all among the
    inputs; whether the MAX_LADDER_SEARCH cut is reached is said out loud"""
    _need(19)
    _, exp = LE.all_expected(19)
    st = LE.statistics(exp)
    assert max(st["hist"]) >= 31
    assert st["backtracked"] >= 100
    if st["ko_with_ladder"] == 0:
        print("no position with a simple ko pending has a non-zero ladder point: the ko refusal inside a search is unpinned")
    else:
        print("%d positions with a simple ko pending have a non-zero ladder point" % st["ko_with_ladder"])
    assert st["ko_with_ladder"] >= 1
    if st["max_calls"] < LE.MAX_LADDER_SEARCH:
        print("largest num_call is %d: no input reaches MAX_LADDER_SEARCH = %d, the cut is unpinned" % (st["max_calls"], LE.MAX_LADDER_SEARCH))
    # only odd depths: the capture falls on the capturer's turn
    assert all(d % 2 == 1 and d >= 3 for d in st["hist"])


def test_search_runs_is_checkladders_test(built):
    """ladder_expected.search_runs on hand-made GroupId4 rows, the second-group quirk included"""
    g = LE.GroupId4()
    g.liberty = 2
    g.ids[0], g.colors[0], g.group_liberties[0] = 5, 2, 3      # enemy (white) group with 3 liberties
    g.ids[2], g.colors[2], g.group_liberties[2] = 7, 1, 1      # own (black) group in atari
    assert LE.Ladder.search_runs(g, 1)
    g.group_liberties[0] = 2
    assert not LE.Ladder.search_runs(g, 1)
    g.group_liberties[0] = 3
    g.liberty = 1
    assert not LE.Ladder.search_runs(g, 1)
    g.liberty = 2
    g.ids[3], g.colors[3], g.group_liberties[3] = 9, 2, 4      # a second enemy group clears the flag
    assert not LE.Ladder.search_runs(g, 1)
    g.colors[3], g.group_liberties[3] = 1, 1                   # a second own group clears the other
    assert not LE.Ladder.search_runs(g, 1)
    assert C.sizeof(LE.GroupId4) == 26


@pytest.fixture(scope="module")
def L(built):
    from elf_amd import _lib
    return _lib.lib()


def test_ladder_entry_point_without_a_gpu(L):
    """declared, exported, mirrored; null / negative arguments are ELFGO_E_BADARG, never a crash; without an engine (which
    cannot exist without a GPU) it refuses like the other entry points"""
    from elf_amd import _lib
    assert "elfgo_ladder_map" in _lib.SIGNATURES and hasattr(L, "elfgo_ladder_map")
    res, args = _lib.SIGNATURES["elfgo_ladder_map"]
    assert res is C.c_int and len(args) == 6
    with open(os.path.join(ROOT, "include", "elf_amd.h")) as f:
        hdr = f.read()
    assert "int elfgo_ladder_map(ElfGoEngine* e, const int32_t* ids, int n, int16_t* depth, int16_t* calls, void* stream);" in hdr
    buf = np.zeros(361, np.int16)
    ids = np.zeros(1, np.int32)
    assert L.elfgo_ladder_map(None, None, 1, buf.ctypes.data, None, None) == ELFGO_E_BADARG
    assert L.elfgo_ladder_map(None, ids.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, None) == ELFGO_E_BADARG
    assert L.elfgo_ladder_map(None, None, -1, buf.ctypes.data, None, None) == ELFGO_E_BADARG
    assert L.elfgo_ladder_map(None, None, 0, None, None, None) == ELFGO_E_BADARG


def test_header_is_plain_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed"
    src = tmp_path / "h.c"
    src.write_text('#include "elf_amd.h"\nint (*p)(ElfGoEngine*, const int32_t*, int, int16_t*, int16_t*, void*) = elfgo_ladder_map;\n')
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "h.o")], check=True)


def test_gtp_lists_the_command():
    from elf_amd.gtp import GtpEngine
    assert hasattr(GtpEngine, "on_elf_ladders")
