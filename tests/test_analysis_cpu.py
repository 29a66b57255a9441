"""CPU: search analysis without a GPU -- the argument checks of elfmcts_analyze / elfsp_* through ctypes (nothing is launched for
a refused call) and the Leela-Zero-style text of elf_amd.gtp.format_analysis on hand-written arrays."""
import ctypes

import numpy as np

BADARG = -1


def test_analyze_refuses_bad_arguments_without_a_gpu(built):
    import elf_amd
    L = elf_amd.lib()
    info = (ctypes.c_int32 * 8)()
    nul = [None] * 7
    # a NULL handle, whatever the rest says
    assert L.elfmcts_analyze(None, 10, 16, info, *nul, None) == BADARG
    assert L.elfmcts_analyze(None, 10, 16, None, *nul, None) == BADARG
    # out-of-range max_moves / max_pv
    for mm, mp in ((0, 16), (-1, 16), (65, 16), (10, 0), (10, -3), (10, 33), (0, 0), (1 << 30, 1 << 30)):
        assert L.elfmcts_analyze(None, mm, mp, info, *nul, None) == BADARG, (mm, mp)
    assert L.elfsp_analyze(None, 0, 10, 16, info, *nul, None) == BADARG
    assert L.elfsp_set_analysis(None, 10, 16) == BADARG
    assert L.elfsp_last_analysis(None, info, *nul) == BADARG
    assert list(info) == [0] * 8


def test_header_limits_match_the_documented_ranges():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "elf_amd.h")).read()
    d = dict(re.findall(r"#define (ELFMCTS_ANALYZE_[A-Z_]+) (\d+)", src))
    assert d == {"ELFMCTS_ANALYZE_WORDS": "8", "ELFMCTS_ANALYZE_MAX_MOVES": "64", "ELFMCTS_ANALYZE_MAX_PV": "32"}


def _coord(n, v):
    from elf_amd.gtp import move2xy
    x, y = move2xy(v)
    return 0 if x < 0 else (y + 1) * (n + 2) + (x + 1)


def _arrays(n, rows, max_moves, max_pv):
    """rows = [(vertex, visits, winrate, prior, [pv vertices])] -> one game's arrays, padded as the kernel pads"""
    coord = np.full(max_moves, -1, np.int32); visits = np.zeros(max_moves, np.int32)
    winrate = np.zeros(max_moves, np.float64); prior = np.zeros(max_moves, np.float32)
    pv_len = np.zeros(max_moves, np.int32); pv = np.full((max_moves, max_pv), -1, np.int32)
    for k, (v, vis, wr, pr, line) in enumerate(rows):
        coord[k], visits[k], winrate[k], prior[k], pv_len[k] = _coord(n, v), vis, wr, pr, len(line)
        pv[k, :len(line)] = [_coord(n, x) for x in line]
    return coord, visits, winrate, prior, pv_len, pv


def test_format_vertices_order_and_rounding():
    from elf_amd.gtp import format_analysis
    n = 19
    rows = [("J9", 120, 0.53126, 0.25004, ["J9", "H8", "pass", "T19"]),     # the letter after H is J; the last column is T
            ("pass", 7, 0.49994, 0.00012, ["pass"]),
            ("A1", 1, 1.0, 0.99996, ["A1", "K10"])]
    text = format_analysis(n, *_arrays(n, rows, 5, 8))
    assert text == ("info move J9 visits 120 winrate 5313 prior 2500 order 0 pv J9 H8 pass T19 "
                    "info move pass visits 7 winrate 4999 prior 1 order 1 pv pass "
                    "info move A1 visits 1 winrate 10000 prior 10000 order 2 pv A1 K10")
    assert "I" not in text.replace("info", "")
    # column index 8 is J on every board size; 9x9's last column is J
    assert format_analysis(9, *_arrays(9, [("J9", 3, 0.5, 0.5, ["J9", "H1"])], 2, 4)) == \
        "info move J9 visits 3 winrate 5000 prior 5000 order 0 pv J9 H1"
    # max_moves candidates, no padding row at the end
    full = format_analysis(9, *_arrays(9, [("A1", 2, 0.25, 0.5, ["A1"]), ("B2", 1, 0.75, 0.25, ["B2"])], 2, 1))
    assert full == "info move A1 visits 2 winrate 2500 prior 5000 order 0 pv A1 info move B2 visits 1 winrate 7500 prior 2500 order 1 pv B2"


def test_format_empty_analysis_is_the_empty_string():
    from elf_amd.gtp import format_analysis
    assert format_analysis(19, *_arrays(19, [], 10, 16)) == ""
    assert format_analysis(9, *_arrays(9, [], 1, 1)) == ""
    z = np.zeros(0, np.int32)
    assert format_analysis(9, z, z, np.zeros(0), np.zeros(0, np.float32), z, np.zeros((0, 0), np.int32)) == ""


def test_winrate_is_for_the_side_to_move():
    """reward is black-positive: the same edge statistics under a Black root and under a White root give complementary win rates"""
    from elf_amd.selfplay import with_winrate
    from elf_amd.gtp import format_analysis
    n, mm, mp = 9, 4, 3

    def analysis(flip):
        info = np.zeros((1, 8), np.int32)
        info[0, :4] = (2, 2, 40, flip)
        a = dict(info=info, coord=np.full((1, mm), -1, np.int32), orig=np.full((1, mm), -1, np.int32),
                 visits=np.zeros((1, mm), np.int32), reward=np.zeros((1, mm), np.float32), prior=np.zeros((1, mm), np.float32),
                 pv_len=np.zeros((1, mm), np.int32), pv=np.full((1, mm, mp), -1, np.int32))
        a["coord"][0, :2] = (_coord(n, "C3"), _coord(n, "pass")); a["visits"][0, :2] = (30, 10)
        a["reward"][0, :2] = (7.5, -10.0); a["prior"][0, :2] = (0.5, 0.125)
        a["pv_len"][0, :2] = (2, 1); a["pv"][0, 0, :2] = (_coord(n, "C3"), _coord(n, "D4")); a["pv"][0, 1, 0] = 0
        return with_winrate(a)
    b, w = analysis(0), analysis(1)
    assert b["winrate"].shape == (1, mm)
    assert b["winrate"][0].tolist() == [0.625, 0.0, 0.0, 0.0] and w["winrate"][0].tolist() == [0.375, 1.0, 0.0, 0.0]
    assert np.array_equal((b["winrate"] + w["winrate"])[0, :2], [1.0, 1.0])          # complementary where there is a candidate

    def text(a):
        return format_analysis(n, a["coord"][0], a["visits"][0], a["winrate"][0], a["prior"][0], a["pv_len"][0], a["pv"][0])
    assert text(b) == "info move C3 visits 30 winrate 6250 prior 5000 order 0 pv C3 D4 info move pass visits 10 winrate 0 prior 1250 order 1 pv pass"
    assert text(w) == "info move C3 visits 30 winrate 3750 prior 5000 order 0 pv C3 D4 info move pass visits 10 winrate 10000 prior 1250 order 1 pv pass"


def test_signature_table_has_the_analysis_entries():
    from elf_amd import _lib
    for name in ("elfmcts_analyze", "elfsp_analyze", "elfsp_set_analysis", "elfsp_last_analysis"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["elfmcts_analyze"][1]) == 12 and len(_lib.SIGNATURES["elfsp_analyze"][1]) == 13
