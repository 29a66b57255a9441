"""CPU: the pieces of position setup that need no GPU -- the restatement the GPU tests lean on (setup_expected.restate) pinned on
the reference's own board engine, the SGF setup-stone reader, the argument checks of the new entry points and the handicap
table of the GTP front-end."""
import ctypes as C

import numpy as np
import pytest

import setup_expected as SE
from pyoracle import Port, RefBoard

ELFGO_E_BADARG = -1

# sgf/sgf_test.cc:93-95 (testJapaneseHandicap)
JAPANESE_HANDICAP = ("(;GM[1]FF[4]CA[UTF-8]AP[CGoban:3]ST[2]RU[Japanese]SZ[9]HA[2]RE[Void]KM[5.50]PW[test_white]PB[test_black]"
                     "AB[gc][cg];W[ee];B[dg])")

# the reference's HandicapTable (base/go_state.cc:36-45) as GTP vertices: letter = column with I skipped, number = line
HANDICAP = {2: "D4 Q16", 3: "D4 Q16 Q4", 4: "D4 Q16 D16 Q4", 5: "D4 Q16 D16 Q4 K10", 6: "D4 Q16 D16 Q4 D10 Q10",
            7: "D4 Q16 D16 Q4 D10 Q10 K10", 8: "D4 Q16 D16 Q4 D10 Q10 K16 K4", 9: "D4 Q16 D16 Q4 D10 Q10 K16 K4 K10"}
DERIVED_FROM = {3: 2, 4: 2, 5: 4, 6: 4, 7: 6, 8: 6, 9: 8}


def _need(n):
    assert RefBoard.available(n), "build() must have produced oracle/_ref/libelfboard%d.so" % n


def _pin(n, games):
    cs, cnt = SE.cases(RefBoard(n), games)
    bad = 0
    for gi, u, rep in cs:
        libs, h, zero = SE.restate(rep["colour"][u], n)
        bad += not (np.array_equal(libs, rep["libs"][u]) and h == int(rep["hash"][u]) and not zero)
    print("restate vs RefBoard %dx%d: %s, mismatches %d" % (n, n, cnt, bad))
    return cnt, bad


def test_restate_equals_the_reference_19(built):
    """all 115 ladder-suite games, every 10th ply moved to the next one with no simple ko pending: liberties per point and hash
    of restate(colour) are the reference's.  12 522 positions, 144 with a ko pending, 1 177 chosen, 9 of them moved."""
    _need(19)
    cnt, bad = _pin(19, SE.ladder_games())
    assert cnt["chosen"] == 1177 and cnt["positions"] == 12522 and cnt["ko"] == 144 and cnt["moved"] == 9
    assert bad == 0


def test_restate_equals_the_reference_9(built):
    _need(9)
    cnt, bad = _pin(9, SE.nine_games(Port(9)))
    assert cnt["chosen"] > 300 and bad == 0


def test_restate_sees_a_group_without_liberty():
    col = np.zeros(81, np.uint8)
    col[0] = 2                      # white corner stone (0,0) ...
    col[1] = col[9] = 1             # ... with black on (0,1) and (1,0)
    libs, h, zero = SE.restate(col, 9)
    assert zero and libs[0] == 0 and libs[1] == 2 and libs[9] == 2
    z = SE.zobrist()
    assert h == SE.swap_halves(z[1 * 11 + 1]) ^ int(z[2 * 11 + 1]) ^ int(z[1 * 11 + 2])


@pytest.fixture(scope="module")
def L(built):
    from elf_amd import _lib
    return _lib.lib()


def test_sgf_setup(L):
    from elf_amd.train import parse_sgf, sgf_setup
    n = 9
    st, k = sgf_setup(n, JAPANESE_HANDICAP)
    want = np.zeros(n * n, np.uint8)
    want[6 * n + 2] = want[2 * n + 6] = 1           # gc = (6, 2), cg = (2, 6)
    assert k == 2 and np.array_equal(st, want)
    pl, mv, hdr = parse_sgf(n, JAPANESE_HANDICAP)   # the move reader is unchanged: W[ee], B[dg]
    assert list(pl) == [2, 1] and list(mv) == [5 * 11 + 5, 7 * 11 + 4] and hdr["handi"] == 2
    # an AW list next to AB; blanks inside a value
    st, k = sgf_setup(n, "(;SZ[9]AB[aa][bb]AW[cc][ dd][ee];B[ff])")
    assert k == 5 and list(np.nonzero(st == 1)[0]) == [0, 1 * n + 1] and list(np.nonzero(st == 2)[0]) == [2 * n + 2, 3 * n + 3, 4 * n + 4]
    # an escaped ']' does not end a value: the comment swallows "AB[aa" up to the visible ']'
    st, k = sgf_setup(n, "(;SZ[9]C[x\\]AB[aa]AB[bb];B[ff])")
    assert k == 1 and st[1 * n + 1] == 1 and st[0] == 0
    # off-board points are ignored; setup properties of later nodes are not the header's
    st, k = sgf_setup(n, "(;SZ[9]AB[aa][tt][zz];B[ff]AB[cc])")
    assert k == 1 and st[0] == 1
    # a compressed point list (an FF[4] rectangle) is not a point: ignored, not read as its first corner
    st, k = sgf_setup(n, "(;SZ[9]AB[aa:cc][dd]AW[e];B[ff])")
    assert k == 1 and st[3 * n + 3] == 1
    st, k = sgf_setup(n, "(;SZ[9]KM[7.5];B[ff];W[dd])")
    assert k == 0 and not st.any()
    st, k = sgf_setup(n, "no node here")
    assert k == 0
    # the header comes back as elfrec_sgf_parse gives it
    from elf_amd.train import SgfHeader
    h = SgfHeader()
    buf = np.zeros(n * n, np.uint8)
    assert L.elfrec_sgf_setup(n, JAPANESE_HANDICAP.encode(), buf.ctypes.data, C.byref(h)) == 2
    assert (h.size, h.handi) == (9, 2) and h.komi == 5.5
    assert L.elfrec_sgf_setup(n, None, buf.ctypes.data, None) == ELFGO_E_BADARG
    assert L.elfrec_sgf_setup(n, b"(;AB[aa])", None, None) == ELFGO_E_BADARG


def test_argument_errors_without_a_gpu(L):
    buf = np.zeros(361, np.uint8)
    ids = np.zeros(1, np.int32)
    assert L.elfgo_setup(None, None, buf.ctypes.data, None, 1, None, None) == ELFGO_E_BADARG
    assert L.elfsp_setup(None, ids.ctypes.data, 1, buf.ctypes.data, None, None) == ELFGO_E_BADARG
    assert L.elfsp_undo(None, ids.ctypes.data, 1, 1, None) == ELFGO_E_BADARG


def test_handicap_table():
    from elf_amd.gtp import HANDICAP_VERTICES, move2xy
    assert sorted(HANDICAP_VERTICES) == list(range(2, 10))
    for k, text in HANDICAP.items():
        vs = text.split()
        assert list(HANDICAP_VERTICES[k]) == vs
        assert len(vs) == k and len(set(vs)) == k
        for v in vs:
            x, y = move2xy(v)
            assert x + 1 in (4, 10, 16) and y + 1 in (4, 10, 16), v
        if k in DERIVED_FROM:
            assert set(HANDICAP[DERIVED_FROM[k]].split()) <= set(vs)
