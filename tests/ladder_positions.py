"""The constructed inputs of the ladder tests: named positions, each (n, stones uint8 [n*n] in action order a = x*n + y, mover),
their 16 images (8 board symmetries x 2 colour assignments), and how to put them on the reference's bare Board.

* hand-built: drawn below as text, row = y, column = x, X = Black, O = White; Black is the victim (the side to move).
* searched: the layouts tools/ladder_search.py found, read from tests/golden/ladder_constructed.npz (stones and movers only).
* ko: legal alternating move lists (reference Coords) that end with a simple ko pending next to a ladder, and the same stones
  as a plain position with no ko.

Nothing here needs a GPU or runs a search for positions."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ladder_constructed.npz")
M_PASS = 0
BLACK, WHITE = 1, 2


# ---- drawing ----------------------------------------------------------------------------------------------------------------
def draw(n, rows, ox=0, oy=0, extra=()):
    """rows[y][x] in 'XO.' (blanks ignored) placed with its top-left corner at (ox, oy); extra = ((x, y, colour), ...)"""
    st = np.zeros((n, n), np.uint8)                    # [x, y]
    for y, row in enumerate(rows):
        for x, ch in enumerate(row.replace(" ", "")):
            if ch != ".":
                st[ox + x, oy + y] = BLACK if ch == "X" else WHITE
    for x, y, c in extra:
        assert st[x, y] == 0
        st[x, y] = c
    return st.reshape(-1)


def coord(n, x, y):
    return (y + 1) * (n + 2) + (x + 1)


# ---- images -----------------------------------------------------------------------------------------------------------------
def sym_xy(n, s, x, y):
    """where point (x, y) goes under board symmetry s in 0..7 (bit 2: transpose first; bits 0-1: quarter turns)"""
    if s & 4:
        x, y = y, x
    for _ in range(s & 3):
        x, y = n - 1 - y, x
    return x, y


def sym(n, stones, s):
    out = np.zeros((n, n), np.uint8)
    g = np.asarray(stones).reshape(n, n)
    for x, y in zip(*np.nonzero(g)):
        out[sym_xy(n, s, int(x), int(y))] = g[x, y]
    return out.reshape(-1)


def sym_perm(n, s):
    """p with image[p[a]] = original[a] for every per-point array in action order"""
    return np.array([sym_xy(n, s, x, y)[0] * n + sym_xy(n, s, x, y)[1] for x in range(n) for y in range(n)])


def swap(stones):
    return np.array([0, 2, 1], np.uint8)[np.asarray(stones)]


def images(n, stones, mover):
    """the 16 images -> list of (s, swapped, stones, mover), (0, False) first"""
    out = []
    for sw in (False, True):
        for s in range(8):
            st = sym(n, stones, s)
            out.append((s, sw, swap(st) if sw else st, 3 - mover if sw else mover))
    return out


def move_images(n, moves):
    """the 16 images of a move list that starts with a Black stone: symmetry s maps the points; the colour swap lets Black pass
    first, so that every stone is played by the other side (one pass, never two in a row)"""
    S = n + 2
    out = []
    for sw in (False, True):
        for s in range(8):
            mv = []
            for c in moves:
                c = int(c)
                if c != M_PASS:
                    c = coord(n, *sym_xy(n, s, c % S - 1, c // S - 1))
                mv.append(c)
            out.append((s, sw, ([M_PASS] if sw else []) + mv))
    return out


# ---- onto the reference's Board ---------------------------------------------------------------------------------------------
def build(RB, stones, mover):
    """a bare Board has no setup call: play the black stones with a pass after each, pass once more, play the white stones with a
    pass after each, and pass once more if Black is to move.  The colours are compared with the intended array, which catches a
    refused or captured stone.  -> Board handle, or None if the stones cannot stand like this"""
    n = RB.n
    st = np.asarray(stones, np.uint8)
    h = RB.new()
    ok = True
    for colour in (BLACK, WHITE):
        for a in np.nonzero(st == colour)[0]:
            ok = ok and RB.play(h, coord(n, int(a) // n, int(a) % n)) == 1
            ok = ok and RB.play(h, M_PASS) == 1
        if colour == BLACK:
            ok = ok and RB.play(h, M_PASS) == 1
    if ok and mover == BLACK:
        ok = RB.play(h, M_PASS) == 1
    if ok:
        info = RB.info(h)
        ok = np.array_equal(RB.board(h)[0], st) and int(info[1]) == mover
    if not ok:
        RB.free(h)
        return None
    return h


def play_list(RB, moves):
    h = RB.new()
    for c in moves:
        assert RB.play(h, int(c)) == 1, "a move of a constructed list was refused"
    return h


# ---- hand-built positions ---------------------------------------------------------------------------------------------------
# the plain ladder: X at (1,2) in atari, candidate (2,2); every capturer's node has a must-block point, the line runs down the
# diagonal (k,k), (k,k+1) to the far side
_DIAG = [". . . .",
         ". O O .",
         "O X . .",
         ". O . ."]
# second line: X at (1,1) in atari, candidate (2,1).  White's wall on the third line leaves every escape point two empty
# neighbours, so every capturer's node is a fork between the first-line point and the second-line point ahead; White creeps
# along the first line (its chain keeps the liberty behind it) and the victim runs into the far border
_SECOND = ". O . . . . . . . . . . . . . . . . ."
_SECOND_ROWS = lambda n: [_SECOND.replace(" ", "")[:n], "OX" + "." * (n - 2), "O" * n]   # noqa: E731
# first line: candidate (3,1); the must-block is ahead on the second line and the victim's flight drops to the first line
_FIRST = [". . O . . .",
          ". O X . . .",
          ". . O O . ."]
# the atari stone is itself in atari: White's block at (3,2) would have the single liberty (3,3)
_SELF_ATARI = [". . . . . .",
               ". O O X . .",
               "O X . . X .",
               ". O . . . ."]
# the first flight (2,3) captures the white stone (2,4); the next capturer's node is a fork whose first line lets the victim
# connect out and whose second move is suicide (refused): both backtracks replay a line with a capture in it
_CAPTURE = [". . . . .",
            ". O O . .",
            "O X . . .",
            "O O . . .",
            ". X O X .",
            ". . X . ."]


def hand_built(n):
    """-> dict name -> (n, stones, mover) on an n x n board (n = 19 or 9)"""
    far = (6, 10, 14) if n == 19 else (4, 5, 6)
    mid = far[1]
    P = {"diagonal": draw(n, _DIAG)}
    for k, d in enumerate(far):
        P["diagonal_breaker%d" % k] = draw(n, _DIAG, extra=((d, d, BLACK),))
    P["diagonal_capturer_stone"] = draw(n, _DIAG, extra=((mid, mid, WHITE),))
    P["second_line"] = draw(n, _SECOND_ROWS(n))
    P["first_line"] = draw(n, _FIRST, ox=2)
    P["self_atari"] = draw(n, _SELF_ATARI)
    P["capture_in_flight"] = draw(n, _CAPTURE)
    return {k: (n, v, BLACK) for k, v in P.items()}


# ---- ko ---------------------------------------------------------------------------------------------------------------------
# White's last move, (2,1) of this drawing, takes the black stone that stood on k: a simple ko is pending at k for Black
_KO = [". O X .",
       "O k O X",
       ". O X ."]


def ko_list(n):
    """-> (move list, ko point as action, stones of the final position): the plain ladder in the top-left corner, a ko shape in
    the bottom-right one (on the ladder's path), played by Black and White in turn.  Black has fewer stones and passes in
    between, never after a pass of White's; White's last move takes the ko, so Black, the ladder's victim, is to move with the
    ko pending against him."""
    ox, oy = n - 4, n - 3
    final = draw(n, _DIAG) + draw(n, [r.replace("k", ".") for r in _KO], ox, oy)
    before = final.reshape(n, n).copy()
    before[ox + 1, oy + 1], before[ox + 2, oy + 1] = BLACK, 0                  # the ko stone stands, the taking stone does not
    b = [coord(n, int(x), int(y)) for x, y in zip(*np.nonzero(before == BLACK))]
    w = [coord(n, int(x), int(y)) for x, y in zip(*np.nonzero(before == WHITE))] + [coord(n, ox + 2, oy + 1)]
    assert len(b) < len(w)
    moves = []
    for i, c in enumerate(w):
        moves += [b[i] if i < len(b) else M_PASS, c]
    return moves, (ox + 1) * n + oy + 1, final


def ko_cases(n):
    """-> (move list with the ko pending, the same stones as a position without a ko, ko point as action)"""
    moves, k, final = ko_list(n)
    return moves, (n, final, BLACK), k


# ---- searched positions -----------------------------------------------------------------------------------------------------
def searched(n):
    """-> dict name -> (n, stones, mover) from the committed fixture"""
    with np.load(FIXTURE) as f:
        names, st, mv = f["names%d" % n], f["stones%d" % n], f["mover%d" % n]
        return {str(k): (n, st[i].copy(), int(mv[i])) for i, k in enumerate(names)}


def all_positions(n):
    P = hand_built(n)
    P["ko_plain"] = ko_cases(n)[1]
    P.update(searched(n))
    return P


def rows(n):
    """every image of every position, the ko lists last -> list of dict(name, s, swapped, stones, mover, moves); moves is None
    where the row is a plain position (reference: build(); device: GoEngine.setup) and a move list where it has to be played"""
    out = []
    for name, (_, st, mover) in all_positions(n).items():
        for s, sw, ist, imv in images(n, st, mover):
            out.append(dict(name=name, s=s, swapped=sw, stones=ist, mover=imv, moves=None))
    moves, (_, st, mover), _ = ko_cases(n)
    for (s, sw, mv), (_, _, ist, imv) in zip(move_images(n, moves), images(n, st, mover)):
        out.append(dict(name="ko_pending", s=s, swapped=sw, stones=ist, mover=imv, moves=mv))
    return out


_expected = {}


def expected(n):
    """rows(n) with the reference's answers added (depth, calls int16 [n*n] from ladder_expected.Ladder.expected, info), computed
    once per process -> (Ladder, rows)"""
    if n not in _expected:
        import ladder_expected as LE
        lad = LE.Ladder(n)
        out = rows(n)
        for r in out:
            h = handle(lad.RB, r)
            assert h is not None, "the stones of %s cannot stand" % r["name"]
            assert np.array_equal(lad.RB.board(h)[0], r["stones"]) and int(lad.RB.info(h)[1]) == r["mover"], r["name"]
            r["depth"], r["calls"] = lad.expected(h)
            r["info"] = lad.RB.info(h)
            lad.RB.free(h)
        _expected[n] = (lad, out)
    return _expected[n]


def handle(RB, r):
    """a fresh Board handle of row r (the caller frees it)"""
    return play_list(RB, r["moves"]) if r["moves"] is not None else build(RB, r["stones"], r["mover"])
