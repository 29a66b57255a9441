"""What elfgo_life_map must return, taken from the reference's own functions as exported, under their C++ names, by the unshimmed
board library pyoracle.RefBoard loads: isEye / isFakeEye / isSemiEye / getEyeColor (base/board.cc:1850-1922), isTrueEye (through
RefBoard), getFastScore (:1924-1952), OneGroupLives (:1198-1221), getBoardBBox and GuessLDAttacker (:1024-1106).  A RefBoard
handle is a plain Board*, which is what these functions take.

GivenGroupLives is static there: it is reached as OneGroupLives(board, colour, &r) with r the 1x1 box on one stone of the group,
because only groups with a stone in the box are asked (tests/test_life_cpu.py proves that reading on the reference alone).  The
groups themselves (which stones belong together) are the flood fill of the colours; the number of living groups in a box is
counted over them."""
import ctypes as C

import numpy as np

import candidates_expected as CE
import ladder_positions as LP
from pyoracle import RefBoard

BLACK, WHITE = 1, 2
RULE_CHINESE, RULE_JAPANESE = 0, 1          # base/board.h:417-418
EYE, FAKE, TRUE, SEMI = 1, 2, 4, 8          # Black's bits of an eye byte; White's are these << 4
SUMMARY_WORDS = 12


class Region(C.Structure):
    """base/board.h:311-314: [left, right) x [top, bottom)"""
    _fields_ = [("left", C.c_int), ("top", C.c_int), ("right", C.c_int), ("bottom", C.c_int)]


def groups_of(colour, n):
    """flood fill of the colours -> (label per point int32 [NP], 0 on empty points, 1.. on stones; first stone (action) per label)"""
    g = np.asarray(colour).reshape(n, n)
    lab = np.zeros((n, n), np.int32)
    first = [None]
    for x0 in range(n):
        for y0 in range(n):
            if g[x0, y0] == 0 or lab[x0, y0]:
                continue
            k = len(first)
            first.append(x0 * n + y0)
            lab[x0, y0] = k
            stack = [(x0, y0)]
            while stack:
                x, y = stack.pop()
                for qx, qy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if 0 <= qx < n and 0 <= qy < n and g[qx, qy] == g[x0, y0] and not lab[qx, qy]:
                        lab[qx, qy] = k
                        stack.append((qx, qy))
    return lab.reshape(-1), first


class Life:
    def __init__(self, n):
        self.n = n
        self.RB = RefBoard(n)
        L = self.RB.L
        vp, us, ub = C.c_void_p, C.c_ushort, C.c_ubyte
        self._is_eye = L["_Z5isEyePK5Boardth"]
        self._is_eye.restype, self._is_eye.argtypes = C.c_bool, [vp, us, ub]
        self._is_fake = L["_Z9isFakeEyePK5Boardth"]
        self._is_fake.restype, self._is_fake.argtypes = C.c_bool, [vp, us, ub]
        self._is_semi = L["_Z9isSemiEyePK5BoardthPt"]
        self._is_semi.restype, self._is_semi.argtypes = C.c_bool, [vp, us, ub, C.POINTER(us)]
        self._eye_colour = L["_Z11getEyeColorPK5Boardt"]
        self._eye_colour.restype, self._eye_colour.argtypes = ub, [vp, us]
        self._fast = L["_Z12getFastScorePK5Boardi"]
        self._fast.restype, self._fast.argtypes = C.c_float, [vp, C.c_int]
        self._lives = L["_Z13OneGroupLivesPK5BoardhPK6Region"]
        self._lives.restype, self._lives.argtypes = C.c_bool, [vp, ub, C.POINTER(Region)]
        self._bbox = L["_Z12getBoardBBoxPK5BoardP6Region"]
        self._bbox.restype, self._bbox.argtypes = None, [vp, C.POINTER(Region)]
        self._attacker = L["_Z15GuessLDAttackerPK5BoardPK6Region"]
        self._attacker.restype, self._attacker.argtypes = ub, [vp, C.POINTER(Region)]
        self.coords = [(y + 1) * (n + 2) + (x + 1) for x in range(n) for y in range(n)]   # action a = x*n + y -> Coord
        self.action = {c: a for a, c in enumerate(self.coords)}

    # ---- the functions, one call each --------------------------------------------------------------------------------------
    def is_eye(self, h, a, player):
        return bool(self._is_eye(h, self.coords[a], player))

    def is_fake_eye(self, h, a, player):
        return bool(self._is_fake(h, self.coords[a], player))

    def is_true_eye(self, h, a, player):
        return self.RB.is_true_eye(h, self.coords[a], player)

    def is_semi_eye(self, h, a, player):
        """-> (answer, the Coord left in *move)"""
        mv = C.c_ushort(0xFFFF)
        r = bool(self._is_semi(h, self.coords[a], player, C.byref(mv)))
        return r, int(mv.value)

    def eye_colour(self, h, a):
        return int(self._eye_colour(h, self.coords[a]))

    def fast_score(self, h, rule):
        v = float(self._fast(h, rule))
        assert v == int(v)
        return int(v)

    def one_group_lives(self, h, player, box=None):
        """box = (left, top, right, bottom) or None (nullptr: every group is asked)"""
        return bool(self._lives(h, player, None if box is None else C.byref(Region(*[int(v) for v in box]))))

    def bbox(self, h):
        r = Region()
        self._bbox(h, C.byref(r))
        return (r.left, r.top, r.right, r.bottom)

    def attacker(self, h, box):
        return int(self._attacker(h, C.byref(Region(*[int(v) for v in box]))))

    # ---- whole rows ----------------------------------------------------------------------------------------------------------
    def eyes(self, h):
        """-> (eye uint8 [NP], semi_move int16 [2, NP]) as elfgo_life_map lays them out"""
        NP = self.n * self.n
        eye, semi = np.zeros(NP, np.uint8), np.full((2, NP), -1, np.int16)
        for a in range(NP):
            v = 0
            for c, player in enumerate((BLACK, WHITE)):
                sm, mv = self.is_semi_eye(h, a, player)
                bits = (EYE * self.is_eye(h, a, player) + FAKE * self.is_fake_eye(h, a, player) + TRUE * self.is_true_eye(h, a, player)
                        + SEMI * sm)
                v |= bits << (4 * c)
                if sm:
                    semi[c, a] = self.action[mv]
            eye[a] = v
        return eye, semi

    def alive(self, h, colour=None):
        """GivenGroupLives of every group, through the 1x1 box on its first stone -> (alive uint8 [NP], labels, living labels)"""
        col = self.RB.board(h)[0] if colour is None else colour
        lab, first = groups_of(col, self.n)
        out = np.zeros(self.n * self.n, np.uint8)
        living = set()
        for k in range(1, len(first)):
            x, y = first[k] // self.n, first[k] % self.n
            if self.one_group_lives(h, int(col[first[k]]), (x, y, x + 1, y + 1)):
                out[lab == k] = 1
                living.add(k)
        return out, lab, living

    def summary(self, h, box, col, alive, lab):
        n = self.n
        s = np.zeros(SUMMARY_WORDS, np.int32)
        s[0], s[1] = self.fast_score(h, RULE_CHINESE), self.fast_score(h, RULE_JAPANESE)
        s[2], s[3] = self.one_group_lives(h, BLACK, box), self.one_group_lives(h, WHITE, box)
        s[4:8] = box
        s[8] = self.attacker(h, box)
        x, y = np.arange(n * n) // n, np.arange(n * n) % n
        inbox = (box[0] <= x) & (x < box[2]) & (box[1] <= y) & (y < box[3])
        for c, player in enumerate((BLACK, WHITE)):
            s[9 + c] = len(set(lab[(alive == 1) & inbox & (col == player)].tolist()))
        return s

    def expected(self, h, box=None):
        """-> dict(eye, semi_move, alive, summary) of the position; box None = getBoardBBox, as a null regions pointer means"""
        col = self.RB.board(h)[0]
        eye, semi = self.eyes(h)
        alive, lab, _ = self.alive(h, col)
        bx = self.bbox(h) if box is None else tuple(int(v) for v in box)
        return dict(eye=eye, semi_move=semi, alive=alive, summary=self.summary(h, bx, col, alive, lab), colour=col, labels=lab,
                    eye_colour=np.array([self.eye_colour(h, a) for a in range(self.n * self.n)], np.uint8),
                    whole=(self.one_group_lives(h, BLACK), self.one_group_lives(h, WHITE)), info=self.RB.info(h))

    def with_box(self, h, exp, box):
        """the same position under another box: only the summary changes"""
        out = dict(exp)
        out["summary"] = self.summary(h, tuple(int(v) for v in box), exp["colour"], exp["alive"], exp["labels"])
        return out


_life = {}


def life(n):
    if n not in _life:
        _life[n] = Life(n)
    return _life[n]


# ---- the game sets of the GPU test, and the reference's answers on them, once per process -------------------------------------
def sampled_plies(name, game, length):
    """every ply of the first 16 9x9 games; every 8th ply plus the final position of the others"""
    if name == "nine" and game < 16:
        return list(range(length + 1))
    return sorted(set(range(0, length + 1, 8)) | {length})


def seeded_box(n, j, rng):
    """row j's box: it touches the left / top / right / bottom edge in turn, then an empty box, then anything"""
    xs, ys = sorted(int(v) for v in rng.integers(0, n + 1, 2)), sorted(int(v) for v in rng.integers(0, n + 1, 2))
    left, right, top, bottom = xs[0], xs[1], ys[0], ys[1]
    kind = j % 6
    if kind == 0:
        left = 0
    elif kind == 1:
        top = 0
    elif kind == 2:
        right = n
    elif kind == 3:
        bottom = n
    elif kind == 4:
        right = left
    return (left, top, right, bottom)


_games = {}


def all_expected(name):
    """-> (n, move lists, rows): rows = list of dict(game, ply, box, plain (Life.expected with no box), boxed (the same under the
    row's seeded box)) over the sampled positions of one game set of candidates_expected.game_sets(), computed once per process"""
    if name not in _games:
        if not CE._sets:
            CE._sets.update(CE.game_sets())
        n, gs = CE._sets[name]
        lf = life(n)
        rng = np.random.default_rng(20261021 + len(name))
        rows = []
        for i, moves in enumerate(gs):
            want = set(sampled_plies(name, i, len(moves)))
            h = lf.RB.new()
            for t in range(len(moves) + 1):
                if t in want:
                    box = seeded_box(n, len(rows), rng)
                    plain = lf.expected(h)
                    rows.append(dict(game=i, ply=t, box=box, plain=plain, boxed=lf.with_box(h, plain, box)))
                if t < len(moves):
                    assert lf.RB.play(h, int(moves[t])) == 1
            lf.RB.free(h)
        _games[name] = (n, gs, rows)
    return _games[name]


def statistics(rows):
    """the input conditions, counted on the reference's answers alone: positions, groups, living groups, semi-eyes, true eyes"""
    groups = sum(int(r["plain"]["labels"].max()) for r in rows)
    living = sum(len(set(r["plain"]["labels"][r["plain"]["alive"] == 1].tolist())) for r in rows)
    semi = sum(int(((r["plain"]["eye"] & SEMI) != 0).sum()) + int(((r["plain"]["eye"] & (SEMI << 4)) != 0).sum()) for r in rows)
    true = sum(int(((r["plain"]["eye"] & TRUE) != 0).sum()) + int(((r["plain"]["eye"] & (TRUE << 4)) != 0).sum()) for r in rows)
    return dict(positions=len(rows), groups=groups, living=living, semi_eyes=semi, true_eyes=true)


# ---- constructed positions -----------------------------------------------------------------------------------------------------
# X = Black, O = White, row = y, column = x.  Lower-case letters mark empty points the facts below name.  Facts, all for the
# drawing's X colour unless said otherwise (hand-derived; tests/test_life_cpu.py holds the reference to them in all 16 images):
#   bits  letter -> the colour's four answers at the point (EYE | FAKE | TRUE | SEMI)
#   semi  letter -> the letter of the point isSemiEye names
#   alive (x, y) of a stone -> GivenGroupLives of its group
_SHAPES = {
    # 1. two eyes: the 1-1 point and a first-line point; two first-line points; two centre points
    "two_eyes_corner": dict(rows=["a X b X .",
                                  "X X X X .",
                                  ". . . . ."], at=("corner",), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(1, 0): 1}),
    "two_eyes_edge": dict(rows=["X a X b X",
                                "X X X X X"], at=("corner", "edge"), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(0, 0): 1}),
    "two_eyes_centre": dict(rows=["X X X X X",
                                  "X a X b X",
                                  "X X X X X"], at=("centre",), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(0, 0): 1}),
    # 2. two eyes diagonal to each other: each has two own stones and the other eye on its diagonals (three of four), and both
    #    touch both groups, so each is in either group's list: both groups live, and neither eye would do without the other
    "diagonal_pair": dict(rows=[". X X .",
                                "X a X X",
                                "X X b X",
                                ". X X ."], at=("centre",), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(1, 0): 1, (0, 1): 1}),
    # 3. a centre eye with one enemy diagonal and three own: true, and it counts
    "one_enemy_diagonal": dict(rows=["O X X X X",
                                     "X a X b X",
                                     "X X X X X"], at=("centre",), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(1, 0): 1}),
    # 4. a centre eye with two empty diagonals that are no eyes: true (no enemy), territory 2 of 4: the group has one
    #    qualifying eye (b) and does not live
    "two_empty_diagonals": dict(rows=[". X . . .",
                                      "X a X X X",
                                      "X X X b X",
                                      ". . X X X"], at=("centre",), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(0, 1): 0, (1, 0): 0}),
    # 5. the lone stone (1,0) touches the eyes a and f only; a's other diagonal d is a true eye, but of the big group alone.  For
    #    the lone stone a has territory 1 + 2 off-board = 3 of 4 (d is not in its list) and only f qualifies: it does not live.
    #    The big group's list holds a, f and d, all three qualify: it lives.  With a board-wide true-eye set a would qualify for
    #    the lone stone too.
    "other_groups_eye": dict(rows=[". X a X X",
                                   "X f X d X",
                                   "X X X X X"], at=("edge",), bits=dict(a=EYE | TRUE, f=EYE | TRUE, d=EYE | TRUE),
                             alive={(1, 0): 0, (0, 1): 1}),
    # 6. the eye is the group's only liberty: playing it is suicide for its owner, and it is an eye all the same
    "suicide_eye": dict(rows=["O O O O O",
                              "O X X X O",
                              "O X a X O",
                              "O X X X O",
                              "O O O O O"], at=("centre",), bits=dict(a=EYE | TRUE), alive={(1, 1): 0}),
    # 8. semi-eyes: centre (one enemy diagonal, one empty one that is no eye), first line (no enemy, one such empty one)
    "semi_centre": dict(rows=["O X m",
                              "X a X",
                              "X X X"], at=("centre",), bits=dict(a=EYE | TRUE | SEMI), semi=dict(a="m"), alive={(1, 0): 0}),
    "semi_edge": dict(rows=["X a X",
                            "m X X"], at=("edge",), bits=dict(a=EYE | TRUE | SEMI), semi=dict(a="m"), alive={(0, 0): 0}),
    # 9. one enemy diagonal, and the only empty diagonal (b) is itself an eye: it is left out of the count, a is no semi-eye
    "semi_excluded": dict(rows=["O X X .",
                                "X a X X",
                                "X X b X",
                                ". X X ."], at=("centre",), bits=dict(a=EYE | TRUE, b=EYE | TRUE), alive={(1, 0): 1}),
}


def _placed(n, rows, where):
    flat = [r.replace(" ", "") for r in rows]
    w, hgt = len(flat[0]), len(flat)
    ox, oy = {"corner": (0, 0), "edge": (n // 2 - 2, 0), "centre": ((n - w) // 2, (n - hgt) // 2)}[where]
    letters = {ch: (ox + x) * n + oy + y for y, r in enumerate(flat) for x, ch in enumerate(r) if ch.islower()}
    clean = ["".join("." if ch.islower() else ch for ch in r) for r in flat]
    return LP.draw(n, clean, ox, oy), letters, (ox, oy)


def constructed(n):
    """name -> dict(stones, mover, bits {action: nibble}, semi {action: action}, alive {action: 0 / 1}) for the drawing's X"""
    P = {}
    for name, d in _SHAPES.items():
        for where in d["at"]:
            st, letters, (ox, oy) = _placed(n, d["rows"], where)
            P["%s_%s" % (name, where)] = dict(
                stones=st, mover=BLACK, bits={letters[k]: v for k, v in d["bits"].items()},
                semi={letters[k]: letters[v] for k, v in d.get("semi", {}).items()},
                alive={(ox + x) * n + oy + y: v for (x, y), v in d["alive"].items()})
    return P


def rows(n):
    """every image of every constructed position; the pending simple ko (a move list: ladder_positions.ko_list: the ko point is
    an eye of the side that took, with two enemy diagonals -- a fake one) and the empty board last
    -> list of dict(name, s, swapped, stones, mover, moves, bits, semi, alive): the facts mapped into the image, `colour` = the
    colour the drawing's X has there"""
    out = []
    for name, d in constructed(n).items():
        for s, sw, ist, imv in LP.images(n, d["stones"], d["mover"]):
            perm = LP.sym_perm(n, s)
            out.append(dict(name=name, s=s, swapped=sw, stones=ist, mover=imv, moves=None, colour=WHITE if sw else BLACK,
                            bits={int(perm[a]): v for a, v in d["bits"].items()},
                            semi={int(perm[a]): int(perm[m]) for a, m in d["semi"].items()},
                            alive={int(perm[a]): v for a, v in d["alive"].items()}))
    moves, (_, st, mover), k = LP.ko_cases(n)
    for (s, sw, mv), (_, _, ist, imv) in zip(LP.move_images(n, moves), LP.images(n, st, mover)):
        # the drawing's O (White) took the ko: k is O's eye; "colour" is the colour O has in the image
        out.append(dict(name="ko_pending", s=s, swapped=sw, stones=ist, mover=imv, moves=mv, colour=BLACK if sw else WHITE,
                        bits={int(LP.sym_perm(n, s)[k]): EYE | FAKE}, semi={}, alive={}))
    out.append(dict(name="empty_board", s=0, swapped=False, stones=np.zeros(n * n, np.uint8), mover=BLACK, moves=[], colour=BLACK,
                    bits={}, semi={}, alive={}))
    return out


# 10. GuessLDAttacker: Black (3,3) and (3,4), White (5,3).  Each scan counts the first stone of every row / column of the box seen
# from one side, and a side is scanned only where the box does not touch that board edge.  By hand, (left, top, right, bottom) ->
# (black count, white count): the full box scans all four sides; the one on the left edge loses Black's two rows and ties.
ATTACKER_STONES = ((3, 3, BLACK), (3, 4, BLACK), (5, 3, WHITE))


def attacker_boxes(n):
    """-> list of (box, black count, white count)"""
    return [((2, 2, 7, 6), 5, 3), ((0, 2, 7, 6), 3, 3), ((2, 0, 7, 6), 4, 2), ((2, 2, n, 6), 4, 2), ((2, 2, 7, n), 4, 2),
            ((0, 0, n, n), 0, 0)]


def attacker_position(n):
    st = np.zeros(n * n, np.uint8)
    for x, y, c in ATTACKER_STONES:
        st[x * n + y] = c
    return st


_rows = {}


def expected(n):
    """rows(n) with the reference's answers added (`plain`: Life.expected with no box; info), computed once per process
    -> (Life, rows)"""
    if n not in _rows:
        lf = life(n)
        out = rows(n)
        for r in out:
            h = LP.handle(lf.RB, r)
            assert h is not None, "the stones of %s cannot stand" % r["name"]
            assert np.array_equal(lf.RB.board(h)[0], r["stones"]) and int(lf.RB.info(h)[1]) == r["mover"], r["name"]
            r["plain"] = lf.expected(h)
            r["legal_mask"] = lf.RB.legal_mask(h)[:-1]
            r["info"] = lf.RB.info(h)
            lf.RB.free(h)
        _rows[n] = (lf, out)
    return _rows[n]
