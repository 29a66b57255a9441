"""What elfgo_candidates / elfgo_playout_cand / elfgo_own_run_cand must return, taken from the reference's own functions:
FindAllCandidateMoves (base/board.cc:850-890) and isSelfAtari (board.cc:254-297) as exported, under their C++ names, by the
unshimmed board library pyoracle.RefBoard loads.  A RefBoard handle is a plain Board*, which is what these functions take.

The playout driver is playout_one of oracle/ref_capi.cc:137-160 restated with the candidate list swapped in: a pyoracle.Ref
GoState gives forward, terminated, super-ko and the move limit; a RefBoard mirrored move for move gives the candidate lists; the
two hashes are compared at every step."""
import ctypes as C

import numpy as np

import ladder_positions as LP
import ownership_expected as OE
import setup_expected as SE
from pyoracle import Port, Ref, RefBoard, playout_seeds

M_PASS = 0
BLACK, WHITE = 1, 2
NO_THRES = 32767            # no group is that large: nothing is dropped
THRESHOLDS = (1, 3, NO_THRES)

# the whole-board 9x9 seki, Black to move (row = y, column = x, X Black, O White): the inner black group (2,0) (2,1) (3,1) (2,2)
# (2,3) (3,3) and the inner white group (4,0) (4,1) (4,2) (4,3) share the liberties (3,0) and (3,2) and nothing else; every other
# empty point is a true eye
SEKI = [". O X . O X . X .",
        "O O X X O X X X X",
        ". O X . O X . X .",
        "O O X X O X X X X",
        "O O O O X X . X .",
        ". O . O X . X X X",
        "O O O O X X X . X",
        ". O . O X . X X .",
        "O O O O X X X X X"]
SEKI_LIBS = ((3, 0), (3, 2))
SEKI_INNER_BLACK = ((2, 0), (2, 1), (3, 1), (2, 2), (2, 3), (3, 3))
SEKI_INNER_WHITE = ((4, 0), (4, 1), (4, 2), (4, 3))


def seki():
    """-> (n, stones, mover)"""
    return 9, LP.draw(9, SEKI), BLACK


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def playout_rng(seed, t):
    """oracle/ref_capi.cc:131-134"""
    seed = int(seed)
    key = fmix32(seed & 0xFFFFFFFF) ^ fmix32(((seed >> 32) + 0x7F4A7C15) & 0xFFFFFFFF)
    return fmix32((key + t * 0x9E3779B9) & 0xFFFFFFFF)


class Cand:
    def __init__(self, n):
        self.n = n
        self.RB = RefBoard(n)
        L = self.RB.L

        class AllMoves(C.Structure):
            """base/board.h:160-164 (Coord = unsigned short)"""
            _fields_ = [("board", C.c_void_p), ("moves", C.c_ushort * (n * n)), ("num_moves", C.c_int)]
        self._am = AllMoves()
        self._find = L["_Z21FindAllCandidateMovesPK5BoardhiP8AllMoves"]
        self._find.restype, self._find.argtypes = None, [C.c_void_p, C.c_ubyte, C.c_int, C.c_void_p]
        self._sa = L["_Z11isSelfAtariPK5BoardPK8GroupId4thPi"]
        self._sa.restype, self._sa.argtypes = C.c_bool, [C.c_void_p, C.c_void_p, C.c_ushort, C.c_ubyte, C.POINTER(C.c_int)]
        self.coords = [(y + 1) * (n + 2) + (x + 1) for x in range(n) for y in range(n)]   # action a = x*n + y -> Coord
        self.action = {c: a for a, c in enumerate(self.coords)}

    def candidates(self, h, player, thres):
        """FindAllCandidateMoves(h, player, thres) in that function's own (x-major) order, as Coords"""
        self._find(h, int(player), int(thres), C.byref(self._am))
        return [int(self._am.moves[i]) for i in range(self._am.num_moves)]

    def mask(self, h, player, thres):
        m = np.zeros(self.n * self.n, np.uint8)
        for c in self.candidates(h, player, thres):
            m[self.action[c]] = 1
        return m

    def self_atari(self, h, a, player):
        """the num_stones isSelfAtari(h, nullptr, point a, player, &num) writes where it returns true, else 0"""
        num = C.c_int(0)
        return num.value if self._sa(h, None, self.coords[a], int(player), C.byref(num)) else 0

    def stones(self, h, player, colour=None):
        """self_atari at every point, int16 [NP]; only empty points are asked (TryPlay refuses the others)"""
        col = self.RB.board(h)[0] if colour is None else colour
        out = np.zeros(self.n * self.n, np.int16)
        for a in np.nonzero(col == 0)[0]:
            out[a] = self.self_atari(h, int(a), player)
        return out

    def game(self, moves, thresholds=THRESHOLDS):
        """the answers at all len(moves) + 1 positions of a game (row 0 = before the first move), for the side to move
        -> dict(stones [k+1, NP], mask {t: [k+1, NP]}, legal [k+1, NP], eyes [k+1, NP] (the mover's true eyes), info [k+1, 10])"""
        RB = self.RB
        rep = RB.replay(moves)
        assert rep["ok"].all()
        h = RB.new()
        st, mk = [], {t: [] for t in thresholds}
        for t in range(len(moves) + 1):
            player = int(rep["info"][t, 1])
            st.append(self.stones(h, player, rep["colour"][t]))
            for th in thresholds:
                mk[th].append(self.mask(h, player, th))
            if t < len(moves):
                assert RB.play(h, int(moves[t])) == 1
        RB.free(h)
        players = rep["info"][:, 1]
        eyes = np.array([rep["eyes"][t, players[t] - 1] for t in range(len(moves) + 1)])
        return dict(stones=np.array(st), mask={t: np.array(v) for t, v in mk.items()}, legal=rep["legal"][:, :-1], eyes=eyes,
                    info=rep["info"])

    # ---- the playout driver ---------------------------------------------------------------------------------------------
    def playout(self, E, s, b, seed, thres, max_steps=100000):
        """plays GoState s (engine E = pyoracle.Ref) and its mirror Board b to the end with the candidate policy -> steps"""
        RB = self.RB
        steps = 0
        while not E.terminated(s) and steps < max_steps:
            info = E.info(s)
            assert E.hash(s) == RB.hash(b)
            cand = self.candidates(b, int(info[1]), thres)
            pick = cand[playout_rng(seed, int(info[0])) % len(cand)] if cand else M_PASS
            if E.forward(s, pick) != 1:
                break
            assert RB.play(b, pick) == 1
            steps += 1
        assert E.hash(s) == RB.hash(b)
        return steps

    def playout_from(self, E, moves, seed, thres, max_steps=100000, keep=False):
        """a game's moves from the empty board, then the driver -> (hash, ply, steps[, end state to free])"""
        s, b = E.new(), self.RB.new()
        for c in moves:
            assert E.forward(s, int(c)) == 1 and self.RB.play(b, int(c)) == 1
        steps = self.playout(E, s, b, seed, thres, max_steps)
        out = (E.hash(s), int(E.info(s)[0]), steps)
        self.RB.free(b)
        if keep:
            return out + (s,)
        E.free(s)
        return out

    def ownership(self, E, moves, seed, K, komi, thres, max_steps=100000):
        """counts int32 [2, NP] and stats int64 [4] of K driver playouts from the position after `moves`
        (ownership_expected.expected with the driver in place of playout_moves)"""
        n = self.n
        counts, stats = np.zeros((2, n * n), np.int32), np.zeros(4, np.int64)
        for k in range(K):
            _, _, steps, s = self.playout_from(E, moves, OE.seed_of(seed, k), thres, max_steps, keep=True)
            am = OE.area_map(E.board(s)[0], n)
            counts[0] += am == 1
            counts[1] += am == 2
            diff = OE.area_diff(am)
            stats[0] += diff
            stats[1] += int(np.float32(diff) - np.float32(komi) > 0)
            stats[2] += int(OE.ended_by_superko(E, s))
            stats[3] += steps
            E.free(s)
        return counts, stats


# ---- the game sets of the GPU test, and the reference's answers on them, once per process -------------------------------------
def game_sets():
    """name -> (n, move lists): the 64 seeded 9x9 playout games, the first 16 ladder-suite games, 4 seeded 19x19 playout games"""
    sets = {"nine": (9, SE.nine_games(Port(9))), "ladder16": (19, SE.ladder_games()[:16])}
    E = Ref(19)
    big = []
    for sd in playout_seeds(4):
        s = E.new()
        big.append(np.asarray(E.playout_moves(s, int(sd)), np.int32))
        E.free(s)
    sets["playout19"] = (19, big)
    return sets


_cand, _sets, _games = {}, {}, {}


def cand(n):
    if n not in _cand:
        _cand[n] = Cand(n)
    return _cand[n]


def all_expected(name):
    """-> (n, move lists, Cand.game dict per game) of one game set, computed once per process"""
    if not _sets:
        _sets.update(game_sets())
    if name not in _games:
        n, gs = _sets[name]
        _games[name] = (n, gs, [cand(n).game(mv) for mv in gs])
    return _games[name]


def statistics(exp):
    """the counts the CPU test pins, over a list of Cand.game dicts: positions, legal points, self-atari points (stones > 0),
    the largest num_stones, points that thres 1 / thres 3 drop from the no-threshold list"""
    pos = sum(len(g["stones"]) for g in exp)
    legal = sum(int(g["legal"].sum()) for g in exp)
    sa = sum(int((g["stones"] > 0).sum()) for g in exp)
    big = max(int(g["stones"].max()) for g in exp)
    d1 = sum(int(g["mask"][NO_THRES].sum()) - int(g["mask"][1].sum()) for g in exp)
    d3 = sum(int(g["mask"][NO_THRES].sum()) - int(g["mask"][3].sum()) for g in exp)
    return dict(positions=pos, legal=legal, self_atari=sa, largest=big, dropped1=d1, dropped3=d3)


# ---- constructed positions -----------------------------------------------------------------------------------------------------
# X = Black = the side to move; `p` marks the played point (empty), `s` a point the text below names (empty).  Every drawing is
# placed with its top-left corner at several offsets.  name -> (rows, num_stones isSelfAtari must give at p, p legal)
_SHAPES = {
    # a throw-in with no empty neighbour whose capture of four stones leaves four liberties: legal, not a self-atari
    "throw_in": ([". . X . .",
                  ". X O X .",
                  "X O p O X",
                  ". X O X .",
                  ". . X . ."], 0, True),
    # the capture of (1,1) leaves exactly one liberty, and the own stone (3,1), whose only liberty is p, joins: self-atari of 2
    "capture_one_liberty": ([". X O O .",
                             "X O p X O",
                             ". X O O ."], 2, True),
    # two own two-liberty groups whose other liberty is the same point s: the union has one liberty, the sum two
    "join_shared": ([". O O O .",
                     "O X p X O",
                     "O X s X O",
                     ". O O O ."], 5, True),
    # two own two-liberty groups with separate second liberties: two liberties after the move
    "join_apart": ([". O O O O O .",
                    "O . X p X . O",
                    ". O O O O O ."], 0, True),
    # an own neighbour with exactly three liberties, p among them: two remain
    "own_three": ([". O O O .",
                   "O p X . O",
                   ". O . O ."], 0, True),
    # the mover's own true eye of a two-liberty group: filling it is a self-atari of all eight stones; never a candidate
    "own_eye": (["O O O O O",
                 "O X X X O",
                 "O X p X O",
                 "O X X . O",
                 "O O O O O"], 8, True),
    # suicide: illegal
    "suicide": ([". O .",
                 "O p O",
                 ". O ."], 0, False),
}
CONSTRUCTED_THRESHOLDS = (1, 2, 5, 8, NO_THRES)


def _shape(n, rows, ox, oy):
    flat = [r.replace(" ", "") for r in rows]
    (px, py), = [(x, y) for y, r in enumerate(flat) for x, ch in enumerate(r) if ch == "p"]
    return LP.draw(n, [r.replace("p", ".").replace("s", ".") for r in flat], ox, oy), (ox + px) * n + oy + py


def placements(n, rows):
    """a corner, the top edge and the centre; at 19x19 also the played point on actions 63 and 64 (a = x*19 + y: (3,6) and (3,7)),
    which puts the merged groups of the joins across the boundary between the bitboard's first two 64-bit words"""
    flat = [r.replace(" ", "") for r in rows]
    (px, py), = [(x, y) for y, r in enumerate(flat) for x, ch in enumerate(r) if ch == "p"]
    out = {"corner": (0, 0), "edge": (n // 2 - 2, 0), "centre": (n // 2 - 3, n // 2 - 2)}
    if n == 19:
        out["a63"] = (3 - px, 6 - py)
        out["a64"] = (3 - px, 7 - py)
    return out


def constructed(n):
    """name -> dict(stones, mover, p (action of the played point, None for the seki), num, legal)"""
    P = {}
    if n == 9:
        P["seki"] = dict(stones=seki()[1], mover=BLACK, p=None, num=None, legal=None)
    for name, (rows, num, legal) in _SHAPES.items():
        for tag, (ox, oy) in placements(n, rows).items():
            st, p = _shape(n, rows, ox, oy)
            P["%s_%s" % (name, tag)] = dict(stones=st, mover=BLACK, p=p, num=num, legal=legal)
    return P


def rows(n):
    """every image of every constructed position, the pending simple ko (a move list: ladder_positions.ko_list) last
    -> list of dict(name, s, swapped, stones, mover, moves, p, num, legal)"""
    out = []
    for name, d in constructed(n).items():
        for s, sw, ist, imv in LP.images(n, d["stones"], d["mover"]):
            p = None if d["p"] is None else int(LP.sym_perm(n, s)[d["p"]])
            out.append(dict(name=name, s=s, swapped=sw, stones=ist, mover=imv, moves=None, p=p, num=d["num"], legal=d["legal"]))
    moves, (_, st, mover), k = LP.ko_cases(n)
    for (s, sw, mv), (_, _, ist, imv) in zip(LP.move_images(n, moves), LP.images(n, st, mover)):
        out.append(dict(name="ko_pending", s=s, swapped=sw, stones=ist, mover=imv, moves=mv, p=int(LP.sym_perm(n, s)[k]), num=0,
                        legal=False))
    return out


_rows = {}


def expected(n):
    """rows(n) with the reference's answers added (stones int16 [NP], mask {t: uint8 [NP]} for CONSTRUCTED_THRESHOLDS, legal,
    info), computed once per process -> (Cand, rows)"""
    if n not in _rows:
        cd = cand(n)
        out = rows(n)
        for r in out:
            h = LP.handle(cd.RB, r)
            assert h is not None, "the stones of %s cannot stand" % r["name"]
            assert np.array_equal(cd.RB.board(h)[0], r["stones"]) and int(cd.RB.info(h)[1]) == r["mover"], r["name"]
            r["stones_sa"] = cd.stones(h, r["mover"])
            r["mask"] = {t: cd.mask(h, r["mover"], t) for t in CONSTRUCTED_THRESHOLDS}
            r["legal_mask"] = cd.RB.legal_mask(h)[:-1]
            r["info"] = cd.RB.info(h)
            cd.RB.free(h)
        _rows[n] = (cd, out)
    return _rows[n]


def xy(n, pts):
    return [x * n + y for x, y in pts]
