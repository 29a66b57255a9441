"""What elfgo_region_moves / elfgo_ld_run must return, taken from the reference's own functions as exported, under their C++ names,
by the unshimmed board library pyoracle.RefBoard loads: FindAllCandidateMovesInRegion (base/board.cc:892-947),
FindAllValidMovesInRegion (:970-1005), GroupInRegion (:1183-1196), and through life_expected OneGroupLives, getBoardBBox and
GuessLDAttacker.  A RefBoard handle is a plain Board*, which is what these functions take.

Two playout drivers, both candidates_expected.Cand.playout with the region list in place of the whole-board list:
  * Reg.playout_state: on positions reached by play.  A pyoracle.Ref GoState gives forward, terminated, super-ko and the move
    limit; a RefBoard mirrored move for move gives the lists; the two hashes are compared at every step.
  * Reg.playout_bare: on set-up positions (GoEngine.setup: ply 1, no super-ko records, no last moves), where the reference has no
    GoState to stand on.  It runs on the bare Board: the ply is counted from `ply0`, GoState::terminated() (go_state.h:141-147) and
    the super-ko rule (go_state.cc:96-121: the pre-move position of every non-pass move is recorded; a position reached by a
    non-pass move that equals a recorded one ends the game) are restated on stone arrays.  tests/test_region_cpu.py proves the
    restatement against playout_state on the played rows.
The oracle exports no per-stone group ids, so the per-stone map of GroupInRegion is the flood fill of the colours
(life_expected.groups_of); test_region_cpu.py holds the count of GroupInRegion over the ids to it."""
import ctypes as C

import numpy as np

import candidates_expected as CE
import ladder_positions as LP
import life_expected as LE
import ownership_expected as OE
from pyoracle import Ref

M_PASS, M_INVALID = 0, 3
BLACK, WHITE = 1, 2
INFO_WORDS, STAT_WORDS = 8, 8
M64 = 0xFFFFFFFFFFFFFFFF


def no_thres(n):
    return n * n + 1


class Reg:
    def __init__(self, n):
        self.n = n
        self.cd = CE.cand(n)
        self.lf = LE.life(n)
        self.RB = self.cd.RB
        L = self.RB.L

        class AllMoves(C.Structure):
            """base/board.h:160-164 (Coord = unsigned short)"""
            _fields_ = [("board", C.c_void_p), ("moves", C.c_ushort * (n * n)), ("num_moves", C.c_int)]
        self._am = AllMoves()
        rp = C.POINTER(LE.Region)
        self._cand = L["_Z29FindAllCandidateMovesInRegionPK5BoardPK6RegionhiP8AllMoves"]
        self._cand.restype, self._cand.argtypes = None, [C.c_void_p, rp, C.c_ubyte, C.c_int, C.c_void_p]
        self._valid = L["_Z25FindAllValidMovesInRegionPK5BoardPK6RegionP8AllMoves"]
        self._valid.restype, self._valid.argtypes = None, [C.c_void_p, rp, C.c_void_p]
        self._gin = L["_Z13GroupInRegionPK5BoardsPK6Region"]
        self._gin.restype, self._gin.argtypes = C.c_bool, [C.c_void_p, C.c_short, rp]
        self.action = self.cd.action
        x, y = np.arange(n * n) // n, np.arange(n * n) % n
        self._xy = (x, y)

    @staticmethod
    def _region(box):
        return None if box is None else C.byref(LE.Region(*[int(v) for v in box]))

    def inbox(self, box):
        """bool [NP]: the points of the half-open box; None = the whole board"""
        if box is None:
            return np.ones(self.n * self.n, bool)
        x, y = self._xy
        return (box[0] <= x) & (x < box[2]) & (box[1] <= y) & (y < box[3])

    # ---- the three functions -----------------------------------------------------------------------------------------------
    def cand_in(self, h, box, player, thres):
        """FindAllCandidateMovesInRegion(h, box, player, thres) in that function's own (x-major) order, as Coords"""
        self._cand(h, self._region(box), int(player), int(thres), C.byref(self._am))
        return [int(self._am.moves[i]) for i in range(self._am.num_moves)]

    def valid_in(self, h, box):
        self._valid(h, self._region(box), C.byref(self._am))
        return [int(self._am.moves[i]) for i in range(self._am.num_moves)]

    def group_in(self, h, gid, box):
        return bool(self._gin(h, int(gid), self._region(box)))

    def groups_in_count(self, h, box):
        """GroupInRegion counted over the ids 1 .. _num_groups - 1"""
        return sum(self.group_in(h, g, box) for g in range(1, int(self.RB.info(h)[9]) + 1))

    def _mask(self, coords):
        m = np.zeros(self.n * self.n, np.uint8)
        for c in coords:
            m[self.action[c]] = 1
        return m

    def groups_map(self, col, lab, box):
        """1 on every stone of a flood-fill group (labels `lab`, life_expected.groups_of) that has a stone in the box"""
        hit = set(lab[(col != 0) & self.inbox(box)].tolist())
        groups = np.isin(lab, sorted(hit)) & (col != 0) if hit else np.zeros(self.n * self.n, bool)
        return groups.astype(np.uint8)

    def masks(self, h, box, thres, col=None):
        """-> (cand, valid, groups) uint8 [NP] as elfgo_region_moves lays them out, for the side to move"""
        col = self.RB.board(h)[0] if col is None else col
        player = int(self.RB.info(h)[1])
        lab, _ = LE.groups_of(col, self.n)
        return self._mask(self.cand_in(h, box, player, thres)), self._mask(self.valid_in(h, box)), self.groups_map(col, lab, box)

    # ---- the playout drivers -----------------------------------------------------------------------------------------------
    def playout_state(self, E, s, b, seed, thres, box, max_steps):
        """plays GoState s and its mirror Board b -> (steps, first move as Coord or None)"""
        RB = self.RB
        steps, first = 0, None
        while not E.terminated(s) and steps < max_steps:
            info = E.info(s)
            assert E.hash(s) == RB.hash(b)
            cand = self.cand_in(b, box, int(info[1]), thres)
            pick = cand[CE.playout_rng(seed, int(info[0])) % len(cand)] if cand else M_PASS
            if E.forward(s, pick) != 1:
                break
            assert RB.play(b, pick) == 1
            if steps == 0:
                first = pick
            steps += 1
        assert E.hash(s) == RB.hash(b)
        return steps, first

    def playout_bare(self, b, seed, thres, box, max_steps, ply0=1, last=(M_INVALID, M_INVALID), records=()):
        """plays the bare Board b -> (steps, first move as Coord or None, ended on a super-ko repeat, ply).  `last` = the two
        moves before the position (newest first), `records` = the stone rows (bytes) GoState would hold on entry."""
        RB, n = self.RB, self.n
        ply, last, rec = int(ply0), list(last), set(records)
        superko, steps, first = False, 0, None
        while steps < max_steps and not ((last[0] == M_PASS and last[1] == M_PASS) or ply >= 2 * n * n or superko):
            player = int(RB.info(b)[1])
            cand = self.cand_in(b, box, player, thres)
            pick = cand[CE.playout_rng(seed, ply) % len(cand)] if cand else M_PASS
            if pick != M_PASS:
                rec.add(RB.board(b)[0].tobytes())
            assert RB.play(b, pick) == 1
            ply += 1
            last = [pick, last[0]]
            superko = pick != M_PASS and RB.board(b)[0].tobytes() in rec
            if steps == 0:
                first = pick
            steps += 1
        return steps, first, superko, ply

    # ---- one row of elfgo_ld_run -------------------------------------------------------------------------------------------
    def frame(self, h, box, attacker):
        """-> (box used, attacker, defender): box None = getBoardBBox, attacker not 1 / 2 = GuessLDAttacker(box)"""
        bx = self.lf.bbox(h) if box is None else tuple(int(v) for v in box)
        att = int(attacker) if attacker in (BLACK, WHITE) else self.lf.attacker(h, bx)
        return bx, att, BLACK + WHITE - att

    def ld_row(self, E, src, seed, K, thres, box=None, attacker=0, max_steps=100000, ends=None):
        """info int32 [8], stats int64 [8] (word 6 as uint64 bits), first int32 [3, NP + 1] of K driver playouts from `src`:
        a move list (played from the empty board, GoState driver) or dict(stones, mover) (a set-up position, bare driver).
        `ends`, if a list, receives per playout (steps, ended by super-ko, cut by max_steps while not terminated)."""
        RB, n = self.RB, self.n
        NP = n * n
        setup = isinstance(src, dict)
        if setup:
            b0 = LP.build(RB, src["stones"], src["mover"])
            assert b0 is not None
            s0 = None
        else:
            s0, b0 = E.new(), RB.new()
            for c in src:
                assert E.forward(s0, int(c)) == 1 and RB.play(b0, int(c)) == 1
        bx, att, dfn = self.frame(b0, box, attacker)
        inb = self.inbox(bx)
        info = np.zeros(INFO_WORDS, np.int32)
        info[0:4] = bx
        info[4], info[5], info[6] = att, dfn, int(RB.info(b0)[1])
        info[7] = self.lf.one_group_lives(b0, dfn, bx)
        stats, first = np.zeros(STAT_WORDS, np.int64), np.zeros((3, NP + 1), np.int32)
        hsum = 0
        for k in range(K):
            sd = OE.seed_of(seed, k)
            b = RB.clone(b0)
            if setup:
                steps, fm, sko, ply = self.playout_bare(b, sd, thres, bx, max_steps)
                cut = steps == max_steps and not (sko or ply >= 2 * NP)   # two passes are checked by the caller where it matters
            else:
                s = E.clone(s0)
                steps, fm = self.playout_state(E, s, b, sd, thres, bx, max_steps)
                sko = OE.ended_by_superko(E, s)
                cut = steps == max_steps and not E.terminated(s)
                E.free(s)
            col = RB.board(b)[0]
            lived = int(self.lf.one_group_lives(b, dfn, bx))
            nd, na = int(((col == dfn) & inb).sum()), int(((col == att) & inb).sum())
            stats[0] += lived
            stats[1] += nd > 0
            stats[2] += nd
            stats[3] += na
            stats[4] += int(sko)
            stats[5] += steps
            hsum = (hsum + RB.hash(b)) & M64
            if steps > 0:
                a = NP if fm == M_PASS else self.action[fm]
                first[0, a] += 1
                first[1, a] += lived
                first[2, a] += nd > 0
            if ends is not None:
                ends.append((steps, bool(sko), bool(cut)))
            RB.free(b)
        stats[6] = np.uint64(hsum).astype(np.int64)
        RB.free(b0)
        if s0 is not None:
            E.free(s0)
        return info, stats, first


_reg, _ref = {}, {}


def reg(n):
    if n not in _reg:
        _reg[n] = Reg(n)
    return _reg[n]


def ref(n):
    if n not in _ref:
        _ref[n] = Ref(n)
    return _ref[n]


# ---- boxes of the region_moves test -----------------------------------------------------------------------------------------------
def list_boxes(n, j, ko=None):
    """the boxes row j is asked with: the whole board as None and as (0, 0, n, n), an empty box, a 1x1 box, one full line, a box
    touching each edge (life_expected.seeded_box's first four kinds) and, for a ko row, a box holding the ko point `ko` (action)"""
    rng = np.random.default_rng(977 * n + j)
    px, py = int(rng.integers(0, n)), int(rng.integers(0, n))
    out = [None, (0, 0, n, n), (px, py, px, py + 1) if j % 2 else (px, py, px + 1, py), (px, py, px + 1, py + 1),
           (px, 0, px + 1, n) if j % 2 else (0, py, n, py + 1)]
    out += [LE.seeded_box(n, kind, rng) for kind in range(4)]
    if ko is not None:
        kx, ky = ko // n, ko % n
        out += [(kx, ky, kx + 1, ky + 1), (max(kx - 1, 0), max(ky - 2, 0), min(kx + 2, n), min(ky + 1, n))]
    return out


def list_thresholds(n):
    return (1, 3, 5, no_thres(n))


_lists = {}


def list_sets(n):
    """the positions of the region_moves test -> list of dict(name, games (move lists), rows [dict(game, ply, ko)]): every 4th
    ply of the games of candidates_expected.game_sets() on this board size, then the 16 images of ladder_positions' pending ko
    (asked at their last ply; ko = the ko point as action)"""
    if n not in _lists:
        if not CE._sets:
            CE._sets.update(CE.game_sets())
        sets = []
        for name, (sz, games) in CE._sets.items():
            if sz == n:
                games = [[int(c) for c in g] for g in games]
                sets.append(dict(name=name, games=games,
                                 rows=[dict(game=i, ply=t, ko=None) for i, g in enumerate(games) for t in range(0, len(g) + 1, 4)]))
        moves, _, k = LP.ko_cases(n)
        imgs = LP.move_images(n, moves)
        sets.append(dict(name="ko", games=[[int(c) for c in mv] for _, _, mv in imgs],
                         rows=[dict(game=i, ply=len(mv), ko=int(LP.sym_perm(n, s)[k])) for i, (s, _, mv) in enumerate(imgs)]))
        _lists[n] = sets
    return _lists[n]


def list_rows(n):
    """list_sets(n) flattened -> list of dict(moves, ko)"""
    return [dict(moves=st["games"][r["game"]][:r["ply"]], ko=r["ko"]) for st in list_sets(n) for r in st["rows"]]


_list_exp = set()


def list_expected(n):
    """list_sets(n) with, per row, `boxes`, `valid` / `groups` [box] and `cand` {thres: [box]} (uint8 [NP] each); the row's
    index over all sets seeds its boxes.  Once per process."""
    if n not in _list_exp:
        rg = reg(n)
        j = 0
        for st in list_sets(n):
            for r in st["rows"]:
                h = LP.play_list(rg.RB, st["games"][r["game"]][:r["ply"]])
                col = rg.RB.board(h)[0]
                player = int(rg.RB.info(h)[1])
                lab, _ = LE.groups_of(col, n)
                r["boxes"] = list_boxes(n, j, r["ko"])
                r["valid"] = [rg._mask(rg.valid_in(h, bx)) for bx in r["boxes"]]
                r["groups"] = [rg.groups_map(col, lab, bx) for bx in r["boxes"]]
                r["cand"] = {t: [rg._mask(rg.cand_in(h, bx, player, t)) for bx in r["boxes"]] for t in list_thresholds(n)}
                rg.RB.free(h)
                j += 1
        _list_exp.add(n)
    return list_sets(n)


# ---- rows of the ld_run test --------------------------------------------------------------------------------------------------------
LD_MAX_STEPS = {19: 48, 9: 40}     # some playouts of every row set are cut, some end by themselves (test_region_cpu.py counts them)
# (playouts, threshold or None for N*N + 1, attackers forced): 5 playouts make rows share a workgroup's group of 4
LD_SETTINGS = ((64, 3, False), (5, 1, True), (5, None, False), (1, 3, True))
_ld_rows = {}


def ld_rows(n):
    """-> list of dict(moves, box, seed, forced (the attacker a forced call names)): 24 19x19 rows at plies 60-250 of the four
    seeded playout games, 48 9x9 rows over the 64 seeded games, with seeded boxes.  At 19x19 every third box is the 8x8 corner."""
    if n not in _ld_rows:
        if not CE._sets:
            CE._sets.update(CE.game_sets())
        rng = np.random.default_rng(40000 + n)
        rows = []
        if n == 19:
            games = CE._sets["playout19"][1]
            for j in range(24):
                g = games[j % len(games)]
                t = int(rng.integers(60, min(250, len(g)) + 1))
                box = (0, 0, 8, 8) if j % 3 == 0 else LE.seeded_box(n, j, rng)
                rows.append(dict(moves=[int(c) for c in g[:t]], box=box))
        else:
            games = CE._sets["nine"][1]
            for j in range(48):
                g = games[j]
                t = int(rng.integers(4, len(g) + 1))
                rows.append(dict(moves=[int(c) for c in g[:t]], box=LE.seeded_box(n, j, rng)))
        for j, r in enumerate(rows):
            r["seed"] = int(rng.integers(1, 1 << 62))
            r["forced"] = 1 + j % 2
        _ld_rows[n] = rows
    return _ld_rows[n]


_ld_exp = {}


def ld_expected(n, setting):
    """-> (info [k, 8], stats [k, 8], first [k, 3, NP + 1], ends per row) of ld_rows(n) under LD_SETTINGS[setting], once per process"""
    key = (n, setting)
    if key not in _ld_exp:
        K, th, forced = LD_SETTINGS[setting]
        th = no_thres(n) if th is None else th
        rg, E = reg(n), ref(n)
        out, ends = [], []
        for r in ld_rows(n):
            e = []
            out.append(rg.ld_row(E, r["moves"], r["seed"], K, th, r["box"], r["forced"] if forced else 0, LD_MAX_STEPS[n], e))
            ends.append(e)
        _ld_exp[key] = (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), ends)
    return _ld_exp[key]


# ---- the straight three in the corner ------------------------------------------------------------------------------------------------
# row = y, column = x, X Black, O White.  Black's three-point eye space (0,0) (1,0) (2,0): Black to move lives at (1,0) and
# nowhere else; White to move kills at (1,0).
STRAIGHT_THREE = [". . . X O . . . .",
                  "X X X X O . . . .",
                  "O O O O O . . . ."]
S3_BOX = (0, 0, 5, 3)
S3_THRES = 3
S3_VITAL, S3_OTHERS = (1, 0), ((0, 0), (2, 0))
S3_SEEDS = (1, 20261021, 0x9E3779B97F4A7C15)


def straight_three(n=9):
    return LP.draw(n, STRAIGHT_THREE)


def box_image(n, s, box):
    """the image of a half-open box under board symmetry s"""
    (x1, y1), (x2, y2) = LP.sym_xy(n, s, box[0], box[1]), LP.sym_xy(n, s, box[2] - 1, box[3] - 1)
    return (min(x1, x2), min(y1, y2), max(x1, x2) + 1, max(y1, y2) + 1)


def s3_images(n=9):
    """the 16 images -> list of dict(s, swapped, stones, box, black (the colour the drawing's X has), vital, others (actions))"""
    out = []
    st = straight_three(n)
    for s, sw, ist, _ in LP.images(n, st, BLACK):
        perm = LP.sym_perm(n, s)
        out.append(dict(s=s, swapped=sw, stones=ist, box=box_image(n, s, S3_BOX), black=WHITE if sw else BLACK,
                        vital=int(perm[S3_VITAL[0] * n + S3_VITAL[1]]), others=[int(perm[x * n + y]) for x, y in S3_OTHERS]))
    return out


def s3_move_list(n=9):
    """the straight three as a legal alternating move list from the empty board, Black first: White has one stone more than Black
    in the drawing, so Black gets filler stones far from the box (bottom-right corner area, two-eyed or not: they never touch the
    box).  -> (moves, stones of the final position); White's stone is the last move, so Black is to move."""
    st = straight_three(n).reshape(n, n).copy()
    b = [(int(x), int(y)) for x, y in zip(*np.nonzero(st == BLACK))]
    w = [(int(x), int(y)) for x, y in zip(*np.nonzero(st == WHITE))]
    filler = [(n - 1, n - 1), (n - 3, n - 1), (n - 1, n - 3), (n - 3, n - 3)]
    while len(b) < len(w):
        x, y = filler.pop(0)
        st[x, y] = BLACK
        b.append((x, y))
    assert len(b) == len(w)
    moves = []
    for pb, pw in zip(b, w):
        moves += [LP.coord(n, *pb), LP.coord(n, *pw)]
    return moves, st.reshape(-1)


S3_PLAYOUTS = 64
# base seeds of the GPU test's rows (row j plays with base + j), chosen so that the reference gives the stated answers on every
# row: about one playout in a hundred that starts at the vital point ends early on a super-ko repeat, with the stones still on
# the board, and a seed under which that happens shows nothing about the reading.  tests/test_region_cpu.py holds the reference
# to the answers under exactly these seeds.
S3_ROW_SEEDS = (1000, 1100)


def s3_rows(n=9):
    """the rows of the GPU test -> list of dict(src (move list or dict(stones, mover)), box, black, vital, others, defends (the
    defender is to move)): the move list with Black and (after a pass) White to move, then the 16 images set up with the
    defender to move, then with the attacker to move"""
    moves, _ = s3_move_list(n)
    base = dict(box=S3_BOX, black=BLACK, vital=S3_VITAL[0] * n + S3_VITAL[1], others=[x * n + y for x, y in S3_OTHERS])
    rows = [dict(base, src=moves, defends=True), dict(base, src=moves + [M_PASS], defends=False)]
    for defends in (True, False):
        for im in s3_images(n):
            rows.append(dict(src=dict(stones=im["stones"], mover=im["black"] if defends else 3 - im["black"]), box=im["box"],
                             black=im["black"], vital=im["vital"], others=im["others"], defends=defends))
    return rows


def s3_holds(row, info, stats, first, K):
    """the stated answers on one row's tensors"""
    v = row["vital"]
    ok = tuple(info[:6]) == tuple(row["box"]) + (3 - row["black"], row["black"]) and info[7] == 0
    ok = ok and info[6] == (row["black"] if row["defends"] else 3 - row["black"])
    ok = ok and first[0].sum() == K and first[0, v] > 0
    if row["defends"]:
        return bool(ok and first[1, v] == first[0, v] and all(first[0, a] > 0 and first[1, a] == 0 for a in row["others"]))
    return bool(ok and first[2, v] == 0)
