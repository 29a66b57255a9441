"""What elfgo_ladder_map must return, taken from the reference's own ladder reader: checkLadder / checkLadderUseSearch
(base/board.cc:299-524) as exported, under their C++ names, by the unshimmed board library pyoracle.RefBoard loads.  A RefBoard
handle is a plain Board*, which is what these functions take."""
import ctypes as C

import numpy as np

import setup_expected as SE
from pyoracle import Port, RefBoard

MAX_LADDER_SEARCH = 1024   # board.cc:299


class GroupId4(C.Structure):
    """base/board.h:78-85 (Coord = unsigned short, Stone = unsigned char)"""
    _fields_ = [("c", C.c_ushort), ("player", C.c_ubyte), ("ids", C.c_short * 4), ("colors", C.c_ubyte * 4),
                ("group_liberties", C.c_short * 4), ("liberty", C.c_short)]


class _Ids(C.Union):
    _fields_ = [("g", GroupId4), ("raw", C.c_ubyte * 512)]   # the functions get 512 bytes to write into, whatever the layout


class Ladder:
    def __init__(self, n):
        self.n = n
        self.RB = RefBoard(n)
        L = self.RB.L
        self.try_play2 = L["_Z8TryPlay2PK5BoardtP8GroupId4"]
        self.try_play2.restype, self.try_play2.argtypes = C.c_bool, [C.c_void_p, C.c_ushort, C.c_void_p]
        self.check_ladder = L["_Z11checkLadderPK5BoardPK8GroupId4h"]
        self.check_ladder.restype, self.check_ladder.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_ubyte]
        self.search = L["_Z20checkLadderUseSearchP5BoardhPii"]
        self.search.restype, self.search.argtypes = C.c_int, [C.c_void_p, C.c_ubyte, C.POINTER(C.c_int), C.c_int]
        self.coords = [(y + 1) * (n + 2) + (x + 1) for x in range(n) for y in range(n)]   # action a = x*n + y -> Coord

    @staticmethod
    def search_runs(g, player):
        """checkLadder's own test (board.cc:480-510) on the GroupId4 the reference filled in: does it go on to search"""
        if g.liberty != 2:
            return False
        enemies = own = 0
        enemy_three = in_atari = False
        for i in range(4):
            if (g.ids[i] & 0xFF) == 0:          # `unsigned char id`
                continue
            if g.colors[i] == 3 - player:
                enemy_three = enemies == 0 and g.group_liberties[i] >= 3
                enemies += 1
            else:
                in_atari = own == 0 and g.group_liberties[i] == 1
                own += 1
        return enemy_three and in_atari

    def direct(self, h, a, player):
        """-> (depth, num_call) of checkLadderUseSearch on a clone of h after point a has been played"""
        c = self.RB.clone(h)
        assert self.RB.play(c, self.coords[a]) == 1
        nc = C.c_int(0)
        d = self.search(c, player, C.byref(nc), 1)
        self.RB.free(c)
        return d, nc.value

    def expected(self, h):
        """-> (depth int16 [NP], calls int16 [NP]) of Board handle h for its next_player: depth = checkLadder at every
        TryPlay2-legal point; calls = num_call of the direct search at the points where checkLadder's own test passes (there
        the direct search must return checkLadder's depth), 0 elsewhere"""
        player = int(self.RB.info(h)[1])
        np_ = self.n * self.n
        depth, calls = np.zeros(np_, np.int16), np.zeros(np_, np.int16)
        u = _Ids()
        for a, c in enumerate(self.coords):
            if not self.try_play2(h, c, C.byref(u)):
                continue
            d = self.check_ladder(h, C.byref(u), player)
            depth[a] = d
            if self.search_runs(u.g, player):
                d2, nc = self.direct(h, a, player)
                assert d2 == d, (a, d, d2)
                calls[a] = nc
            else:
                assert d == 0, (a, d)
        return depth, calls

    def game(self, moves):
        """expected maps of all len(moves) + 1 positions of a game (row 0 = before the first move)
        -> dict(depth [k+1, NP], calls [k+1, NP], info [k+1, 10])"""
        h = self.RB.new()
        dep, cal, info = [], [], []
        for t in range(len(moves) + 1):
            d, c = self.expected(h)
            dep.append(d)
            cal.append(c)
            info.append(self.RB.info(h))
            if t < len(moves):
                assert self.RB.play(h, int(moves[t])) == 1, "no suite move is refused"
        self.RB.free(h)
        return dict(depth=np.array(dep), calls=np.array(cal), info=np.array(info))


_cache = {}


def games(n):
    """the test inputs: the 115 ladder-suite games (19x19) / 64 seeded playouts (9x9)"""
    return SE.ladder_games() if n == 19 else SE.nine_games(Port(9))


def all_expected(n):
    """-> (move lists, Ladder.game dict per game), computed once per process"""
    if n not in _cache:
        lad = Ladder(n)
        gs = games(n)
        _cache[n] = (gs, [lad.game(mv) for mv in gs])
    return _cache[n]


def statistics(exp):
    """the counts the CPU test pins, over a list of Ladder.game dicts"""
    hist = {}
    positions = with_ladder = searches = nonzero = backtracked = ko_with_ladder = max_calls = 0
    for g in exp:
        positions += len(g["depth"])
        nz = g["depth"] > 0
        with_ladder += int(nz.any(axis=1).sum())
        searches += int((g["calls"] > 0).sum())
        nonzero += int(nz.sum())
        backtracked += int((nz & (g["calls"] > g["depth"])).sum())
        ko_with_ladder += int((SE.ko_pending(g["info"]) & nz.any(axis=1)).sum())
        max_calls = max(max_calls, int(g["calls"].max()))
        for d in g["depth"][nz]:
            hist[int(d)] = hist.get(int(d), 0) + 1
    return dict(positions=positions, with_ladder=with_ladder, searches=searches, nonzero=nonzero, backtracked=backtracked,
                ko_with_ladder=ko_with_ladder, max_calls=max_calls, hist=dict(sorted(hist.items())))
