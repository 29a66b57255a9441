"""What elfgo_df_extract / elfgo_df_placed must return, taken from the reference's own BoardFeature::extract
(base/board_feature.cc:43-237) as exported, under its C++ name, by the reference library pyoracle.Ref loads.

A BoardFeature is four fields in 32 bytes (board_feature.h:152-158): `const GoState& s_`, `Rot _rot`, `bool _flip` and a
shared_ptr logger that extract and the single getters never touch.  A pyoracle.Ref handle is a GoState*, so a ctypes structure of
that layout passed as `this` runs the reference's member functions under any D4 code; tests/test_df_cpu.py proves the layout by
calling extractAGZ the same way and comparing with Ref.extract_agz."""
import ctypes as C

import numpy as np

import candidates_expected as CE
from pyoracle import Ref

PLANES = 25
S_EMPTY, S_BLACK, S_WHITE = 0, 1, 2
FAR = np.float32(10000.0)   # getDistanceMap's value where the colour has no stone


class BoardFeature(C.Structure):
    _fields_ = [("s", C.c_void_p), ("rot", C.c_int), ("flip", C.c_bool), ("logger", C.c_void_p * 2)]


assert C.sizeof(BoardFeature) == 32

_GETTERS = {"liberty3": "_ZNK12BoardFeature20getLibertyMap3binaryEhPf", "stones": "_ZNK12BoardFeature9getStonesEhPf",
            "simple_ko": "_ZNK12BoardFeature11getSimpleKoEhPf", "history": "_ZNK12BoardFeature10getHistoryEhPf",
            "history_exp": "_ZNK12BoardFeature13getHistoryExpEhPf", "distance": "_ZNK12BoardFeature14getDistanceMapEhPf"}


class Df:
    def __init__(self, n):
        self.n = n
        self.E = Ref(n)
        L = self.E.L
        self._extract = L["_ZNK12BoardFeature7extractEPf"]
        self._agz = L["_ZNK12BoardFeature10extractAGZEPf"]
        for f in (self._extract, self._agz):
            f.restype, f.argtypes = None, [C.c_void_p, C.c_void_p]
        self._get = {}
        for k, sym in _GETTERS.items():
            f = L[sym]
            f.restype, f.argtypes = C.c_bool, [C.c_void_p, C.c_ubyte, C.c_void_p]
            self._get[k] = f

    @staticmethod
    def feature(state, d4):
        """BoardFeature(state) after setD4Code(d4) (board_feature.h:88-92)"""
        return BoardFeature(state, d4 % 4, (d4 >> 2) == 1, (C.c_void_p * 2)())

    def planes(self, state, d4=0):
        """BoardFeature::extract -> float32 [25, n, n]"""
        out = np.full((PLANES, self.n, self.n), np.nan, np.float32)
        bf = self.feature(state, d4)
        self._extract(C.byref(bf), out.ctypes.data)
        return out

    def agz(self, state, d4=0):
        """BoardFeature::extractAGZ through the stand-in object -> float32 [18, n, n]"""
        out = np.full((18, self.n, self.n), np.nan, np.float32)
        bf = self.feature(state, d4)
        self._agz(C.byref(bf), out.ctypes.data)
        return out

    def getter(self, name, state, player, d4=0, planes=1):
        """one of the single getters -> float32 [planes, n, n] (getDistanceMap writes every element, the others clear first)"""
        out = np.full((planes, self.n, self.n), np.nan, np.float32)
        bf = self.feature(state, d4)
        self._get[name](C.byref(bf), int(player), out.ctypes.data)
        return out

    def last_placed(self, state):
        """Info::last_placed of every point, action order: getHistory(S_EMPTY, ...) under code 0 returns every point's entry"""
        return self.getter("history", state, S_EMPTY)[0].reshape(-1).astype(np.int64)

    def game(self, moves, code_of=lambda t: 0):
        """the answers at all len(moves) + 1 positions of a game (row 0 = before the first move)
        -> dict(planes [k+1, 25, n, n] under code_of(t), placed [k+1, NP], colour [k+1, NP], info [k+1, 10])"""
        E = self.E
        s = E.new()
        pl, lp, col, info = [], [], [], []
        for t in range(len(moves) + 1):
            pl.append(self.planes(s, code_of(t)))
            lp.append(self.last_placed(s))
            col.append(E.board(s)[0])
            info.append(E.info(s))
            if t < len(moves):
                assert E.forward(s, int(moves[t])) == 1
        E.free(s)
        return dict(planes=np.array(pl), placed=np.array(lp), colour=np.array(col), info=np.array(info))


_df, _sets, _games = {}, {}, {}


def df(n):
    if n not in _df:
        _df[n] = Df(n)
    return _df[n]


def code_of(game, ply):
    return (game + ply) % 8


def game_set(name):
    """-> (n, move lists) of candidates_expected.game_sets(): nine, ladder16, playout19"""
    if not _sets:
        _sets.update(CE.game_sets())
    return _sets[name]


def all_expected(name):
    """-> (n, move lists, Df.game dict per game with code (game + ply) % 8), computed once per process"""
    if name not in _games:
        n, gs = game_set(name)
        _games[name] = (n, gs, [df(n).game(mv, lambda t, g=g: code_of(g, t)) for g, mv in enumerate(gs)])
    return _games[name]


def libm_exp_table(n):
    """float32(libm exp(-d / 10.0)) for d in [0, 2 n*n]: the C library's double exp, not numpy's own"""
    m = C.CDLL("libm.so.6")
    m.exp.restype, m.exp.argtypes = C.c_double, [C.c_double]
    return np.array([m.exp((0 - d) / 10.0) for d in range(2 * n * n + 1)], np.float64).astype(np.float32)


def statistics(n, games, exp):
    """the counts the CPU test pins over a list of Df.game dicts"""
    pl = [g["planes"] for g in exp]
    far = sum(int((p[:, 14] == FAR).all(axis=(1, 2)).sum()) + int((p[:, 15] == FAR).all(axis=(1, 2)).sum()) for p in pl)
    finite = max(float(p[:, 14:16][p[:, 14:16] < FAR].max()) for p in pl)
    return dict(positions=sum(len(p) for p in pl), ko=sum(int(p[:, 6].any(axis=(1, 2)).sum()) for p in pl), far_maps=far,
                largest_finite=int(finite), passes=sum(int((np.asarray(m) == 0).sum()) for m in games),
                plane_sums=[int(sum(float(p[:, k].sum()) for p in pl)) for k in range(6)])


def bits(a):
    """float32 array -> its uint32 image (every comparison of planes is bit equality)"""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def numpy_planes(n, colour, libs, player, d4=0):
    """planes 0-9 and 14-17 read off an export_board (colour, libs in action order) with numpy alone; the others stay 0
    -> float32 [25, n, n] under D4 code d4"""
    col = np.asarray(colour).reshape(n, n)
    lib = np.asarray(libs).reshape(n, n)
    opp = 3 - player
    src = np.zeros((PLANES, n, n), np.float32)
    for base, who in ((0, player), (3, opp)):
        src[base + 0] = (col == who) & (lib == 1)
        src[base + 1] = (col == who) & (lib == 2)
        src[base + 2] = (col == who) & (lib >= 3)
    src[7], src[8], src[9] = col == player, col == opp, col == 0
    xs, ys = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for plane, who in ((14, player), (15, opp)):
        pts = np.argwhere(col == who)
        if len(pts) == 0:
            src[plane] = FAR
        else:
            src[plane] = np.min(np.abs(xs[None] - pts[:, 0, None, None]) + np.abs(ys[None] - pts[:, 1, None, None]), axis=0)
    src[16 if player == S_BLACK else 17] = 1.0
    return transform_planes(n, src, d4)


def transform_planes(n, src, d4):
    """out[p, Transform(x, y)] = src[p, x, y] (board_feature.h:97-113, :160-163)"""
    from elf_amd.engine import d4_transform
    out = np.empty_like(src)
    for x in range(n):
        for y in range(n):
            tx, ty = d4_transform(n, d4, x, y)
            out[:, tx, ty] = src[:, x, y]
    return out
