"""CPU: the instrument of tests/test_gpu_df.py.  df_expected runs the reference's own BoardFeature::extract through a ctypes stand-in
for the BoardFeature object; these tests prove that stand-in (field layout, D4 code) on functions whose answers are known by
another route, pin hand-derived vectors and the statistics of the game set, and check the host-side exponent table of
elfgo_df_exp_table against the C library.  Every comparison is bit equality."""
import ctypes as C

import numpy as np
import pytest

import df_expected as DE
import ownership_expected as OE
from pyoracle import Ref, coord


@pytest.fixture(scope="module")
def ref(built):
    assert Ref.available(9) and Ref.available(19), "build() must have produced oracle/_ref/libelfref{9,19}.so"
    return True


def same(a, b):
    return np.array_equal(DE.bits(a), DE.bits(b))


def play(E, moves):
    s = E.new()
    for c in moves:
        assert E.forward(s, int(c)) == 1
    return s


@pytest.mark.parametrize("n", [9, 19])
def test_stand_in_object_runs_extract_agz_under_every_code(ref, n):
    """extractAGZ through the stand-in equals Ref.extract_agz (which builds a real BoardFeature) for all 8 codes on a mid-game
    position: the field layout and the D4 code are right"""
    D = DE.df(n)
    s, _ = OE.prefix(D.E, 12345, 60 if n == 19 else 30)
    for d4 in range(8):
        assert same(D.agz(s, d4), D.E.extract_agz(s, d4)), d4
    assert not same(D.agz(s, 1), D.agz(s, 0)), "the position is not symmetric: the codes differ"
    D.E.free(s)


@pytest.mark.parametrize("n", [9, 19])
def test_single_getters_equal_the_planes_of_extract(ref, n):
    D = DE.df(n)
    # a live simple ko with White to move, and the same position one move later (the ko point has aged: plane 6 is empty)
    for d4, extra in ((0, []), (5, []), (3, [coord(n, n - 2, n - 3)])):
        s = play(D.E, OE.ko_moves(n) + extra)
        P = D.planes(s, d4)
        me = int(D.E.info(s)[1])
        assert bool(P[6].any()) == (not extra)
        assert same(D.getter("simple_ko", s, me, d4)[0], P[6])
        assert same(D.getter("stones", s, me, d4)[0], P[7])
        assert same(D.getter("stones", s, 3 - me, d4)[0], P[8])
        assert same(D.getter("stones", s, DE.S_EMPTY, d4)[0], P[9])
        assert same(D.getter("liberty3", s, me, d4, planes=3), P[0:3]) and same(D.getter("liberty3", s, 3 - me, d4, planes=3), P[3:6])
        assert same(D.getter("history_exp", s, me, d4)[0], P[10]) and same(D.getter("history_exp", s, 3 - me, d4)[0], P[11])
        assert same(D.getter("distance", s, me, d4)[0], P[14]) and same(D.getter("distance", s, 3 - me, d4)[0], P[15])
        D.E.free(s)


@pytest.mark.parametrize("n", [9, 19])
def test_empty_board(ref, n):
    D = DE.df(n)
    s = D.E.new()
    P = D.planes(s)
    want = np.zeros((25, n, n), np.float32)
    want[9] = 1
    want[14] = want[15] = 10000
    want[16] = 1
    assert same(P, want)
    assert not D.last_placed(s).any()
    D.E.free(s)


def test_one_black_stone_seen_by_white(ref):
    n = 9
    D = DE.df(n)
    s = play(D.E, [coord(n, 2, 2)])
    P = D.planes(s)
    a = np.zeros((n, n), np.float32)
    a[2, 2] = 1
    want = np.zeros((25, n, n), np.float32)
    want[8] = a            # the opponent's (Black's) stone
    want[5] = a            # four liberties: the ">= 3" class
    want[9] = 1 - a
    want[11] = a * DE.libm_exp_table(n)[1]   # placed at ply 1, seen at ply 2
    xs, ys = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    want[15] = np.abs(xs - 2) + np.abs(ys - 2)
    want[14] = 10000
    want[17] = 1
    assert same(P, want)
    assert DE.bits(P[11, 2, 2]) == DE.bits(DE.libm_exp_table(n)[1])
    lp = D.last_placed(s)
    assert lp[2 * n + 2] == 1 and lp.sum() == 1
    D.E.free(s)


@pytest.mark.parametrize("n", [9, 19])
def test_ko_point_under_every_code(ref, n):
    """ownership_expected.ko_moves: White faces a live simple ko at (1,0)"""
    from elf_amd.engine import d4_transform
    D = DE.df(n)
    s = play(D.E, OE.ko_moves(n))
    for d4 in range(8):
        want = np.zeros((n, n), np.float32)
        want[d4_transform(n, d4, 1, 0)] = 1
        assert same(D.planes(s, d4)[6], want), d4
    D.E.free(s)


def test_statistics_of_the_nine_by_nine_games(ref):
    n, games, exp = DE.all_expected("nine")
    st = DE.statistics(n, games, exp)
    print(st)
    assert st == dict(positions=7055, ko=60, far_maps=230, largest_finite=16, passes=229,
                      plane_sums=[17705, 26220, 113294, 18006, 25581, 118980])


@pytest.mark.parametrize("n", [9, 19])
def test_exp_table_is_the_c_librarys(built, n):
    import elf_amd
    L = elf_amd.lib()
    tab = np.full(2 * n * n + 1, np.nan, np.float32)
    assert L.elfgo_df_exp_table(n, tab.ctypes.data) == 0
    assert same(tab, DE.libm_exp_table(n))
    assert tab[0] == 1.0 and (np.diff(tab) < 0).all()
    assert L.elfgo_df_exp_table(13, tab.ctypes.data) == -2 and L.elfgo_df_exp_table(n, None) == -1


def test_every_history_value_of_the_games_is_in_the_table(ref):
    """planes 10 / 11 of every position of `nine` hold table[ply - last_placed] under every stone: what the kernel looks up"""
    import elf_amd
    from elf_amd.engine import d4_transform
    n, games, exp = DE.all_expected("nine")
    tab = np.zeros(2 * n * n + 1, np.float32)
    assert elf_amd.lib().elfgo_df_exp_table(n, tab.ctypes.data) == 0
    perm = {d4: np.array([np.ravel_multi_index(d4_transform(n, d4, x, y), (n, n)) for x in range(n) for y in range(n)]) for d4 in range(8)}
    checked = 0
    for g, e in enumerate(exp):
        for t in range(len(e["planes"])):
            ply, col, lp = int(e["info"][t, 0]), e["colour"][t], e["placed"][t]
            assert ply == t + 1
            stones = np.nonzero(col)[0]
            hist = (e["planes"][t, 10] + e["planes"][t, 11]).reshape(-1)     # disjoint supports
            got = hist[perm[DE.code_of(g, t)][stones]]
            assert same(got, tab[ply - lp[stones]]), (g, t)
            checked += len(stones)
    assert checked > 100000
