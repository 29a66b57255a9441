"""CPU: the instrument of tests/test_gpu_train_df.py (train_df_expected).  A replayed sample has no Info::last_placed; the store
keeps the ply every accepted placement wrote (place_ply, per move) and a sample takes, per point, the maximum over the moves
below its move_to.  These tests prove that rule against the reference's own table on every ply of every game of the three game
sets, pin the counts that make those games a test of it (points played again after a capture, inside one checkpoint interval
and across many; passes), and state the constructed record with refused moves."""
import numpy as np
import pytest

import df_expected as DE
import train_df_expected as TE
from pyoracle import Ref


@pytest.fixture(scope="module")
def ref(built):
    assert Ref.available(9) and Ref.available(19), "build() must have produced oracle/_ref/libelfref{9,19}.so"
    return True


def test_max_rule_rebuilds_last_placed_on_every_stone_of_all_84_games(ref):
    games_seen = stones = 0
    for name in ("nine", "ladder16", "playout19"):
        n, games, exp = DE.all_expected(name)
        for g, mv in enumerate(games):
            pp = TE.place_plies(n, mv)
            # every move of these games is accepted (Df.game asserts it): a placement at move t wrote ply t + 1
            want_pp = np.where(np.asarray(mv) != 0, np.arange(1, len(mv) + 1), 0)
            assert np.array_equal(pp, want_pp), (name, g)
            for t in range(len(mv) + 1):
                on = exp[g]["colour"][t] != 0
                got = TE.placed_from(n, mv, pp, t)
                assert np.array_equal(got[on], exp[g]["placed"][t][on]), (name, g, t)
                stones += int(on.sum())
            games_seen += 1
    assert games_seen == 84 and stones == 981772


def test_counts_that_make_the_game_sets_meaningful(ref):
    """(moves, re-played points, index of the first one, passes) of the five games the GPU test sweeps"""
    got = {}
    for name, g in TE.EVERY_PLY_GAMES:
        n, games = DE.game_set(name)
        k, first, distinct, passes = TE.replays(n, games[g])
        got[name, g] = (len(games[g]), k, first, passes)
    print(got)
    assert got == {("nine", 0): (102, 20, 37, 4), ("nine", 1): (105, 22, 73, 2), ("nine", 2): (111, 27, 69, 3),
                   ("ladder16", 0): (200, 10, 49, 0), ("playout19", 0): (446, 92, 285, 3)}
    # a point is played again inside the checkpoint interval of its first stone, and many intervals later
    n, games = DE.game_set("playout19")
    mv = [int(c) for c in games[0]]
    gaps = [t - max(u for u in range(t) if mv[u] == c) for t, c in enumerate(mv) if c != 0 and c in mv[:t]]
    assert min(gaps) < TE.CK and max(gaps) > 10 * TE.CK
    same = [t for t, c in enumerate(mv) if c != 0 and c in mv[t - t % TE.CK:t]]
    assert same, "a placement is overwritten inside one checkpoint interval"


def test_rows_of_a_whole_game_equal_df_expected(ref):
    """train_df_expected.rows (replay with the skip rule) and df_expected.Df.game (asserting replay) agree where both are defined"""
    n, games, exp = DE.all_expected("nine")
    _, mv, got = TE.every_ply("nine", 1)
    assert np.array_equal(DE.bits(got), DE.bits(exp[1]["planes"]))


def test_refused_moves_do_not_count(ref):
    """the constructed record: a move onto an occupied point, M_INVALID and a pass write no placement ply, and every placement
    behind a refused entry carries the ply that does not count it"""
    n, mv = TE.refused_record_moves()
    pp = TE.place_plies(n, mv)
    assert pp.tolist() == [1, 2, 3, 4, 5, 0, 6, 7, 8, 0, 9, 10, 11, 12, 13, 14, 15, 0, 16, 17, 0] + list(range(19, 30))
    played, before = TE.walk(n, mv, lambda t, s: None)
    assert (~played).nonzero()[0].tolist() == [5, 9, 17]
    D = DE.df(n)
    seen = []

    def visit(t, s):
        on = D.E.board(s)[0] != 0
        assert np.array_equal(TE.placed_from(n, mv, pp, t)[on], D.last_placed(s)[on]), t
        seen.append((int(on.sum()), int(D.E.info(s)[0])))
    TE.walk(n, mv, visit)
    assert seen[-1] == (28, 30)                  # 28 stones, 29 counted plies behind 32 entries
    # the rows: the skip is visible -- the position behind a refused entry is the position in front of it, one entry later
    r = TE.rows(n, mv, [5, 6, 9, 10, 17, 18, 40], [3] * 7)
    assert np.array_equal(r[0], r[1]) and np.array_equal(r[2], r[3]) and np.array_equal(r[4], r[5])
    assert np.array_equal(r[6], TE.rows(n, mv, [len(mv)], [3])[0])
    assert not np.array_equal(r[1], r[2])
