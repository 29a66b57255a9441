"""CPU: the inputs of tests/test_gpu_ownership_edges.py are what that file takes them to be -- conditions on the reference side
alone, checked before anything on the device is compared with it."""
import numpy as np
import pytest

import ownership_expected as oe
from pyoracle import playout_seeds

AREA_TEST_PLIES = {9: (20, 40), 19: (60, 200)}      # test_gpu_ownership.test_area_map's


@pytest.mark.parametrize("n", [9, 19])
def test_two_area_maps_agree_on_the_shapes(n):
    """the queue-labelled components and the masked dilation give one map for every constructed shape, every group has a
    liberty, and the named points are where the names say"""
    sh = oe.shapes(n)
    assert len(sh) >= 17
    for name, col in sh.items():
        assert col.shape == (n * n,) and col.dtype == np.uint8 and col.max(initial=0) <= 2, name
        assert oe.groups_have_liberties(col, n), name
        assert np.array_equal(oe.area_map_bfs(col, n), oe.area_map(col, n)), name
    assert not sh["empty"].any() and not oe.area_map_bfs(sh["empty"], n).any()
    assert (oe.area_map_bfs(sh["black_corner"], n) == 1).all() and (oe.area_map_bfs(sh["white_centre"], n) == 2).all()
    assert (oe.area_map_bfs(sh["comb"], n) == 1).all() and (oe.area_map_bfs(sh["full_but_one"], n) == 1).all()
    for name in ("dame_x", "dame_y"):           # the line is neutral, point for point, and nothing else is
        am = oe.area_map_bfs(sh[name], n)
        assert np.array_equal(am == 0, sh[name] == 0) and (am == 0).sum() == n
    for name in ("snake", "snake_T", "snake_swapped", "spiral", "comb_white", "borders"):     # both colours reach every empty point
        assert np.array_equal(oe.area_map_bfs(sh[name], n), sh[name]), name
    assert oe.word_rows(19)[:2] == [3, 6] and oe.word_rows(9) == [7]


def test_area_map_bfs_tells_colours_apart():
    """a position the two formulations could both get wrong the same way only by accident: three regions, one per answer"""
    n = 9
    g = np.zeros((n, n), np.uint8)
    g[2, :] = 1                      # rows 0-1 black's
    g[6, :] = 2                      # rows 7-8 white's, rows 3-5 neutral
    want = g.copy()
    want[:2] = 1
    want[7:] = 2
    assert np.array_equal(oe.area_map_bfs(g.reshape(-1), n), want.reshape(-1))
    assert np.array_equal(oe.area_map(g.reshape(-1), n), want.reshape(-1))


def test_the_battery_is_as_hard_as_claimed(built):
    """trips of the kernel's fixed-point loop: the snake and the spiral each reach at least 100 (19x19) and 30 (9x9) in one of
    their two orientations -- corridors along a row or across rows -- while the positions of test_area_map, played to the end or not, stay within 8
    (its one position of fewer than 20 plies within n)"""
    for n, least in ((19, 100), (9, 30)):
        trips = {name: oe.kernel_trips(col, n) for name, col in oe.shapes(n).items()}
        print(n, trips)
        assert max(trips["snake"], trips["snake_T"]) >= least and max(trips["spiral"], trips["spiral_T"]) >= least
        assert trips["snake_T"] > 3 * trips["snake"] // 2         # a vertical step costs a trip, an in-row run a sixth of one
        E = oe.oracle(n)
        lists = oe.area_test_lists(E, n, AREA_TEST_PLIES[n])
        states = oe.states_of(E, lists)
        old = [oe.kernel_trips(E.board(s)[0], n) for s in states]
        for s, sd in zip(states, playout_seeds(len(lists), base=500)):
            E.playout_moves(s, int(sd))
            old.append(oe.kernel_trips(E.board(s)[0], n))
            E.free(s)
        print(n, "test_area_map's positions, then the same played out:", old)
        # Positions of 20 plies and more, and all the played-out ones: within 8.  The one shorter position (10 plies of the ladder
        # game, 19x19) takes 16: ten stones on an open board, across which a fill gains at least a row per trip -- at most n.
        sparse = [i for i, mv in enumerate(lists) if 0 < len(mv) < 20]
        assert len(sparse) <= 1 and all(old[i] <= n for i in sparse)
        assert 2 <= max(t for i, t in enumerate(old) if i not in sparse) <= 8


def test_kernel_trips_counts_the_unchanged_trip():
    n = 9
    assert oe.kernel_trips(np.zeros(n * n, np.uint8), n) == 1                 # nothing to spread: the one trip that finds that out
    g = np.zeros((n, n), np.uint8)
    g[0, 0] = 1
    assert oe.kernel_trips(g.reshape(-1), n) == n                             # one row per trip for 8 trips, and the unchanged one
    g[:] = 0
    g[:8, :] = 2                     # White is done after one trip; Black walks along the last row, six points per trip
    g[8, :3] = 1
    assert oe.kernel_trips(g.reshape(-1), n) == 2                             # six empty points: all in the first trip
    g[8, 2] = 0
    assert oe.kernel_trips(g.reshape(-1), n) == 3                             # seven: the last one in the second


@pytest.mark.parametrize("n", [9, 19])
def test_moves_for_replays_to_the_shape(built, n):
    E = oe.oracle(n)
    for name, col in oe.shapes(n).items():
        mv = oe.moves_for(col, n)
        assert all(a or b for a, b in zip(mv, mv[1:])), name                 # never two passes in a row
        s = E.new()
        for c in mv:
            assert E.forward(s, c) == 1, name
        assert np.array_equal(E.board(s)[0], col), name
        assert not E.terminated(s), name
        E.free(s)


def test_the_step_limit_row_is_mixed(built):
    E = oe.oracle(9)
    row = oe.STEP_ROW
    src, _ = oe.row_source(E, row)
    cut = [ln for _, ln in oe.playout_diffs(E, src, row["seed"], row["K"], row["max_steps"])]
    full = [ln for _, ln in oe.playout_diffs(E, src, row["seed"], row["K"])]
    print(cut, full)
    assert max(cut) == row["max_steps"] and min(cut) < row["max_steps"]
    assert sum(c == row["max_steps"] for c in cut) >= 1 and sum(c < row["max_steps"] for c in cut) >= 1
    assert all(c == min(f, row["max_steps"]) for c, f in zip(cut, full))
    assert len(set(ln for _, ln in oe.playout_diffs(E, src, row["seed"], row["K"], 1))) == 1      # a cut at 1 cuts them all
    E.free(src)


def test_the_tie_row_has_a_tie(built):
    """with komi = the area difference of playout 0, that playout (at least) has diff == komi: no win; some others win, some lose"""
    E = oe.oracle(9)
    row = oe.TIE_ROW
    src, _ = oe.row_source(E, row)
    diffs = [d for d, _ in oe.playout_diffs(E, src, row["seed"], row["K"])]
    d0 = diffs[0]
    assert sum(d == d0 for d in diffs) >= 1 and any(d > d0 for d in diffs) and any(d < d0 for d in diffs)
    _, ws = oe.expected(E, src, row["seed"], row["K"], float(d0))
    assert ws[1] == sum(d > d0 for d in diffs) < sum(d >= d0 for d in diffs)
    assert max(diffs) == 81 and min(diffs) > -81         # komi 81 is a tie for a board all black's; komi -81 is a win for every playout
    E.free(src)


def test_the_superko_source_ends_by_superko(built):
    E = oe.oracle(9)
    game = oe.superko_source(E)
    s = E.new()
    for c in game:
        assert not E.terminated(s) and E.forward(s, c) == 1
    assert E.terminated(s) and oe.ended_by_superko(E, s)
    assert game[-1] != 0 and game[-2:] != [0, 0]          # the last move is a stone: it is the repeat that ends the game
    assert E.playout_moves(s, 5).size == 0                # and a playout from there plays nothing
    E.free(s)
    # one move short of the end, playouts often open with that very move: an ending decided by the source's own records
    s = oe.replay(E, game[:-1])
    at_once = 0
    for sd in playout_seeds(16, base=6000):
        c = E.clone(s)
        at_once += int(len(E.playout_moves(c, int(sd))) == 1 and oe.ended_by_superko(E, c))
        E.free(c)
    assert 4 <= at_once <= 12
    E.free(s)


def test_the_geometry_rows_have_both_signs(built):
    """the seven rows of the geometry sweep: among the expected stats[0] there is a negative and a positive one for every K"""
    E = oe.oracle(9)
    states = oe.states_of(E, oe.mixed_rows(E, 9))
    for K in oe.GEOMETRY_K:
        s0 = [int(oe.expected(E, states[i], sd, K, 7.5)[1][0]) for i, sd in zip(oe.GEOMETRY_IDS, oe.geometry_seeds())]
        assert min(s0) < 0 < max(s0), (K, s0)
