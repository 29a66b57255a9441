"""GPU: search contexts of a thousand games and more (the benchmarked shape) against the per-game oracle.

Per-game results do not depend on node ids, so game g of a G-game context must reproduce, search for search and bit for bit,
the CPU restatement's single game seeded seed + g (oracle/mcts_oracle.cc, pinned on the reference's fixtures), whatever G is.
What only runs at these sizes: the second and third regime of k_mcts_rowbase (16 waves through wsum[], the 1024-game chunk
loop) and the u64 running row total; a second pass of the mark / sweep grids (more than 8192 x 256 node ids) and a third of
k_mcts_count_live; a thousand waves popping the shared free stacks in one launch; k_mcts_clear_mark with more than one block;
the expansion grid of G x K waves with the row count read on the device; the per-game host work of a move boundary at G > 1000.
tests/test_mcts_scale_cpu.py keeps the comparison discriminating (the games' logs are pairwise distinct)."""
import time

import numpy as np
import pytest

from mcts_scale_cases import (LOCKSTEP, UNEVEN_FORCED, UNEVEN_G, UNEVEN_N, UNEVEN_NODES, UNEVEN_SEARCHES, lockstep_cfg,
                              uneven_cfg)
from sp_drive import drive_stub, oracle_per_game, per_game, sp_from_fixture_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def _logs(sp, n, G):
    rec, coord, visits, prior, reward = sp.search_log()
    na = n * n + 1
    return per_game(rec, coord[:, :na], visits[:, :na], prior[:, :na], reward[:, :na], G)


def _check_pool(sp, actor=0):
    """the node records' invariants, and every node id accounted for: live in a game's tree or free, counted two ways"""
    assert sp.validate_trees()[0] == 0, sp.validate_trees()
    p = sp.pool_info(actor)
    assert p["live"] + p["small_free"] + p["big_free"] == p["small_total"] + p["big_total"], p
    live = sp.count_live(actor)
    assert int(live.sum()) == p["live"], (int(live.sum()), p)
    return live


def _first_difference(got, want, G, searches):
    """None, or (game, search) of the first game whose log differs -- and how many games differ in all: the boundary that
    breaks names the code"""
    bad = [g for g in range(G) if got[g][:searches] != want[g][:searches]]
    if not bad:
        return None
    g = bad[0]
    k = next((k for k in range(searches) if k >= len(got[g]) or got[g][k] != want[g][k]), searches)
    return "game %d search %d; %d of %d games differ (first %s, last %d)" % (g, k, len(bad), G, bad[:8], bad[-1])


_WAITED = {}     # the logs of the lock-step runs that waited for the row count, for the run that does not


def _lockstep_run(elf, n, G, roll, bs, searches, nodes, wait_rows=True):
    cfg = lockstep_cfg(G, roll, bs)
    t0 = time.perf_counter()
    want = oracle_per_game(n, cfg, G, searches)
    t1 = time.perf_counter()
    sp = sp_from_fixture_cfg(elf, n, cfg, log_searches=G * searches, nodes_per_game=nodes)
    rows = drive_stub(sp, n, cfg, lambda sp: sp.progress()["searches"] >= G * searches, wait_rows=wait_rows)
    got = _logs(sp, n, G)
    t2 = time.perf_counter()
    print("n %d G %d: context %d bytes, oracle %.2f s, GPU run %.2f s" % (n, G, elf.tree_bytes_per_game(n, nodes) * G, t1 - t0, t2 - t1))
    assert all(len(got[g]) == searches for g in range(G))
    diff = _first_difference(got, want, G, searches)
    assert diff is None, diff
    live = _check_pool(sp)
    assert live.min() >= 1
    st = sp.stats()
    assert st["moves"] == G * searches
    if wait_rows:
        assert st["rows"] == sum(rows) and sum(rows) > 0     # the u64 running total of the scan against the steps' own counts
    sp.close()
    return got, st


@pytest.mark.parametrize("n,G,roll,bs,searches,nodes", LOCKSTEP)
def test_lockstep_context_equals_the_oracle_game_by_game(elf, n, G, roll, bs, searches, nodes):
    """Every game of the context searching in the same step, persistent trees, Dirichlet noise on.  The sizes are the boundaries
    of the row scan (65: a second wave; 1024 / 1025: one full chunk, one game more; 2111: a partial third chunk, no multiple of
    64) and of the sweep: 2111 games at 1024 node ids each are 2 161 664 small ids, more than the 8192 x 256 the mark and sweep
    grids cover in one pass.  That context takes tree_bytes_per_game(9, 1024) x 2111 = 2 244 057 x 2111 = 4 737 204 327 bytes
    (4.41 GiB, under the 16 GiB at which the other cases would have had to shrink); the others 0.04 to 0.87 GiB."""
    assert elf.tree_bytes_per_game(9, 1024) * 2111 < 16 << 30
    got, st = _lockstep_run(elf, n, G, roll, bs, searches, nodes)
    _WAITED[(n, G)] = (got, st)


def test_device_side_row_count_at_1025_games(elf):
    """begin_step without the host wait: the expansion grid is G x K waves and each reads the row count on the device.  The
    same logs as the run that waits, and as the oracle."""
    case = next(c for c in LOCKSTEP if c[:2] == (9, 1025))
    if case[:2] not in _WAITED:
        _WAITED[case[:2]] = _lockstep_run(elf, *case)
    got, st = _lockstep_run(elf, *case, wait_rows=False)
    assert got == _WAITED[case[:2]][0]
    assert st["rows"] == _WAITED[case[:2]][1]["rows"]


def _uneven_run(elf, G, base=0, on_step=None):
    """G evaluation games (job-wide games base .. base + G - 1), every odd job-wide game one forced move ahead"""
    n, S = UNEVEN_N, UNEVEN_SEARCHES
    cfg = uneven_cfg(G)
    sp = sp_from_fixture_cfg(elf, n, cfg, log_searches=G * (S + 2), nodes_per_game=UNEVEN_NODES, game_idx_base=base)
    forced = np.where((base + np.arange(G)) % 2 == 1, UNEVEN_FORCED, -1).astype(np.int32)
    sp.play(forced)
    n_forced = int((forced >= 0).sum())

    def enough(sp):
        if sp.progress()["searches"] < n_forced + G * S:
            return False
        rec = sp.search_log()[0]
        return np.bincount([x.game for x in rec], minlength=G).min() >= S

    rows = drive_stub(sp, n, cfg, enough, on_step)
    got = _logs(sp, n, G)
    return sp, got, rows


def test_a_forced_move_and_the_oracles_preload_agree_on_the_next_search_only(elf):
    """elfsp_play's partial move list against GameOptions.preload_sgf of the oracle, at G = 4: the first search after the move
    (White's, at ply 1) is the same.  The later ones are not comparable, by design: a game that follows a preloaded SGF is
    finished (FR_MAX_STEP) by the search that finds the list exhausted, so the oracle's game with a one-move list restarts from
    the empty board after its first search, while a game that was forced a move just plays on.  The uneven test below therefore
    takes the odd games' first search from the oracle and their later ones from small contexts."""
    G = 4
    sp, got, _ = _uneven_run(elf, G)
    want = oracle_per_game(UNEVEN_N, uneven_cfg(), UNEVEN_G, UNEVEN_SEARCHES)
    ahead = oracle_per_game(UNEVEN_N, uneven_cfg(), UNEVEN_G, 1, preload=(UNEVEN_FORCED,))
    for g in range(G):
        if g % 2:
            assert got[g][0] == ahead[g][0], "game %d" % g
        else:
            assert got[g][:UNEVEN_SEARCHES] == want[g], "game %d" % g
    sp.close()


def test_out_of_phase_games_with_uneven_rows_equal_the_oracle(elf):
    """1100 evaluation games, Black searching 16 rollouts at 8 per batch (2 steps per move), White 12 at 4 (3 steps), every odd
    game one forced move ahead: even games start with Black's search, odd games with White's, the two populations interleave
    game by game and stay out of phase, so in each AI's context neighbouring games have 0 / 1 / 4 / 8 rows and the scan's prefix
    is not g x constant -- on both sides of game 1024.  Even games against the oracle; odd games' first search against the
    oracle's preload, all their searches against 8-game contexts at 16 places of the 1100 (see the test above for why)."""
    n, G, S = UNEVEN_N, UNEVEN_G, UNEVEN_SEARCHES
    cfg = uneven_cfg()
    t0 = time.perf_counter()
    want = oracle_per_game(n, cfg, G, S)
    ahead = oracle_per_game(n, cfg, G, 1, preload=(UNEVEN_FORCED,))
    t1 = time.perf_counter()
    L = elf.lib()
    actors, both_rows = [], []

    def record(sp, rows_total):
        actors.append([L.elfsp_game_actor(sp._h, g) for g in range(G)])
        both_rows.append(tuple(rows_total))

    sp, got, rows = _uneven_run(elf, G, on_step=record)
    t2 = time.perf_counter()
    print("G %d two AIs: 2 contexts of %d bytes, oracle %.2f s, GPU run %.2f s, %d steps" %
          (G, elf.tree_bytes_per_game(n, UNEVEN_NODES) * G, t1 - t0, t2 - t1, len(actors)))
    # genuinely uneven: at some step games searching with different AIs coexist, below game 1024 and from it on
    a = np.array(actors)
    for lo, hi in ((0, 1024), (1024, G)):
        assert any((row[lo:hi] == 0).any() and (row[lo:hi] == 1).any() for row in a), (lo, hi)
    assert rows[0] > 0 and rows[1] > 0
    diff = _first_difference({g // 2: got[g] for g in range(0, G, 2)}, {g // 2: want[g] for g in range(0, G, 2)}, G // 2, S)
    assert diff is None, "even games (index = game / 2): " + diff
    bad = [g for g in range(1, G, 2) if len(got[g]) < S or got[g][0] != ahead[g][0]]
    assert not bad, "first search of the odd games: %d differ, first %s" % (len(bad), bad[:8])
    for a_ in (0, 1):
        assert _check_pool(sp, a_).min() >= 1
    st = sp.stats()
    assert st["rows"] == sum(rows)
    sp.close()
    # the odd games' later searches: the same job-wide games in contexts of 8
    t3 = time.perf_counter()
    for g0 in (0, 62, 126, 250, 510, 640, 766, 898, 1010, 1016, 1020, 1024, 1030, 1056, 1086, 1092):
        sp8, got8, _ = _uneven_run(elf, 8, base=g0)
        for j in range(8):
            assert got8[j][:S] == got[g0 + j][:S], "game %d against the 8-game context at %d" % (g0 + j, g0)
            if (g0 + j) % 2 == 0:
                assert got8[j][:S] == want[g0 + j]
        sp8.close()
    print("16 contexts of 8 games: %.2f s" % (time.perf_counter() - t3))


def test_clearing_700_scattered_games_at_a_move_boundary(elf):
    """restart() of 700 of 1100 games, scattered over both chunks of the scan, between two searches: k_mcts_clear_mark with three
    blocks, then the sweep.  The cleared games hold a fresh root and nothing else, the others keep every node and go on equal to
    the oracle; a cleared game's next search is a first search of a fresh tree (the all-at-root first batch adds no visit)."""
    n, G, roll, bs, nodes = 9, 1100, 12, 4, 256
    cfg = lockstep_cfg(G, roll, bs)
    want = oracle_per_game(n, cfg, G, 4)
    sp = sp_from_fixture_cfg(elf, n, cfg, log_searches=G * 4, nodes_per_game=nodes)
    drive_stub(sp, n, cfg, lambda sp: sp.stats()["logged"] >= 2 * G)
    assert sp.stats()["logged"] == 2 * G
    before = _check_pool(sp)
    cleared = np.random.default_rng(1100).permutation(G)[:700].astype(np.int32)
    kept = np.setdiff1d(np.arange(G), cleared)
    assert (cleared < 1024).sum() > 100 and (cleared >= 1024).sum() > 10 and len(kept) == 400
    sp.restart(cleared)
    after = _check_pool(sp)
    assert (after[cleared] == 1).all(), after[cleared]
    assert np.array_equal(after[kept], before[kept]) and before[kept].min() >= 1 and before[cleared].max() > 1
    drive_stub(sp, n, cfg, lambda sp: sp.stats()["logged"] >= 4 * G)
    got = _logs(sp, n, G)
    assert all(len(got[g]) == 4 for g in range(G))
    diff = _first_difference({i: got[g] for i, g in enumerate(kept)}, {i: want[g] for i, g in enumerate(kept)}, len(kept), 4)
    assert diff is None, "untouched games (index into the sorted list of them): " + diff
    for g in cleared:
        assert got[g][:2] == want[g][:2], "game %d before it was cleared" % g
        assert got[g][2][3] == roll - bs, "game %d: total visits of the first search after the clear" % g
    assert _check_pool(sp).min() >= 1
    sp.close()
