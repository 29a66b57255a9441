"""GPU: the edges of k_area_map and k_playout_own (elf_amd/csrc/ownership.cuh, launched from ownership_host.h) -- long flood fills
on constructed shapes, the deal of (row, playout) pairs to waves and workgroups, the step limit, the record-prefix cache, the win
count at a tie, special sources, argument refusals and stream order.  Expected values come from the CPU oracle's playouts and from
ownership_expected.area_map_bfs; tests/test_ownership_edges_cpu.py checks the inputs.  Every comparison is integer equality."""
import numpy as np
import pytest

import ownership_expected as oe
from ownership_expected import oracle, play_all, states_of
from pyoracle import playout_seeds

pytestmark = pytest.mark.gpu

ELFGO_E_BADARG = -1
EMPTY, MID, LATE, KO, DONE, STEP = range(6)          # the slots of `six`


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def npy(t):
    return t.cpu().numpy()


def snapshot(eng, ids=None):
    col, lib = eng.export_board(ids)
    return [npy(t) for t in (eng.info(ids), col, lib, eng.legal_mask(ids))]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def run(eng, seeds, **kw):
    own = eng.ownership(seeds, **kw)
    return npy(own["counts"]), npy(own["stats"])


@pytest.fixture(scope="module")
def six(elf):
    """a 9x9 engine of six slots -- the five mixed rows and the step-limit row's source -- with the oracle's states of the same"""
    E = oracle(9)
    lists = oe.mixed_rows(E, 9) + [oe.row_source(E, oe.STEP_ROW)[1]]
    eng = elf.GoEngine(9, len(lists), 0)
    play_all(eng, lists)
    states = states_of(E, lists)
    assert int(E.info(states[KO])[5]) != 0 and int(E.info(states[KO])[4]) == 0 and E.terminated(states[DONE])
    before = snapshot(eng)
    yield eng, E, states
    assert same(before, snapshot(eng))               # no test below changes a slot of this engine
    eng.close()


def expected_rows(E, states, ids, seeds, K, komi=7.5, max_steps=100000):
    both = [oe.expected(E, states[i], sd, K, komi, max_steps) for i, sd in zip(ids, seeds)]
    return np.stack([c for c, _ in both]), np.stack([s for _, s in both])


# ---- 1. area map of constructed shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 19])
def test_area_map_of_constructed_shapes(elf, n):
    """every shape set up in a slot of its own: the area map equals the queue-labelled one (the snakes and spirals take the fill's
    loop through 41 / 181 trips), evaluate follows from it, and k_playout_own's copy of the fill, reached with max_steps = 0, counts
    the same map K times over"""
    sh = oe.shapes(n)
    names = list(sh)
    stones = np.stack([sh[k] for k in names])
    want = np.stack([oe.area_map_bfs(c, n) for c in stones])
    diff = np.array([oe.area_diff(a) for a in want])
    eng = elf.GoEngine(n, len(names), 0)
    assert (npy(eng.setup(stones)) == 1).all()
    am = npy(eng.area_map())
    assert [k for i, k in enumerate(names) if not np.array_equal(am[i], want[i])] == []
    for komi in (7.5, 0.0):
        assert np.array_equal(npy(eng.evaluate(komi=komi)), (diff - komi).astype(np.float32)), komi
    K = 3
    for lanes in (0, 1):
        counts, stats = run(eng, playout_seeds(len(names)), playouts=K, max_steps=0, max_lanes=lanes)
        bad = [k for i, k in enumerate(names) if not (np.array_equal(counts[i, 0], K * (want[i] == 1)) and
                                                      np.array_equal(counts[i, 1], K * (want[i] == 2)) and
                                                      stats[i].tolist() == [K * diff[i], K * int(diff[i] - 7.5 > 0), 0, 0])]
        assert bad == [], lanes
    eng.close()


@pytest.mark.parametrize("n", [9, 19])
def test_area_map_of_shapes_through_ragged_ids(elf, n):
    """the shapes three at a time in slots 5, 0 and 3 of an engine of eight, listed in that order"""
    sh = oe.shapes(n)
    names = list(sh)
    ids = [5, 0, 3]
    eng = elf.GoEngine(n, 8, 0)
    for j in range(0, len(names), 3):
        part = names[j:j + 3]
        use = ids[:len(part)]
        assert (npy(eng.setup(np.stack([sh[k] for k in part]), ids=use)) == 1).all()
        am = npy(eng.area_map(use))
        want = [oe.area_map_bfs(sh[k], n) for k in part]
        assert [k for r, k in enumerate(part) if not np.array_equal(am[r], want[r])] == []
        for komi in (7.5, 0.0):
            val = npy(eng.evaluate(use, komi))
            assert val.tolist() == [oe.area_diff(w) - komi for w in want], (part, komi)
    assert not npy(eng.export_board([1, 2, 4, 6, 7])[0]).any()          # the slots that were not listed stayed empty
    eng.close()


@pytest.mark.parametrize("n", [9, 19])
def test_area_map_of_shapes_that_were_played(elf, n):
    """the same shapes reached move by move (moves_for): slots with a history give the same maps"""
    sh = oe.shapes(n)
    names = list(sh)
    eng = elf.GoEngine(n, len(names), 0)
    play_all(eng, [oe.moves_for(sh[k], n) for k in names])
    assert np.array_equal(npy(eng.export_board()[0]), np.stack([sh[k] for k in names]))
    am = npy(eng.area_map())
    assert [k for i, k in enumerate(names) if not np.array_equal(am[i], oe.area_map_bfs(sh[k], n))] == []
    eng.close()


# ---- 2. geometry sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", oe.GEOMETRY_K)
def test_geometry_sweep(six, K):
    """seven rows and K playouts each on one workgroup, two, three and one per group of four pairs: groups straddle rows and
    workgroup boundaries fall inside rows, and counts and stats are the oracle's whatever the deal"""
    eng, E, states = six
    ids, seeds = oe.GEOMETRY_IDS, oe.geometry_seeds()
    wc, ws = expected_rows(E, states, ids, seeds, K)
    assert ws[:, 0].min() < 0 < ws[:, 0].max()
    for lanes in oe.GEOMETRY_LANES:
        counts, stats = run(eng, seeds, ids=ids, playouts=K, max_lanes=lanes)
        for r in range(len(ids)):
            assert np.array_equal(counts[r], wc[r]), (K, lanes, r)
            assert np.array_equal(stats[r], ws[r]), (K, lanes, r, stats[r].tolist(), ws[r].tolist())


def test_geometry_19(elf):
    n, K = 19, 5
    E = oracle(n)
    lists = oe.mixed_rows(E, n)[1:4]                 # mid game, late game, the simple ko
    eng = elf.GoEngine(n, 3, 0)
    play_all(eng, lists)
    states = states_of(E, lists)
    seeds = oe.geometry_seeds(3)
    wc, ws = expected_rows(E, states, range(3), seeds, K)
    counts, stats = run(eng, seeds, playouts=K, max_lanes=8)
    assert np.array_equal(counts, wc) and np.array_equal(stats, ws)
    eng.close()


# ---- 3. slot switching -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids,K", [([LATE, EMPTY, MID, DONE, KO, STEP, EMPTY, MID, LATE, DONE, STEP, MID], 1),
                                   ([LATE, EMPTY, LATE, KO, LATE, EMPTY], 2),
                                   (None, 3)])
def test_slot_switching_on_one_workgroup(six, ids, K):
    """max_lanes = 1 is one workgroup of four waves.  In the first list wave 0 plays rows 0, 4 and 8 -- the late game (a long
    record prefix), the ko (five records), the late game again -- and every other wave changes slot at each step as well; in the
    second every wave alternates; ids = None is row = slot.  The record prefix a wave holds must be the current slot's."""
    eng, E, states = six
    rows = list(range(6)) if ids is None else ids
    if len(rows) == 12:
        assert rows[0] == rows[8] == LATE and rows[4] == KO
        assert int(E.info(states[LATE])[0]) > 5 * int(E.info(states[KO])[0])
    seeds = playout_seeds(len(rows), base=3000 + 100 * K)
    wc, ws = expected_rows(E, states, rows, seeds, K)
    before = snapshot(eng)
    counts, stats = run(eng, seeds, ids=ids, playouts=K, max_lanes=1)
    assert np.array_equal(counts, wc) and np.array_equal(stats, ws)
    assert same(before, snapshot(eng))


def test_both_policies_run_one_harness(six):
    """self_atari_thres = 82 is above 9 * 9, so the candidate policy drops nothing: k_playout_own<N, CandPolicy> must return the
    counts and stats of k_playout_own<N, EyePolicy>, and the oracle's, bit for bit -- where groups straddle two rows (the
    geometry rows at K = 3 under every deal) and where every wave changes slot between playouts (the twelve rows on one workgroup)"""
    eng, E, states = six
    switching = [LATE, EMPTY, MID, DONE, KO, STEP, EMPTY, MID, LATE, DONE, STEP, MID]
    cases = [(oe.GEOMETRY_IDS, oe.geometry_seeds(), 3, lanes) for lanes in oe.GEOMETRY_LANES]
    cases.append((switching, playout_seeds(len(switching), base=3100), 1, 1))
    for ids, seeds, K, lanes in cases:
        wc, ws = expected_rows(E, states, ids, seeds, K)
        eye = run(eng, seeds, ids=ids, playouts=K, max_lanes=lanes)
        cand = run(eng, seeds, ids=ids, playouts=K, max_lanes=lanes, self_atari_thres=82)
        for got in (eye, cand):
            assert np.array_equal(got[0], wc) and np.array_equal(got[1], ws), (K, lanes)


def test_out_of_pool_ids_are_not_played(six):
    """A row whose slot id lies outside the pool is not played (elfgo_ld_run's rule): its counts and stats stay zero and the rows
    around it are the oracle's.  Out-of-pool rows stand first and last, between two rows of the late game (with K = 3 on one
    workgroup wave 3 plays pairs 3, 7 and 11 -- late game, skipped, late game -- so the record prefix it holds must survive the
    skip) and between rows of two different slots; groups of four pairs straddle in-pool and out-of-pool rows both ways."""
    eng, E, states = six
    cap, K = eng.capacity, 3
    ids = [cap, LATE, -1, LATE, MID, cap + 7, KO, EMPTY, cap, STEP, DONE, -1]
    live = [r for r, b in enumerate(ids) if 0 <= b < cap]
    dead = [r for r in range(len(ids)) if r not in live]
    assert len(live) == 7 and dead == [0, 2, 5, 8, 11]
    seeds = playout_seeds(len(ids), base=7000)
    wc, ws = expected_rows(E, states, [ids[r] for r in live], seeds[live], K)
    assert ws[:, 3].max() > 0                        # the in-pool rows are played
    before = snapshot(eng)
    for thres in (None, 82):
        for lanes in (1, 0):
            counts, stats = run(eng, seeds, ids=ids, playouts=K, max_lanes=lanes, self_atari_thres=thres)
            for j, r in enumerate(live):
                assert np.array_equal(counts[r], wc[j]), (thres, lanes, r)
                assert np.array_equal(stats[r], ws[j]), (thres, lanes, r, stats[r].tolist(), ws[j].tolist())
            assert not counts[dead].any() and not stats[dead].any(), (thres, lanes)
    assert same(before, snapshot(eng))


def test_record_prefix_decides_the_playout(elf):
    """Sources whose records matter at once: the super-ko game one move short of its end, where about every other playout opens
    with the move that repeats a position of the game's own history (an ending by super-ko after one step -- found only in the
    records the wave holds), dealt to the four waves of one workgroup between rows of the late game, whose playouts write their
    own records over the tail of the wave's record area.  Each wave sees late, short, late, short, or the other way round."""
    n, K = 9, 1
    E = oracle(n)
    lists = [oe.mixed_rows(E, n)[LATE], oe.superko_source(E)[:-1]]
    assert len(lists[1]) > len(lists[0])             # the late game's playouts write where the longer game's records lie
    eng = elf.GoEngine(n, 2, 0)
    play_all(eng, lists)
    states = states_of(E, lists)
    for ids in ([0] * 4 + [1] * 4 + [0] * 4 + [1] * 4, [1] * 4 + [0] * 4 + [1] * 4 + [0] * 4):
        seeds = playout_seeds(len(ids), base=6000 + 4 * ids[0])          # the short rows get the same seeds in either order
        wc, ws = expected_rows(E, states, ids, seeds, K)
        at_once = [r for r, i in enumerate(ids) if i == 1 and ws[r, 2] == 1 and ws[r, 3] == 1]
        assert 2 <= len(at_once) <= 6, at_once       # some of the eight short rows end on the repeat at once, some do not
        assert {r // 8 for r in at_once} == {0, 1}   # in a wave's first visit to the slot and in its second
        counts, stats = run(eng, seeds, ids=ids, playouts=K, max_lanes=1)
        assert np.array_equal(stats, ws), (stats.tolist(), ws.tolist())
        assert np.array_equal(counts, wc)
    eng.close()


# ---- 4. step limit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", [0, 1, oe.STEP_ROW["max_steps"], None])
def test_step_limit(six, max_steps):
    """a row of which the limit of 60 cuts some playouts and not others; a limit of 0 plays nothing: K times the source's map"""
    eng, E, states = six
    K, seed = oe.STEP_ROW["K"], np.array([oe.STEP_ROW["seed"]], np.uint64)
    kw = {} if max_steps is None else dict(max_steps=max_steps)
    wc, ws = oe.expected(E, states[STEP], seed[0], K, 7.5, **kw)
    counts, stats = run(eng, seed, ids=[STEP], playouts=K, **kw)
    assert np.array_equal(counts[0], wc) and np.array_equal(stats[0], ws), (stats[0].tolist(), ws.tolist())
    if max_steps is not None:
        assert stats[0, 3] <= K * max_steps
    if max_steps == 0:
        am = oe.area_map_bfs(E.board(states[STEP])[0], 9)
        assert np.array_equal(counts[0, 0], K * (am == 1)) and np.array_equal(counts[0, 1], K * (am == 2)) and stats[0, 3] == 0
    if max_steps == 1:
        assert stats[0, 3] == K


# ---- 5. win count at ties --------------------------------------------------------------------------------------------------------
def test_win_count_at_ties(six):
    """komi equal to an area difference that occurs: (float)diff - komi > 0 is false there, and the count is the oracle's"""
    eng, E, states = six
    assert oe.TIE_ROW["prefix"] == oe.STEP_ROW["prefix"]                      # slot STEP holds the tie row's source as well
    K, seed = oe.TIE_ROW["K"], np.array([oe.TIE_ROW["seed"]], np.uint64)
    diffs = [d for d, _ in oe.playout_diffs(E, states[STEP], seed[0], K)]
    d0 = diffs[0]
    for komi in (0.0, 7.0, -3.0, 81.0, -81.0, float(d0)):
        wc, ws = oe.expected(E, states[STEP], seed[0], K, komi)
        assert ws[1] == sum(d > komi for d in diffs)
        counts, stats = run(eng, seed, ids=[STEP], playouts=K, komi=komi)
        assert np.array_equal(stats[0], ws), (komi, stats[0].tolist(), ws.tolist())
        assert np.array_equal(counts[0], wc), komi
    assert sum(d == d0 for d in diffs) >= 1 and 81 in diffs


# ---- 6. special sources ----------------------------------------------------------------------------------------------------------
def test_source_already_ended_by_superko(elf):
    """the slot comes in with its super-ko flag set: no step, every playout counted as a super-ko ending, K times its map"""
    n, K = 9, 4
    E = oracle(n)
    game = oe.superko_source(E)
    eng = elf.GoEngine(n, 1, 0)
    play_all(eng, [game])
    info = npy(eng.info())
    assert info[0, 9] == 1 and info[0, 10] == 1                                   # terminated, by super-ko
    s = oe.replay(E, game)
    am = oe.area_map_bfs(E.board(s)[0], n)
    diff = oe.area_diff(am)
    counts, stats = run(eng, np.array([99], np.uint64), playouts=K, komi=7.5)
    assert stats[0].tolist() == [K * diff, K * int(diff - 7.5 > 0), K, 0]
    assert np.array_equal(counts[0, 0], K * (am == 1)) and np.array_equal(counts[0, 1], K * (am == 2))
    wc, ws = oe.expected(E, s, 99, K, 7.5)
    assert np.array_equal(counts[0], wc) and np.array_equal(stats[0], ws)
    E.free(s)
    eng.close()


def device_playouts(eng, src, spare, seed, komi):
    """copies of slot `src` in the slots `spare`, copy k played out by k_playout with seed(seed, k): the sums ownership must show"""
    K = len(spare)
    eng.copy(spare, [src] * K)
    out = npy(eng.playout(np.array([oe.seed_of(seed, k) for k in range(K)], np.uint64), ids=spare)).view(np.uint32)
    am = npy(eng.area_map(spare))
    info = npy(eng.info(spare))
    diffs = [oe.area_diff(a) for a in am]
    counts = np.stack([(am == 1).sum(0), (am == 2).sum(0)]).astype(np.int32)
    stats = [sum(diffs), sum(int(np.float32(d) - np.float32(komi) > 0) for d in diffs), int(info[:, 10].sum()), int(out[:, 3].astype(np.int64).sum())]
    return counts, np.array(stats, np.int64)


def test_setup_source_equals_the_playout_kernel(elf):
    """a slot made by elfgo_setup holds stones and no record (sk_len 0): ownership of it is the sum over copies of it that
    k_playout played with the same seeds"""
    n, K, seed = 9, 6, 0xABCDEF0123456789
    E = oracle(n)
    src, _ = oe.row_source(E, oe.STEP_ROW)
    eng = elf.GoEngine(n, 1 + K, 0)
    assert npy(eng.setup(E.board(src)[0], ids=[0], next_player=[int(E.info(src)[1])])).tolist() == [1]
    assert int(npy(eng.info([0]))[0, 12]) == 0
    before = snapshot(eng, [0])
    for lanes in (0, 1):
        counts, stats = run(eng, np.array([seed], np.uint64), ids=[0], playouts=K, komi=0.5, max_lanes=lanes)
        wc, ws = device_playouts(eng, 0, list(range(1, 1 + K)), seed, 0.5)
        assert np.array_equal(counts[0], wc) and np.array_equal(stats[0], ws), (stats[0].tolist(), ws.tolist())
    assert ws[3] > 20 * K and same(before, snapshot(eng, [0]))
    E.free(src)
    eng.close()


def test_undone_source_equals_the_playout_kernel_and_the_oracle(elf):
    """a game board 30 moves on and 7 taken back: ownership of it is the sum over copies played by k_playout, and the oracle's
    for the 23 moves"""
    n, K, seed = 9, 6, 0x1234567
    E = oracle(n)
    moves = oe.row_source(E, oe.STEP_ROW)[1]
    assert len(moves) == 30
    sp = elf.SelfPlay(board_size=n, num_games=1 + K, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048, seed=5)
    boards = sp.board_engine()
    for c in moves:
        sp.play([c] + [-1] * K)
    sp.undo(7, [0])
    assert int(npy(boards.info([0]))[0, 0]) == 24
    counts, stats = run(boards, np.array([seed], np.uint64), ids=[0], playouts=K, komi=7.5, max_lanes=1)
    wc, ws = device_playouts(boards, 0, list(range(1, 1 + K)), seed, 7.5)
    assert np.array_equal(counts[0], wc) and np.array_equal(stats[0], ws), (stats[0].tolist(), ws.tolist())
    s = oe.replay(E, moves[:23])
    oc, os_ = oe.expected(E, s, seed, K, 7.5)
    assert np.array_equal(counts[0], oc) and np.array_equal(stats[0], os_)
    E.free(s)
    boards.close()
    sp.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(six):
    """bad arguments are ELFGO_E_BADARG and nothing is launched: the output buffers keep what they held"""
    import torch
    eng, E, states = six
    L, cap, np_ = eng.L, eng.capacity, 81
    seeds = playout_seeds(3, base=4000)
    run(eng, seeds, ids=[MID, LATE, KO], playouts=2)                      # makes the handle
    h = eng._own[1]
    big = 65536
    dev = eng.device
    ids = torch.zeros(big, dtype=torch.int32, device=dev)
    sd = torch.ones(big, dtype=torch.int64, device=dev)
    counts = torch.full((big, 2, np_), -7, dtype=torch.int32, device=dev)          # large enough for every row count below
    stats = torch.full((big, 4), -7, dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr()
    call = lambda o, i, s, n, k, c, st: L.elfgo_own_run(o, i, s, n, k, 100, 7.5, c, st, None)
    assert call(None, p(ids), p(sd), 1, 1, p(counts), p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), None, 1, 1, p(counts), p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), 1, 1, None, p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), 1, 1, p(counts), None) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), 0, 1, p(counts), p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), -1, 1, p(counts), p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), 1, 0, p(counts), p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), 1, -1, p(counts), p(stats)) == ELFGO_E_BADARG
    assert call(h, p(ids), p(sd), big, big, p(counts), p(stats)) == ELFGO_E_BADARG     # 2^32 pairs
    assert call(h, None, p(sd), cap + 1, 1, p(counts), p(stats)) == ELFGO_E_BADARG
    out = torch.full((big, np_), 9, dtype=torch.uint8, device=dev)
    area = lambda e, i, n, o: L.elfgo_area_map(e, i, n, o, None)
    assert area(eng._h, None, 0, p(out)) == 0 and area(eng._h, None, 0, None) == 0
    assert area(eng._h, None, 1, None) == ELFGO_E_BADARG
    assert area(eng._h, None, cap + 1, p(out)) == ELFGO_E_BADARG
    assert area(eng._h, None, -1, p(out)) == ELFGO_E_BADARG and area(None, None, 1, p(out)) == ELFGO_E_BADARG
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((stats == -7).all()) and bool((out == 9).all())
    # a call that is accepted, with the same handle
    wc, ws = expected_rows(E, states, [MID, LATE, KO], seeds, 2)
    c2, s2 = run(eng, seeds, ids=[MID, LATE, KO], playouts=2)
    assert eng._own[1] is h and np.array_equal(c2, wc) and np.array_equal(s2, ws)
    am = npy(eng.area_map())
    for i, s in enumerate(states):
        assert np.array_equal(am[i], oe.area_map_bfs(E.board(s)[0], 9)), i


# ---- 8. stream order -------------------------------------------------------------------------------------------------------------
def test_stream_order(elf):
    """forward, ownership, forward on a stream of the caller's with no host wait in between: the memsets and the launch follow that
    stream, so the ownership is that of the position between the two plies"""
    import torch
    n, K = 9, 8
    E = oracle(n)
    moves = oe.mixed_rows(E, n)[LATE]
    m1, m2 = moves[-2], moves[-1]
    eng = elf.GoEngine(n, 1, 0)
    play_all(eng, [moves[:-2]])
    seeds = playout_seeds(1, base=5000)
    run(eng, seeds, playouts=1)                                            # the handle exists before the stream is used
    dev = eng.device
    ids = torch.zeros(1, dtype=torch.int32, device=dev)
    mv1, mv2 = (torch.tensor([m], dtype=torch.int32, device=dev) for m in (m1, m2))
    sd = torch.from_numpy(seeds.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ok1 = eng.forward(ids, mv1)
        own = eng.ownership(sd, ids=ids, playouts=K)
        ok2 = eng.forward(ids, mv2)
    stream.synchronize()
    assert npy(ok1).tolist() == [1] and npy(ok2).tolist() == [1]
    s = oe.replay(E, moves[:-1])
    wc, ws = oe.expected(E, s, seeds[0], K, 7.5)
    assert np.array_equal(npy(own["counts"])[0], wc) and np.array_equal(npy(own["stats"])[0], ws)
    assert E.forward(s, m2) == 1 and int(eng.info_host()["hash"][0]) == E.hash(s)
    # the position before and the position after would have given other sums
    for other in (moves[:-2], moves):
        t = oe.replay(E, other)
        assert not np.array_equal(oe.expected(E, t, seeds[0], K, 7.5)[0], wc)
        E.free(t)
    E.free(s)
    eng.close()
