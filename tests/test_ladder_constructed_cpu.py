"""CPU: the constructed inputs of the ladder tests (ladder_positions) under the reference's ladder reader, the kernel's search
loop restated over the reference's board primitives (ladder_restated) against that reader, and the conditions the inputs must
meet before tests/test_gpu_ladder_constructed.py means anything.

Every expected number comes from checkLadder / checkLadderUseSearch of oracle/_ref's unshimmed board library at test time.

The ko cases.  The input one would want is a position in which the candidate point of a would-be ladder is the pending ko
point, so that the prefilter's ko test (`ko_live && a == bd.ko_a`) decides the answer.  No such position exists.  A simple ko
is recorded (base/board.cc:1384-1389) when a single stone with one liberty has just taken a single stone; the taken stone had
no empty and no friendly neighbour, and while the ko is pending (only passes keep its age at 0) every neighbour of the ko point
is the taker's colour or the border.  The prefilter wants two empty neighbours there.  Nor does a ko refuse a move inside a
search: the candidate move and every flight join a group of the victim's, so the victim never makes a ko; and where the
capturer makes one, the ko point held a stone that was no neighbour of the victim's last stone (it would have belonged to its
group), while the flight goes to a neighbour of that stone.  What is left to pin, and is pinned here: with the ko pending
TryPlay2 refuses the ko point and without it TryPlay2 accepts it (the two answers that do differ), the ladder depth there is 0
both times, the maps are equal everywhere although a long search runs into the ko's stones, and on all 12 522 suite positions
no pending ko point has an empty neighbour."""
import numpy as np
import pytest

import ladder_expected as LE
import ladder_positions as LP
import ladder_restated as LR
from pyoracle import RefBoard

# counts of the constructed inputs, from a run of statistics() on them; plays, longest and forks are the restated loop's
WANT_19 = dict(positions=272, with_ladder=160, searches=336, nonzero=224, backtracked=118, max_calls=1108,
               hist={3: 40, 5: 18, 7: 24, 9: 24, 11: 12, 13: 4, 17: 10, 19: 8, 21: 6, 23: 14, 25: 8, 31: 24, 33: 8, 37: 2, 47: 4, 51: 2, 63: 16},
               max_plays=18408, longest=75, max_forks=23)
WANT_9 = dict(positions=208, with_ladder=96, searches=224, nonzero=112, backtracked=48, max_calls=171,
              hist={3: 40, 5: 8, 7: 8, 11: 16, 13: 8, 19: 16, 23: 16}, max_plays=898, longest=27, max_forks=12)
# for comparison, the restated loop on all plies of the 115 suite games (test_restated_loop_equals_the_reference_on_the_suite_games
# prints it): largest plays 271, longest line 55, most open forks 6, largest num_call 77.
# Head room under the kernel's bounds on the constructed inputs (test_bounds_hold_on_every_input prints it):
#   19x19: largest plays 18 408 / 32 000 = 0.575, longest line 75 / 1024 = 0.073, most open forks 23
#   9x9:   largest plays    898 / 32 000 = 0.028, longest line 27 / 1024 = 0.026, most open forks 12
# MAX_LADDER_SEARCH: three of the 19x19 layouts reach it (num_call 1108, 1097, 1069 in the stored image), so the cut is pinned at
# 19x19; at 9x9 the largest num_call is 171 after 500 s of search and the cut is unpinned there.


def _need(n):
    assert RefBoard.available(n), "build() must have produced oracle/_ref/libelfboard%d.so" % n


_restated = {}


def restated(n):
    """LP.expected(n) with the restated loop's maps and per-point results added, once per process"""
    if n not in _restated:
        lad, rows = LP.expected(n)
        rs = LR.Restated(lad.RB)
        for r in rows:
            h = LP.handle(lad.RB, r)
            r["rdepth"], r["rcalls"], r["res"] = rs.maps(h)
            lad.RB.free(h)
        _restated[n] = rows
    return _restated[n]


def statistics(rows):
    hist = {}
    nz_all = np.array([r["depth"] for r in rows]) > 0
    calls = np.array([r["calls"] for r in rows])
    for r in rows:
        for d in r["depth"][r["depth"] > 0]:
            hist[int(d)] = hist.get(int(d), 0) + 1
    res = [x for r in rows for _, x in r["res"]]
    return dict(positions=len(rows), with_ladder=int(nz_all.any(axis=1).sum()), searches=int((calls > 0).sum()), nonzero=int(nz_all.sum()),
                backtracked=int((nz_all & (calls > np.array([r["depth"] for r in rows]))).sum()), max_calls=int(calls.max()),
                hist=dict(sorted(hist.items())), max_plays=max(x.plays for x in res), longest=max(x.longest for x in res),
                max_forks=max(x.forks for x in res))


def by_position(rows):
    out = {}
    for r in rows:
        out.setdefault(r["name"], []).append(r)
    return out


# ---- the inputs themselves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_every_position_has_its_16_images(built, n):
    _need(n)
    _, rows = LP.expected(n)
    pos = by_position(rows)
    want = set(LP.hand_built(n)) | set(LP.searched(n)) | {"ko_plain", "ko_pending"}
    assert set(pos) == want
    for name, rs in pos.items():
        assert [(r["s"], r["swapped"]) for r in rs] == [(s, sw) for sw in (False, True) for s in range(8)], name
        base = rs[0]
        for r in rs:
            st = LP.sym(n, base["stones"], r["s"])
            assert np.array_equal(r["stones"], LP.swap(st) if r["swapped"] else st)
            assert r["mover"] == (3 - base["mover"] if r["swapped"] else base["mover"])
            assert int((r["stones"] == 1).sum()) == int((base["stones"] == (2 if r["swapped"] else 1)).sum())
    # the eight symmetries are eight different maps of the board
    probe = np.arange(n * n)
    assert len({tuple(LP.sym_perm(n, s)) for s in range(8)}) == 8
    for s in range(8):
        p = LP.sym_perm(n, s)
        assert sorted(p) == list(probe)
        marked = np.zeros(n * n, np.uint8)
        marked[5] = 1
        assert LP.sym(n, marked, s)[p[5]] == 1


def test_the_fixture_holds_stones_and_movers_only():
    with np.load(LP.FIXTURE) as f:
        assert sorted(f.files) == ["budget_seconds19", "budget_seconds9", "mover19", "mover9", "names19", "names9", "stones19", "stones9"]
        for n in (19, 9):
            st, mv, names = f["stones%d" % n], f["mover%d" % n], f["names%d" % n]
            assert st.dtype == np.uint8 and st.shape == (len(names), n * n) and st.max() <= 2
            assert mv.dtype == np.uint8 and set(mv.tolist()) <= {1, 2}
            assert len(set(names.tolist())) == len(names)
        assert len(f["names19"]) >= 6


def test_build_catches_stones_that_cannot_stand(built):
    _need(9)
    RB = RefBoard(9)
    st = LP.draw(9, [". X .", "X O X", ". X ."])          # the white stone has no liberty
    assert LP.build(RB, st, LP.BLACK) is None
    st = LP.draw(9, [". X .", "X O .", ". X ."])
    for mover in (LP.BLACK, LP.WHITE):
        h = LP.build(RB, st, mover)
        assert h is not None and int(RB.info(h)[1]) == mover and np.array_equal(RB.board(h)[0], st)
        assert RB.info(h)[5] == 0                           # no ko
        RB.free(h)


# ---- pinned statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_statistics(built, n):
    _need(n)
    st = statistics(restated(n))
    print("constructed ladder statistics %dx%d:" % (n, n), st)
    assert st == (WANT_19 if n == 19 else WANT_9)


# ---- the restated loop is the reference's search ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_restated_loop_equals_the_reference_on_the_constructed_inputs(built, n):
    _need(n)
    searched = 0
    for r in restated(n):
        assert np.array_equal(r["rdepth"], r["depth"]) and np.array_equal(r["rcalls"], r["calls"]), (r["name"], r["s"], r["swapped"])
        assert [a for a, _ in r["res"]] == list(np.nonzero(r["calls"] > 0)[0])     # the prefilter is checkLadder's own test
        searched += len(r["res"])
    assert searched > 0


def test_restated_loop_equals_the_reference_on_the_suite_games(built):
    _need(19)
    gs, exp = LE.all_expected(19)
    RB = RefBoard(19)
    rs = LR.Restated(RB)
    searched = positions = 0
    most = dict(plays=0, longest=0, forks=0)
    for mv, e in zip(gs, exp):
        h = RB.new()
        for t in range(len(mv) + 1):
            d, c, res = rs.maps(h)
            assert np.array_equal(d, e["depth"][t]) and np.array_equal(c, e["calls"][t]), t
            searched += len(res)
            positions += 1
            for _, x in res:
                most = dict(plays=max(most["plays"], x.plays), longest=max(most["longest"], x.longest), forks=max(most["forks"], x.forks))
            if t < len(mv):
                assert RB.play(h, int(mv[t])) == 1
        RB.free(h)
    print("restated loop on the suite games: %d positions, %d searches, largest %s" % (positions, searched, most))
    assert positions == 12522 and searched == 2432


def test_the_cut_and_the_bounds_of_the_restated_loop(built):
    """MAX_LADDER_SEARCH.  The searched layouts reach it: at their heaviest points the reference counts past 1024 nodes, and the
    restated loop gives the reference's depth and num_call there only because it has the rule -- without it the same point gives
    other numbers.  Below the limit the rule changes nothing, and with the limit at 1 no fork is ever opened.
    The kernel's own two bounds end a point with calls = -1 and depth 0, exactly from the first play / move that does not fit."""
    _need(19)
    lad, rows = LP.expected(19)
    over = [(r, int(a)) for r in rows for a in np.nonzero(r["calls"] >= LR.MAX_LADDER_SEARCH)[0]]
    assert len(over) >= 16, "at least one position reaches the cut, in every image"
    differ = 0
    for r, a in over[::7]:
        h = LP.handle(lad.RB, r)
        full = LR.Restated(lad.RB).search(h, a)
        assert (full.depth, full.calls) == (int(r["depth"][a]), int(r["calls"][a]))
        free = LR.Restated(lad.RB, max_search=1 << 30, max_plays=1 << 30).search(h, a)
        differ += (free.depth, free.calls) != (full.depth, full.calls)
        lad.RB.free(h)
    assert differ > 0, "the rule decides an answer on these inputs"
    # a heavy search below the limit
    r, a = max(((r, int(a)) for r in rows for a in np.nonzero((r["calls"] > 0) & (r["calls"] < LR.MAX_LADDER_SEARCH))[0]),
               key=lambda ra: int(ra[0]["calls"][ra[1]]))
    h = LP.handle(lad.RB, r)
    full = LR.Restated(lad.RB).search(h, a)
    assert (full.depth, full.calls) == (int(r["depth"][a]), int(r["calls"][a])) and full.calls >= 500 and full.forks >= 8
    same = LR.Restated(lad.RB, max_search=full.calls + 1).search(h, a)
    assert (same.depth, same.calls, same.plays, same.forks) == (full.depth, full.calls, full.plays, full.forks)
    line = LR.Restated(lad.RB, max_search=1).search(h, a)
    assert line.forks == 0 and line.plays - line.calls in (0, 1) and line.plays <= full.plays      # one line, no replay
    cut = LR.Restated(lad.RB, max_plays=full.plays - 1).search(h, a)
    assert cut.over and (cut.depth, cut.calls) == (0, -1)
    cut = LR.Restated(lad.RB, stack=full.longest - 1).search(h, a)
    assert cut.over and (cut.depth, cut.calls) == (0, -1)
    fits = LR.Restated(lad.RB, max_plays=full.plays, stack=full.longest).search(h, a)
    assert not fits.over and (fits.depth, fits.calls) == (full.depth, full.calls)
    lad.RB.free(h)


# ---- conditions on the inputs: requirements, not measurements ----------------------------------------------------------------
def test_conditions_on_the_inputs(built):
    _need(19)
    _need(9)
    r19, r9 = restated(19), restated(9)
    s19, s9 = statistics(r19), statistics(r9)
    assert max(s19["hist"]) > 55 and max(s9["hist"]) > 7           # deeper than anything the game plies have
    assert s19["max_calls"] >= 150
    heavy = sum(int(((r["calls"] > 0) & (r["calls"] > 2 * r["depth"])).sum()) for r in r19 + r9)
    assert heavy >= 10
    # White is the victim of a deep search too
    assert max(int(r["depth"].max()) for r in r19 if r["mover"] == LP.WHITE) > 55
    for rows in (r19, r9):
        # the reference's answer is not symmetric: the first line that works depends on the L, T, R, B order
        stored = [rs for name, rs in by_position(rows).items() if name.startswith("searched_")]
        assert any(len({int(r["depth"].max()) for r in rs[:8]}) > 1 for rs in stored)
        assert any(len({int(r["calls"].max()) for r in rs[:8]}) > 1 for rs in stored)
        # ... but it is colour blind: the swapped image of every image gives the same maps
        for name, rs in by_position(rows).items():
            for k in range(8):
                assert np.array_equal(rs[k]["depth"], rs[k + 8]["depth"]) and np.array_equal(rs[k]["calls"], rs[k + 8]["calls"]), (name, k)


@pytest.mark.parametrize("n", [19, 9])
def test_hand_built_positions_do_what_they_were_drawn_for(built, n):
    _need(n)
    pos = by_position(restated(n))

    def only(r):
        assert len(r["res"]) == 1, "one candidate point"
        return r["res"][0][1]
    deep = 63 if n == 19 else 23                                    # recorded: the diagonal ladder from (2,2) to the far side
    for r in pos["diagonal"]:
        assert only(r).depth == deep
    assert {only(r).calls for r in pos["diagonal"]} == {deep, deep + 4}
    lengths = []
    for k in range(3):
        for r in pos["diagonal_breaker%d" % k]:
            x = only(r)
            assert x.depth == 0 and x.forks == 1 and x.plays == 2 * x.calls    # one backtrack that replays the whole line
        lengths.append(only(pos["diagonal_breaker%d" % k][0]).calls)
    assert lengths == sorted(lengths) and len(set(lengths)) == 3
    for r in pos["diagonal_capturer_stone"]:
        assert 0 < only(r).depth < deep
    # along the border: every capturer's node is a fork with the border next to it; the orientation decides which line is first
    assert {only(r).depth for r in pos["second_line"]} == {3, 2 * n - 5}
    assert max(only(r).forks for r in pos["second_line"]) == n - 3
    assert all(only(r).depth == 3 for r in pos["first_line"])
    for r in pos["self_atari"]:
        x = only(r)
        assert (x.depth, x.calls, x.forks) == (0, 3, 1)              # the atari stone in atari fails at the victim's node
    for r in pos["capture_in_flight"]:
        x = only(r)
        assert (x.depth, x.calls, x.plays, x.forks) == (0, 4, 9, 1)  # the backtrack replays the flight that captures


@pytest.mark.parametrize("n", [19, 9])
def test_ko_cases(built, n):
    """see the module's docstring: the two TryPlay2 answers at the ko point differ, the ladder answers cannot"""
    _need(n)
    lad, rows = LP.expected(n)
    pos = by_position(rows)
    _, _, k = LP.ko_cases(n)
    for pend, plain in zip(pos["ko_pending"], pos["ko_plain"]):
        assert np.array_equal(pend["stones"], plain["stones"]) and pend["mover"] == plain["mover"]
        a = int(LP.sym_perm(n, pend["s"])[k])
        assert pend["info"][5] == lad.coords[a] and pend["info"][4] == 0 and pend["info"][6] == pend["mover"]   # pending, against the mover
        assert not (plain["info"][5] != 0 and plain["info"][4] == 0)
        hp, hq = LP.handle(lad.RB, pend), LP.handle(lad.RB, plain)
        assert lad.RB.try_play(hp, lad.coords[a]) == 0 and lad.RB.try_play(hq, lad.coords[a]) == 1
        lad.RB.free(hp)
        lad.RB.free(hq)
        assert pend["depth"][a] == 0 and plain["depth"][a] == 0
        assert np.array_equal(pend["depth"], plain["depth"]) and np.array_equal(pend["calls"], plain["calls"])
        assert pend["calls"].max() >= 2 * n                          # a long search runs next to the pending ko


def test_no_pending_ko_point_has_an_empty_neighbour(built):
    _need(19)
    gs, exp = LE.all_expected(19)
    RB = RefBoard(19)
    pending = 0
    for mv, e in zip(gs, exp):
        rep = RB.replay(mv)
        for t in np.nonzero((e["info"][:, 5] != 0) & (e["info"][:, 4] == 0))[0]:
            c = int(e["info"][t, 5])
            x, y = c % 21 - 1, c // 21 - 1
            col = rep["colour"][t].reshape(19, 19)
            nb = [col[p, q] for p, q in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)) if 0 <= p < 19 and 0 <= q < 19]
            assert col[x, y] == 0 and all(v == 3 - e["info"][t, 6] for v in nb)
            pending += 1
    assert pending > 100


# ---- the kernel's bounds ----------------------------------------------------------------------------------------------------
def test_bounds_hold_on_every_input(built):
    """every input stays below LADDER_MAX_PLAYS and LADDER_STACK by the restated loop's count, so the GPU test may demand that
    no point reports -1.  Reported, not asserted: the head room, and whether MAX_LADDER_SEARCH is reached"""
    _need(19)
    _need(9)
    with np.load(LP.FIXTURE) as f:
        budget = int(f["budget_seconds19"]), int(f["budget_seconds9"])
    for n, sec in zip((19, 9), budget):
        rows = restated(n)
        assert not any(x.over for r in rows for _, x in r["res"])
        st = statistics(rows)
        assert st["max_plays"] < LR.LADDER_MAX_PLAYS and st["longest"] < LR.LADDER_STACK
        print("%dx%d head room: largest plays %d / %d = %.4f, longest line %d / %d = %.4f, most open forks %d"
              % (n, n, st["max_plays"], LR.LADDER_MAX_PLAYS, st["max_plays"] / LR.LADDER_MAX_PLAYS, st["longest"], LR.LADDER_STACK,
                 st["longest"] / LR.LADDER_STACK, st["max_forks"]))
        if st["max_calls"] >= LR.MAX_LADDER_SEARCH:
            print("%dx%d: an input reaches num_call %d >= MAX_LADDER_SEARCH: the cut is pinned" % (n, n, st["max_calls"]))
        else:
            print("%dx%d: largest num_call is %d after %d s of search: no input reaches MAX_LADDER_SEARCH = %d, the cut is still unpinned"
                  % (n, n, st["max_calls"], sec, LR.MAX_LADDER_SEARCH))
