"""No GPU: proves the instrument of the candidate-move tests (candidates_expected) on the reference alone.

* with a threshold nothing reaches, the playout driver IS the config-2 playout: it reproduces the committed fixture
  tests/golden/playout_9.npz row for row;
* on the whole-board seki the reference's candidate lists are what the issue measured: empty at thres 5 for either side,
  the two shared liberties at thres 8;
* the constructed shapes have the properties their comments claim, by isSelfAtari / TryPlay of the reference itself;
* the sizes of the GPU test's input sets and the number of self-atari points in them, as the reference counts them."""
import os

import numpy as np
import pytest

import candidates_expected as CE
import ladder_positions as LP
from pyoracle import Ref, RefBoard

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert RefBoard.available(9) and RefBoard.available(19) and Ref.available(9) and Ref.available(19), \
        "build() must have produced oracle/_ref/libelfboard{9,19}.so and libelfref{9,19}.so"


def test_the_driver_without_a_threshold_reproduces_the_playout_fixture():
    g = np.load(os.path.join(GOLDEN, "playout_9.npz"))
    E, cd = Ref(9), CE.cand(9)
    for i in range(32):
        h, ply, steps = cd.playout_from(E, [], int(g["seeds"][i]), CE.NO_THRES)
        assert (h & 0xFFFFFFFF, h >> 32, ply, steps) == tuple(int(v) for v in g["out"][i]), i


def test_the_rng_is_the_oracles():
    """playout_rng restates oracle/ref_capi.cc:131-134: one ply of the reference's own playout picks what it picks"""
    E, cd = Ref(9), CE.cand(9)
    for sd in (1, 0x9E3779BA, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0):
        s = E.new()
        mv = E.playout_moves(s, sd, 3)
        E.free(s)
        b = cd.RB.new()
        for t, c in enumerate(mv):
            cand = cd.candidates(b, 1 + t % 2, CE.NO_THRES)
            assert cand[CE.playout_rng(sd, 1 + t) % len(cand)] == int(c)
            assert cd.RB.play(b, int(c)) == 1
        cd.RB.free(b)


def test_seki_candidate_lists():
    n, stones, mover = CE.seki()
    cd = CE.cand(n)
    libs = CE.xy(n, CE.SEKI_LIBS)
    seen = 0
    for s, sw, ist, imv in LP.images(n, stones, mover):
        perm = LP.sym_perm(n, s)
        want = sorted(cd.coords[int(perm[a])] for a in libs)
        black_group_colour = CE.WHITE if sw else CE.BLACK      # the colour of the image of the drawing's black stones
        for player in (CE.BLACK, CE.WHITE):
            h = LP.build(cd.RB, ist, player)
            assert h is not None
            for t in (1, 2, 3, 4, 5):
                assert cd.candidates(h, player, t) == [], (s, sw, player, t)
            assert sorted(cd.candidates(h, player, 8)) == want, (s, sw, player)
            num = 7 if player == black_group_colour else 5
            st = cd.stones(h, player)
            assert [int(st[int(perm[a])]) for a in libs] == [num, num]
            assert int((st > 0).sum()) == 2
            cd.RB.free(h)
            seen += 1
    assert seen == 32


@pytest.mark.parametrize("n", [9, 19])
def test_constructed_positions_are_what_their_comments_say(n):
    cd, rows = CE.expected(n)
    names = {r["name"] for r in rows}
    assert len(rows) == 16 * len(names)
    for r in rows:
        if r["p"] is None:
            continue
        p = r["p"]
        assert int(r["stones_sa"][p]) == r["num"] and int(r["legal_mask"][p]) == int(r["legal"]), (r["name"], r["s"], r["swapped"])
        if r["name"].startswith("own_eye"):
            assert all(r["mask"][t][p] == 0 for t in CE.CONSTRUCTED_THRESHOLDS)
        elif r["legal"]:
            assert r["mask"][CE.NO_THRES][p] == 1
            assert all(r["mask"][t][p] == int(not (r["num"] and r["num"] >= t)) for t in CE.CONSTRUCTED_THRESHOLDS)
        if r["name"] == "ko_pending":
            assert r["info"][5] == cd.coords[p] and r["info"][4] == 0
    if n == 19:
        # the played point on both sides of the first 64-bit word boundary, and a merged group across it
        assert {r["p"] for r in rows if r["name"].endswith("_a63") and r["s"] == 0} == {63}
        assert {r["p"] for r in rows if r["name"].endswith("_a64") and r["s"] == 0} == {64}
        for tag in ("a63", "a64"):
            r = [r for r in rows if r["name"] == "join_shared_" + tag and r["s"] == 0 and not r["swapped"]][0]
            mine = np.nonzero(r["stones"] == CE.BLACK)[0]
            assert mine.min() < 64 <= mine.max()


def test_input_sets_as_the_reference_counts_them():
    """what test_gpu_candidates.py compares point for point: the counts below were printed by this test's first run"""
    want = {
        "nine": dict(positions=7055, legal=235602, self_atari=15345, largest=33, dropped1=14686, dropped3=2432),
        "ladder16": dict(positions=3123, legal=843873, self_atari=12246, largest=19, dropped1=12141, dropped3=597),
        "playout19": dict(positions=1888, legal=280795, self_atari=12600, largest=31, dropped1=12363, dropped3=1780),
    }
    sizes = {"nine": (9, 64), "ladder16": (19, 16), "playout19": (19, 4)}
    for name in want:
        n, games, exp = CE.all_expected(name)
        assert (n, len(games)) == sizes[name]
        got = CE.statistics(exp)
        print(name, got)
        assert got == want[name], name
        for g in exp:
            # with no threshold the list is "legal and not the mover's own true eye"; stones sit on legal points only; a point
            # leaves the list at thres t exactly when it is a self-atari of t stones or more (or is an own true eye)
            base = g["legal"] & (1 - g["eyes"])
            assert np.array_equal(g["mask"][CE.NO_THRES], base)
            assert not (g["stones"] > 0)[g["legal"] == 0].any()
            for t in (1, 3):
                assert np.array_equal(g["mask"][t], base & ~((g["stones"] >= t) & (g["stones"] > 0)))
