"""No GPU: proves the instrument of the life-reading tests (life_expected) on the reference alone.

* GivenGroupLives is static in the reference; the instrument reaches it as OneGroupLives over the 1x1 box on one stone of the
  group.  On every sampled position the OR of those answers over a colour's groups is OneGroupLives(colour, nullptr), and on the
  constructed positions every stone of a group gives its group's answer;
* getEyeColor is the two isTrueEye answers, White asked first; getFastScore is what its source says, with the board's own capture
  counts under the Japanese rule and a _rollout_passes of 0;
* the constructed positions get the answers derived by hand, in all 8 symmetries and both colourings;
* the game sets hold enough living groups and semi-eyes for the GPU comparison to mean something."""
import numpy as np
import pytest

import candidates_expected as CE
import ladder_positions as LP
import life_expected as LE
from pyoracle import Ref, RefBoard

B, W = LE.BLACK, LE.WHITE


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert RefBoard.available(9) and RefBoard.available(19) and Ref.available(9) and Ref.available(19), \
        "build() must have produced oracle/_ref/libelfboard{9,19}.so and libelfref{9,19}.so"


def nibble(eye, colour):
    return (eye >> (4 * (colour - 1))) & 15


def check_row(exp, n):
    """the relations between the reference's own answers at one position"""
    eye, col = exp["eye"], exp["colour"]
    for c in (B, W):
        nb = nibble(eye, c)
        assert not (nb[col != 0] & (LE.EYE | LE.TRUE | LE.SEMI)).any(), "eye, true eye and semi-eye are answers about empty points"
        assert np.array_equal((nb & LE.TRUE) != 0, ((nb & LE.EYE) != 0) & ((nb & LE.FAKE) == 0))
        assert not ((nb & LE.SEMI) != 0)[(nb & LE.EYE) == 0].any()
        sm = exp["semi_move"][c - 1]
        assert np.array_equal(sm >= 0, (nb & LE.SEMI) != 0)
        for a in np.nonzero(sm >= 0)[0]:
            m = int(sm[a])
            assert abs(m // n - a // n) == 1 and abs(m % n - a % n) == 1 and col[m] == 0 and not nibble(eye[m], c) & LE.EYE
        # the OR of the per-group 1x1-box answers is the whole-board answer
        assert bool(exp["alive"][col == c].any()) == exp["whole"][c - 1]
    tb, tw = (nibble(eye, B) & LE.TRUE) != 0, (nibble(eye, W) & LE.TRUE) != 0
    assert np.array_equal(exp["eye_colour"], np.where(tw, W, np.where(tb, B, 0))), "getEyeColor asks White first"
    s = exp["summary"]
    eb, ew = int((exp["eye_colour"] == B).sum()), int((exp["eye_colour"] == W).sum())
    assert s[0] == eb + int((col == B).sum()) - ew - int((col == W).sum())
    assert s[1] == eb - ew + int(exp["info"][7]) - int(exp["info"][8]), "Japanese: eyes and the board's captures, no rollout passes"


@pytest.mark.parametrize("name", ["nine", "ladder16", "playout19"])
def test_game_sets_one_by_one_box_and_eye_colour(name):
    n, games, rows = LE.all_expected(name)
    caps = 0
    for r in rows:
        check_row(r["plain"], n)
        caps += int(r["plain"]["info"][7]) + int(r["plain"]["info"][8])
        # the box changes the summary's box-dependent words only; a box that holds every stone gives the whole-board answers
        assert np.array_equal(r["boxed"]["summary"][:2], r["plain"]["summary"][:2])
        assert tuple(r["boxed"]["summary"][4:8]) == r["box"]
        assert tuple(r["plain"]["summary"][2:4]) == tuple(int(v) for v in r["plain"]["whole"])
    assert caps > 0, "the Japanese score was compared on positions with captures"
    kinds = {(b[0] == 0, b[1] == 0, b[2] == n, b[3] == n, b[0] == b[2]) for b in (r["box"] for r in rows)}
    assert any(k[0] for k in kinds) and any(k[1] for k in kinds) and any(k[2] for k in kinds) and any(k[3] for k in kinds) and any(k[4] for k in kinds)


def test_input_conditions():
    """counted on the reference's answers alone; the figures below were printed by this test's first run"""
    want = {
        "nine": dict(positions=2437, groups=34561, living=2186, semi_eyes=767, true_eyes=8398),
        "ladder16": dict(positions=406, groups=16558, living=84, semi_eyes=363, true_eyes=1399),
        "playout19": dict(positions=241, groups=14208, living=513, semi_eyes=354, true_eyes=3181),
    }
    total = dict(living=0, semi_eyes=0)
    for name in want:
        st = LE.statistics(LE.all_expected(name)[2])
        print(name, st)
        assert st == want[name], name
        for k in total:
            total[k] += st[k]
    assert total["living"] >= 100 and total["semi_eyes"] >= 100, total
    # each board size on its own, too
    for name in ("nine", "playout19"):
        assert want[name]["living"] >= 100 and want[name]["semi_eyes"] >= 100


@pytest.mark.parametrize("n", [9, 19])
def test_constructed_positions_get_the_answers_derived_by_hand(n):
    lf, rows = LE.expected(n)
    names = {r["name"] for r in rows}
    assert len(rows) == 16 * (len(names) - 1) + 1
    for r in rows:
        exp, c = r["plain"], r["colour"]
        check_row(exp, n)
        tag = (r["name"], r["s"], r["swapped"])
        for a, v in r["bits"].items():
            assert int(nibble(exp["eye"][a], c)) == v, tag
            assert not int(nibble(exp["eye"][a], 3 - c)) & (LE.EYE | LE.TRUE | LE.SEMI), tag
        for a, m in r["semi"].items():
            assert int(exp["semi_move"][c - 1][a]) == m, tag
        for a, v in r["alive"].items():
            assert int(exp["colour"][a]) == c and int(exp["alive"][a]) == v, tag
        # every stone of a group gives its group's answer through its own 1x1 box
        h = LP.handle(lf.RB, r)
        for a in np.nonzero(exp["colour"])[0]:
            x, y = int(a) // n, int(a) % n
            assert lf.one_group_lives(h, int(exp["colour"][a]), (x, y, x + 1, y + 1)) == bool(exp["alive"][a]), tag
            # and a box next to the stone that does not hold it asks nobody
        assert not lf.one_group_lives(h, B, (0, 0, 0, 0)) and not lf.one_group_lives(h, W, (n, n, 0, 0))
        lf.RB.free(h)
        if r["name"].startswith("suicide_eye"):
            (a,) = r["bits"]
            assert r["mover"] == c and int(r["legal_mask"][a]) == 0, "the eye's owner is to move and may not play it"
        if r["name"] == "ko_pending":
            (a,) = r["bits"]
            assert r["info"][5] == lf.coords[a] and r["info"][4] == 0 and r["info"][6] == r["mover"] == 3 - c, "the ko is pending on the eye"
            assert int(r["legal_mask"][a]) == 0
        if r["name"] == "empty_board":
            assert tuple(exp["summary"]) == (0, 0, 0, 0, n, n, 0, 0, W, 0, 0, 0)
            assert not exp["eye"].any() and not exp["alive"].any() and (exp["semi_move"] == -1).all()


@pytest.mark.parametrize("n", [9, 19])
def test_an_eye_of_another_group_does_not_count(n):
    """position 5: the lone stone does not live, although every true eye next to it would qualify if an empty diagonal counted
    whenever it is a true eye of the colour anywhere on the board"""
    lf, rows = LE.expected(n)
    seen = 0
    for r in rows:
        if not r["name"].startswith("other_groups_eye"):
            continue
        exp, c = r["plain"], r["colour"]
        (lone,) = [a for a, v in r["alive"].items() if v == 0]
        (big,) = [a for a, v in r["alive"].items() if v == 1]
        assert exp["alive"][lone] == 0 and exp["alive"][big] == 1
        true = (nibble(exp["eye"], c) & LE.TRUE) != 0
        col = exp["colour"].reshape(n, n)
        tg = true.reshape(n, n)
        x, y = lone // n, lone % n
        mine = [(qx, qy) for qx, qy in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)) if 0 <= qx < n and 0 <= qy < n and tg[qx, qy]]
        assert len(mine) == 2

        def qualifies(ex, ey, eyes):
            off = terr = 0
            for dx, dy in ((-1, -1), (-1, 1), (1, -1), (1, 1)):
                qx, qy = ex + dx, ey + dy
                if not (0 <= qx < n and 0 <= qy < n):
                    off += 1
                elif col[qx, qy] == c or (col[qx, qy] == 0 and (qx, qy) in eyes):
                    terr += 1
            return off + terr == 4 if off >= 1 else terr >= 3
        board_wide = {(int(a) // n, int(a) % n) for a in np.nonzero(true)[0]}
        assert sum(qualifies(ex, ey, board_wide) for ex, ey in mine) == 2, "with a board-wide eye set the lone stone would live"
        assert sum(qualifies(ex, ey, set(mine)) for ex, ey in mine) == 1, "with its own list it has one qualifying eye"
        seen += 1
    assert seen == 16


@pytest.mark.parametrize("n", [9, 19])
def test_attacker_and_bounding_box(n):
    lf = LE.life(n)
    st = LE.attacker_position(n)
    for sw in (False, True):
        h = LP.build(lf.RB, LP.swap(st) if sw else st, B)
        assert h is not None
        assert lf.bbox(h) == (3, 3, 6, 5)
        for box, nb, nw in LE.attacker_boxes(n):
            if sw:
                nb, nw = nw, nb
            assert lf.attacker(h, box) == (B if nb > nw else W), (sw, box)
        lf.RB.free(h)
    # the tie and every board edge are among the boxes
    boxes = [b for b, _, _ in LE.attacker_boxes(n)]
    assert any(nb == nw and nb > 0 for _, nb, nw in LE.attacker_boxes(n))
    assert any(b[0] == 0 for b in boxes) and any(b[1] == 0 for b in boxes) and any(b[2] == n for b in boxes) and any(b[3] == n for b in boxes)
    h = lf.RB.new()
    assert lf.bbox(h) == (n, n, 0, 0) and lf.attacker(h, (n, n, 0, 0)) == W
    assert not lf.one_group_lives(h, B) and not lf.one_group_lives(h, W)
    lf.RB.free(h)
