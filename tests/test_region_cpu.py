"""tests/region_expected.py on the reference alone (no GPU): the region lists are the whole-board lists clipped to the box, a null
region is the whole board, GroupInRegion counts what the flood fill counts, the bare-Board playout driver equals the GoState
driver on played rows, the chosen rows hold super-ko endings and playouts cut by max_steps, and the straight three reads as the
issue states it."""
import numpy as np
import pytest

import ladder_positions as LP
import life_expected as LE
import ownership_expected as OE
import region_expected as RE
from pyoracle import Ref, RefBoard


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    assert RefBoard.available(9) and RefBoard.available(19) and Ref.available(9) and Ref.available(19), \
        "build() must have produced oracle/_ref/libelfboard{9,19}.so and libelfref{9,19}.so"


BLACK, WHITE = 1, 2


def _sample(n, step):
    return RE.list_rows(n)[::step] + RE.list_rows(n)[-16:]


@pytest.mark.parametrize("n", [9, 19])
def test_lists_are_the_whole_board_lists_clipped(n):
    rg = RE.reg(n)
    asked = 0
    for j, r in enumerate(_sample(n, 7 if n == 9 else 3)):
        h = LP.play_list(rg.RB, r["moves"])
        player = int(rg.RB.info(h)[1])
        legal = rg.RB.legal_mask(h)[:-1]
        for t in RE.list_thresholds(n):
            whole = rg.cd.mask(h, player, t)
            for bx in RE.list_boxes(n, j, r["ko"]):
                cand, valid, _ = rg.masks(h, bx, t)
                inb = rg.inbox(bx)
                assert np.array_equal(cand, whole * inb), (j, t, bx)
                assert np.array_equal(valid, legal * inb), (j, t, bx)
                asked += 1
            # the function's own order is the whole-board order
            bx = RE.list_boxes(n, j, r["ko"])[5]
            inside = [c for c in rg.cd.candidates(h, player, t) if rg.inbox(bx)[rg.action[c]]]
            assert rg.cand_in(h, bx, player, t) == inside
        # nullptr = the whole board, for all three functions
        assert rg.cand_in(h, None, player, 3) == rg.cd.candidates(h, player, 3)
        assert rg.valid_in(h, None) == [int(c) for c in rg.RB.valid_moves(h, player)]
        assert rg.groups_in_count(h, None) == int(rg.RB.info(h)[9])
        rg.RB.free(h)
    assert asked > 500


@pytest.mark.parametrize("n", [9, 19])
def test_group_in_region_counts_the_flood_fill(n):
    """the ids carry no colour in the exported interface, so both colours are counted together; the per-stone map the GPU test
    uses is the flood fill, whose per-colour split is checked here against a one-colour count: the groups of one colour with a
    stone in the box are the labels of that colour's stones in the box"""
    rg = RE.reg(n)
    total = 0
    for j, r in enumerate(_sample(n, 7 if n == 9 else 3)):
        h = LP.play_list(rg.RB, r["moves"])
        col = rg.RB.board(h)[0]
        lab, first = LE.groups_of(col, n)
        assert int(rg.RB.info(h)[9]) == len(first) - 1
        for bx in RE.list_boxes(n, j, r["ko"])[1:]:
            inb = rg.inbox(bx)
            per_colour = [len(set(lab[(col == c) & inb].tolist())) for c in (BLACK, WHITE)]
            assert rg.groups_in_count(h, bx) == sum(per_colour), (j, bx)
            groups = rg.masks(h, bx, 1, col)[2]
            for c in (BLACK, WHITE):
                assert len(set(lab[(groups == 1) & (col == c)].tolist())) == per_colour[c - 1]
            assert not groups[col == 0].any()
            total += sum(per_colour)
        rg.RB.free(h)
    assert total > 100


def _bare_entry(rg, moves):
    """what GoState holds after `moves`: ply, the last two moves, the recorded pre-move positions"""
    rep = rg.RB.replay(moves)
    assert rep["ok"].all()
    records = {rep["colour"][t].tobytes() for t, c in enumerate(moves) if int(c) != RE.M_PASS}
    last = [int(c) for c in moves[::-1][:2]] + [RE.M_INVALID] * 2
    return int(rep["info"][-1, 0]), (last[0], last[1]), records


@pytest.mark.parametrize("n", [9, 19])
def test_bare_driver_equals_the_gostate_driver(n):
    rg, E = RE.reg(n), RE.ref(n)
    checked = sko = 0
    for r in RE.ld_rows(n)[:: (2 if n == 9 else 3)]:
        ply0, last, records = _bare_entry(rg, r["moves"])
        for k in range(6):
            sd = OE.seed_of(r["seed"], k)
            for th in (1, 3):
                s, b = E.new(), rg.RB.new()
                for c in r["moves"]:
                    assert E.forward(s, c) == 1 and rg.RB.play(b, c) == 1
                assert int(E.info(s)[0]) == ply0
                b2 = rg.RB.clone(b)
                steps, first = rg.playout_state(E, s, b, sd, th, r["box"], RE.LD_MAX_STEPS[n])
                steps2, first2, sko2, ply2 = rg.playout_bare(b2, sd, th, r["box"], RE.LD_MAX_STEPS[n], ply0, last, records)
                assert (steps, first) == (steps2, first2)
                assert rg.RB.hash(b) == rg.RB.hash(b2) and np.array_equal(rg.RB.board(b)[0], rg.RB.board(b2)[0])
                assert OE.ended_by_superko(E, s) == sko2 and int(E.info(s)[0]) == ply2
                sko += sko2
                checked += 1
                E.free(s)
                rg.RB.free(b)
                rg.RB.free(b2)
    assert checked >= 96


@pytest.mark.parametrize("n", [9, 19])
def test_rows_hold_superko_endings_and_cut_playouts(n):
    """over the settings of the GPU test: at least one playout ends on a super-ko repeat, one is cut by max_steps, one ends by
    itself, and one row's source position is already terminated or has an empty box"""
    sko = cut = own = 0
    for setting in range(len(RE.LD_SETTINGS)):
        info, stats, first, ends = RE.ld_expected(n, setting)
        K = RE.LD_SETTINGS[setting][0]
        assert (first[:, 0].sum(axis=1) <= K).all()
        for e in ends:
            sko += sum(x[1] for x in e)
            cut += sum(x[2] for x in e)
            own += sum(not x[2] and not x[1] for x in e)
        assert stats[:, 4].sum() == sum(x[1] for e in ends for x in e)
    assert sko >= 1 and cut >= 1 and own >= 1, (sko, cut, own)


def test_straight_three():
    n = 9
    rg, E = RE.reg(n), RE.ref(n)
    NP = n * n
    vital = RE.S3_VITAL[0] * n + RE.S3_VITAL[1]
    others = [x * n + y for x, y in RE.S3_OTHERS]
    moves, final = RE.s3_move_list(n)
    h = LP.play_list(rg.RB, moves)
    assert np.array_equal(rg.RB.board(h)[0], final) and int(rg.RB.info(h)[1]) == BLACK
    assert rg.lf.attacker(h, RE.S3_BOX) == WHITE and not rg.lf.one_group_lives(h, BLACK, RE.S3_BOX)
    rg.RB.free(h)
    longest = 0
    for seed in RE.S3_SEEDS:
        for src in (moves, dict(stones=RE.straight_three(n), mover=BLACK)):
            ends = []
            info, stats, first = rg.ld_row(E, src, seed, 400, RE.S3_THRES, RE.S3_BOX, 0, ends=ends)
            assert tuple(info[:7]) == RE.S3_BOX + (WHITE, BLACK, BLACK) and info[7] == 0
            assert first[0, vital] > 0 and first[1, vital] == first[0, vital]
            assert all(first[0, a] > 0 and first[1, a] == 0 for a in others)
            assert first[1].sum() == first[1, vital]                    # no other first move lives
            longest = max(longest, max(e[0] for e in ends))
        for src in (moves + [RE.M_PASS], dict(stones=RE.straight_three(n), mover=WHITE)):
            info, stats, first = rg.ld_row(E, src, seed, 400, RE.S3_THRES, RE.S3_BOX, 0)
            assert tuple(info[4:7]) == (WHITE, BLACK, WHITE)
            assert first[0, vital] > 0 and first[2, vital] == 0          # every playout that starts at (1,0) kills
            rest = [a for a in range(NP + 1) if a != vital and first[0, a]]
            assert rest and all(first[1, a] == first[0, a] for a in rest)   # every other playout ends alive
    assert longest < 60      # short games: the box holds three empty points (a rare playout ends on a super-ko repeat)
    # threshold 1: the attacker may not throw in, and the reading is blind: not one playout removes the black stones
    info, stats, first = rg.ld_row(E, dict(stones=RE.straight_three(n), mover=WHITE), 1, 64, 1, RE.S3_BOX, 0)
    assert stats[1] == 64 and first[2, vital] == first[0, vital] > 0


def test_straight_three_rows_of_the_gpu_test():
    """the stated answers hold, under the reference, on every row and seed the GPU test uses"""
    n = 9
    rg, E = RE.reg(n), RE.ref(n)
    import torch
    from elf_amd.engine import LdReading
    rows = RE.s3_rows(n)
    assert len(rows) == 34 and sum(r["defends"] for r in rows) == 17
    for base in RE.S3_ROW_SEEDS:
        for j, r in enumerate(rows):
            info, stats, first = rg.ld_row(E, r["src"], base + j, RE.S3_PLAYOUTS, RE.S3_THRES, r["box"], 0)
            assert RE.s3_holds(r, info, stats, first, RE.S3_PLAYOUTS), (base, j)
            rd = LdReading(n, RE.S3_PLAYOUTS, torch.from_numpy(info[None]), torch.from_numpy(stats[None]), torch.from_numpy(first[None]))
            assert rd.best_move() == [r["vital"]], (base, j)


def test_box_image_and_images():
    n = 9
    for im in RE.s3_images(n):
        inb = RE.reg(n).inbox(im["box"])
        want = LP.sym(n, RE.reg(n).inbox(RE.S3_BOX).astype(np.uint8), im["s"]).astype(bool)
        assert np.array_equal(inb, want)
        assert im["stones"][im["vital"]] == 0 and all(im["stones"][a] == 0 for a in im["others"])
