"""CPU: the C restatement (pyoracle.Port) and the stand-in build of the reference (pyoracle.Ref, oracle/shim on its include path)
against pyoracle.RefBoard -- the reference's base/board.cc + base/common.cc compiled with NO stand-in header at all
(oracle/_ref/libelfboard{19,9}.so, oracle/ref_board_capi.cc).  Every ply: Zobrist hash, info words 0..8 (ply, next player, last two
moves, ko age, simple ko point and colour, captures), per-point colours, group liberties, legal mask; every 8th ply also the true-eye
masks of both colours.  Integer equality throughout.

RefBoard is a plain Board.  Positions that a playout ENDS by super-ko are a GoState-level matter (the hash history lives in
GoState, go_state.cc:96-121): the move lists below stop where GoState stopped them and RefBoard just replays the given moves; the
harness does not restate super-ko, and `terminated` is not among the things compared here."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ownership_expected import ko_moves
from pyoracle import Port, Ref, RefBoard, playout_seeds

REFERENCE_TREE = "/root/reference/src_cpp"


def _need(n):
    if not RefBoard.available(n) and not os.path.isdir(REFERENCE_TREE):
        pytest.skip("oracle/_ref/libelfboard%d.so absent and no reference tree to build it from" % n)
    assert RefBoard.available(n), "build() must have produced oracle/_ref/libelfboard%d.so: the reference tree is present" % n


def engines(n):
    return [Port(n)] + ([Ref(n)] if Ref.available(n) else [])


def agree_every_ply(E, rep, moves, tag):
    """engine E (Port / Ref interface) replays `moves`; after every ply it must hold what RefBoard.replay recorded in `rep`"""
    s = E.new()
    for t in range(len(moves) + 1):
        where = (type(E).__name__, tag, t)
        assert E.hash(s) == int(rep["hash"][t]), where
        assert np.array_equal(E.info(s)[:9], rep["info"][t][:9]), (where, E.info(s), rep["info"][t])
        col, lib = E.board(s)
        assert np.array_equal(col, rep["colour"][t]), where
        assert np.array_equal(lib, rep["libs"][t]), where
        assert np.array_equal(E.legal_mask(s), rep["legal"][t]), where
        if t % 8 == 0:
            for k, player in enumerate((1, 2)):
                assert np.array_equal(E.true_eye_mask(s, player), rep["eyes"][t][k]), (where, player)
        if t < len(moves):
            assert E.forward(s, int(moves[t])) == int(rep["ok"][t]), where
    E.free(s)


def check_games(n, games, tag):
    RB = RefBoard(n)
    reps = [RB.replay(mv) for mv in games]
    for E in engines(n):
        for i, (mv, rep) in enumerate(zip(games, reps)):
            agree_every_ply(E, rep, mv, (tag, i))
    return reps


def test_harness_basics(built):
    """the harness's single-position entry points say what its batched replay says, and FindAllValidMoves is the legal mask's
    points in x-major order"""
    for n in (19, 9):
        _need(n)
        RB, P = RefBoard(n), Port(n)
        s = P.new()
        mv = P.playout_moves(s, 4711, 60)
        P.free(s)
        rep = RB.replay(mv)
        b = RB.new()
        for t in range(len(mv) + 1):
            assert RB.hash(b) == int(rep["hash"][t]) and np.array_equal(RB.info(b), rep["info"][t])
            assert np.array_equal(RB.legal_mask(b), rep["legal"][t])
            assert all(np.array_equal(x, y) for x, y in zip(RB.board(b), (rep["colour"][t], rep["libs"][t])))
            mover = int(rep["info"][t][1])
            assert mover == 1 + t % 2
            vm = RB.valid_moves(b, mover)
            acts = np.nonzero(rep["legal"][t][: n * n])[0]
            assert np.array_equal(vm, [(a % n + 1) * (n + 2) + a // n + 1 for a in acts])
            assert rep["legal"][t][n * n] == 1 and not RB.is_game_end(b)
            if t < len(mv):
                c = RB.clone(b)
                assert RB.play(b, int(mv[t])) == 1 and rep["ok"][t] == 1
                assert RB.hash(c) == int(rep["hash"][t])        # the clone stayed behind
                RB.free(c)
        assert RB.play(b, 0) == 1 and not RB.is_game_end(b)
        assert RB.play(b, 0) == 1 and RB.is_game_end(b)          # two passes: board.cc:2073-2077
        RB.free(b)


def test_config1_sgf_every_ply(built):
    _need(19)
    g = np.load(os.path.join(GOLDEN, "sgf_406844.npz"))
    rep, = check_games(19, [g["moves"].astype(np.int32)], "sgf_406844")
    # the committed fixture (made by the stand-in build) holds what the unshimmed build says
    assert np.array_equal(rep["hash"], g["hash"].astype(np.uint64))
    assert np.array_equal(rep["info"][:, :9], g["info"][:, :9])
    assert np.array_equal(rep["legal"], np.unpackbits(g["mask"], axis=1)[:, :362])
    assert rep["ok"].all()


def test_ladder_suite_every_ply(built):
    _need(19)
    g = np.load(os.path.join(GOLDEN, "ladder_suite.npz"))
    games = [g["moves"][g["offsets"][i]:g["offsets"][i + 1]].astype(np.int32) for i in range(len(g["names"]))]
    reps = check_games(19, games, "ladder")
    for i, rep in enumerate(reps):
        assert rep["ok"].all()
        assert int(rep["hash"][-1]) == int(g["final_hash"][i]) and int(rep["info"][-1][0]) == int(g["final_ply"][i])
        assert np.array_equal(rep["legal"][-1], np.unpackbits(g["final_mask"][i])[:362])


@pytest.mark.parametrize("n,count", [(19, 256), (9, 1024)])
def test_config2_playouts_every_ply(built, n, count):
    """SURVEY.md 8(d) config 2 move lists (random legal non-true-eye play, seeds playout_seeds(count)); the list of a game that
    super-ko ended stops there (GoState-level, see the module docstring)"""
    _need(n)
    P = Port(n)
    games = []
    for sd in playout_seeds(count):
        s = P.new()
        games.append(P.playout_moves(s, int(sd)))
        P.free(s)
    reps = check_games(n, games, "config2")
    assert all(rep["ok"].all() for rep in reps)
    # the candidate list the playout policy draws from, taken from the unshimmed build alone, reproduces every move of the lists
    RB = RefBoard(n)
    for mv, sd in list(zip(games, playout_seeds(count)))[:: max(1, count // 16)]:
        b = RB.new()
        for t, c in enumerate(mv):
            mover = 1 + t % 2
            cand = [int(m) for m in RB.valid_moves(b, mover) if not RB.is_true_eye(b, m, mover)]
            want = cand[playout_rng(int(sd), t + 1) % len(cand)] if cand else 0
            assert want == int(c), (int(sd), t)
            RB.play(b, int(c))
        RB.free(b)


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def playout_rng(seed, t):
    """this project's counter RNG (oracle/go_oracle.c playout_rng): t is the ply counter of the position (1 on the empty board)"""
    key = fmix32(seed & 0xFFFFFFFF) ^ fmix32(((seed >> 32) + 0x7F4A7C15) & 0xFFFFFFFF)
    return fmix32((key + t * 0x9E3779B9) & 0xFFFFFFFF)


@pytest.mark.parametrize("n", [19, 9])
def test_ko_sequence(built, n):
    """the corner ko of tests/ownership_expected.py: after Black takes, White's recapture at (1,0) is refused by every engine and
    the ko words (age, point, colour) agree; after a White move elsewhere and Black's answer the point is open again"""
    _need(n)
    S = n + 2
    recapture = 1 * S + 2                                       # (x, y) = (1, 0)
    away_w, away_b = (n - 1) * S + (n - 1), (n - 2) * S + (n - 2)
    moves = np.array(ko_moves(n) + [recapture, away_w, away_b, recapture], np.int32)
    rep, = check_games(n, [moves], "ko")
    assert list(rep["ok"]) == [1, 1, 1, 1, 1, 0, 1, 1, 1]
    assert int(rep["info"][5][5]) == recapture and int(rep["info"][5][6]) == 2      # simple ko point, forbidden to White
    assert rep["legal"][5][1 * n + 0] == 0 and rep["legal"][8][1 * n + 0] == 1
