"""GPU: position setup (elfgo_setup / k_setup), undo and set-up games in a self-play context, and the GTP commands on top.

What a set-up slot must hold comes from the reference's own board engine (pyoracle.RefBoard.replay rows, read from
oracle/_ref) and from twin slots that PLAYED the same game with the existing kernels; every comparison is integer equality."""
import json

import numpy as np
import pytest

import setup_expected as SE
from pyoracle import Port, Ref, RefBoard

pytestmark = pytest.mark.gpu

ELFGO_E_BADARG = -1


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def _need(n):
    assert RefBoard.available(n), "build() must have produced oracle/_ref/libelfboard%d.so" % n


def npy(t):
    return t.cpu().numpy()


def hash_of(info):
    return info[:, 13].astype(np.uint32).astype(np.uint64) | (info[:, 14].astype(np.uint32).astype(np.uint64) << np.uint64(32))


def snapshot(eng, ids):
    """everything a slot shows: info (16 words), colour, liberties, legal mask, the planes under all 8 D4 codes"""
    ids = list(ids)
    col, lib = eng.export_board(ids)
    return dict(info=npy(eng.info(ids)), col=npy(col), lib=npy(lib), mask=npy(eng.legal_mask(ids)),
                planes=np.stack([npy(eng.extract_agz(ids, d4=[d] * len(ids))) for d in range(8)]))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def pick(snap, idx):
    """the rows `idx` of a snapshot"""
    return {k: (v[:, idx] if k == "planes" else v[idx]) for k, v in snap.items()}


def games_of(n):
    return SE.ladder_games() if n == 19 else SE.nine_games(Port(9))


def make_actor(n, seed=0):
    """the stub actor of the GTP tests"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)

    def actor(batch):
        b = batch["s"].shape[0]
        pi = torch.softmax(2.0 * torch.randn((b, n * n + 1), device="cuda", generator=g), dim=1)
        v = torch.round(torch.tanh(torch.randn((b,), device="cuda", generator=g)) * 64) / 64
        return dict(pi=pi, V=v)
    return actor


# ---- 5. setup equals the reference's position ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_setup_equals_the_reference(elf, n):
    _need(n)
    games = games_of(n)
    cs, cnt = SE.cases(RefBoard(n), games)
    K = len(cs)
    if n == 19:
        assert K == 1177
    eng = elf.GoEngine(n, 2 * K)
    stones = np.stack([rep["colour"][u] for _, u, rep in cs])
    players = np.array([rep["info"][u][1] for _, u, rep in cs], np.uint8)
    ok = npy(eng.setup(stones, ids=np.arange(K), next_player=players))        # ONE launch
    assert (ok == 1).all()
    col, lib = eng.export_board(np.arange(K))
    info = npy(eng.info(np.arange(K)))
    assert np.array_equal(npy(col), stones)
    assert np.array_equal(npy(lib), np.stack([rep["libs"][u] for _, u, rep in cs]))
    assert np.array_equal(hash_of(info), np.array([rep["hash"][u] for _, u, rep in cs], np.uint64))
    assert np.array_equal(info[:, 1], players) and (info[:, 0] == 1).all()                # next player, ply 1
    assert (info[:, 2] == 3).all() and (info[:, 3] == 3).all()                            # last moves M_INVALID
    assert (info[:, 4:11] == 0).all()                                                     # no ko, no captures, not terminated
    assert (info[:, 11] == 1).all() and (info[:, 12] == 0).all()                          # hist_len 1, sk_len 0
    # no ko is pending at these plies, so the masks agree on all N*N + 1 entries
    assert np.array_equal(npy(eng.legal_mask(np.arange(K))), np.stack([rep["legal"][u] for _, u, rep in cs]))
    # twins that played the game to that ply
    us = np.array([u for _, u, _ in cs])
    for t in range(int(us.max())):
        idx = np.nonzero(us > t)[0]
        okf = npy(eng.forward(K + idx, [int(games[cs[j][0]][t]) for j in idx]))
        assert (okf == 1).all()
    twins = K + np.arange(K)
    assert np.array_equal(hash_of(npy(eng.info(twins))), hash_of(info))
    assert np.array_equal(npy(eng.area_map(np.arange(K))), npy(eng.area_map(twins)))
    assert np.array_equal(npy(eng.evaluate(np.arange(K), komi=7.5)), npy(eng.evaluate(twins, komi=7.5)))
    eng.close()


# ---- 6 / 7. the tables it builds survive play; planes --------------------------------------------------------------------------
def _sixteen(n=19):
    RB = RefBoard(n)
    out = []
    for mv in SE.ladder_games():
        if len(mv) < 100:
            continue
        rep = RB.replay(mv)
        u = SE.first_no_ko(SE.ko_pending(rep["info"]), 60)
        assert u is not None
        out.append((mv, rep, u))
        if len(out) == 16:
            break
    assert len(out) == 16
    return out


def _setup_sixteen(elf, gs, n=19):
    eng = elf.GoEngine(n, len(gs))
    ok = eng.setup(np.stack([rep["colour"][u] for _, rep, u in gs]), next_player=np.array([rep["info"][u][1] for _, rep, u in gs], np.uint8))
    assert (npy(ok) == 1).all()
    return eng


def test_tables_survive_play(elf):
    _need(19)
    gs = _sixteen()
    eng = _setup_sixteen(elf, gs)
    steps = max(len(mv) - u for mv, _, u in gs)
    checked = 0
    for k in range(1, steps + 1):
        idx = [j for j, (mv, _, u) in enumerate(gs) if u + k <= len(mv)]
        okf = npy(eng.forward(idx, [int(gs[j][0][gs[j][2] + k - 1]) for j in idx]))
        assert (okf == 1).all(), k
        col, lib = eng.export_board(idx)
        col, lib, info, mask = npy(col), npy(lib), npy(eng.info(idx)), npy(eng.legal_mask(idx))
        for r, j in enumerate(idx):
            mv, rep, u = gs[j]
            t = u + k
            where = (j, t)
            assert np.array_equal(col[r], rep["colour"][t]) and np.array_equal(lib[r], rep["libs"][t]), where
            assert int(hash_of(info[r:r + 1])[0]) == int(rep["hash"][t]), where
            assert np.array_equal(mask[r], rep["legal"][t]), where
            assert info[r][1] == rep["info"][t][1] and info[r][0] == 1 + k, where
            assert info[r][2] == rep["info"][t][2], where                                           # last move
            assert info[r][7] == rep["info"][t][7] - rep["info"][u][7] and info[r][8] == rep["info"][t][8] - rep["info"][u][8], where
            checked += 1
    assert checked > 16 * 40
    eng.close()


def test_planes_after_setup(elf):
    _need(19)
    E = Ref(19) if Ref.available(19) else Port(19)
    gs = _sixteen()
    eng = _setup_sixteen(elf, gs)
    states = []
    for mv, _, u in gs:
        s = E.new()
        for c in mv[:u]:
            assert E.forward(s, int(c)) == 1
        states.append(s)
    G = len(gs)
    for k in range(0, 11):
        if k:
            assert (npy(eng.forward(None, [int(mv[u + k - 1]) for mv, _, u in gs])) == 1).all()
            for s, (mv, _, u) in zip(states, gs):
                assert E.forward(s, int(mv[u + k - 1])) == 1
        for d4 in range(8):
            got = npy(eng.extract_agz(d4=[d4] * G))
            for j, s in enumerate(states):
                want = E.extract_agz(s, d4)
                top = min(2 * k + 2, 16)
                assert np.array_equal(got[j][:top], want[:top]), (j, k, d4)
                assert not got[j][top:16].any(), (j, k, d4)
                assert np.array_equal(got[j][16:], want[16:]), (j, k, d4)
                if k >= 7:
                    assert np.array_equal(got[j], want), (j, k, d4)
    for s in states:
        E.free(s)
    eng.close()


# ---- 8. super-ko after a setup -------------------------------------------------------------------------------------------------
# A 9x9 game that ends on a positional repetition (a send-two-return-one cycle on the edge): the position after move 76 is the
# position after move 73.  Reference Coords.
from superko_lines import SUPERKO_GAME  # noqa: E402  (the search's own tests walk the same game: tests/superko_lines.py)


def test_superko_after_setup(elf):
    n = 9
    _need(n)
    mv = np.array(SUPERKO_GAME, np.int32)
    L = len(mv)
    rep = RefBoard(n).replay(mv)
    assert rep["ok"].all()
    assert [t for t in range(L) if np.array_equal(rep["colour"][t], rep["colour"][L])] == [73]   # the one earlier occurrence
    P = Port(n)
    s = P.new()
    for c in mv:
        assert not P.terminated(s) and P.forward(s, int(c)) == 1
    assert P.terminated(s)                                     # the oracle's GoState ends this game on the repetition
    P.free(s)
    pend = SE.ko_pending(rep["info"])
    starts = [40, 70, 73]                                      # 73: the set-up position itself is the one that repeats
    assert not pend[starts].any()
    eng = elf.GoEngine(n, 1 + len(starts))
    ok = eng.setup(np.stack([rep["colour"][t] for t in starts]), ids=[1 + i for i in range(len(starts))],
                   next_player=np.array([rep["info"][t][1] for t in starts], np.uint8))
    assert (npy(ok) == 1).all()
    for t in range(L):
        live = [0] + [1 + i for i, t0 in enumerate(starts) if t0 <= t]
        assert (npy(eng.forward(live, [int(mv[t])] * len(live))) == 1).all(), t
        info = npy(eng.info(live))
        assert (info[:, 9] == info[0, 9]).all() and (info[:, 10] == info[0, 10]).all(), t      # terminated, superko
        assert (hash_of(info) == np.uint64(rep["hash"][t + 1])).all(), t
        assert info[0, 10] == (1 if t == L - 1 else 0), t
    assert len(live) == 1 + len(starts) and (info[:, 10] == 1).all()
    assert (npy(eng.forward(live, [0] * len(live))) == 0).all()                                 # a terminated game takes no move
    eng.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_refusals_leave_the_slot_alone(elf, n):
    import torch
    eng = elf.GoEngine(n, 6)
    S = n + 2
    for c in (2 * S + 3, 3 * S + 3, 4 * S + 5, 3 * S + 2, 5 * S + 5):      # every slot holds a position with some history
        assert (npy(eng.forward(None, [c] * 6)) == 1).all()
    before = snapshot(eng, range(6))
    good = np.zeros(n * n, np.uint8)
    good[[0, n + 1, 3 * n + 3]] = 1
    good[[1, 2 * n + 2]] = 2
    dead = np.zeros(n * n, np.uint8)                 # a white corner stone with both its neighbours black
    dead[0] = 2
    dead[[1, n]] = 1
    big = np.ones(n * n, np.uint8)                   # a full board: one group, no liberty
    three = good.copy()
    three[n * n - 1] = 3
    rows = np.stack([good, dead, three, good, big, good])
    players = np.array([1, 1, 2, 0, 1, 2], np.uint8)
    ok = npy(eng.setup(rows, next_player=players))
    assert list(ok) == [1, 0, 0, 0, 0, 1]
    after = snapshot(eng, range(6))
    assert same(pick(before, [1, 2, 3, 4]), pick(after, [1, 2, 3, 4]))          # info, board, mask, planes: unchanged
    for j in (0, 5):
        libs, h, zero = SE.restate(good, n)
        assert not zero and np.array_equal(after["col"][j], good) and np.array_equal(after["lib"][j], libs)
        assert int(hash_of(after["info"][j:j + 1])[0]) == h and after["info"][j][1] == players[j] and after["info"][j][0] == 1
    # player 3 and a NULL player array (= Black)
    ok = npy(eng.setup(good, ids=[2], next_player=[3]))
    assert list(ok) == [0]
    ok = npy(eng.setup(np.stack([good, good]), ids=[3, 4]))
    assert list(ok) == [1, 1] and (npy(eng.info([3, 4]))[:, 1] == 1).all()
    torch.cuda.synchronize()
    eng.close()


# ---- 10. round trip and scale --------------------------------------------------------------------------------------------------
def test_round_trip_4096(elf):
    from pyoracle import playout_seeds
    n, K = 19, 4096
    eng = elf.GoEngine(n, 2 * K)
    src, dst = np.arange(K), K + np.arange(K)
    out = npy(eng.playout(playout_seeds(K), ids=src, max_steps=160)).astype(np.uint32)
    sinfo = npy(eng.info(src))
    assert (sinfo[:, 0] > 100).mean() > 0.9                    # mid-game positions
    col, lib = eng.export_board(src)
    ok = eng.setup(col, dst, next_player=sinfo[:, 1].astype(np.uint8))
    assert (npy(ok) == 1).all()
    dcol, dlib = eng.export_board(dst)
    dinfo = npy(eng.info(dst))
    assert np.array_equal(npy(dcol), npy(col)) and np.array_equal(npy(dlib), npy(lib))
    assert np.array_equal(hash_of(dinfo), hash_of(sinfo))
    assert np.array_equal(npy(eng.area_map(dst)), npy(eng.area_map(src)))
    no_ko = ~((sinfo[:, 5] != 0) & (sinfo[:, 4] == 0))
    assert no_ko.sum() > K // 2
    assert np.array_equal(npy(eng.legal_mask(dst))[no_ko], npy(eng.legal_mask(src))[no_ko])
    eng.playout(playout_seeds(K), ids=dst)
    assert (npy(eng.info(dst))[:, 9] == 1).all()               # every copy plays to the end of a game
    eng.close()


# ---- 11. undo ------------------------------------------------------------------------------------------------------------------
def _four_games():
    gs = [mv for mv in SE.ladder_games() if len(mv) >= 40][:4]
    assert len(gs) == 4
    return np.stack([mv[:30] for mv in gs])          # [4, 30]


def _played(elf, moves, k, n=19):
    """a fresh engine whose slot g played moves[g][:k]"""
    eng = elf.GoEngine(n, moves.shape[0])
    for t in range(k):
        assert (npy(eng.forward(None, moves[:, t])) == 1).all()
    return eng


def test_undo(elf):
    import torch
    from elf_amd._lib import ElfGoError
    from elf_amd.train import sgfstr_to_coords
    n, G = 19, 4
    moves = _four_games()
    actor = make_actor(n)
    sp = elf.SelfPlay(board_size=n, num_games=G, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048,
                      keep_records=8, seed=5)
    sp.reg_callback("actor_black", actor)
    boards = sp.board_engine()
    for t in range(30):
        sp.play(moves[:, t])
    s30 = snapshot(boards, range(G))
    sp.undo(7)
    f23 = _played(elf, moves, 23)
    s23 = snapshot(boards, range(G))
    assert same(s23, snapshot(f23, range(G)))                  # info (all 16 words), board, mask, all 8 plane sets
    # more moves than were played: refused, nothing changes
    with pytest.raises(ElfGoError):
        sp.undo(24)
    assert sp.L.elfsp_undo(sp._h, np.arange(G, dtype=np.int32).ctypes.data, G, 0, None) == ELFGO_E_BADARG
    assert same(s23, snapshot(boards, range(G)))
    # the 7 moves again: the state before the undo
    for t in range(23, 30):
        sp.play(moves[:, t])
    assert same(s30, snapshot(boards, range(G)))
    sp.undo(7)
    assert same(s23, snapshot(boards, range(G)))
    # while a search is open
    base = sp.progress()["searches"]
    rows = sp.begin_step()
    assert rows > 0
    with pytest.raises(ElfGoError):
        sp.undo(1)
    reply = actor({"s": sp.s[:rows]})
    sp.end_step(reply["pi"], reply["V"])
    # the search runs to a legal move (an error word such as ELFMCTS_E_ROOT_HASH would raise)
    P = Port(n)
    while sp.progress()["searches"] < base + G:
        sp.run()
    assert sp.progress()["open"] == 0
    last = sp.last_moves()
    info = boards.info_host(n=G)
    for g in range(G):
        s = P.new()
        for c in moves[g][:23]:
            P.forward(s, int(c))
        assert P.forward(s, int(last[g])) == 1 and int(info["hash"][g]) == P.hash(s) and int(info["ply"][g]) == 25
        P.free(s)
    # a search move taken back takes its predicted value with it
    sp.undo(1, [0])
    assert same(pick(s23, [0]), snapshot(boards, [0]))
    sp.finish(list(range(G)), 2)
    recs = [json.loads(r) for r in sp.pop_records()]
    assert len(recs) == G
    for j in recs:
        g = int(j["thread_id"])
        want = [int(c) for c in moves[g][:23]] + ([] if g == 0 else [int(last[g])])
        assert [int(c) for c in sgfstr_to_coords(n, j["result"]["content"])] == want, g
        assert j["result"]["num_move"] == len(want) and len(j["result"]["values"]) == (0 if g == 0 else 1), g
    torch.cuda.synchronize()
    f23.close()
    boards.close()
    sp.close()


def test_undo_rebuilds_superko_records(elf):
    """playout with one seed from the undone game boards and from fresh slots that played the same 23 moves: the same
    {hash, ply, steps} -- the playouts read the super-ko records and Bloom words the undo rebuilt"""
    from pyoracle import playout_seeds
    n, G = 19, 4
    moves = _four_games()
    sp = elf.SelfPlay(board_size=n, num_games=G, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048, seed=5)
    boards = sp.board_engine()
    for t in range(30):
        sp.play(moves[:, t])
    sp.undo(7)
    f23 = _played(elf, moves, 23)
    seeds = playout_seeds(1).repeat(G)
    a, b = npy(boards.playout(seeds)), npy(f23.playout(seeds))
    assert np.array_equal(a, b) and (a[:, 3] > 50).all()
    assert same(snapshot(boards, range(G)), snapshot(f23, range(G)))
    f23.close()
    boards.close()
    sp.close()


# ---- 12. set-up games in a context ---------------------------------------------------------------------------------------------
def test_setup_games_in_a_context(elf):
    from elf_amd._lib import ElfGoError
    from elf_amd.gtp import HANDICAP_VERTICES, move2xy
    n, G = 19, 2
    actor = make_actor(n, 1)
    sp = elf.SelfPlay(board_size=n, num_games=G, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048,
                      keep_records=8, seed=7)
    sp.reg_callback("actor_black", actor)
    boards = sp.board_engine()
    st = np.zeros(n * n, np.uint8)
    for v in HANDICAP_VERTICES[4]:
        x, y = move2xy(v)
        st[x * n + y] = 1
    sp.setup(st, [0], 2)
    info = boards.info_host(n=G)
    assert list(info["next_player"]) == [2, 1] and list(info["ply"]) == [1, 1] and list(info["hist_len"]) == [1, 0]
    assert np.array_equal(npy(boards.export_board([0])[0])[0], st)
    mask = npy(boards.legal_mask([0]))[0]
    assert mask[: n * n].sum() == n * n - 4
    while sp.progress()["searches"] < G:
        sp.run()
    c = int(sp.last_moves()[0])
    x, y = c % (n + 2) - 1, c // (n + 2) - 1
    assert c == 0 or mask[x * n + y] == 1                       # a legal White move
    info = boards.info_host(n=G)
    assert list(info["next_player"]) == [1, 2] and list(info["ply"]) == [2, 2]
    col = npy(boards.export_board([0])[0])[0]
    assert (col == 1).sum() == 4 and (col == 2).sum() == (0 if c == 0 else 1)
    # set up after a move: refused
    with pytest.raises(ElfGoError):
        sp.setup(st, [1], 2)
    # two passes finish the set-up game like any other -- but it leaves no Record
    pending = sp.L.elfsp_records_pending(sp._h)
    if c != 0:
        sp.play([0, -1])                                        # Black passes
    want = float(npy(boards.evaluate([0], komi=7.5))[0])       # passes do not change the score
    sp.play([0, -1])                                            # the second pass in a row
    assert float(sp.last_score()[0]) == want
    out = np.zeros(8, np.float32)
    assert sp.L.elfsp_take_finished(sp._h, out.ctypes.data, 8) == 1 and float(out[0]) == want
    assert sp.L.elfsp_records_pending(sp._h) == pending == 0
    info = boards.info_host(n=G)
    assert int(info["ply"][0]) == 1 and int(info["hist_len"][0]) == 0      # restarted from the empty board
    sp.finish([1], 2)                                                       # a game that was not set up does leave one
    assert sp.L.elfsp_records_pending(sp._h) == 1
    # a set-up game can be undone back to its stones
    sp.setup(st, [0], 2)
    S = n + 2
    sp.play([3 * S + 3, -1])
    sp.play([3 * S + 4, -1])
    sp.undo(2, [0])
    info = boards.info_host(n=G)
    assert int(info["ply"][0]) == 1 and int(info["next_player"][0]) == 2 and int(info["sk_len"][0]) == 0
    assert np.array_equal(npy(boards.export_board([0])[0])[0], st)
    with pytest.raises(ElfGoError):
        sp.undo(1, [0])
    boards.close()
    sp.close()


# ---- 13. GTP -------------------------------------------------------------------------------------------------------------------
JAPANESE_HANDICAP = ("(;GM[1]FF[4]CA[UTF-8]AP[CGoban:3]ST[2]RU[Japanese]SZ[9]HA[2]RE[Void]KM[5.50]PW[test_white]PB[test_black]"
                     "AB[gc][cg];W[ee];B[dg])")


def _board_rows(text):
    """showboard reply -> {(x, y): '.', 'X' or 'O'}"""
    out = {}
    for line in text.split("\n"):
        p = line.split()
        if len(p) > 2 and p[0].isdigit() and p[-1] == p[0]:
            for x, ch in enumerate(p[1:-1]):
                out[(x, int(p[0]) - 1)] = ch
    return out


def test_gtp_handicap_undo(elf):
    from elf_amd.gtp import GtpEngine, move2xy
    n = 19
    eng = GtpEngine(make_actor(n), board_size=n, mcts_rollout_per_thread=32, nodes_per_game=2048)
    assert eng.command("known_command undo") == "= true\n\n" and eng.command("known_command foo") == "= false\n\n"
    lc = eng.command("list_commands")
    for c in ("undo", "fixed_handicap", "place_free_handicap", "set_free_handicap", "loadsgf", "known_command"):
        assert c in lc.split()
    assert eng.command("undo") == "? cannot undo\n\n"
    assert eng.command("fixed_handicap 1") == "? invalid handicap\n\n" and eng.command("fixed_handicap 10") == "? invalid handicap\n\n"
    assert eng.command("fixed_handicap 4") == "= D4 Q16 D16 Q4\n\n"
    sb = eng.command("showboard")
    rows = _board_rows(sb)
    assert {k for k, v in rows.items() if v == "X"} == {move2xy(v) for v in ("D4", "Q16", "D16", "Q4")}
    assert "O" not in rows.values() and "Next: W" in sb
    assert eng.command("fixed_handicap 2") == "? board not empty\n\n"
    r = eng.command("genmove w")
    assert r.startswith("= ") and r[2:].strip() not in ("resign",)
    assert int(eng.boards.info_host(n=1)["ply"][0]) == 2
    assert eng.command("undo") == "= \n\n"
    info = eng.boards.info_host(n=1)
    assert int(info["ply"][0]) == 1 and int(info["next_player"][0]) == 2
    assert _board_rows(eng.command("showboard")) == rows
    assert eng.command("undo") == "? cannot undo\n\n"          # the stones are not a move
    assert eng.command("clear_board") == "= \n\n"              # a board that was only set up is cleared
    assert set(_board_rows(eng.command("showboard")).values()) == {"."}
    assert int(eng.boards.info_host(n=1)["hist_len"][0]) == 0
    assert eng.command("set_free_handicap D4") == "? invalid handicap\n\n"
    assert eng.command("set_free_handicap D4 D4") == "? invalid handicap\n\n"
    assert eng.command("set_free_handicap C3 R17 K10") == "= \n\n"
    sb = eng.command("showboard")
    assert {k for k, v in _board_rows(sb).items() if v == "X"} == {move2xy(v) for v in ("C3", "R17", "K10")} and "Next: W" in sb
    assert eng.command("play w E5") == "= \n\n" and eng.command("undo") == "= \n\n"
    assert eng.command("clear_board") == "= \n\n"
    assert eng.command("place_free_handicap 9").split() == ["=", "D4", "Q16", "D16", "Q4", "D10", "Q10", "K16", "K4", "K10"]
    eng.close()
    eng9 = GtpEngine(make_actor(9), board_size=9, mcts_rollout_per_thread=32, nodes_per_game=2048)
    assert eng9.command("fixed_handicap 2") == "? invalid handicap\n\n"     # the reference has no table for 9x9
    eng9.close()


def test_gtp_loadsgf(elf, tmp_path):
    from elf_amd.gtp import GtpEngine
    n = 9
    f = tmp_path / "handicap.sgf"
    f.write_text(JAPANESE_HANDICAP)
    eng = GtpEngine(make_actor(n), board_size=n, mcts_rollout_per_thread=32, nodes_per_game=2048, status_playouts=64)
    assert eng.command("loadsgf %s" % (tmp_path / "missing.sgf")) == "? cannot load file\n\n"
    assert eng.command("loadsgf %s" % f) == "= \n\n"
    rows = _board_rows(eng.command("showboard"))
    assert {k for k, v in rows.items() if v == "X"} == {(6, 2), (2, 6), (3, 6)}        # gc, cg and B[dg]
    assert {k for k, v in rows.items() if v == "O"} == {(4, 4)}                         # W[ee]
    info = eng.boards.info_host(n=1)
    assert int(info["ply"][0]) == 3 and int(info["next_player"][0]) == 2
    assert eng.command("loadsgf %s 2" % f) == "= \n\n"                                  # stops after W[ee]
    rows = _board_rows(eng.command("showboard"))
    assert {k for k, v in rows.items() if v == "X"} == {(6, 2), (2, 6)} and {k for k, v in rows.items() if v == "O"} == {(4, 4)}
    assert int(eng.boards.info_host(n=1)["next_player"][0]) == 1
    assert eng.command("undo") == "= \n\n" and eng.command("undo") == "? cannot undo\n\n"
    assert eng.command("loadsgf %s" % f) == "= \n\n"
    r = eng.command("final_status_list dead")
    assert r.startswith("= ")
    r = eng.command("elf-ownership")
    assert r.startswith("= \n") and len(r.strip().split("\n")) == 1 + n
    # an illegal move in the file: refused, board cleared
    bad = tmp_path / "bad.sgf"
    bad.write_text("(;SZ[9]AB[aa];W[aa])")
    assert eng.command("loadsgf %s" % bad) == "? cannot load file\n\n"
    assert set(_board_rows(eng.command("showboard")).values()) == {"."}
    junk = tmp_path / "junk.sgf"
    junk.write_text("not an sgf")
    assert eng.command("loadsgf %s" % junk) == "? cannot load file\n\n"
    eng.close()


# ---- the side to move of a game that was set up with White to move -------------------------------------------------------------
def _handicap4(n=19):
    from elf_amd.gtp import HANDICAP_VERTICES, move2xy
    st = np.zeros(n * n, np.uint8)
    for v in HANDICAP_VERTICES[4]:
        x, y = move2xy(v)
        st[x * n + y] = 1
    return st


def _constant_value_actor(n, value, seed=2):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)

    def actor(batch):
        b = batch["s"].shape[0]
        pi = torch.softmax(2.0 * torch.randn((b, n * n + 1), device="cuda", generator=g), dim=1)
        return dict(pi=pi, V=torch.full((b,), value, device="cuda"))          # values are Black-positive
    return actor


def test_resignation_follows_the_side_to_move_of_a_setup(elf):
    """The same stones with White to move (game 0) and with Black to move (game 1), 50 moves on, a net that sees Black far
    ahead and a resign threshold of 0.1: the side to move resigns iff it is White.  elfsp_finish(FR_RESIGN): the side to move
    loses -- White in game 0 (+1), Black in game 1 (-1)."""
    n, G = 19, 2
    st = _handicap4(n)
    sp = elf.SelfPlay(board_size=n, num_games=G, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048,
                      resign_thres=0.1, never_resign_prob=0.0, seed=3)
    sp.reg_callback("actor_black", _constant_value_actor(n, 0.96875))
    boards = sp.board_engine()
    sp.setup(np.stack([st, st]), [0, 1], [2, 1])
    sp.finish([0, 1], 0)                                        # FR_RESIGN straight from the set-up positions
    assert list(sp.last_score()) == [1.0, -1.0]
    sp.setup(np.stack([st, st]), [0, 1], [2, 1])
    # 50 moves on points with even x and y: never adjacent to each other, never on a handicap point, so legal for either colour
    pts = [(x, y) for x in range(0, n, 2) for y in range(0, n, 2)][:50]
    for x, y in pts:
        c = (y + 1) * (n + 2) + (x + 1)
        sp.play([c, c])
    info = boards.info_host(n=G)
    assert list(info["ply"]) == [51, 51] and list(info["next_player"]) == [2, 1]
    base = sp.progress()["searches"]
    while sp.progress()["searches"] < base + G:
        sp.run()
    last = sp.last_moves()
    assert int(last[0]) == 1 and float(sp.last_score()[0]) == 1.0            # White, far behind, resigned: Black wins
    assert int(last[1]) != 1                                                  # Black, far ahead, played on
    info = boards.info_host(n=G)
    assert list(info["ply"]) == [1, 52]
    boards.close()
    sp.close()


def test_two_models_follow_the_side_to_move_of_a_setup(elf):
    """Evaluation games (a model for each colour): White's AI (tree pool 1) searches the first move of a game set up with White
    to move, Black's AI (pool 0) the first move of the same stones with Black to move, and they swap for the second move."""
    import torch
    n, G = 19, 2
    st = _handicap4(n)
    sp = elf.SelfPlay(board_size=n, num_games=G, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048, seed=4)
    sp.set_request(0, 1)
    actor = make_actor(n, 5)
    boards = sp.board_engine()
    sp.setup(np.stack([st, st]), [0, 1], [2, 1])

    def step():
        rb, rw = sp.begin_step2()
        who = [sp.L.elfsp_game_actor(sp._h, g) for g in range(G)]
        rep = [None, None]
        for a, (rows, s, ver) in enumerate(((rb, sp.s, 0), (rw, sp.s_white, 1))):
            if rows:
                r = actor({"s": s[:rows]})
                rep[a] = (r["pi"], r["V"], torch.full((rows,), ver, dtype=torch.int64, device=sp.device))
        sp.end_step2(rep)
        return who, (rb, rw)

    who, rows = step()
    assert who == [1, 0] and rows[0] > 0 and rows[1] > 0
    while sp.progress()["searches"] < G:
        step()
    info = boards.info_host(n=G)
    assert list(info["ply"]) == [2, 2] and list(info["next_player"]) == [1, 2]
    who, rows = step()
    assert who == [0, 1]
    while sp.progress()["open"]:
        step()
    boards.close()
    sp.close()


# ---- refusal paths of the context's entry points -------------------------------------------------------------------------------
def test_setup_refused_row_and_partial_undo(elf):
    from elf_amd._lib import ElfGoError
    n, G = 9, 3
    sp = elf.SelfPlay(board_size=n, num_games=G, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, nodes_per_game=2048, seed=6)
    boards = sp.board_engine()
    good = np.zeros(n * n, np.uint8)
    good[[2 * n + 2, 6 * n + 6]] = 1
    dead = np.zeros(n * n, np.uint8)
    dead[0] = 2
    dead[[1, n]] = 1
    with pytest.raises(ElfGoError):
        sp.setup(np.stack([good, dead, good]), [0, 1, 2], [2, 2, 1])
    info = boards.info_host(n=G)
    assert list(info["hist_len"]) == [1, 0, 1] and list(info["next_player"]) == [2, 1, 1] and list(info["ply"]) == [1, 1, 1]
    col = npy(boards.export_board()[0])
    assert np.array_equal(col[0], good) and not col[1].any() and np.array_equal(col[2], good)
    # the refused game is an untouched game: it can still be set up, and is not one that leaves no record
    sp.setup(good, [1], 1)
    # undo of a list in which one game has too few moves: nothing changes for any of them
    S = n + 2
    for c in (4 * S + 4, 5 * S + 5, 4 * S + 6):
        sp.play([c, -1, -1])
    sp.play([-1, 4 * S + 4, -1])
    before = snapshot(boards, range(G))
    with pytest.raises(ElfGoError):
        sp.undo(2, [0, 1])
    with pytest.raises(ElfGoError):
        sp.undo(1)                                               # game 2 has not moved
    assert same(before, snapshot(boards, range(G)))
    sp.undo(1, [0, 1])                                           # and the host lists are intact: both can still be undone
    info = boards.info_host(n=G)
    assert list(info["ply"]) == [3, 1, 1] and list(info["next_player"]) == [2, 1, 1]
    sp.undo(2, [0])
    with pytest.raises(ElfGoError):
        sp.undo(1, [0])
    assert np.array_equal(npy(boards.export_board([0])[0])[0], good)
    boards.close()
    sp.close()


def test_gtp_setup_board_is_scored_and_double_pass_is_not_loadable(elf, tmp_path):
    from elf_amd.gtp import GtpEngine
    n = 9
    eng = GtpEngine(make_actor(n), board_size=n, mcts_rollout_per_thread=32, nodes_per_game=2048)
    # a finished game leaves a last score; a board that is only set up answers with ITS score, not that one
    assert eng.command("play b E5") == "= \n\n" and eng.command("clear_board") == "= \n\n"
    last = eng.command("final_score")
    f = tmp_path / "stones.sgf"
    f.write_text("(;SZ[9]AB[aa][ab][ba]AW[hh][hi][ih][ii])")
    assert eng.command("loadsgf %s" % f) == "= \n\n"
    info = eng.boards.info_host(n=1)
    assert int(info["ply"][0]) == 1 and int(info["next_player"][0]) == 2
    score = float(eng.boards.evaluate(komi=eng.komi, n=1).cpu()[0])
    want = ("B+%.1f" % score) if score > 0 else ("W+%.1f" % -score)
    assert eng.command("final_score") == "= %s\n\n" % want and want == "W+8.5" and want != last[2:].strip()
    # W passes, then W again: the bridging pass would be the second pass in a row and end the game inside the file
    g = tmp_path / "passes.sgf"
    g.write_text("(;SZ[9];B[ee];W[];W[cc];B[dd])")
    assert eng.command("loadsgf %s" % g) == "? cannot load file\n\n"
    assert int(eng.boards.info_host(n=1)["hist_len"][0]) == 0
    eng.close()
