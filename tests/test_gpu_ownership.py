"""GPU: elfgo_area_map and elfgo_own_run (k_area_map, k_playout_own) against the CPU oracle's playouts, and the GTP commands
built on them.  Every comparison is integer equality."""
import numpy as np
import pytest

import ownership_expected as oe
from ownership_expected import mixed_rows, oracle, play_all, states_of
from pyoracle import playout_seeds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def check_area(eng, E, states, ids=None):
    n = E.n
    am = eng.area_map(ids, n=len(states)).cpu().numpy()
    val = eng.evaluate(ids, 7.5, n=len(states)).cpu().numpy()
    for i, s in enumerate(states):
        assert np.array_equal(am[i], oe.area_map(E.board(s)[0], n)), i
        if not oe.ended_by_superko(E, s):
            assert oe.area_diff(am[i]) - 7.5 == val[i], i


@pytest.mark.parametrize("n,plies", [(9, (20, 40)), (19, (60, 200))])
def test_area_map(elf, n, plies):
    E = oracle(n)
    lists = oe.area_test_lists(E, n, plies)
    eng = elf.GoEngine(n, len(lists), 0)
    play_all(eng, lists)
    states = states_of(E, lists)
    assert int(E.info(states[3])[0]) > 1
    check_area(eng, E, states)
    # the same boards played to the end
    pseeds = playout_seeds(len(lists), base=500)
    eng.playout(pseeds)
    for s, sd in zip(states, pseeds):
        E.playout_moves(s, int(sd))
        assert E.terminated(s)
    check_area(eng, E, states)


@pytest.mark.parametrize("n", [9, 19])
def test_one_playout_is_the_playout_kernels_game(elf, n):
    """ownership(K=1) of a slot == the area map of a copy of that slot after eng.playout with the same seed; same step count"""
    E = oracle(n)
    lists = mixed_rows(E, n)
    k = len(lists)
    eng = elf.GoEngine(n, 2 * k, 0)
    play_all(eng, lists)
    eng.copy(list(range(k, 2 * k)), list(range(k)))
    seeds = playout_seeds(k, base=9)
    own = eng.ownership(seeds, ids=list(range(k)), playouts=1)
    out = eng.playout(seeds, ids=list(range(k, 2 * k))).cpu().numpy().view(np.uint32)
    am = eng.area_map(list(range(k, 2 * k))).cpu().numpy()
    counts, stats = own["counts"].cpu().numpy(), own["stats"].cpu().numpy()
    assert np.array_equal(counts[:, 0], (am == 1).astype(np.int32)) and np.array_equal(counts[:, 1], (am == 2).astype(np.int32))
    assert np.array_equal(stats[:, 3], out[:, 3].astype(np.int64))
    assert stats[4, 3] == 0                       # the finished game plays no step


@pytest.mark.parametrize("n,K", [(9, 128), (19, 64)])
def test_ownership_equals_the_oracle_and_leaves_the_sources_alone(elf, n, K):
    """mixed rows in one call (the late-game slot twice, with different seeds), komi 7.5 and 0.5: counts and all four stats
    equal the oracle's; afterwards the source slots are what they were -- info, stones, legal mask, features -- and go on to
    the oracle's playout result, which needs their super-ko records and Bloom words intact."""
    E = oracle(n)
    lists = mixed_rows(E, n)
    k = len(lists)
    eng = elf.GoEngine(n, k, 0)
    play_all(eng, lists)
    states = states_of(E, lists)
    assert int(E.info(states[3])[5]) != 0 and int(E.info(states[3])[4]) == 0      # the simple ko is live
    assert E.terminated(states[4])
    ids = list(range(k)) + [2]
    seeds = playout_seeds(len(ids), base=1000)

    def snapshot():
        col, lib = eng.export_board()
        return [t.cpu().numpy() for t in (eng.info(), col, lib, eng.legal_mask(), eng.extract_agz())]

    before = snapshot()
    for komi in (7.5, 0.5):
        own = eng.ownership(seeds, ids=ids, playouts=K, komi=komi)
        counts, stats = own["counts"].cpu().numpy(), own["stats"].cpu().numpy()
        for r, (i, sd) in enumerate(zip(ids, seeds)):
            wc, ws = oe.expected(E, states[i], sd, K, komi)
            print("n=%d komi=%.1f row %d: stats %s expected %s" % (n, komi, r, stats[r].tolist(), ws.tolist()))
            assert np.array_equal(counts[r], wc), (komi, r)
            assert np.array_equal(stats[r], ws), (komi, r)
        assert np.array_equal(own["own"].cpu().numpy(), ((counts[:, 0] - counts[:, 1]) / np.float32(K)).astype(np.float32))
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    pseeds = playout_seeds(k, base=77)
    out = eng.playout(pseeds).cpu().numpy().view(np.uint32)
    for i, (s, sd) in enumerate(zip(states, pseeds)):
        mv = E.playout_moves(s, int(sd))
        h = E.hash(s)
        assert (int(out[i, 0]), int(out[i, 1]), int(out[i, 2]), int(out[i, 3])) == (h & 0xFFFFFFFF, h >> 32, int(E.info(s)[0]), len(mv)), i


def test_many_more_playouts_than_lanes(elf):
    """one 9x9 row, 4096 playouts on 64 lanes: equal to the oracle, to the default geometry and to a second run"""
    n, K = 9, 4096
    E = oracle(n)
    mv = oe.prefix(E, 12345, 30)[1]
    eng = elf.GoEngine(n, 2, 0)
    play_all(eng, [[], mv])
    src = states_of(E, [mv])[0]
    seed = np.array([0xDEADBEEF12345678], np.uint64)
    wc, ws = oe.expected(E, src, seed[0], K, 7.5)
    runs = [eng.ownership(seed, ids=[1], playouts=K, max_lanes=lanes) for lanes in (64, 64, 0)]
    for own in runs:
        assert np.array_equal(own["counts"].cpu().numpy()[0], wc)
        assert np.array_equal(own["stats"].cpu().numpy()[0], ws)


def test_gtp_final_status_list(elf):
    """A 9x9 position in which White has plainly lost stones: the dead / alive lists and the score estimate are the rule of
    GtpEngine.on_final_status_list applied to the oracle's counts for status_seed."""
    import torch
    from elf_amd.gtp import GtpEngine, move2xy, xy2move
    n, K, seed = 9, 128, 7

    def actor(batch):
        b = batch["s"].shape[0]
        return dict(pi=torch.full((b, n * n + 1), 1.0 / (n * n + 1), device="cuda"), V=torch.zeros(b, device="cuda"))

    eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=16, nodes_per_game=1024, status_playouts=K, status_seed=seed)
    E = oracle(n)
    st = E.new()
    black = ["C3", "C5", "C7", "E3", "E5", "E7", "G3", "G5", "G7", "D4", "F6", "D6", "F4"]
    white = ["A1", "J9"] + ["pass"] * (len(black) - 2)
    for b, w in zip(black, white):
        for colour, mv in (("b", b), ("w", w)):
            assert eng.command("play %s %s" % (colour, mv)) == "= \n\n"
            x, y = move2xy(mv)
            assert E.forward(st, 0 if x < 0 else (y + 1) * (n + 2) + (x + 1)) == 1
    score = E.evaluate(st, 7.5)
    final = "= %s\n\n" % (("B+%.1f" % score) if score > 0 else ("W+%.1f" % -score))
    assert eng.command("final_score") == final
    counts, _ = oe.expected(E, st, seed, K, 7.5)
    col = E.board(st)[0]
    dead = ((col == 1) & (counts[1] > counts[0])) | ((col == 2) & (counts[0] > counts[1]))
    names = lambda m: " ".join(xy2move(a // n, a % n) for a in range(n * n) if m[a])
    assert eng.command("final_status_list dead") == "= %s\n\n" % names(dead)
    assert eng.command("final_status_list alive") == "= %s\n\n" % names((col != 0) & ~dead)
    assert names(dead).split() == ["A1", "J9"]
    assert eng.command("final_status_list seki") == "= \n\n"
    assert eng.command("final_status_list foo").startswith("?") and eng.command("final_status_list").startswith("?")
    est = float(int((counts[0] > counts[1]).sum()) - int((counts[1] > counts[0]).sum())) - 7.5
    assert eng.command("elf-score_estimate") == "= %s\n\n" % (("B+%.1f" % est) if est > 0 else ("W+%.1f" % -est))
    rows = eng.command("elf-ownership").strip("=\n ").split("\n")
    assert len(rows) == n and all(len(r.split()) == n for r in rows)
    own = (counts[0] - counts[1]).reshape(n, n) / float(K)
    assert rows[0].split() == ["%.2f" % own[x, n - 1] for x in range(n)]
    assert "final_status_list" in eng.command("list_commands") and "elf-ownership" in eng.command("list_commands")
    assert eng.command("final_score") == final            # the reference's meaning, untouched by the new commands
    eng.close()
