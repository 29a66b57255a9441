"""GPU: elfgo_candidates (k_candidates), elfgo_playout_cand (k_playout_cand) and elfgo_own_run_cand (k_playout_own<N, CandPolicy>)
against the reference's own FindAllCandidateMoves / isSelfAtari (candidates_expected, proven by tests/test_candidates_cpu.py).  Every
comparison is integer equality; every expected number is computed by the reference at test time, once per process."""
import ctypes as C
import os

import numpy as np
import pytest

import candidates_expected as CE
import ownership_expected as OE
import setup_expected as SE
from pyoracle import Ref, RefBoard, playout_seeds

pytestmark = pytest.mark.gpu

NO = CE.NO_THRES


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    assert RefBoard.available(9) and RefBoard.available(19) and Ref.available(9) and Ref.available(19), \
        "build() must have produced oracle/_ref/libelfboard{9,19}.so and libelfref{9,19}.so"
    return elf_amd


def npy(t):
    return t.cpu().numpy()


def u32(t):
    return npy(t).astype(np.uint32)


def words(h, ply, steps):
    return (h & 0xFFFFFFFF, h >> 32, ply, steps)


# ---- 1. mask and stones on every ply of whole games ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nine", "ladder16", "playout19"])
def test_every_ply_equals_the_reference(elf, name):
    import torch
    n, games, exp = CE.all_expected(name)
    eng = elf.GoEngine(n, len(games))
    got = {t: [] for t in CE.THRESHOLDS}
    stones, legal, order = [], [], []
    longest = max(len(m) for m in games)
    for t in range(longest + 1):
        live = [i for i, m in enumerate(games) if t <= len(m)]
        for th in CE.THRESHOLDS:
            m, s = eng.candidates(live, self_atari_thres=th)
            got[th].append(m)
            if th == CE.THRESHOLDS[0]:
                stones.append(s)
            else:
                assert torch.equal(s, stones[-1]), "stones does not depend on the threshold"
        legal.append(eng.legal_mask(live)[:, :-1])
        order += [(i, t) for i in live]
        fwd = [i for i in live if t < len(games[i])]
        if fwd:
            ok = eng.forward(fwd, [int(games[i][t]) for i in fwd])
            assert bool((ok == 1).all())
    got = {th: npy(torch.cat(v)) for th, v in got.items()}
    stones, legal = npy(torch.cat(stones)), npy(torch.cat(legal))
    eng.close()
    want_s = np.array([exp[i]["stones"][t] for i, t in order])
    assert np.array_equal(stones, want_s), "stones: first differing (game, ply) %s" % (order[int(np.nonzero((stones != want_s).any(axis=1))[0][0])],)
    for th in CE.THRESHOLDS:
        want_m = np.array([exp[i]["mask"][th][t] for i, t in order])
        bad = np.nonzero((got[th] != want_m).any(axis=1))[0]
        assert bad.size == 0, "mask at thres %d: first differing (game, ply) %s" % (th, order[int(bad[0])])
    eyes = np.array([exp[i]["eyes"][t] for i, t in order])
    assert np.array_equal(got[NO], legal & (1 - eyes)), "no threshold: legal_mask minus the mover's own true eyes"
    assert np.array_equal(legal, np.array([exp[i]["legal"][t] for i, t in order]))
    print("%s: %d positions, %d self-atari points, largest %d" % (name, len(order), int((stones > 0).sum()), int(stones.max())))


# ---- 2. constructed positions, all 16 images -----------------------------------------------------------------------------------
def setup_rows(eng, rows, n):
    plain = [j for j, r in enumerate(rows) if r["moves"] is None]
    ok = eng.setup(np.array([rows[j]["stones"] for j in plain]), ids=plain, next_player=[rows[j]["mover"] for j in plain])
    assert (npy(ok) == 1).all()
    played = [j for j, r in enumerate(rows) if r["moves"] is not None]
    for t in range(max(len(rows[j]["moves"]) for j in played)):
        idx = [j for j in played if t < len(rows[j]["moves"])]
        assert (npy(eng.forward(idx, [int(rows[j]["moves"][t]) for j in idx])) == 1).all()
    K = len(rows)
    assert np.array_equal(npy(eng.export_board(n=K)[0]), np.array([r["stones"] for r in rows]))
    assert np.array_equal(npy(eng.info(n=K))[:, 1], np.array([r["mover"] for r in rows]))


@pytest.mark.parametrize("n", [9, 19])
def test_constructed_positions(elf, n):
    _, rows = CE.expected(n)
    K = len(rows)
    eng = elf.GoEngine(n, K)
    setup_rows(eng, rows, n)
    want_s = np.array([r["stones_sa"] for r in rows])
    for th in CE.CONSTRUCTED_THRESHOLDS:
        m, s = [npy(t) for t in eng.candidates(n=K, self_atari_thres=th)]
        want_m = np.array([r["mask"][th] for r in rows])
        bad = [(r["name"], r["s"], r["swapped"]) for j, r in enumerate(rows)
               if not (np.array_equal(m[j], want_m[j]) and np.array_equal(s[j], want_s[j]))]
        assert not bad, (th, bad[:8])
    # the played points themselves (what the CPU test pins on the reference)
    _, s = [npy(t) for t in eng.candidates(n=K)]
    for j, r in enumerate(rows):
        if r["p"] is not None:
            assert int(s[j, r["p"]]) == r["num"], r["name"]
    eng.close()


# ---- 3. playouts equal the driver ----------------------------------------------------------------------------------------------
def _driver_rows(n, move_lists, seeds, t):
    E, cd = Ref(n), CE.cand(n)
    return np.array([words(*cd.playout_from(E, mv, int(sd), t)) for mv, sd in zip(move_lists, seeds)], np.uint64).astype(np.uint32)


@pytest.mark.parametrize("t", [1, 4])
def test_playout_from_the_empty_board_9(elf, t):
    seeds = playout_seeds(64)
    eng = elf.GoEngine(9, 64)
    got = u32(eng.playout(seeds, self_atari_thres=t))
    eng.close()
    assert np.array_equal(got, _driver_rows(9, [[]] * 64, seeds, t))


@pytest.mark.parametrize("t", [1, 4])
def test_playout_from_ply_30_of_the_seeded_games(elf, t):
    _, games, _ = CE.all_expected("nine")
    lists = [[int(c) for c in g[:30]] for g in games[:32]]
    assert all(len(m) == 30 for m in lists)
    seeds = playout_seeds(32, base=500)
    eng = elf.GoEngine(9, 32)
    OE.play_all(eng, lists)
    got = u32(eng.playout(seeds, self_atari_thres=t))
    eng.close()
    assert np.array_equal(got, _driver_rows(9, lists, seeds, t))


@pytest.mark.parametrize("t", [1, 4])
def test_playout_19(elf, t):
    seeds = playout_seeds(8, base=40)
    eng = elf.GoEngine(19, 8)
    got = u32(eng.playout(seeds, self_atari_thres=t))
    eng.close()
    assert np.array_equal(got, _driver_rows(19, [[]] * 8, seeds, t))


def test_playout_without_a_threshold_is_the_existing_playout(elf):
    g = np.load(os.path.join(SE.GOLDEN, "playout_9.npz"))
    seeds = g["seeds"][:64]
    eng = elf.GoEngine(9, 64)
    a = u32(eng.playout(seeds, self_atari_thres=NO))
    eng.reset()
    b = u32(eng.playout(seeds))
    eng.close()
    assert np.array_equal(a, b) and np.array_equal(a, g["out"][:64])
    for n, k in ((19, 8),):
        eng = elf.GoEngine(n, k)
        sd = playout_seeds(k, base=40)
        a = u32(eng.playout(sd, self_atari_thres=NO))
        eng.reset()
        assert np.array_equal(a, u32(eng.playout(sd)))
        eng.close()


# ---- 4. ownership ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,t,plies", [(9, 16, 1, (30, 45)), (9, 16, 4, (30, 45)), (19, 8, 3, (120,))])
def test_ownership_equals_the_sums_over_the_driver(elf, n, K, t, plies):
    _, games, _ = CE.all_expected("nine" if n == 9 else "playout19")
    lists = [[int(c) for c in games[i][:p]] for i, p in enumerate(plies)]
    assert all(len(m) == p for m, p in zip(lists, plies))
    seeds = playout_seeds(len(lists), base=900)
    E, cd = Ref(n), CE.cand(n)
    want = [cd.ownership(E, mv, int(sd), K, 7.5, t) for mv, sd in zip(lists, seeds)]
    eng = elf.GoEngine(n, len(lists))
    OE.play_all(eng, lists)
    before = npy(eng.info())
    for lanes in (0, 1):
        own = eng.ownership(seeds, ids=list(range(len(lists))), playouts=K, komi=7.5, max_lanes=lanes, self_atari_thres=t)
        assert np.array_equal(npy(own["counts"]), np.array([w[0] for w in want])), lanes
        assert np.array_equal(npy(own["stats"]), np.array([w[1] for w in want])), lanes
    assert np.array_equal(npy(eng.info()), before), "the source slots are only read"
    eng.close()


def test_ownership_of_the_seki(elf):
    n, stones, mover = CE.seki()
    eng = elf.GoEngine(n, 1)
    assert (npy(eng.setup(stones[None], next_player=[mover])) == 1).all()
    am = npy(eng.area_map())[0]
    assert np.array_equal(am, OE.area_map(stones, n))
    own = eng.ownership(np.array([11], np.uint64), ids=[0], playouts=64, self_atari_thres=5)
    counts, stats = npy(own["counts"])[0], npy(own["stats"])[0]
    assert np.array_equal(counts[0], 64 * (am == 1)) and np.array_equal(counts[1], 64 * (am == 2))
    for a in CE.xy(n, CE.SEKI_LIBS):
        assert counts[0, a] == 0 and counts[1, a] == 0
    assert int(stats[3]) == 128 and int(stats[2]) == 0
    # today's policy fills a shared liberty in every playout: the six inner black stones never stand at the end
    plain = npy(eng.ownership(np.array([11], np.uint64), ids=[0], playouts=64)["counts"])[0]
    assert all(plain[0, a] == 0 for a in CE.xy(n, CE.SEKI_INNER_BLACK))
    eng.close()


# ---- 5. GTP ---------------------------------------------------------------------------------------------------------------------
def test_gtp_on_the_seki(elf):
    import torch
    from elf_amd.gtp import GtpEngine, xy2move
    n, stones, mover = CE.seki()

    def actor(batch):
        b = batch["s"].shape[0]
        return dict(pi=torch.full((b, n * n + 1), 1.0 / (n * n + 1), device="cuda"), V=torch.zeros(b, device="cuda"))

    names = lambda pts: " ".join(xy2move(a // n, a % n) for a in sorted(pts))
    inner = CE.xy(n, CE.SEKI_INNER_BLACK + CE.SEKI_INNER_WHITE)
    everything = [a for a in range(n * n) if stones[a]]
    replies = {}
    for thres in (5, None):
        eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=16, nodes_per_game=1024, status_playouts=64, status_seed=3,
                        status_self_atari_thres=thres)
        eng.sp.setup(stones, [0], mover)
        replies[thres] = [eng.command("final_status_list " + w) for w in ("seki", "dead", "alive")]
        if thres == 5:
            assert "elf-candidates" in eng.command("list_commands").split()
            assert eng.command("elf-candidates 5") == "= \n\n"
            libs = [xy2move(x, y) for x, y in CE.SEKI_LIBS]
            assert eng.command("elf-candidates 8") == "= %s\n\n" % " ".join(v + ":7" for v in libs)
            assert eng.command("elf-candidates") == "= \n\n"                      # the default threshold is 1
            assert eng.command("elf-candidates 32767") == eng.command("elf-candidates 8")
        else:
            own = eng.boards.ownership(np.array([3], np.uint64), ids=[0], playouts=64, komi=eng.komi)
            cb, cw = npy(own["counts"])[0]
        eng.close()
    assert replies[5] == ["= %s\n\n" % names(inner), "= \n\n", "= %s\n\n" % names(set(everything) - set(inner))]
    # the default: today's replies, i.e. today's rule over the existing entry point's counts; the inner black stones are dead
    dead = {a for a in everything if (cw[a] > cb[a] if stones[a] == 1 else cb[a] > cw[a])}
    assert replies[None] == ["= \n\n", "= %s\n\n" % names(dead), "= %s\n\n" % names(set(everything) - dead)]
    assert set(CE.xy(n, CE.SEKI_INNER_BLACK)) <= dead


# ---- 6. arguments ---------------------------------------------------------------------------------------------------------------
def test_arguments(elf):
    import torch
    n, cap = 9, 6
    eng = elf.GoEngine(n, cap)
    _, games, exp = CE.all_expected("nine")
    lists = [[int(c) for c in games[i][:40 + 5 * i]] for i in range(cap)]
    OE.play_all(eng, lists)
    L, h, st = eng.L, eng._h, eng._stream()
    mask = torch.full((cap, n * n), 77, dtype=torch.uint8, device=eng.device)
    stones = torch.full((cap, n * n), 77, dtype=torch.int16, device=eng.device)
    mp, sp = C.c_void_p(mask.data_ptr()), C.c_void_p(stones.data_ptr())
    BAD = -1
    assert L.elfgo_candidates(h, None, 0, 1, mp, sp, st) == BAD
    assert L.elfgo_candidates(h, None, -3, 1, mp, sp, st) == BAD
    assert L.elfgo_candidates(h, None, cap, 1, None, None, st) == BAD
    assert L.elfgo_candidates(None, None, cap, 1, mp, sp, st) == BAD
    assert L.elfgo_candidates(h, None, cap + 1, 1, mp, sp, st) == BAD          # ids NULL names slots [0, n): n is bounded by the pool
    eng.sync()
    assert bool((mask == 77).all()) and bool((stones == 77).all()), "nothing was launched"
    want_m = np.array([exp[i]["mask"][1][len(lists[i])] for i in range(cap)])
    want_s = np.array([exp[i]["stones"][len(lists[i])] for i in range(cap)])
    # ids=None, and each output alone
    m, s = eng.candidates()
    assert np.array_equal(npy(m), want_m) and np.array_equal(npy(s), want_s)
    assert L.elfgo_candidates(h, None, cap, 1, mp, None, st) == 0 and L.elfgo_candidates(h, None, cap, 1, None, sp, st) == 0
    assert np.array_equal(npy(mask), want_m) and np.array_equal(npy(stones), want_s)
    # a slot named twice, out-of-pool ids in between
    ids = [3, cap, 3, -1, 0, 1 << 20, 5]
    m, s = [npy(t) for t in eng.candidates(ids)]
    for r, b in enumerate(ids):
        if 0 <= b < cap:
            assert np.array_equal(m[r], want_m[b]) and np.array_equal(s[r], want_s[b])
        else:
            assert (m[r] == 0).all() and (s[r] == -1).all()
    # the slots are only read
    info, (col, lib) = npy(eng.info()), [npy(t) for t in eng.export_board()]
    for i in range(cap):
        assert int(info[i, 0]) == int(exp[i]["info"][len(lists[i]), 0])
    eng.candidates(self_atari_thres=3)
    assert np.array_equal(npy(eng.info()), info) and np.array_equal(npy(eng.export_board()[0]), col) and np.array_equal(npy(eng.export_board()[1]), lib)
    eng.close()
