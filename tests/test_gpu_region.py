"""GPU: elfgo_region_moves (k_region_moves), elfgo_ld_run (k_playout_ld), GoEngine.region_moves / ld_read / LdReading and the GTP
commands over them against the reference's own FindAllCandidateMovesInRegion / FindAllValidMovesInRegion / GroupInRegion /
OneGroupLives / getBoardBBox / GuessLDAttacker and the playout drivers of region_expected (proven by tests/test_region_cpu.py).
Every comparison is integer equality; every expected number is computed by the reference at test time, once per process."""
import ctypes as C

import numpy as np
import pytest

import candidates_expected as CE
import ladder_positions as LP
import ownership_expected as OE
import region_expected as RE
from pyoracle import Ref, RefBoard

pytestmark = pytest.mark.gpu

BLACK, WHITE = 1, 2


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    assert RefBoard.available(9) and RefBoard.available(19) and Ref.available(9) and Ref.available(19), \
        "build() must have produced oracle/_ref/libelfboard{9,19}.so and libelfref{9,19}.so"
    return elf_amd


def npy(t):
    return t.cpu().numpy()


def same(got, want, tags, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
    if bad.size:
        j = int(bad[0])
        d = got[j] != want[j]
        raise AssertionError("%s differs in %d of %d rows, first %s at %s: got %s want %s" % (
            what, bad.size, len(want), tags[j], np.argwhere(d)[:6].tolist(), got[j][d][:6].tolist(), want[j][d][:6].tolist()))


def snapshot(eng, k):
    return [npy(t) for t in eng.export_board(n=k)] + [npy(eng.info(n=k))]


# ---- 1. region lists --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 19])
def test_region_moves_equal_the_reference(elf, n):
    """every row of region_expected.list_sets under every box of the row and every threshold; the boxed calls name each slot once
    per box (repeated ids), the whole board is asked as a null pointer and as (0, 0, N, N)"""
    total = 0
    for st in RE.list_expected(n):
        games, rows = st["games"], st["rows"]
        eng = elf.GoEngine(n, len(games))
        at = {}
        for j, r in enumerate(rows):
            at.setdefault(r["ply"], []).append(j)
        got = {}      # (row, box index, thres) -> (cand, valid, groups)
        for t in range(max(len(m) for m in games) + 1):
            sel = at.get(t, [])
            if sel:
                ids_null = [rows[j]["game"] for j in sel]
                pairs = [(j, q) for j in sel for q in range(1, len(rows[j]["boxes"]))]
                ids = [rows[j]["game"] for j, _ in pairs]
                boxes = [rows[j]["boxes"][q] for j, q in pairs]
                for th in RE.list_thresholds(n):
                    c0, v0, g0 = [npy(x) for x in eng.region_moves(ids_null, self_atari_thres=th)]
                    for i, j in enumerate(sel):
                        got[(j, 0, th)] = (c0[i], v0[i], g0[i])
                    c1, v1, g1 = [npy(x) for x in eng.region_moves(ids, regions=boxes, self_atari_thres=th)]
                    for i, (j, q) in enumerate(pairs):
                        got[(j, q, th)] = (c1[i], v1[i], g1[i])
            fwd = [i for i, m in enumerate(games) if t < len(m)]
            if fwd:
                assert bool((eng.forward(fwd, [int(games[i][t]) for i in fwd]) == 1).all())
        eng.close()
        keys = [(j, q, th) for j, r in enumerate(rows) for q in range(len(r["boxes"])) for th in RE.list_thresholds(n)]
        assert sorted(got) == sorted(keys)
        tags = [(st["name"], rows[j]["game"], rows[j]["ply"], rows[j]["boxes"][q], th) for j, q, th in keys]
        same([got[k][0] for k in keys], [rows[j]["cand"][th][q] for j, q, th in keys], tags, "cand")
        same([got[k][1] for k in keys], [rows[j]["valid"][q] for j, q, th in keys], tags, "valid")
        same([got[k][2] for k in keys], [rows[j]["groups"][q] for j, q, th in keys], tags, "groups")
        total += len(keys)
    print("region_moves %d: %d (row, box, threshold) answers" % (n, total))
    assert total > 40000


CAP = 7


@pytest.fixture(scope="module")
def pool(elf):
    """seven 9x9 positions (one with the ko pending) on a pool of seven slots, and the row dicts they came from"""
    sets = RE.list_expected(9)
    nine, ko = sets[0], sets[-1]
    pick = [(nine, r) for r in nine["rows"][5:600:100]] + [(ko, ko["rows"][3])]
    assert len(pick) == CAP
    eng = elf.GoEngine(9, CAP)
    OE.play_all(eng, [st["games"][r["game"]][:r["ply"]] for st, r in pick])
    yield eng, [r for _, r in pick]
    eng.close()


def test_rows_ids_and_each_output_alone_in_guarded_buffers(pool):
    import torch
    eng, pick = pool
    n, NP = 9, 81
    before = snapshot(eng, CAP)
    L, h, st = eng.L, eng._h, eng._stream()
    names = ("cand", "valid", "groups")
    # n = 1, an odd n, repeated ids, out-of-pool ids; box q of every row
    for ids in ([3], [6, 0, 2], [1, 1, 5, 1, 6, 6, 0], [0, -1, 4, CAP, 6, 1 << 20, -(1 << 31)]):
        for q in (0, 3, 5, 8):
            live = [r for r, b in enumerate(ids) if 0 <= b < CAP]
            boxes = None if q == 0 else [pick[b]["boxes"][q] if 0 <= b < CAP else (0, 0, n, n) for b in ids]
            got = [npy(x) for x in eng.region_moves(ids, regions=boxes, self_atari_thres=3)]
            want = [np.array([pick[ids[r]][k][3][q] if k == "cand" else pick[ids[r]][k][q] for r in live]) for k in names]
            for g, w, k in zip(got, want, names):
                same(g[live], w, [ids[r] for r in live], "%s ids %s box %d" % (k, ids, q))
                assert not g[[r for r in range(len(ids)) if r not in live]].any()
    # each output NULL in turn, guarded
    GUARD, POISON = 64, 0xA5
    size = CAP * NP
    off = {k: GUARD + i * ((size + 15) // 16 * 16 + GUARD) for i, k in enumerate(names)}
    total = off["groups"] + (size + 15) // 16 * 16 + GUARD
    boxes = torch.tensor([pick[b]["boxes"][5] for b in range(CAP)], dtype=torch.int32, device=eng.device)
    want = dict(cand=np.array([r["cand"][1][5] for r in pick]), valid=np.array([r["valid"][5] for r in pick]),
                groups=np.array([r["groups"][5] for r in pick]))
    for live in (names,) + tuple(tuple(k for k in names if k != dead) for dead in names) + tuple((k,) for k in names):
        buf = torch.full((total,), POISON, dtype=torch.uint8, device=eng.device)
        ptr = {k: C.c_void_p(buf.data_ptr() + off[k]) if k in live else None for k in names}
        assert L.elfgo_region_moves(h, None, CAP, C.c_void_p(boxes.data_ptr()), 1, ptr["cand"], ptr["valid"], ptr["groups"], st) == 0
        eng.sync()
        raw = npy(buf)
        written = np.zeros(total, bool)
        for k in live:
            written[off[k]:off[k] + size] = True
            assert np.array_equal(raw[off[k]:off[k] + size].reshape(CAP, NP), want[k]), (live, k)
        assert (raw[~written] == POISON).all(), "a byte outside the live outputs was written (%s)" % (live,)
    # refusals: nothing is launched
    BAD = -1
    buf = torch.full((total,), POISON, dtype=torch.uint8, device=eng.device)
    p = C.c_void_p(buf.data_ptr() + off["cand"])
    assert L.elfgo_region_moves(h, None, CAP, None, 1, None, None, None, st) == BAD
    assert L.elfgo_region_moves(h, None, 0, None, 1, p, None, None, st) == BAD
    assert L.elfgo_region_moves(h, None, -2, None, 1, p, None, None, st) == BAD
    assert L.elfgo_region_moves(h, None, CAP + 1, None, 1, p, None, None, st) == BAD
    assert L.elfgo_region_moves(None, None, CAP, None, 1, p, None, None, st) == BAD
    eng.sync()
    assert bool((buf == POISON).all())
    # regions outside the board are clamped by the kernel
    wild = torch.tensor([[-5, -(1 << 30), 1 << 30, 40]] * CAP, dtype=torch.int32, device=eng.device)
    out = torch.empty((CAP, NP), dtype=torch.uint8, device=eng.device)
    assert L.elfgo_region_moves(h, None, CAP, C.c_void_p(wild.data_ptr()), 1, C.c_void_p(out.data_ptr()), None, None, st) == 0
    assert np.array_equal(npy(out), np.array([r["cand"][1][1] for r in pick]))
    # a device tensor of boxes is used as it is
    dev = [npy(x) for x in eng.region_moves(regions=wild, self_atari_thres=1)] + [npy(x) for x in eng.region_moves(regions=boxes, self_atari_thres=1)]
    assert np.array_equal(dev[0], npy(out)) and all(np.array_equal(dev[3 + i], want[k]) for i, k in enumerate(names))
    with pytest.raises(ValueError):
        eng.region_moves(regions=boxes[:3], self_atari_thres=1)
    # ValueError boxes before any launch
    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("%s was called" % name)
    real, eng.L = eng.L, NoLaunch()
    try:
        for box in ((-1, 0, 3, 3), (0, 0, 10, 3), (4, 0, 3, 3), (0, 5, 3, 4), (0, 0, 3, 10), (0, -1, 3, 3)):
            with pytest.raises(ValueError):
                eng.region_moves([0, 1], regions=[(0, 0, 9, 9), box])
            with pytest.raises(ValueError):
                eng.ld_read(np.array([1, 2], np.uint64), [0, 1], regions=[(0, 0, 9, 9), box])
        with pytest.raises(ValueError):
            eng.region_moves([0, 1], regions=[(0, 0, 9, 9)])
        with pytest.raises(ValueError):
            eng.ld_read(np.array([1, 2], np.uint64), [0, 1], attackers=[1])
    finally:
        eng.L = real
    for a, b in zip(before, snapshot(eng, CAP)):
        assert np.array_equal(a, b)


# ---- 2. / 3. / 6. the reader against the driver ----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[9, 19])
def ld(elf, request):
    n = request.param
    rows = RE.ld_rows(n)
    eng = elf.GoEngine(n, len(rows))
    OE.play_all(eng, [r["moves"] for r in rows])
    yield n, eng, rows
    eng.close()


def ld_call(eng, n, rows, setting, sel=None, **kw):
    K, th, forced = RE.LD_SETTINGS[setting]
    th = RE.no_thres(n) if th is None else th
    sel = list(range(len(rows))) if sel is None else sel
    return eng.ld_read(np.array([rows[j]["seed"] for j in sel], np.uint64), sel, regions=[rows[j]["box"] for j in sel], playouts=K,
                       self_atari_thres=th, attackers=[rows[j]["forced"] for j in sel] if forced else None,
                       max_steps=RE.LD_MAX_STEPS[n], **kw)


@pytest.mark.parametrize("setting", range(len(RE.LD_SETTINGS)))
def test_ld_run_equals_the_driver(ld, setting):
    n, eng, rows = ld
    before = snapshot(eng, len(rows))
    info, stats, first, _ = RE.ld_expected(n, setting)
    rd = ld_call(eng, n, rows, setting)
    tags = list(range(len(rows)))
    same(npy(rd.info), info, tags, "info")
    same(npy(rd.stats), stats, tags, "stats")
    same(npy(rd.first), first, tags, "first")
    K = RE.LD_SETTINGS[setting][0]
    # the rates are one float64 division on the device: within an ulp of numpy's, and they round back to the counts
    for rate, col in ((rd.live_rate, 0), (rd.survive_rate, 1)):
        assert rate.is_cuda and np.allclose(npy(rate), stats[:, col] / K, rtol=4e-16, atol=0) and np.array_equal(np.rint(npy(rate) * K), stats[:, col])
    for a, b in zip(before, snapshot(eng, len(rows))):     # 6. export, info and hash of the source slots
        assert np.array_equal(a, b)
    print("ld_run %d setting %s: lived %d survived %d superko %d steps %d of %d playouts" % (
        n, RE.LD_SETTINGS[setting], stats[:, 0].sum(), stats[:, 1].sum(), stats[:, 4].sum(), stats[:, 5].sum(), K * len(rows)))


def test_ld_run_does_not_depend_on_the_lanes(ld):
    """n * playouts = 23 * 5 and 47 * 5: no multiple of 4; four lanes = one workgroup walks every group, rows change inside groups"""
    n, eng, rows = ld
    sel = list(range(len(rows) - 1))
    assert (len(sel) * 5) % 4
    info, stats, first, _ = RE.ld_expected(n, 1)
    a = ld_call(eng, n, rows, 1, sel, max_lanes=4)
    got_a = [npy(a.info), npy(a.stats), npy(a.first)]
    b = ld_call(eng, n, rows, 1, sel)
    for x, y, w in zip(got_a, [npy(b.info), npy(b.stats), npy(b.first)], (info, stats, first)):
        assert np.array_equal(x, y)
        same(x, w[sel], sel, "four lanes")


# ---- 4. the whole-board box plays the candidate playouts -----------------------------------------------------------------------------
@pytest.mark.parametrize("thres", [1, 3, None])
def test_whole_board_box_is_the_candidate_playout(ld, elf, thres):
    n, eng, rows = ld
    th = RE.no_thres(n) if thres is None else thres
    k = min(len(rows), 12)
    seeds = np.array([r["seed"] for r in rows[:k]], np.uint64)
    full = [(0, 0, n, n)] * k
    rd = eng.ld_read(seeds, list(range(k)), regions=full, playouts=6, self_atari_thres=th)
    own = eng.ownership(seeds, list(range(k)), playouts=6, self_atari_thres=th)
    st, ost = npy(rd.stats), npy(own["stats"])
    assert np.array_equal(st[:, 4], ost[:, 2]) and np.array_equal(st[:, 5], ost[:, 3])
    assert st[:, 5].sum() > 0
    # one playout: the hash sum is the hash the candidate playout leaves on a copy of the slot
    rd1 = eng.ld_read(seeds, list(range(k)), regions=full, playouts=1, self_atari_thres=th)
    two = elf.GoEngine(n, k)
    OE.play_all(two, [r["moves"] for r in rows[:k]])
    out = npy(two.playout(seeds, self_atari_thres=th)).astype(np.uint32).astype(np.uint64)
    two.close()
    want = (out[:, 0] | (out[:, 1] << np.uint64(32))).view(np.int64)
    s1 = npy(rd1.stats)
    assert np.array_equal(s1[:, 6], want) and np.array_equal(s1[:, 5], out[:, 3].astype(np.int64))


# ---- 5. edge cases of the playout loop -----------------------------------------------------------------------------------------------
def test_step_limits_and_a_terminated_source(ld):
    n, eng, rows = ld
    rg, E = RE.reg(n), RE.ref(n)
    k = min(len(rows), 16)
    sel = list(range(k))
    seeds = np.array([rows[j]["seed"] for j in sel], np.uint64)
    boxes = [rows[j]["box"] for j in sel]
    # max_steps = 0: every playout is the source position
    rd = eng.ld_read(seeds, sel, regions=boxes, playouts=7, max_steps=0)
    info, stats, first = npy(rd.info), npy(rd.stats), npy(rd.first)
    assert np.array_equal(stats[:, 0], 7 * info[:, 7].astype(np.int64)) and not first.any() and not stats[:, 5].any()
    want = [rg.ld_row(E, rows[j]["moves"], rows[j]["seed"], 7, 3, rows[j]["box"], 0, 0) for j in sel]
    same(info, [w[0] for w in want], sel, "info, no step")
    same(stats, [w[1] for w in want], sel, "stats, no step")
    # max_steps = 3
    rd = eng.ld_read(seeds, sel, regions=boxes, playouts=7, max_steps=3)
    want = [rg.ld_row(E, rows[j]["moves"], rows[j]["seed"], 7, 3, rows[j]["box"], 0, 3) for j in sel]
    same(npy(rd.info), [w[0] for w in want], sel, "info, three steps")
    same(npy(rd.stats), [w[1] for w in want], sel, "stats, three steps")
    same(npy(rd.first), [w[2] for w in want], sel, "first, three steps")
    assert int(npy(rd.stats)[:, 5].sum()) > 0


def test_a_finished_game_is_read_where_it_stands(elf):
    n = 9
    rg, E = RE.reg(n), RE.ref(n)
    if not CE._sets:
        CE._sets.update(CE.game_sets())
    games = [[int(c) for c in g] for g in CE._sets["nine"][1][:3]]
    eng = elf.GoEngine(n, len(games))
    OE.play_all(eng, games)
    assert npy(eng.info())[:, 9].all()                      # terminated
    seeds = np.array([5, 6, 7], np.uint64)
    for box in (None, (0, 0, 5, 9)):
        rd = eng.ld_read(seeds, regions=None if box is None else [box] * 3, playouts=5)
        want = [rg.ld_row(E, g, int(s), 5, 3, box, 0) for g, s in zip(games, seeds)]
        same(npy(rd.info), [w[0] for w in want], [0, 1, 2], "info")
        same(npy(rd.stats), [w[1] for w in want], [0, 1, 2], "stats")
        assert not npy(rd.first).any() and not npy(rd.stats)[:, 5].any()
        assert rd.best_move() == [None] * 3
    eng.close()


# ---- 7. the straight three ------------------------------------------------------------------------------------------------------------
def test_straight_three(elf):
    """region_expected.s3_rows: the move list and the 16 images through setup, defender and attacker to move"""
    n, K = 9, RE.S3_PLAYOUTS
    rows = RE.s3_rows(n)
    eng = elf.GoEngine(n, len(rows))
    OE.play_all(eng, [r["src"] for r in rows[:2]])
    ids = list(range(2, len(rows)))
    ok = eng.setup(np.array([r["src"]["stones"] for r in rows[2:]]), ids=ids, next_player=[r["src"]["mover"] for r in rows[2:]])
    assert (npy(ok) == 1).all()
    rg, E = RE.reg(n), RE.ref(n)
    for base in RE.S3_ROW_SEEDS:
        rd = eng.ld_read(np.array([base + j for j in range(len(rows))], np.uint64), regions=[r["box"] for r in rows], playouts=K,
                         self_atari_thres=RE.S3_THRES)
        info, stats, first = npy(rd.info), npy(rd.stats), npy(rd.first)
        best = rd.best_move()
        for j, r in enumerate(rows):
            v = r["vital"]
            assert RE.s3_holds(r, info[j], stats[j], first[j], K), (base, j, info[j], stats[j], first[j][:, [v] + r["others"]])
            if r["defends"]:      # spelled out: lived equals playouts at the vital point and is 0 at the two others
                assert first[j, 1, v] == first[j, 0, v] > 0 and not first[j, 1, r["others"]].any()
            else:                 # survived is 0 at the vital point
                assert first[j, 0, v] > 0 and first[j, 2, v] == 0
            assert best[j] == v, (base, j, best[j], v)
        # the driver's numbers on every row: the move lists (GoState driver) and the set-up images (bare driver)
        sel = list(range(len(rows)))
        want = [rg.ld_row(E, rows[j]["src"], base + j, K, RE.S3_THRES, rows[j]["box"], 0) for j in sel]
        same(info[sel], [w[0] for w in want], sel, "info")
        same(stats[sel], [w[1] for w in want], sel, "stats")
        same(first[sel], [w[2] for w in want], sel, "first")
    eng.close()


# ---- 8. argument errors and GTP ----------------------------------------------------------------------------------------------------------
def test_ld_run_argument_errors(pool):
    import torch
    eng, _ = pool
    L, st = eng.L, eng._stream()
    own = eng._own_handle(0)[1]
    NA = 82
    seeds = torch.ones(CAP, dtype=torch.int64, device=eng.device)
    POISON = 0x5A
    info = torch.full((CAP * 8 * 4,), POISON, dtype=torch.uint8, device=eng.device)
    stats = torch.full((CAP * 8 * 8,), POISON, dtype=torch.uint8, device=eng.device)
    first = torch.full((CAP * 3 * NA * 4,), POISON, dtype=torch.uint8, device=eng.device)
    sp, ip, tp, fp = [C.c_void_p(t.data_ptr()) for t in (seeds, info, stats, first)]
    BAD = -1
    assert L.elfgo_ld_run(None, None, sp, CAP, 4, 10, 3, None, None, ip, tp, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, None, CAP, 4, 10, 3, None, None, ip, tp, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, CAP, 4, 10, 3, None, None, None, tp, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, CAP, 4, 10, 3, None, None, ip, None, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, CAP, 4, 10, 3, None, None, ip, tp, None, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, 0, 4, 10, 3, None, None, ip, tp, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, CAP, 0, 10, 3, None, None, ip, tp, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, CAP + 1, 4, 10, 3, None, None, ip, tp, fp, st) == BAD
    assert L.elfgo_ld_run(own, None, sp, CAP, 1 << 30, 10, 3, None, None, ip, tp, fp, st) == BAD
    eng.sync()
    assert bool((info == POISON).all()) and bool((stats == POISON).all()) and bool((first == POISON).all())
    # an id outside the pool is not played: its rows stay zero, the others are what they are alone
    rd = eng.ld_read(np.array([9, 9, 9], np.uint64), [2, CAP, -1], playouts=3)
    alone = eng.ld_read(np.array([9], np.uint64), [2], playouts=3)
    for a, b in ((rd.info, alone.info), (rd.stats, alone.stats), (rd.first, alone.first)):
        assert np.array_equal(npy(a)[0], npy(b)[0]) and not npy(a)[1:].any()
    assert int(npy(alone.stats)[0, 5]) > 0


def test_ld_read_on_a_track_placed_engine(elf):
    """ld_read only reads the slots, so it works where playout() raises, and the placement table stays true"""
    n = 9
    moves, _ = RE.s3_move_list(n)
    plain, tracked = elf.GoEngine(n, 1), elf.GoEngine(n, 1, track_placed=True)
    for e in (plain, tracked):
        OE.play_all(e, [moves])
    placed = npy(tracked.placed())
    with pytest.raises(ValueError):
        tracked.playout(np.array([1], np.uint64))
    a = plain.ld_read(np.array([4], np.uint64), regions=[RE.S3_BOX], playouts=16)
    b = tracked.ld_read(np.array([4], np.uint64), regions=[RE.S3_BOX], playouts=16)
    assert np.array_equal(npy(a.stats), npy(b.stats)) and np.array_equal(npy(a.first), npy(b.first)) and int(npy(a.stats)[0, 5]) > 0
    assert np.array_equal(npy(tracked.placed()), placed)
    plain.close()
    tracked.close()


def test_gtp(elf):
    import torch
    from elf_amd.gtp import GtpEngine, xy2move
    n, K, SEED = 9, 48, 11
    rg, E = RE.reg(n), RE.ref(n)

    def actor(batch):
        b = batch["s"].shape[0]
        return dict(pi=torch.full((b, n * n + 1), 1.0 / (n * n + 1), device="cuda"), V=torch.zeros(b, device="cuda"))

    eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=16, nodes_per_game=1024, status_playouts=K, ld_seed=SEED)
    for name in ("elf-region_candidates", "elf-ld_read"):
        assert name in eng.command("list_commands").split()
        assert eng.command("known_command " + name) == "= true\n\n"
    v = lambda a: "pass" if a == n * n else xy2move(a // n, a % n)

    def reply(src, box, playouts):
        info, stats, first = rg.ld_row(E, src, SEED, playouts, 3, box, 0)
        rd_first = first.astype(np.int64)
        best, sign = None, (1 if info[6] == info[5] else -1)
        for a in np.nonzero(rd_first[0])[0]:
            p, l = int(rd_first[0, a]), int(rd_first[1, a])
            if best is None or sign * (l * best[1] - best[2] * p) > 0 or (l * best[1] == best[2] * p and p > best[1]):
                best = (int(a), p, l)
        lines = ["attacker %s defender %s to_move %s lives %d/%d survives %d/%d best %s" % (
            " bw"[info[4]], " bw"[info[5]], " bw"[info[6]], stats[0], playouts, stats[1], playouts, "none" if best is None else v(best[0]))]
        lines += ["%s %d %d %d" % (v(a), first[0, a], first[1, a], first[2, a]) for a in range(n * n + 1) if first[0, a]]
        return "= %s\n\n" % "\n".join(lines), best

    stones = RE.straight_three(n)
    for mover in (BLACK, WHITE):
        if mover == WHITE:
            eng.sp.restart([0])
        eng.sp.setup(stones, [0], mover)
        src = dict(stones=stones, mover=mover)
        want, best = reply(src, RE.S3_BOX, K)
        assert eng.command("elf-ld_read A1 E3") == want == eng.command("elf-ld_read e3 a1 %d" % K)
        assert best[0] == RE.S3_VITAL[0] * n + RE.S3_VITAL[1] and " best B1\n" in want
        want16, _ = reply(src, None, 16)                                   # no vertices: the bounding box of the stones
        assert eng.command("elf-ld_read 16") == want16
        assert eng.command("elf-ld_read") == reply(src, None, K)[0]
        h = LP.build(rg.RB, stones, mover)
        for th in (1, 3):
            mask = rg.masks(h, RE.S3_BOX, th)[0]
            sa = rg.cd.stones(h, mover)
            want_c = " ".join(v(a) + (":%d" % sa[a] if sa[a] > 0 else "") for a in range(n * n) if mask[a])
            assert eng.command("elf-region_candidates A1 E3 %d" % th) == "= %s\n\n" % want_c
        assert eng.command("elf-region_candidates A1 E3") == eng.command("elf-region_candidates E3 A1 1")
        rg.RB.free(h)
    assert eng.command("elf-region_candidates A1").startswith("?") and eng.command("elf-region_candidates A1 Z3").startswith("?")
    assert eng.command("elf-ld_read A1 K9").startswith("?") and eng.command("elf-ld_read 0").startswith("?")
    assert eng.command("elf-ld_read A1 E3 12 13").startswith("?")
    eng.close()
