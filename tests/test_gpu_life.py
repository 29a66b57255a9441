"""GPU: elfgo_life_map (k_life_map), GoEngine.life_map / fast_score and the GTP commands over them against the reference's own
isEye / isFakeEye / isSemiEye / isTrueEye / getEyeColor / getFastScore / OneGroupLives / getBoardBBox / GuessLDAttacker
(life_expected, proven by tests/test_life_cpu.py).  Every comparison is integer equality; every expected number is computed by the
reference at test time, once per process."""
import ctypes as C

import numpy as np
import pytest

import candidates_expected as CE
import ladder_positions as LP
import life_expected as LE
import ownership_expected as OE
from pyoracle import Ref, RefBoard

pytestmark = pytest.mark.gpu

OUTPUTS = ("eye", "semi_move", "alive", "summary")


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    assert RefBoard.available(9) and RefBoard.available(19) and Ref.available(9) and Ref.available(19), \
        "build() must have produced oracle/_ref/libelfboard{9,19}.so and libelfref{9,19}.so"
    return elf_amd


def npy(t):
    return t.cpu().numpy()


def got_of(lm):
    return {k: npy(getattr(lm, k)) for k in OUTPUTS}


def compare(got, want, tags, what):
    """got: dict of arrays [K, ...]; want: list of Life.expected dicts"""
    for k in OUTPUTS:
        w = np.array([e[k] for e in want])
        assert got[k].shape == w.shape and got[k].dtype == w.dtype, (what, k, got[k].shape, got[k].dtype)
        bad = np.nonzero((got[k] != w).reshape(len(want), -1).any(axis=1))[0]
        if bad.size:
            j = int(bad[0])
            where = np.argwhere(got[k][j] != w[j])[:6].tolist()
            raise AssertionError("%s: %s differs in %d rows, first %s at %s: got %s want %s" % (
                what, k, bad.size, tags[j], where, got[k][j][got[k][j] != w[j]][:6].tolist(), w[j][got[k][j] != w[j]][:6].tolist()))


# ---- (a) whole games -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nine", "ladder16", "playout19"])
def test_games_equal_the_reference(elf, name):
    n, games, rows = LE.all_expected(name)
    eng = elf.GoEngine(n, len(games))
    at = {}
    for j, r in enumerate(rows):
        at.setdefault(r["ply"], []).append(j)
    plain, boxed, order = {k: [] for k in OUTPUTS}, {k: [] for k in OUTPUTS}, []
    for t in range(max(len(m) for m in games) + 1):
        sel = at.get(t, [])
        if sel:
            ids = [rows[j]["game"] for j in sel]
            for dst, lm in ((plain, eng.life_map(ids)), (boxed, eng.life_map(ids, regions=[rows[j]["box"] for j in sel]))):
                for k, v in got_of(lm).items():
                    dst[k].append(v)
            order += sel
        fwd = [i for i, m in enumerate(games) if t < len(m)]
        if fwd:
            assert bool((eng.forward(fwd, [int(games[i][t]) for i in fwd]) == 1).all())
    eng.close()
    assert sorted(order) == list(range(len(rows)))
    tags = [(rows[j]["game"], rows[j]["ply"]) for j in order]
    compare({k: np.concatenate(v) for k, v in plain.items()}, [rows[j]["plain"] for j in order], tags, name + ", no box")
    compare({k: np.concatenate(v) for k, v in boxed.items()}, [rows[j]["boxed"] for j in order], tags, name + ", seeded boxes")
    print(name, LE.statistics(rows))


# ---- (b) constructed positions ---------------------------------------------------------------------------------------------------
def setup_rows(eng, rows, n):
    eng.reset()
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


def nibble(eye, colour):
    return (eye >> (4 * (colour - 1))) & 15


@pytest.mark.parametrize("n", [9, 19])
def test_constructed_positions(elf, n):
    _, rows = LE.expected(n)
    K = len(rows)
    eng = elf.GoEngine(n, K)
    setup_rows(eng, rows, n)
    lm = eng.life_map(n=K)
    got = got_of(lm)
    compare(got, [r["plain"] for r in rows], [(r["name"], r["s"], r["swapped"]) for r in rows], "constructed %d" % n)
    assert np.array_equal(npy(lm.eye_colour), np.array([r["plain"]["eye_colour"] for r in rows]))
    # the hand-derived facts themselves (what the CPU test holds the reference to)
    for j, r in enumerate(rows):
        c = r["colour"]
        for a, v in r["bits"].items():
            assert int(nibble(got["eye"][j, a], c)) == v, r["name"]
        for a, m in r["semi"].items():
            assert int(got["semi_move"][j, c - 1, a]) == m, r["name"]
        for a, v in r["alive"].items():
            assert int(got["alive"][j, a]) == v, r["name"]
        if r["name"] == "empty_board":
            assert tuple(got["summary"][j]) == (0, 0, 0, 0, n, n, 0, 0, 2, 0, 0, 0)
    eng.close()


def sym_box(n, s, box):
    """the image of a non-empty box under board symmetry s"""
    (x0, y0), (x1, y1) = LP.sym_xy(n, s, box[0], box[1]), LP.sym_xy(n, s, box[2] - 1, box[3] - 1)
    return (min(x0, x1), min(y0, y1), max(x0, x1) + 1, max(y0, y1) + 1)


@pytest.mark.parametrize("n", [9, 19])
def test_attacker_boxes_in_every_image(elf, n):
    lf = LE.life(n)
    st = LE.attacker_position(n)
    stones, boxes, want, tags = [], [], [], []
    for s, sw, ist, imv in LP.images(n, st, LE.BLACK):
        h = LP.build(lf.RB, ist, imv)
        assert h is not None
        exp = lf.expected(h)
        for box, nb, nw in LE.attacker_boxes(n):
            bx = sym_box(n, s, box)
            stones.append(ist)
            boxes.append(bx)
            want.append(lf.with_box(h, exp, bx))
            tags.append((s, sw, bx))
            if sw:
                nb, nw = nw, nb
            assert want[-1]["summary"][8] == (1 if nb > nw else 2), tags[-1]
        lf.RB.free(h)
    K = len(stones)
    eng = elf.GoEngine(n, K)
    assert (npy(eng.setup(np.array(stones))) == 1).all()
    compare(got_of(eng.life_map(regions=boxes)), want, tags, "attacker %d" % n)
    eng.close()


# ---- (c) launch geometry, (d) slots untouched ---------------------------------------------------------------------------------------
CAP = 70


@pytest.fixture(scope="module")
def pool(elf):
    """70 9x9 slots holding sampled positions of the first sixteen seeded games (captures and kos included)"""
    n, games, rows = LE.all_expected("nine")
    pick = [r for r in rows if r["game"] < 16 and r["ply"] >= 20][::19][:CAP]
    assert len(pick) == CAP
    eng = elf.GoEngine(n, CAP)
    OE.play_all(eng, [[int(c) for c in games[r["game"]][:r["ply"]]] for r in pick])
    yield eng, pick
    eng.close()


@pytest.mark.parametrize("k", [1, 63, 64, 65, CAP])
def test_row_counts(pool, k):
    eng, pick = pool
    compare(got_of(eng.life_map(n=k)), [r["plain"] for r in pick[:k]], list(range(k)), "n = %d" % k)


def test_shuffled_repeated_and_out_of_pool_ids(pool):
    eng, pick = pool
    rng = np.random.default_rng(5)
    ids = [int(v) for v in rng.permutation(CAP)] + [3, 3, CAP - 1, 0]
    for pos, bad in ((5, CAP), (17, -1), (40, 1 << 20), (len(ids), -(1 << 30))):
        ids.insert(pos, bad)
    boxes = [LE.seeded_box(9, j, rng) for j in range(len(ids))]
    lf = LE.life(9)
    for regions in (None, boxes):
        got = got_of(eng.life_map(ids, regions=regions))
        keep = [r for r, b in enumerate(ids) if 0 <= b < CAP]
        want = []
        for r in keep:
            e = pick[ids[r]]["plain"]
            if regions is not None:
                h = LP.play_list(lf.RB, eng_moves(pick[ids[r]]))
                e = lf.with_box(h, e, boxes[r])
                lf.RB.free(h)
            want.append(e)
        compare({k: v[keep] for k, v in got.items()}, want, [ids[r] for r in keep], "ids, regions %s" % (regions is not None))
        for r, b in enumerate(ids):
            if not 0 <= b < CAP:
                assert not got["eye"][r].any() and not got["alive"][r].any() and (got["semi_move"][r] == -1).all() and (got["summary"][r] == -1).all()


def eng_moves(row):
    _, games, _ = LE.all_expected("nine")
    return [int(c) for c in games[row["game"]][:row["ply"]]]


def test_each_output_alone_in_guarded_buffers_and_slots_untouched(pool):
    import torch
    eng, pick = pool
    n, NP = 9, 81
    before = [npy(t) for t in eng.export_board()] + [npy(eng.info())]
    L, h, st = eng.L, eng._h, eng._stream()
    sizes = dict(eye=CAP * NP, semi_move=CAP * 2 * NP * 2, alive=CAP * NP, summary=CAP * 12 * 4)
    dtypes = dict(eye=np.uint8, semi_move=np.int16, alive=np.uint8, summary=np.int32)
    shapes = dict(eye=(CAP, NP), semi_move=(CAP, 2, NP), alive=(CAP, NP), summary=(CAP, 12))
    GUARD, POISON = 64, 0xA5
    off, total = {}, GUARD
    for k in OUTPUTS:
        off[k] = total
        total += (sizes[k] + 15) // 16 * 16 + GUARD
    ids = torch.arange(CAP, dtype=torch.int32, device=eng.device)
    want = {k: np.array([r["plain"][k] for r in pick]) for k in OUTPUTS}
    for live in (OUTPUTS,) + tuple((k,) for k in OUTPUTS):
        buf = torch.full((total,), POISON, dtype=torch.uint8, device=eng.device)
        ptr = {k: C.c_void_p(buf.data_ptr() + off[k]) if k in live else None for k in OUTPUTS}
        assert L.elfgo_life_map(h, C.c_void_p(ids.data_ptr()), CAP, None, ptr["eye"], ptr["semi_move"], ptr["alive"], ptr["summary"], st) == 0
        eng.sync()
        raw = npy(buf)
        written = np.zeros(total, bool)
        for k in live:
            written[off[k]:off[k] + sizes[k]] = True
            got = raw[off[k]:off[k] + sizes[k]].view(dtypes[k]).reshape(shapes[k])
            assert np.array_equal(got, want[k]), (live, k)
        assert (raw[~written] == POISON).all(), "a byte outside the live outputs was written (%s)" % (live,)
    # all four null, and the other refusals: nothing is launched
    BAD = -1
    buf = torch.full((total,), POISON, dtype=torch.uint8, device=eng.device)
    p = C.c_void_p(buf.data_ptr() + off["eye"])
    assert L.elfgo_life_map(h, None, CAP, None, None, None, None, None, st) == BAD
    assert L.elfgo_life_map(h, None, 0, None, p, None, None, None, st) == BAD
    assert L.elfgo_life_map(h, None, -2, None, p, None, None, None, st) == BAD
    assert L.elfgo_life_map(h, None, CAP + 1, None, p, None, None, None, st) == BAD
    assert L.elfgo_life_map(None, None, CAP, None, p, None, None, None, st) == BAD
    eng.sync()
    assert bool((buf == POISON).all())
    # regions that lie outside the board are clamped by the kernel: what the clamped box gives
    wild = torch.tensor([[-5, -(1 << 30), 1 << 30, 40]] * CAP, dtype=torch.int32, device=eng.device)
    summ = torch.empty((CAP, 12), dtype=torch.int32, device=eng.device)
    assert L.elfgo_life_map(h, None, CAP, C.c_void_p(wild.data_ptr()), None, None, None, C.c_void_p(summ.data_ptr()), st) == 0
    full = npy(eng.life_map(regions=[(0, 0, n, n)] * CAP).summary)
    assert np.array_equal(npy(summ), full) and (full[:, 4:8] == (0, 0, n, n)).all()
    # (d) the slots are only read
    after = [npy(t) for t in eng.export_board()] + [npy(eng.info())]
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    info = eng.info_host()
    for i, r in enumerate(pick):
        assert int(info["ply"][i]) == int(r["plain"]["info"][0]) and int(info["b_cap"][i]) == int(r["plain"]["info"][7])


# ---- (e) Python and GTP ------------------------------------------------------------------------------------------------------------
def test_fast_score_eye_colour_and_bad_boxes(pool):
    eng, pick = pool
    want = np.array([r["plain"]["summary"] for r in pick])
    assert np.array_equal(npy(eng.fast_score()), want[:, 0]) and np.array_equal(npy(eng.fast_score(rule="chinese")), want[:, 0])
    assert np.array_equal(npy(eng.fast_score(rule="japanese")), want[:, 1])
    assert (want[:, 0] != want[:, 1]).any()
    assert np.array_equal(npy(eng.fast_score([4, 2], rule="japanese")), want[[4, 2], 1])
    with pytest.raises(ValueError):
        eng.fast_score(rule="aga")
    lm = eng.life_map()
    assert np.array_equal(npy(lm.eye_colour), np.array([r["plain"]["eye_colour"] for r in pick])) and lm.eye_colour.is_cuda
    assert int((npy(lm.eye_colour) == 1).sum()) > 0 and int((npy(lm.eye_colour) == 2).sum()) > 0

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("%s was called" % name)
    real, eng.L = eng.L, NoLaunch()
    try:
        for box in ((-1, 0, 3, 3), (0, 0, 10, 3), (4, 0, 3, 3), (0, 5, 3, 4), (0, 0, 3, 10), (0, -1, 3, 3)):
            with pytest.raises(ValueError):
                eng.life_map([0, 1], regions=[(0, 0, 9, 9), box])
        with pytest.raises(ValueError):
            eng.life_map([0, 1], regions=[(0, 0, 9, 9)])
    finally:
        eng.L = real


def gtp_expected(n, exp):
    from elf_amd.gtp import xy2move
    v = lambda a: xy2move(int(a) // n, int(a) % n)
    eyes = []
    for a in range(n * n):
        for c, tag in ((0, "b"), (1, "w")):
            bits = int(exp["eye"][a]) >> (4 * c)
            if bits & LE.TRUE:
                eyes.append("%s:%s" % (v(a), tag))
            if bits & LE.SEMI:
                eyes.append("%s:%s?%s" % (v(a), tag, v(exp["semi_move"][c, a])))
    return " ".join(eyes), " ".join(v(a) for a in range(n * n) if exp["alive"][a])


def test_gtp(elf):
    import torch
    from elf_amd.gtp import GtpEngine, xy2move
    n = 9
    lf = LE.life(n)

    def actor(batch):
        b = batch["s"].shape[0]
        return dict(pi=torch.full((b, n * n + 1), 1.0 / (n * n + 1), device="cuda"), V=torch.zeros(b, device="cuda"))

    eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=16, nodes_per_game=1024, status_playouts=64, status_seed=3)
    for name in ("elf-eyes", "elf-life", "elf-fast_score"):
        assert name in eng.command("list_commands").split()
    assert eng.command("elf-eyes") == "= \n\n" and eng.command("elf-life") == "= \n\n" and eng.command("elf-fast_score") == "= 0\n\n"
    # the seki: the outer groups live by two eyes, the inner ones do not
    _, stones, mover = CE.seki()
    eng.sp.setup(stones, [0], mover)
    h = LP.build(lf.RB, stones, mover)
    exp = lf.expected(h)
    lf.RB.free(h)
    eyes, alive = gtp_expected(n, exp)
    assert eng.command("elf-eyes") == "= %s\n\n" % eyes and eng.command("elf-life") == "= %s\n\n" % alive
    inner = set(CE.xy(n, CE.SEKI_INNER_BLACK + CE.SEKI_INNER_WHITE))
    listed = set(alive.split())
    assert listed == {xy2move(a // n, a % n) for a in range(n * n) if stones[a] and a not in inner}
    assert eng.command("elf-fast_score") == "= %d\n\n" % exp["summary"][0] == eng.command("elf-fast_score chinese")
    assert eng.command("elf-fast_score japanese") == "= %d\n\n" % exp["summary"][1]
    assert eng.command("elf-fast_score aga").startswith("?")
    # a semi-eye
    st = LE.constructed(n)["semi_centre_centre"]
    eng.sp.restart([0])
    eng.sp.setup(st["stones"], [0], st["mover"])
    h = LP.build(lf.RB, st["stones"], st["mover"])
    exp = lf.expected(h)
    lf.RB.free(h)
    eyes, alive = gtp_expected(n, exp)
    (a, m), = st["semi"].items()
    v = lambda p: xy2move(p // n, p % n)
    assert eyes == "%s:b %s:b?%s" % (v(a), v(a), v(m)) and alive == ""
    assert eng.command("elf-eyes") == "= %s\n\n" % eyes and eng.command("elf-life") == "= \n\n"
    assert eng.command("elf-fast_score") == "= %d\n\n" % exp["summary"][0]
    eng.close()
