"""GPU: elfgo_df_extract / elfgo_extract_df (k_extract_df) and the placement-ply table behind GoEngine(track_placed=True)
(k_df_note and the other elfgo_df_* forms) against the reference's own BoardFeature::extract (df_expected, proven by
tests/test_df_cpu.py).  Every comparison is bit equality, float32 compared as uint32; every row is compared."""
import ctypes as C

import numpy as np
import pytest

import df_expected as DE
import ownership_expected as OE
from pyoracle import Ref, coord

pytestmark = pytest.mark.gpu

M_INVALID = 3


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    assert Ref.available(9) and Ref.available(19), "build() must have produced oracle/_ref/libelfref{9,19}.so"
    return elf_amd


def npy(t):
    return t.cpu().numpy()


def assert_planes(got, want, what):
    g, w = DE.bits(got), DE.bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        r, p = [int(v[0]) for v in np.nonzero((g != w).any(axis=(2, 3)))]
        raise AssertionError("%s: first differing row %d, plane %d\ngot\n%s\nwant\n%s" % (what, r, p, got[r, p], want[r, p]))


def check_rows(eng, D, ids, states, codes, what):
    """planes of slots `ids` under `codes` and their table rows against the reference states"""
    assert_planes(npy(eng.extract_df(ids, d4=codes)), np.array([D.planes(s, c) for s, c in zip(states, codes)]), what)
    pl = npy(eng.placed(ids)).astype(np.int64)
    for r, s in enumerate(states):
        on = D.E.board(s)[0] != 0
        assert np.array_equal(pl[r][on], D.last_placed(s)[on]), (what, "placed", r)


def play_both(eng, D, ids, states, moves):
    ok = npy(eng.forward(ids, moves))
    for r, (s, c) in enumerate(zip(states, moves)):
        assert int(ok[r]) == D.E.forward(s, int(c)) == 1, (r, c)


# ---- 1. every ply of whole games ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nine", "ladder16", "playout19"])
def test_every_ply_equals_the_reference(elf, name):
    n, games, exp = DE.all_expected(name)
    eng = elf.GoEngine(n, len(games), track_placed=True)
    longest = max(len(m) for m in games)
    rows = deepest = 0
    for t in range(longest + 1):
        live = [i for i, m in enumerate(games) if t <= len(m)]
        got = npy(eng.extract_df(live, d4=[DE.code_of(i, t) for i in live]))
        assert_planes(got, np.array([exp[i]["planes"][t] for i in live]), "%s ply %d (games %s...)" % (name, t, live[:4]))
        pl = npy(eng.placed(live)).astype(np.int64)
        for r, i in enumerate(live):
            on = exp[i]["colour"][t] != 0
            assert np.array_equal(pl[r][on], exp[i]["placed"][t][on]), (name, "placed", i, t)
            if on.any():
                deepest = max(deepest, int(exp[i]["info"][t, 0] - exp[i]["placed"][t][on].min()))
        rows += len(live)
        fwd = [i for i in live if t < len(games[i])]
        if fwd:
            assert bool((eng.forward(fwd, [int(games[i][t]) for i in fwd]) == 1).all())
    eng.close()
    assert rows == sum(len(m) + 1 for m in games)
    if name == "nine":
        assert longest == 2 * n * n - 1, "the longest of these games runs to the move limit"
    print("%s: %d rows, oldest stone %d plies" % (name, rows, deepest))


# ---- 2. all 8 codes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,count", [("nine", 64), ("ladder16", 1)])
def test_all_eight_codes_at_every_16th_ply(elf, name, count):
    n, games = DE.game_set(name)
    games = games[:count]
    D = DE.df(n)
    eng = elf.GoEngine(n, len(games), track_placed=True)
    states = [D.E.new() for _ in games]
    checked = 0
    for t in range(max(len(m) for m in games) + 1):
        live = [i for i, m in enumerate(games) if t <= len(m)]
        if t % 16 == 0:
            for d4 in range(8):
                check_rows(eng, D, live, [states[i] for i in live], [d4] * len(live), "%s ply %d code %d" % (name, t, d4))
            checked += 8 * len(live)
        fwd = [i for i in live if t < len(games[i])]
        if fwd:
            play_both(eng, D, fwd, [states[i] for i in fwd], [int(games[i][t]) for i in fwd])
    eng.close()
    for s in states:
        D.E.free(s)
    assert checked >= 8 * len(games)


# ---- 3. the simple ko -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 19])
def test_ko_position_under_every_code(elf, n):
    D = DE.df(n)
    eng = elf.GoEngine(n, 8, track_placed=True)
    states = [D.E.new() for _ in range(8)]
    ids = list(range(8))
    for c in OE.ko_moves(n):
        play_both(eng, D, ids, states, [c] * 8)
    got = npy(eng.extract_df(ids, d4=ids))
    assert [int(got[d4, 6].sum()) for d4 in range(8)] == [1] * 8 and int(npy(eng.info())[0, 4]) == 0
    check_rows(eng, D, ids, states, ids, "ko %d" % n)
    play_both(eng, D, ids, states, [coord(n, n - 2, n - 3)] * 8)          # one more move elsewhere: ko_age 1
    assert int(npy(eng.info())[0, 4]) == 1 and not npy(eng.extract_df(ids, d4=ids))[:, 6].any()
    check_rows(eng, D, ids, states, ids, "aged ko %d" % n)
    eng.close()
    for s in states:
        D.E.free(s)


# ---- 4. refused moves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 19])
def test_refused_moves_leave_table_and_planes(elf, n):
    D = DE.df(n)
    ko = OE.ko_moves(n)                                                      # White to move, ko at (1,0), Black stone on (0,0)
    corner = [coord(n, 1, 0), coord(n, 5, 5), coord(n, 0, 1)]                # White to move, (0,0) is suicide
    lists = [ko, ko, corner, ko]
    tries = [coord(n, 0, 0), coord(n, 1, 0), coord(n, 0, 0), M_INVALID]      # occupied, the ko retake, suicide, M_INVALID
    eng = elf.GoEngine(n, 4, track_placed=True)
    states = OE.states_of(D.E, lists)
    OE.play_all(eng, lists)
    ids, codes = [0, 1, 2, 3], [0, 3, 5, 6]
    before = (npy(eng.placed()), npy(eng.extract_df(d4=codes)), npy(eng.info()))
    check_rows(eng, D, ids, states, codes, "before")
    ok = npy(eng.forward(ids, tries))
    assert ok.tolist() == [0, 0, 0, 255]
    assert [D.E.forward(s, c) for s, c in zip(states, tries)] == [0, 0, 0, -1]
    after = (npy(eng.placed()), npy(eng.extract_df(d4=codes)), npy(eng.info()))
    for b, a in zip(before, after):
        assert np.array_equal(b.view(np.uint8), a.view(np.uint8))
    check_rows(eng, D, ids, states, codes, "after the refusals")
    play_both(eng, D, ids, states, [coord(n, 6, 6)] * 4)
    assert bool((eng.forward(ids, [0] * 4) == 1).all()) and all(D.E.forward(s, 0) == 1 for s in states)   # a pass writes nothing
    check_rows(eng, D, ids, states, codes, "one move and a pass later")
    eng.close()
    for s in states:
        D.E.free(s)


# ---- 5. set-up positions --------------------------------------------------------------------------------------------------------
def _expected_after_setup(elf, eng, n, ids, model, codes):
    """planes 0-9, 14-17 from export_board with numpy; plane 6 from the info record; 10 / 11 = table[ply - model] on the stones"""
    tab = np.zeros(2 * n * n + 1, np.float32)
    assert eng.L.elfgo_df_exp_table(n, tab.ctypes.data) == 0
    col, lib = [npy(t) for t in eng.export_board(ids)]
    info = npy(eng.info(ids))
    want = []
    for r in range(len(ids)):
        player, ply = int(info[r, 1]), int(info[r, 0])
        src = DE.numpy_planes(n, col[r], lib[r], player)
        if info[r, 4] == 0 and info[r, 5] != 0:
            x, y = elf.coord_xy(n, int(info[r, 5]))
            src[6, x, y] = 1
        hist = np.where(col[r] != 0, tab[np.clip(ply - model[r], 0, 2 * n * n)], np.float32(0)).astype(np.float32).reshape(n, n)
        src[10] = hist * (col[r].reshape(n, n) == player)
        src[11] = hist * (col[r].reshape(n, n) == 3 - player)
        want.append(DE.transform_planes(n, src, codes[r]))
    return np.array(want), col


@pytest.mark.parametrize("n,name,ply", [(9, "nine", 30), (19, "playout19", 150)])
def test_setup_positions(elf, n, name, ply):
    _, games, exp = DE.all_expected(name)
    K = 4
    stones = np.array([exp[i]["colour"][ply] for i in range(K)], np.uint8)
    assert all((stones[i] == 1).any() and (stones[i] == 2).any() for i in range(K))
    eng = elf.GoEngine(n, K, track_placed=True)
    OE.play_all(eng, [[int(c) for c in games[i][:12]] for i in range(K)])    # the table rows hold something else first
    ids, codes = list(range(K)), [1, 4, 6, 7]
    assert npy(eng.setup(stones, next_player=[2] * K)).tolist() == [1] * K
    model = (stones != 0).astype(np.int64)
    for step in range(8):
        pl, info = npy(eng.placed()).astype(np.int64), npy(eng.info())
        assert (info[:, 0] == 1 + step).all() and (info[:, 1] == (2 if step % 2 == 0 else 1)).all()
        want, col = _expected_after_setup(elf, eng, n, ids, model, codes)
        assert np.array_equal(pl[col != 0], model[col != 0]), step
        if step == 0:
            assert np.array_equal(pl, model), "1 under every stone and 0 elsewhere"
        assert_planes(npy(eng.extract_df(d4=codes)), want, "set-up + %d moves" % step)
        if step < 7:
            legal = npy(eng.legal_mask())[:, :-1]
            acts = [int(np.nonzero(legal[r])[0][(5 * step + r) % int(legal[r].sum())]) for r in range(K)]
            assert bool((eng.forward(ids, [coord(n, a // n, a % n) for a in acts]) == 1).all())
            for r, a in enumerate(acts):
                model[r, a] = 1 + step
    # a refused set-up (a white stone without a liberty) leaves slot, table row and planes as they were
    bad = np.zeros((1, n * n), np.uint8)
    bad[0, [1 * n + 0, 0 * n + 1]] = 1
    bad[0, 0] = 2
    before = (npy(eng.placed()), npy(eng.extract_df(d4=codes)), npy(eng.info()), npy(eng.export_board()[0]))
    assert npy(eng.setup(bad, ids=[2], next_player=[1])).tolist() == [0]
    after = (npy(eng.placed()), npy(eng.extract_df(d4=codes)), npy(eng.info()), npy(eng.export_board()[0]))
    for b, a in zip(before, after):
        assert np.array_equal(b.view(np.uint8), a.view(np.uint8))
    eng.close()


# ---- 6. copy and reset ----------------------------------------------------------------------------------------------------------
def test_copy_then_different_continuations(elf):
    n, games = DE.game_set("nine")
    D = DE.df(n)
    K = 4
    eng = elf.GoEngine(n, 2 * K, track_placed=True)
    lists = [[int(c) for c in games[i][:24]] for i in range(K)]
    OE.play_all(eng, lists + [[int(c) for c in games[K + i][:9]] for i in range(K)])   # the destination rows are not blank
    src = OE.states_of(D.E, lists)
    eng.copy(list(range(K, 2 * K)), list(range(K)))
    cpy = [D.E.clone(s) for s in src]
    ids, states, codes = list(range(2 * K)), src + cpy, [0, 1, 2, 3, 4, 5, 6, 7]
    check_rows(eng, D, ids, states, codes, "after the copy")
    for t in range(10):
        mv = [int(games[i][24 + t]) for i in range(K)]
        for r in range(K):   # the copy plays the last legal point that is not the source's move
            legal = np.nonzero(D.E.legal_mask(cpy[r])[:-1])[0]
            a = int([a for a in legal if coord(n, a // n, a % n) != mv[r]][-1 - t])
            mv.append(coord(n, a // n, a % n))
        play_both(eng, D, ids, states, mv)
        check_rows(eng, D, ids, states, codes, "continuation %d" % t)
    # reset: rows to 0, the planes of the empty board
    eng.reset([1, K + 2])
    for i in (1, K + 2):
        D.E.reset(states[i])
    assert not npy(eng.placed([1, K + 2])).any() and npy(eng.placed([0])).any()
    check_rows(eng, D, ids, states, codes, "after the reset")
    eng.close()
    for s in states:
        D.E.free(s)


# ---- 7. launch geometry and buffers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool(elf):
    """per board size: a tracked engine of 8 slots at different plies and the reference states of the slots"""
    made = {}

    def get(n):
        if n not in made:
            _, games = DE.game_set("nine" if n == 9 else "playout19")
            D = DE.df(n)
            lists = [[int(c) for c in games[i % len(games)][:(13 if n == 9 else 40) * (i + 1)]] for i in range(8)]
            eng = elf.GoEngine(n, 8, track_placed=True)
            OE.play_all(eng, lists)
            made[n] = (eng, D, OE.states_of(D.E, lists))
        return made[n]
    yield get
    for eng, D, states in made.values():
        eng.close()
        for s in states:
            D.E.free(s)


@pytest.mark.parametrize("n", [9, 19])
@pytest.mark.parametrize("k", [1, 5, 67])
def test_launch_geometry(elf, pool, n, k):
    import torch
    eng, D, states = pool(n)
    cap, row = eng.capacity, 25 * n * n
    ids = [(7 - j) % 8 for j in range(k)]                      # descending, and slots named several times
    codes = [(3 * j + 1) % 8 for j in range(k)]
    if k >= 5:
        ids[1], ids[3] = cap, -1                               # zero rows between correct neighbours
    want = np.array([D.planes(states[b], c) if 0 <= b < cap else np.zeros((25, n, n), np.float32) for b, c in zip(ids, codes)])
    # contiguous rows: 25 N^2 floats is 4 bytes past a multiple of 16, so consecutive rows start at every 4-byte phase
    assert_planes(npy(eng.extract_df(ids, d4=codes)), want, "contiguous")
    # a row stride of 25 N^2 + 3 floats in a buffer filled with NaN, once from an aligned base and once from 4 bytes behind one
    for shift in (0, 1):
        buf = torch.full((k * (row + 3) + 4,), float("nan"), dtype=torch.float32, device=eng.device)
        out = buf[shift:shift + k * (row + 3)].view(k, row + 3)[:, :row].unflatten(1, (25, n, n))
        assert eng.extract_df(ids, d4=codes, out=out) is out
        assert_planes(npy(out), want, "strided, shift %d" % shift)
        gaps = npy(buf[shift:shift + k * (row + 3)].view(k, row + 3)[:, row:])
        assert np.isnan(gaps).all() and np.isnan(npy(buf[:shift])).all() and np.isnan(npy(buf[shift + k * (row + 3):])).all()
    pl = npy(eng.placed(ids))
    for r, b in enumerate(ids):
        if not 0 <= b < cap:
            assert not pl[r].any()
    # ids=None with n rows
    if k <= cap:
        assert_planes(npy(eng.extract_df(n=k)), np.array([D.planes(states[b]) for b in range(k)]), "ids None")


# ---- 8. the caller's rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [9, 19])
def test_callers_rows_equal_the_handles(elf, pool, n):
    import torch
    eng, D, states = pool(n)
    ids, codes = [5, 2, 7, 0, 3, 3], [2, 7, 0, 5, 1, 6]
    rows = eng.placed(ids).contiguous()
    idt = torch.tensor(ids, dtype=torch.int32, device=eng.device)
    d4t = torch.tensor(codes, dtype=torch.int32, device=eng.device)
    out = torch.full((len(ids), 25, n, n), float("nan"), dtype=torch.float32, device=eng.device)
    st = eng._stream()
    assert eng.L.elfgo_extract_df(eng._df, C.c_void_p(idt.data_ptr()), C.c_void_p(d4t.data_ptr()), len(ids), C.c_void_p(rows.data_ptr()),
                                  C.c_void_p(out.data_ptr()), 25 * n * n, st) == 0
    eng.sync()
    assert_planes(npy(out), npy(eng.extract_df(ids, d4=codes)), "caller's rows")
    assert_planes(npy(out), np.array([D.planes(states[b], c) for b, c in zip(ids, codes)]), "caller's rows against the reference")
    # rows that say "placed one ply earlier" move every history value one table entry on, and nothing else
    older = (rows - 1).clamp(min=0)
    out2 = torch.empty_like(out)
    assert eng.L.elfgo_extract_df(eng._df, C.c_void_p(idt.data_ptr()), C.c_void_p(d4t.data_ptr()), len(ids), C.c_void_p(older.data_ptr()),
                                  C.c_void_p(out2.data_ptr()), 25 * n * n, st) == 0
    eng.sync()
    a, b = npy(out), npy(out2)
    keep = [p for p in range(25) if p not in (10, 11)]
    assert np.array_equal(DE.bits(a[:, keep]), DE.bits(b[:, keep])) and (b[:, 10:12][a[:, 10:12] > 0] < a[:, 10:12][a[:, 10:12] > 0]).all()


# ---- 9. API errors --------------------------------------------------------------------------------------------------------------
def test_api_errors(elf, pool):
    import torch
    n = 9
    eng, D, states = pool(n)
    plain = elf.GoEngine(n, 2)
    with pytest.raises(ValueError):
        plain.extract_df()
    with pytest.raises(ValueError):
        plain.placed()
    plain.close()
    with pytest.raises(ValueError):
        eng.playout(np.arange(8, dtype=np.uint64))
    assert elf.NUM_DF_PLANES == 25
    L, df, st, BAD = eng.L, eng._df, eng._stream(), -1
    out = torch.full((8, 25 * n * n), 7.0, dtype=torch.float32, device=eng.device)
    rows = eng.placed().contiguous()
    op, rp = C.c_void_p(out.data_ptr()), C.c_void_p(rows.data_ptr())
    assert L.elfgo_df_extract(None, None, None, 8, op, 25 * n * n, st) == BAD
    assert L.elfgo_df_extract(df, None, None, -1, op, 25 * n * n, st) == BAD
    assert L.elfgo_df_extract(df, None, None, 9, op, 25 * n * n, st) == BAD          # ids NULL names slots [0, n)
    assert L.elfgo_df_extract(df, None, None, 8, None, 25 * n * n, st) == BAD
    assert L.elfgo_df_extract(df, None, None, 8, op, 25 * n * n - 1, st) == BAD      # rows would overlap
    assert L.elfgo_df_extract(df, None, None, 8, C.c_void_p(out.data_ptr() + 2), 25 * n * n, st) == BAD
    assert L.elfgo_extract_df(df, None, None, 8, None, op, 25 * n * n, st) == BAD
    assert L.elfgo_extract_df(None, None, None, 8, rp, op, 25 * n * n, st) == BAD
    assert L.elfgo_df_placed(df, None, 9, rp, st) == BAD and L.elfgo_df_placed(df, None, 8, None, st) == BAD
    assert L.elfgo_df_placed(None, None, 8, rp, st) == BAD
    assert L.elfgo_df_forward(None, None, None, 8, None, st) == BAD and L.elfgo_df_forward(df, None, None, 8, None, st) == BAD
    assert L.elfgo_df_reset(None, None, 8, st) == BAD and L.elfgo_df_copy(df, None, None, 8, st) == BAD
    assert L.elfgo_df_setup(None, None, None, None, 8, None, st) == BAD and L.elfgo_df_setup(df, None, None, None, 8, None, st) == BAD
    assert L.elfgo_df_create(None, None) == BAD and L.elfgo_df_destroy(None) == BAD
    assert L.elfgo_df_extract(df, None, None, 0, None, 0, st) == 0
    eng.sync()
    assert bool((out == 7.0).all()), "nothing was launched"
    check_rows(eng, D, list(range(8)), states, [0] * 8, "the pool after the refused calls")
