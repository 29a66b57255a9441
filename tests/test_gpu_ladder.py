"""GPU: elfgo_ladder_map (k_ladder_map) against the reference's own ladder reader.

Every expected number comes from checkLadder / checkLadderUseSearch of oracle/_ref's unshimmed board library (ladder_expected);
the games come from tests/golden and from seeded 9x9 playouts.  Every comparison is integer equality over all points of all
positions: no sampling, no tolerance.

test_depth_equals_the_reference asserts depth equality on everything, with its input set pinned (115 suite games, 12 522
positions).  test_calls_equal_the_reference re-asserts depth equality first and only then compares the call counts: where
the device searched (calls > 0) the reference's direct search on a clone gives the same depth and the same num_call, where it
did not (calls == 0) checkLadder returned 0, and no point reports the overflow status -1."""
import numpy as np
import pytest

import ladder_expected as LE
import setup_expected as SE
from pyoracle import RefBoard

pytestmark = pytest.mark.gpu

M_PASS = 0


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


_maps = {}


def device_maps(elf, n):
    """the games played in lock step, one slot per game, one ladder_map launch per ply over the games that are still running
    -> per game (depth [k+1, NP], calls [k+1, NP]), computed once per process"""
    if n in _maps:
        return _maps[n]
    gs, _ = LE.all_expected(n)
    G = len(gs)
    eng = elf.GoEngine(n, G)
    dep = [np.zeros((len(mv) + 1, n * n), np.int16) for mv in gs]
    cal = [np.zeros((len(mv) + 1, n * n), np.int16) for mv in gs]
    for t in range(max(len(mv) for mv in gs) + 1):
        idx = [g for g in range(G) if t <= len(gs[g])]
        d, c = eng.ladder_map(idx, with_calls=True)
        d, c = npy(d), npy(c)
        for j, g in enumerate(idx):
            dep[g][t], cal[g][t] = d[j], c[j]
        idx = [g for g in range(G) if t < len(gs[g])]
        if idx:
            assert (npy(eng.forward(idx, [int(gs[g][t]) for g in idx])) == 1).all()
    eng.close()
    _maps[n] = (dep, cal)
    return _maps[n]


def _depth_mismatches(elf, n):
    _, exp = LE.all_expected(n)
    dep, _ = device_maps(elf, n)
    bad = sum(int((dep[g] != exp[g]["depth"]).sum()) for g in range(len(exp)))
    positions = sum(len(e["depth"]) for e in exp)
    nonzero = sum(int((d > 0).sum()) for d in dep)
    print("ladder depth %dx%d: %d positions, %d non-zero device answers, %d mismatching elements" % (n, n, positions, nonzero, bad))
    return bad, positions


# ---- 1. depth equality on every position of both sets ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_depth_equals_the_reference(elf, n):
    _need(n)
    bad, positions = _depth_mismatches(elf, n)
    assert positions == (12522 if n == 19 else 7055)
    assert bad == 0


# ---- 2. call-count equality -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_calls_equal_the_reference(elf, n):
    _need(n)
    bad, _ = _depth_mismatches(elf, n)
    assert bad == 0, "step 1 has to pass before the call counts are compared"
    _, exp = LE.all_expected(n)
    dep, cal = device_maps(elf, n)
    overflow = searched_wrong = calls_wrong = zero_wrong = 0
    for g, e in enumerate(exp):
        overflow += int((cal[g] == -1).sum())
        on = cal[g] > 0
        # e["calls"] > 0 exactly where checkLadder's own test passes, and there Ladder.expected has already asserted that the
        # direct search on the clone returns checkLadder's depth
        searched_wrong += int((on != (e["calls"] > 0)).sum())
        calls_wrong += int((on & (cal[g] != e["calls"])).sum())
        zero_wrong += int(((cal[g] == 0) & (e["depth"] != 0)).sum())
    print("ladder calls %dx%d: overflow %d, searched-set differences %d, num_call differences %d, unsearched non-zero %d"
          % (n, n, overflow, searched_wrong, calls_wrong, zero_wrong))
    assert overflow == 0
    assert searched_wrong == 0 and calls_wrong == 0 and zero_wrong == 0


# ---- 3. rows the reference's Board-level play treats differently from GoState ---------------------------------------------------
def _ladder_positions(n, want, no_ko=False):
    """up to `want` (game, ply) with a non-zero ladder point, from different games"""
    gs, exp = LE.all_expected(n)
    out = []
    for g, e in enumerate(exp):
        ok = (e["depth"] > 0).any(axis=1)
        if no_ko:
            ok &= ~SE.ko_pending(e["info"])
        ts = np.nonzero(ok)[0]
        if len(ts):
            out.append((g, int(ts[len(ts) // 2])))
        if len(out) == want:
            break
    assert len(out) == want
    return out


def _play_to(eng, gs, where, base=0):
    """slot base + j <- game where[j][0] at ply where[j][1]"""
    for t in range(max(u for _, u in where)):
        idx = [j for j, (_, u) in enumerate(where) if u > t]
        assert (npy(eng.forward([base + j for j in idx], [int(gs[where[j][0]][t]) for j in idx])) == 1).all()


def test_after_two_passes(elf):
    """two passes end a GoState (terminated() refuses every further forward), not a Board: the map is still the reference's"""
    _need(19)
    n = 19
    gs, exp = LE.all_expected(n)
    where = _ladder_positions(n, 16)
    K = len(where)
    eng = elf.GoEngine(n, K)
    _play_to(eng, gs, where)
    for _ in range(2):
        assert (npy(eng.forward(list(range(K)), [M_PASS] * K)) == 1).all()
    assert (npy(eng.info(list(range(K))))[:, 9] == 1).all()                      # terminated
    assert (npy(eng.forward(list(range(K)), [int(gs[g][min(u, len(gs[g]) - 1)]) for g, u in where])) == 0).all()
    d, c = eng.ladder_map(with_calls=True)
    d, c = npy(d), npy(c)
    lad = LE.Ladder(n)
    nonzero = 0
    for j, (g, u) in enumerate(where):
        h = lad.RB.new()
        for m in list(gs[g][:u]) + [M_PASS, M_PASS]:
            assert lad.RB.play(h, int(m)) == 1
        wd, wc = lad.expected(h)
        lad.RB.free(h)
        assert np.array_equal(d[j], wd) and np.array_equal(c[j], wc), (g, u)
        nonzero += int((wd > 0).sum())
    assert nonzero >= K      # the mover is the same after two passes: the ladders are still there
    eng.close()


def test_after_copy_and_after_setup(elf):
    """a copied row gives the source's map.  A row made by GoEngine.setup holds the stones of a played position but neither its
    last moves nor a ko; the reference's search reads stones, liberties, the ko point and the side to move (last moves only
    after it has played two of its own), so at plies with no ko pending the expected map is that of the played position."""
    _need(19)
    n = 19
    gs, exp = LE.all_expected(n)
    where = _ladder_positions(n, 16, no_ko=True)
    K = len(where)
    eng = elf.GoEngine(n, 3 * K)
    _play_to(eng, gs, where)
    src = list(range(K))
    eng.copy([K + j for j in src], src)
    col, _ = eng.export_board(src)
    players = npy(eng.info(src))[:, 1].astype(np.uint8)
    assert (npy(eng.setup(col, ids=[2 * K + j for j in src], next_player=players)) == 1).all()
    d, c = eng.ladder_map(with_calls=True)
    d, c = npy(d), npy(c)
    for j, (g, u) in enumerate(where):
        for row in (j, K + j, 2 * K + j):
            assert np.array_equal(d[row], exp[g]["depth"][u]) and np.array_equal(c[row], exp[g]["calls"][u]), (g, u, row)
        assert (d[j] > 0).any()
    eng.close()


# ---- 4. the call changes nothing ------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing(elf):
    _need(19)
    n = 19
    gs, exp = LE.all_expected(n)
    where = _ladder_positions(n, 32)
    K = len(where)
    eng = elf.GoEngine(n, K)
    _play_to(eng, gs, where)
    ids = list(range(K))

    def snap():
        col, lib = eng.export_board(ids)
        return [npy(eng.info(ids)), npy(col), npy(lib), npy(eng.legal_mask(ids)), npy(eng.extract_agz(ids))]
    before = snap()
    d = npy(eng.ladder_map(ids))
    assert (d > 0).any(axis=1).all()
    after = snap()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # a forward afterwards gives the reference's position
    RB = RefBoard(n)
    going = [j for j, (g, u) in enumerate(where) if u < len(gs[g])]
    assert len(going) >= K // 2
    assert (npy(eng.forward(going, [int(gs[where[j][0]][where[j][1]]) for j in going])) == 1).all()
    info = npy(eng.info(going))
    col, lib = eng.export_board(going)
    for k, j in enumerate(going):
        g, u = where[j]
        rep = RB.replay(gs[g][:u + 1])
        assert int(hash_of(info[k:k + 1])[0]) == int(rep["hash"][u + 1])
        assert np.array_equal(npy(col)[k], rep["colour"][u + 1]) and np.array_equal(npy(lib)[k], rep["libs"][u + 1])
    eng.close()


# ---- 5. ids handling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_ids_handling(elf, n):
    _need(n)
    gs, exp = LE.all_expected(n)
    where = _ladder_positions(n, 24)
    K = len(where)
    eng = elf.GoEngine(n, K)                       # capacity = K: the full call is the n = capacity case
    _play_to(eng, gs, where)
    full_d, full_c = [npy(t) for t in eng.ladder_map(with_calls=True)]
    for j, (g, u) in enumerate(where):
        assert np.array_equal(full_d[j], exp[g]["depth"][u]) and np.array_equal(full_c[j], exp[g]["calls"][u])
    again_d, again_c = [npy(t) for t in eng.ladder_map(with_calls=True)]
    assert np.array_equal(again_d, full_d) and np.array_equal(again_c, full_c)
    assert np.array_equal(npy(eng.ladder_map()), full_d)                        # calls == NULL
    rng = np.random.RandomState(5)
    perm = rng.permutation(K)
    d, c = [npy(t) for t in eng.ladder_map(perm, with_calls=True)]
    assert np.array_equal(d, full_d[perm]) and np.array_equal(c, full_c[perm])
    sub = perm[: K // 3]
    d, c = [npy(t) for t in eng.ladder_map(sub, with_calls=True)]
    assert np.array_equal(d, full_d[sub]) and np.array_equal(c, full_c[sub])
    dup = [3, 3, 0, 3]
    assert np.array_equal(npy(eng.ladder_map(dup)), full_d[dup])
    for j in (0, K - 1):
        assert np.array_equal(npy(eng.ladder_map([j]))[0], full_d[j])           # n = 1
    assert np.array_equal(npy(eng.ladder_map(n=1))[0], full_d[0])               # ids == NULL, n = 1
    assert np.array_equal(npy(eng.ladder_map(n=5)), full_d[:5])
    # a slot id outside the pool reads nothing: depth 0, calls -1 for the row; its neighbours are untouched
    d, c = [npy(t) for t in eng.ladder_map([0, K, -1, 1], with_calls=True)]
    assert np.array_equal(d[[0, 3]], full_d[[0, 1]]) and np.array_equal(c[[0, 3]], full_c[[0, 1]])
    assert (d[1:3] == 0).all() and (c[1:3] == -1).all()
    # argument errors are status codes
    from elf_amd import _lib
    import ctypes as C
    assert eng.L.elfgo_ladder_map(eng._h, None, K + 1, C.c_void_p(1), None, None) == -1     # ids NULL and n > capacity
    assert eng.L.elfgo_ladder_map(eng._h, None, 1, None, None, None) == -1                  # no output
    assert eng.L.elfgo_ladder_map(eng._h, None, -1, C.c_void_p(1), None, None) == -1
    assert eng.L.elfgo_ladder_map(eng._h, None, 0, None, None, None) == 0
    eng.close()


# ---- 6. GTP ---------------------------------------------------------------------------------------------------------------------
def test_gtp_elf_ladders(elf, tmp_path):
    import torch
    from elf_amd.gtp import GtpEngine, xy2move
    _need(19)
    n = 19
    gs, exp = LE.all_expected(n)

    def actor(batch):
        b = batch["s"].shape[0]
        return dict(pi=torch.full((b, n * n + 1), 1.0 / (n * n + 1), device="cuda"), V=torch.zeros((b,), device="cuda"))
    eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=32, nodes_per_game=2048)
    assert eng.command("known_command elf-ladders") == "= true\n\n"
    assert "elf-ladders" in eng.command("list_commands").split()
    assert eng.command("elf-ladders") == "= \n\n"                                           # the empty board
    S = n + 2
    checked = 0
    for g, u in _ladder_positions(n, 3):
        text = "(;SZ[19]" + "".join(";%s[%s%s]" % ("BW"[t % 2], chr(97 + int(c) % S - 1), chr(97 + int(c) // S - 1))
                                     for t, c in enumerate(gs[g])) + ")"
        f = tmp_path / ("game%d.sgf" % g)
        f.write_text(text)
        assert eng.command("loadsgf %s %d" % (f, u + 1)) == "= \n\n"
        want = exp[g]["depth"][u]
        pairs = " ".join("%s:%d" % (xy2move(a // n, a % n), int(want[a])) for a in range(n * n) if want[a])
        assert pairs
        assert eng.command("elf-ladders") == "= %s\n\n" % pairs
        checked += 1
    assert checked == 3
    assert eng.command("clear_board") == "= \n\n" and eng.command("elf-ladders") == "= \n\n"
    eng.close()
