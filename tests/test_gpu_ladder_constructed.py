"""GPU: elfgo_ladder_map (k_ladder_map) on the constructed inputs of ladder_positions: hand-built ladders, ko cases and the
layouts of tests/golden/ladder_constructed.npz, each in its 8 board symmetries and both colour assignments.

Every image sits in a slot of its own (GoEngine.setup; the pending ko is played in through forward), one engine per board size,
and one ladder_map launch covers all slots.  Every expected number comes from checkLadder / checkLadderUseSearch of oracle/_ref's
unshimmed board library at test time; every comparison is integer equality over all points of all rows.
tests/test_ladder_constructed_cpu.py holds the conditions these inputs meet (deep lines, hundreds of nodes, many open forks, all
below the kernel's own bounds, so no point may report -1)."""
import numpy as np
import pytest

import ladder_positions as LP
from pyoracle import RefBoard

pytestmark = pytest.mark.gpu

HEAVY = 6     # rows for the tests that look at the slots themselves
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


_dev = {}


@pytest.fixture(scope="module", autouse=True)
def engines_closed_at_the_end():
    yield
    for eng, _, _ in _dev.values():
        eng.close()
    _dev.clear()


def device(elf, n):
    """-> (engine with row j of LP.expected(n) in slot j and HEAVY spare slots, depth [K, NP], calls [K, NP] of one launch over
    all rows), once per process"""
    if n in _dev:
        return _dev[n]
    _need(n)
    _, rows = LP.expected(n)
    K = len(rows)
    eng = elf.GoEngine(n, K + HEAVY)
    plain = [j for j, r in enumerate(rows) if r["moves"] is None]
    ok = eng.setup(np.array([rows[j]["stones"] for j in plain]), ids=plain, next_player=[rows[j]["mover"] for j in plain])
    assert (npy(ok) == 1).all()
    played = [j for j, r in enumerate(rows) if r["moves"] is not None]
    for t in range(max(len(rows[j]["moves"]) for j in played)):
        idx = [j for j in played if t < len(rows[j]["moves"])]
        assert (npy(eng.forward(idx, [int(rows[j]["moves"][t]) for j in idx])) == 1).all()
    col, _ = eng.export_board(n=K)
    info = npy(eng.info(n=K))
    assert np.array_equal(npy(col), np.array([r["stones"] for r in rows]))
    assert np.array_equal(info[:, 1], np.array([r["mover"] for r in rows]))
    d, c = eng.ladder_map(n=K, with_calls=True)
    _dev[n] = (eng, npy(d), npy(c))
    return _dev[n]


def heaviest(n):
    """the heaviest image (largest num_call) of each of the HEAVY heaviest positions"""
    _, rows = LP.expected(n)
    best = {}
    for j, r in enumerate(rows):
        w = int(r["calls"].max())
        if r["name"] not in best or w > best[r["name"]][0]:
            best[r["name"]] = (w, j)
    return [j for _, j in sorted(best.values(), reverse=True)[:HEAVY]]


# ---- 1. integer equality on every point of every image -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_maps_equal_the_reference(elf, n):
    _, rows = LP.expected(n)
    _, d, c = device(elf, n)
    want_d, want_c = np.array([r["depth"] for r in rows]), np.array([r["calls"] for r in rows])
    bad = [(r["name"], r["s"], r["swapped"]) for j, r in enumerate(rows)
           if not (np.array_equal(d[j], want_d[j]) and np.array_equal(c[j], want_c[j]))]
    print("constructed ladders %dx%d: %d rows, %d searches, largest num_call %d, largest depth %d, overflow %d, rows that differ %d"
          % (n, n, len(rows), int((want_c > 0).sum()), int(want_c.max()), int(want_d.max()), int((c == -1).sum()), len(bad)))
    assert (c != -1).all(), "every input stays below the kernel's bounds"
    assert not bad, bad[:8]
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


def test_the_pending_ko_is_on_the_device(elf):
    """the ko rows went in through forward: the slot has the ko the reference has, and refuses the ko point"""
    n = 19
    lad, rows = LP.expected(n)
    eng, d, c = device(elf, n)
    idx = [j for j, r in enumerate(rows) if r["name"] == "ko_pending"]
    assert len(idx) == 16
    legal = npy(eng.legal_mask(idx))
    plain = [j for j, r in enumerate(rows) if r["name"] == "ko_plain"]
    legal_plain = npy(eng.legal_mask(plain))
    _, _, k = LP.ko_cases(n)
    for i, (j, p) in enumerate(zip(idx, plain)):
        a = int(LP.sym_perm(n, rows[j]["s"])[k])
        assert rows[j]["info"][5] == lad.coords[a]
        assert legal[i, a] == 0 and legal_plain[i, a] == 1 and d[j, a] == 0 and d[p, a] == 0
        assert np.array_equal(d[j], d[p]) and np.array_equal(c[j], c[p]) and c[j].max() >= 2 * n


# ---- 2. heavy rows next to trivial ones ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_a_permuted_launch_gives_the_same_rows(elf, n):
    _, rows = LP.expected(n)
    eng, d, c = device(elf, n)
    order = np.argsort([-int(r["calls"].sum()) for r in rows], kind="stable")
    K = len(rows)
    perm = np.empty(K, np.int64)
    perm[0::2], perm[1::2] = order[:(K + 1) // 2], order[::-1][:K // 2]       # heaviest, lightest, second heaviest, ...
    assert sorted(perm) == list(range(K))
    pd, pc = [npy(t) for t in eng.ladder_map(perm, with_calls=True)]
    assert np.array_equal(pd, d[perm]) and np.array_equal(pc, c[perm])
    rng = np.random.RandomState(11)
    perm = rng.permutation(K)
    pd, pc = [npy(t) for t in eng.ladder_map(perm, with_calls=True)]
    assert np.array_equal(pd, d[perm]) and np.array_equal(pc, c[perm])
    assert np.array_equal(npy(eng.ladder_map(perm)), d[perm])                  # calls == NULL


# ---- 3. the call changes nothing, and the slot plays on as the reference does ------------------------------------------------
@pytest.mark.parametrize("n", [19, 9])
def test_the_call_changes_nothing_on_the_heaviest_rows(elf, n):
    lad, rows = LP.expected(n)
    eng, d, c = device(elf, n)
    ids = heaviest(n)
    assert len(ids) == HEAVY and len({rows[j]["name"] for j in ids}) == HEAVY and all(c[j].max() >= n for j in ids)

    def snap():
        col, lib = eng.export_board(ids)
        return [npy(eng.info(ids)), npy(col), npy(lib), npy(eng.legal_mask(ids)), npy(eng.extract_agz(ids))]
    before = snap()
    hd, hc = [npy(t) for t in eng.ladder_map(ids, with_calls=True)]
    assert np.array_equal(hd, d[ids]) and np.array_equal(hc, c[ids])
    assert all(np.array_equal(hd[i], rows[j]["depth"]) and np.array_equal(hc[i], rows[j]["calls"]) for i, j in enumerate(ids))
    after = snap()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # one further forward, on copies in the spare slots: the most searched point of each row, which TryPlay2 accepts
    K = len(rows)
    spare = [K + i for i in range(HEAVY)]
    eng.copy(spare, ids)
    moves = [int(lad.coords[int(rows[j]["calls"].argmax())]) for j in ids]
    assert (npy(eng.forward(spare, moves)) == 1).all()
    info = npy(eng.info(spare))
    col, lib = [npy(t) for t in eng.export_board(spare)]
    for i, j in enumerate(ids):
        h = LP.handle(lad.RB, rows[j])
        assert lad.RB.play(h, moves[i]) == 1
        wc, wl = lad.RB.board(h)
        assert int(hash_of(info[i:i + 1])[0]) == lad.RB.hash(h), rows[j]["name"]
        assert np.array_equal(col[i], wc) and np.array_equal(lib[i], wl), rows[j]["name"]
        assert info[i, 1] == lad.RB.info(h)[1]
        lad.RB.free(h)
    # the rows themselves are still what they were
    assert all(np.array_equal(a, b) for a, b in zip(before, snap()))
