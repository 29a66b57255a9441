"""GPU: the trainer's replay path at its edges -- k_replay_checkpoint + k_replay_extract<KEEP = false> (elf_amd/csrc/train.cuh) and
the dirty list of elftrain_extract (train_capi.hip).  Every ply of long records, superko across a checkpoint, stores whose
max_moves is below / not a multiple of the checkpoint interval, slot reuse, partial workgroups, NULL outputs, padded rows.

Every expected row is computed on the CPU inside the test by `oracle_rows`: one Port state forwarded move by move, the row
taken at each requested ply, field by field as pyoracle.port_train_sample states it (and cross-checked against that function
wherever it is defined: it does not accept move_to == num_moves).  Every comparison is exact; predicted_value and mcts_scores by
bit pattern (rows of a recorded policy that sums to zero are 0 / 0 on both sides: NaN, any payload).

Every output buffer is prefilled with a sentinel (NaN bit patterns for floats, odd patterns for integers) and has GUARD rows
behind the last sample which must keep their bytes; the index arrays carry GUARD valid entries behind the last sample too."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from pyoracle import Port, action2coord, coord, coord2action, playout_seeds, port_train_sample, sgfstr2coords

pytestmark = pytest.mark.gpu

CK = 16          # CK_INTERVAL of train.cuh
GUARD = 2
FIELDS = ("offline_a", "winner", "mcts_scores", "predicted_value", "move_idx", "num_move", "aug_code", "selfplay_ver")
# sentinels as integer bit patterns: f32 / f16 quiet NaNs with a payload, odd integers
SENT = {"f32": 0x7FC0BEEF, "f16": 0x7E5B, "i32": 0x5A5A5A5B, "i64": 0x5A5A5A5A5A5A5A5B}
KIND = dict(offline_a="i64", winner="f32", mcts_scores="f32", predicted_value="f32", move_idx="i32", num_move="i32", aug_code="i32",
            selfplay_ver="i64")
INT_OF = {"f32": np.int32, "f16": np.int16, "i32": np.int32, "i64": np.int64}


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


# ---- records (CPU) ----------------------------------------------------------------------------------------------------------
def make_record(elf, n, moves, seed, black_ver, reward):
    """A Record dict as ReplayLoader.put / port_train_sample read it: a random quantised policy and a value for every ply."""
    from elf_amd.train import coords_to_sgfstr
    rng = np.random.default_rng(seed)
    moves = np.asarray(moves, np.uint16)
    content = coords_to_sgfstr(n, moves)
    assert np.array_equal(sgfstr2coords(n, content), moves)
    pol = rng.integers(0, 256, (len(moves), (n + 2) ** 2), dtype=np.uint8)
    pol[:, 0] |= 1                               # the pass entry: no row sums to zero
    vals = rng.uniform(-1, 1, len(moves)).astype(np.float32)
    return {"request": {"vers": {"black_ver": int(black_ver)}}, "seq": 0,
            "result": {"content": content, "num_move": len(moves), "policies": pol.tolist(), "values": [float(v) for v in vals],
                       "reward": float(reward)}}


def playout(n, base, max_steps=100000):
    port = Port(n)
    st = port.new()
    mv = port.playout_moves(st, int(playout_seeds(1, base=base)[0]), max_steps)
    info = port.info(st)
    term = port.terminated(st)
    port.free(st)
    return mv, int(info[0]), term


_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def golden19(num_move):
    def load():
        g = np.load(os.path.join(GOLDEN, "train_19.npz"))
        return {r["result"]["num_move"]: r for r in (json.loads(str(t)) for t in g["records"])}
    return cached("golden19", load)[num_move]


def playout19(elf):
    def make():
        mv, ply, term = playout(19, 0)
        assert term and len(mv) > 400 and (mv == 0).sum() >= 2
        return make_record(elf, 19, mv, seed=190, black_ver=(1 << 40) + 7, reward=-3.5)
    return cached("playout19", make)


def full9(elf):
    """9x9, num_moves == max_moves == 162: a config-2 playout that runs into the move limit (the game ends when the ply counter
    reaches 162, i.e. after 161 moves, not by two passes) and the one further move a record of 162 can hold, which the engine
    refuses like every move after the end."""
    def make():
        mv, ply, term = playout(9, 63)
        assert len(mv) == 161 and ply == 162 and term and not (mv[-1] == 0 and mv[-2] == 0)
        rec = make_record(elf, 9, list(mv) + [coord(9, 4, 4)], seed=90, black_ver=-5, reward=0.5)
        assert rec["result"]["num_move"] == 162 == 2 * 9 * 9
        return rec
    return cached("full9", make)


def part9(elf, base, k):
    """the first k moves of a 9x9 playout (base picks the playout)"""
    def make():
        mv, _, _ = playout(9, base, k)
        assert len(mv) == k
        return make_record(elf, 9, mv, seed=1000 * base + k, black_ver=100 + base, reward=(-1) ** k * 2.5)
    return cached(("part9", base, k), make)


def superko19(elf, f):
    """ "sending two returning one" in the corner behind f filler moves; the recapture (index f + 8) repeats the position after
    White's tenuki; 30 more recorded moves follow.  Asserts on the port where the game ends."""
    def make():
        n = 19
        mv = [coord(n, 4 + i, 12 + (i % 2)) for i in range(f)]                      # far from the corner, colours alternate
        mv += [coord(n, 1, 0), coord(n, 0, 1), coord(n, 2, 1), coord(n, 1, 1), coord(n, 3, 0), coord(n, 15, 15)]
        mv += [coord(n, 0, 0), coord(n, 2, 0), coord(n, 1, 0)]
        recap = f + 8
        assert len(mv) == recap + 1 and len(set(mv[:f])) == f
        rng = np.random.default_rng(f)
        tail = [coord(n, int(x), int(y)) for x, y in rng.integers(0, n, (30, 2))]
        tail[3] = 0                                                                    # a pass among the refused moves
        mv += tail
        port = Port(n)
        st = port.new()
        for t, c in enumerate(mv):
            assert port.terminated(st) == (t > recap), (f, t)
            ok = port.forward(st, c)
            assert ok == (1 if t <= recap else 0), (f, t)
        assert port.terminated(st) and int(port.info(st)[0]) == recap + 2              # the ply stays behind the recapture
        port.free(st)
        return make_record(elf, n, mv, seed=500 + f, black_ver=f, reward=1.0), recap
    return cached(("superko19", f), make)


# ---- the oracle: one incremental replay per record -----------------------------------------------------------------------
_perm = {}


def action_perm(n, d4):
    if (n, d4) not in _perm:
        _perm[n, d4] = np.array([action2coord(n, a, d4) for a in range(n * n + 1)])
    return _perm[n, d4]


def oracle_rows(port, record, move_to, d4, nfa):
    """Rows of the "train" batch for samples (move_to[i], d4[i]) of one record; move_to beyond the record counts as num_moves."""
    n = port.n
    res = record["result"]
    mv = sgfstr2coords(n, res["content"])
    nm = len(mv)
    vals, pol = res["values"], res.get("policies") or []
    k = len(move_to)
    out = dict(s=np.zeros((k, 18, n, n), np.float32), offline_a=np.zeros((k, nfa), np.int64), winner=np.zeros(k, np.float32),
               mcts_scores=np.zeros((k, n * n + 1), np.float32), predicted_value=np.zeros(k, np.float32),
               move_idx=np.zeros(k, np.int32), num_move=np.full(k, nm, np.int32), aug_code=np.asarray(d4, np.int32).copy(),
               selfplay_ver=np.full(k, int(record["request"]["vers"]["black_ver"]), np.int64))
    out["winner"][:] = 1.0 if res["reward"] > 0 else -1.0
    at = {}
    for i, mt in enumerate(move_to):
        at.setdefault(min(int(mt), nm), []).append(i)
    st = port.new()
    for t in range(nm + 1):
        if t in at:
            idx = int(port.info(st)[0]) - 1
            for i in at[t]:
                d = int(d4[i])
                out["s"][i] = port.extract_agz(st, d)
                out["move_idx"][i] = idx
                if idx < len(vals):
                    out["predicted_value"][i] = np.float32(vals[idx])
                for j in range(nfa):
                    if idx + j < nm:
                        out["offline_a"][i, j] = coord2action(n, int(mv[idx + j]), d)
                if idx < len(pol):
                    p = np.asarray(pol[idx], np.float32)[action_perm(n, d)]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        out["mcts_scores"][i] = p / p.sum(dtype=np.float32)
                elif idx < nm:
                    out["mcts_scores"][i, coord2action(n, int(mv[idx]), d)] = 1.0
        if t < nm and int(mv[t]) != 3:
            port.forward(st, int(mv[t]))
    port.free(st)
    return out


def assert_rows_equal(got, want, ctx=""):
    """got, want: dicts of numpy arrays, rows = samples"""
    for k in want:
        if k not in got:
            continue
        g, w = got[k], want[k]
        assert g.shape == w.shape, (ctx, k, g.shape, w.shape)
        if k in ("mcts_scores", "predicted_value"):
            fin = np.isfinite(w)
            assert np.isnan(g[~fin]).all(), (ctx, k)
            bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)) & fin)[0]
        else:
            bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (ctx, k, "first differing sample", int(bad[0]), "of", g.shape[0])


def cross_check(port, record, want, move_to, d4, nfa):
    """the incremental oracle against port_train_sample itself on a few plies (first, around a checkpoint, last)"""
    nm = record["result"]["num_move"]
    for i in sorted({0, 1, min(15, len(move_to) - 1), min(16, len(move_to) - 1), min(17, len(move_to) - 1), len(move_to) // 2, len(move_to) - 1}):
        if move_to[i] + nfa > nm:
            continue
        o = port_train_sample(port, record, int(move_to[i]), int(d4[i]), nfa)
        assert_rows_equal({k: np.asarray(want[k][i])[None] for k in want}, {k: np.asarray(o[k])[None] for k in o}, ("cross", i))


def sweep_args(nm, nfa):
    mt = np.arange(0, nm - nfa + 1, dtype=np.int32)
    d4 = ((3 * mt + mt // CK) % 8).astype(np.int32)          # all eight codes, not in step with the checkpoint interval
    return mt, d4


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def alloc(torch, n, rows, nfa, fmt, stride=None, base_off=0):
    """prefilled device buffers for `rows` rows; s is flat: base_off elements, then rows of `stride` elements"""
    row = 18 * n * n
    stride = stride or row
    kind_s = "f16" if fmt == "f16_nhwc" else "f32"

    def full(shape, kind):
        it = {"f32": torch.int32, "f16": torch.int16, "i32": torch.int32, "i64": torch.int64}[kind]
        ft = {"f32": torch.float32, "f16": torch.float16, "i32": torch.int32, "i64": torch.int64}[kind]
        return torch.full(shape, SENT[kind], dtype=it, device="cuda").view(ft)
    b = dict(s=full((base_off + rows * stride + 8,), kind_s), offline_a=full((rows, nfa), "i64"), winner=full((rows,), "f32"),
             mcts_scores=full((rows, n * n + 1), "f32"), predicted_value=full((rows,), "f32"), move_idx=full((rows,), "i32"),
             num_move=full((rows,), "i32"), aug_code=full((rows,), "i32"), selfplay_ver=full((rows,), "i64"))
    b["_geom"] = (n, rows, row, stride, base_off, fmt)
    return b


def collect(torch, b, k, null=()):
    """host copy of the first k rows; asserts that everything else -- guard rows, padding between rows of s, the buffers of
    outputs that were not passed -- still holds the sentinel's bytes"""
    torch.cuda.synchronize()
    n, rows, row, stride, base_off, fmt = b["_geom"]
    kind_s = "f16" if fmt == "f16_nhwc" else "f32"
    raw = b["s"].cpu().numpy()
    bits = raw.view(INT_OF[kind_s])
    keep = np.ones(raw.shape, bool)
    s = np.zeros((k, 18, n, n), np.float32)
    for i in range(k):
        lo = base_off + i * stride
        keep[lo:lo + row] = False
        r = raw[lo:lo + row].astype(np.float32)
        s[i] = r.reshape(n, n, 18).transpose(2, 0, 1) if fmt == "f16_nhwc" else r.reshape(18, n, n)
    assert (bits[keep] == SENT[kind_s]).all(), "s: bytes outside the rows were written"
    out = dict(s=s)
    for f in FIELDS:
        a = b[f].cpu().numpy()
        ab = a.view(INT_OF[KIND[f]])
        lo = 0 if f in null else k
        assert (ab[lo:] == SENT[KIND[f]]).all(), (f, "guard rows / unused buffer were written")
        if f not in null:
            out[f] = a[:k]
    return out


def padded(torch, a, fill):
    """device int32 array with GUARD valid entries behind the samples; returns the view of the samples"""
    a = np.asarray(a, np.int32)
    t = torch.tensor(np.concatenate([a, np.full(GUARD, fill, np.int32)]), device="cuda")
    return t[: a.size]


def loader_extract(torch, ld, slot, move_to, d4, fmt):
    """ReplayLoader.extract into prefilled buffers with guard rows -> host rows"""
    k = len(move_to)
    b = alloc(torch, ld.n, k + GUARD, ld.nfa, fmt)
    n = ld.n
    out = {f: b[f] for f in FIELDS}
    flat = b["s"][: (k + GUARD) * 18 * n * n]
    out["s"] = flat.view(k + GUARD, n, n, 18).permute(0, 3, 1, 2) if fmt == "f16_nhwc" else flat.view(k + GUARD, 18, n, n)
    ld.extract(padded(torch, np.full(k, slot), slot), padded(torch, move_to, 0), padded(torch, d4, 0), out=out)
    return collect(torch, b, k)


def sweep_and_check(torch, elf, port, ld, slot, record, nfa, fmt, ctx=""):
    nm = record["result"]["num_move"]
    mt, d4 = sweep_args(nm, nfa)
    want = oracle_rows(port, record, mt, d4, nfa)
    got = loader_extract(torch, ld, slot, mt, d4, fmt)
    assert_rows_equal(got, want, ctx)
    return got, want, mt, d4


def abi_extract(torch, elf, ld, rec, move_to, d4, nfa, fmt, null=(), stride=None, base_off=0, n_launch=None):
    """elftrain_extract through the C ABI: optional outputs in `null` are passed as NULL, d4 = None passes NULL"""
    from elf_amd.train import TrainBatch
    L = elf.lib()
    k = len(rec)
    b = alloc(torch, ld.n, k + GUARD, nfa, fmt, stride, base_off)
    esz = 2 if fmt == "f16_nhwc" else 4
    ptr = {f: (None if f in null else b[f].data_ptr()) for f in FIELDS}
    tb = TrainBatch(b["s"].data_ptr() + base_off * esz, stride or 18 * ld.n * ld.n, 1 if fmt == "f16_nhwc" else 0, nfa, ptr["offline_a"],
                    ptr["winner"], ptr["mcts_scores"], ptr["predicted_value"], ptr["move_idx"], ptr["num_move"], ptr["aug_code"],
                    ptr["selfplay_ver"])
    r_t, m_t = padded(torch, rec, rec[0] if k else 0), padded(torch, move_to, 0)
    d_t = None if d4 is None else padded(torch, d4, 0)
    rc = L.elftrain_extract(ld._h, C.c_void_p(r_t.data_ptr()), C.c_void_p(m_t.data_ptr()), C.c_void_p(d_t.data_ptr()) if d_t is not None else None,
                            k if n_launch is None else n_launch, C.byref(tb), ld._stream())
    assert rc == 0
    return collect(torch, b, k if n_launch is None else n_launch, null)


# ---- A. every move_to of long records ---------------------------------------------------------------------------------------
def records_a(elf, name):
    if name == "19_golden508":
        return 19, golden19(508)          # the longest fixture record: values for every ply, no recorded policy (one-hot rows)
    if name == "19_golden471":
        return 19, golden19(471)          # a real quantised policy for every ply
    if name == "19_playout":
        return 19, playout19(elf)
    return 9, full9(elf)


@pytest.mark.parametrize("fmt", ["f32_nchw", "f16_nhwc"])
@pytest.mark.parametrize("name,keep", [("19_golden508", False), ("19_golden471", False), ("19_playout", False), ("9_full", False), ("9_full", True)])
def test_every_move_to_of_long_records(elf, name, keep, fmt):
    import torch
    n, record = records_a(elf, name)
    res = record["result"]
    nm = res["num_move"]
    if name == "19_golden508":
        assert nm == 508 and len(res["values"]) == 508
    if name == "19_golden471":
        assert len(res["policies"]) == nm == 471
    port = Port(n)
    for nfa in (1, 3):
        mt, d4 = sweep_args(nm, nfa)
        assert mt[0] == 0 and mt[-1] == nm - nfa and {0, 1, CK - 1} <= set((mt % CK).tolist()) and set(d4.tolist()) == set(range(8))
        ld = elf.ReplayLoader(board_size=n, capacity=2, batchsize=len(mt) + GUARD, num_future_actions=nfa, feature_format=fmt, keep_states=keep)
        if name == "9_full":
            assert ld.max_moves == nm == 162
            if nfa == 1:      # the last checkpoint, move_to // 16 == nck: plies 160 and 161 (nfa = 3 ends at 159, below it)
                assert (mt // CK == ld.max_moves // CK).sum() == 2
        ld.put(1, record)
        got, want, mt, d4 = sweep_and_check(torch, elf, port, ld, 1, record, nfa, fmt, (name, nfa))
        cross_check(port, record, want, mt, d4, nfa)
        if keep:
            info = ld.engine.info(n=len(mt)).cpu().numpy()
            assert np.array_equal(info[:, 0], got["move_idx"] + 1)
        ld.close()


# ---- B. superko across a checkpoint -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32_nchw", "f16_nhwc"])
@pytest.mark.parametrize("f", [6, 8, 10])
def test_superko_across_a_checkpoint(elf, f, fmt):
    """f = 6: the checkpoint after move 16 stores a terminated state; f = 8: the recapture (index 16) is the first move forwarded
    from it and repeats a position recorded before it; f = 10: the repeated position is the one the checkpoint stores."""
    import torch
    record, recap = superko19(elf, f)
    assert recap == {6: 14, 8: 16, 10: 18}[f]
    port = Port(19)
    nm = record["result"]["num_move"]
    ld = elf.ReplayLoader(board_size=19, capacity=2, batchsize=nm + GUARD, num_future_actions=1, feature_format=fmt)
    ld.put(1, record)
    got, want, mt, d4 = sweep_and_check(torch, elf, port, ld, 1, record, 1, fmt, ("superko", f))
    cross_check(port, record, want, mt, d4, 1)
    # move_idx = ply - 1 grows with move_to up to the recapture and stands from there on: every later move is refused
    assert np.array_equal(got["move_idx"], np.minimum(mt, recap + 1))
    ld.close()


# ---- C. store geometry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [15, 16, 17, 40])
def test_store_geometry_and_move_to_clamp(elf, m):
    """max_moves below the checkpoint interval (no checkpoint buffer), equal to it, and with a partial interval at the end; a record
    of exactly max_moves moves and a shorter one; move_to >= num_moves is taken as num_moves."""
    import torch
    port = Port(9)
    long, short = part9(elf, 3, m), part9(elf, 5, m - 8)
    for fmt, nfa in (("f32_nchw", 1), ("f16_nhwc", 3)):
        ld = elf.ReplayLoader(board_size=9, capacity=2, batchsize=m + 8, max_moves=m, num_future_actions=nfa, feature_format=fmt)
        assert ld.L.elftrain_max_moves(ld._h) == m
        ld.put(0, long)
        ld.put(1, short)
        sweep_and_check(torch, elf, port, ld, 0, long, nfa, fmt, ("long", m))
        _, want, mt, d4 = sweep_and_check(torch, elf, port, ld, 1, short, nfa, fmt, ("short", m))
        cross_check(port, short, want, mt, d4, nfa)
        # the clamp: move_to = num_moves and num_moves + 5 (still inside the store's own row: zeroed moves, read as passes, if the
        # clamp were missing) both give the row of the fully replayed game
        nm = m - 8
        mv = sgfstr2coords(9, short["result"]["content"])
        st = port.new()
        assert all(port.forward(st, int(c)) == 1 for c in mv) and nm + 5 <= m
        d4c = np.array([5, 2], np.int32)
        got = loader_extract(torch, ld, 1, np.array([nm, nm + 5], np.int32), d4c, fmt)
        for i in range(2):
            assert np.array_equal(got["s"][i], port.extract_agz(st, int(d4c[i])))
        port.free(st)
        assert (got["move_idx"] == nm).all() and (got["num_move"] == nm).all() and (got["offline_a"] == 0).all()
        assert (got["mcts_scores"].view(np.uint32) == 0).all() and (got["predicted_value"].view(np.uint32) == 0).all()
        assert_rows_equal(got, oracle_rows(port, short, [nm, nm + 5], d4c, nfa), ("clamp", m))
        ld.close()


# ---- D. slot reuse and the dirty list ---------------------------------------------------------------------------------------
def test_slot_reuse_long_short_long(elf):
    """A slot that held a long game and then holds a short, different one (stale checkpoints and superko records behind it), and
    back; two puts into one slot with no extraction in between."""
    import torch
    port = Port(9)
    a, b = full9(elf), part9(elf, 7, 45)
    assert b["result"]["num_move"] % CK != 0 and b["result"]["num_move"] < a["result"]["num_move"]
    ld = elf.ReplayLoader(board_size=9, capacity=4, batchsize=162 + GUARD, num_future_actions=1)
    ld.put(1, a)
    sweep_and_check(torch, elf, port, ld, 1, a, 1, "f32_nchw", "A")
    ld.put(1, b)
    sweep_and_check(torch, elf, port, ld, 1, b, 1, "f32_nchw", "B over A")
    ld.put(1, a)
    sweep_and_check(torch, elf, port, ld, 1, a, 1, "f32_nchw", "A over B")
    ld.put(1, b)
    sweep_and_check(torch, elf, port, ld, 1, b, 1, "f32_nchw", "B again")
    ld.put(1, b)
    ld.put(1, a)
    sweep_and_check(torch, elf, port, ld, 1, a, 1, "f32_nchw", "B then A, one extraction")
    assert len(ld) == 1
    ld.close()


def test_records_put_in_keep_mode_get_their_checkpoints_after_the_switch(elf):
    """Records put (and sampled) while keep_states is on stay on the dirty list: after elftrain_set_keep_states(h, 0) the next
    extraction writes their checkpoints.  The same for a record put during a later keep phase."""
    import torch
    L = elf.lib()
    port = Port(9)
    r1, r2, r3 = full9(elf), part9(elf, 7, 45), part9(elf, 2, 100)
    ld = elf.ReplayLoader(board_size=9, capacity=4, batchsize=162 + GUARD, num_future_actions=1, keep_states=True)
    ld.put(1, r1)
    ld.put(2, r2)
    for slot, r in ((1, r1), (2, r2)):
        mt, d4 = np.array([0, 17, 33, 44], np.int32), np.array([1, 6, 3, 4], np.int32)
        assert_rows_equal(loader_extract(torch, ld, slot, mt, d4, "f32_nchw"), oracle_rows(port, r, mt, d4, 1), ("keep", slot))
    assert L.elftrain_set_keep_states(ld._h, 0) == 0
    sweep_and_check(torch, elf, port, ld, 1, r1, 1, "f32_nchw", "r1 after the switch")
    sweep_and_check(torch, elf, port, ld, 2, r2, 1, "f32_nchw", "r2 after the switch")
    assert L.elftrain_set_keep_states(ld._h, 1) == 0
    ld.put(3, r3)
    mt, d4 = np.array([16, 99], np.int32), np.array([7, 2], np.int32)
    assert_rows_equal(loader_extract(torch, ld, 3, mt, d4, "f32_nchw"), oracle_rows(port, r3, mt, d4, 1), "keep r3")
    assert L.elftrain_set_keep_states(ld._h, 0) == 0
    sweep_and_check(torch, elf, port, ld, 3, r3, 1, "f32_nchw", "r3 after the second switch")
    sweep_and_check(torch, elf, port, ld, 1, r1, 1, "f32_nchw", "r1 untouched")
    ld.close()


# ---- E. launch shape and optional outputs -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(elf):
    """one 9x9 checkpointed store with two records, shared by the launch-shape tests (they only read it)"""
    ld = elf.ReplayLoader(board_size=9, capacity=3, batchsize=64, num_future_actions=2)
    recs = {1: part9(elf, 2, 100), 2: part9(elf, 7, 45)}
    for slot, r in recs.items():
        ld.put(slot, r)
    yield ld, recs
    ld.close()


def small_samples(k):
    rec = np.array([1 + i % 2 for i in range(k)], np.int32)
    mt = np.array([(0, 16, 43, 31, 98, 15, 32)[i % 7] for i in range(k)], np.int32)
    d4 = np.array([(i * 3 + 1) % 8 for i in range(k)], np.int32)
    return rec, mt, d4


def small_want(recs, rec, mt, d4, nfa):
    port = Port(9)
    rows = [oracle_rows(port, recs[int(r)], [int(m)], [int(d)], nfa) for r, m, d in zip(rec, mt, d4)]
    return {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}


@pytest.mark.parametrize("k", [1, 2, 3, 5, 7])
def test_partial_workgroups_leave_the_guard_rows(elf, small, k):
    import torch
    ld, recs = small
    rec, mt, d4 = small_samples(k)
    for fmt in ("f32_nchw", "f16_nhwc"):
        got = abi_extract(torch, elf, ld, rec, mt, d4, 2, fmt)          # collect() asserts the guard rows
        assert_rows_equal(got, small_want(recs, rec, mt, d4, 2), (k, fmt))


@pytest.mark.parametrize("null", [(f,) for f in FIELDS] + [FIELDS], ids=lambda t: "all" if len(t) > 1 else t[0])
def test_null_outputs(elf, small, null):
    import torch
    ld, recs = small
    rec, mt, d4 = small_samples(6)
    got = abi_extract(torch, elf, ld, rec, mt, d4, 2, "f32_nchw", null=null)
    assert set(got) == {"s"} | (set(FIELDS) - set(null))
    assert_rows_equal(got, small_want(recs, rec, mt, d4, 2), null)


def test_null_d4_is_code_zero(elf, small):
    import torch
    ld, recs = small
    rec, mt, _ = small_samples(6)
    got = abi_extract(torch, elf, ld, rec, mt, None, 2, "f32_nchw")
    assert_rows_equal(got, small_want(recs, rec, mt, np.zeros(6, np.int32), 2), "d4 NULL")
    assert (got["aug_code"] == 0).all()


@pytest.mark.parametrize("fmt,pad", [("f32_nchw", 5), ("f16_nhwc", 3)])
def test_padded_row_stride(elf, small, fmt, pad):
    """rows s_stride > 18 * 81 elements apart at the weakest alignment extract_agz_row takes (tests/test_gpu_board.py
    test_feature_row_formats_and_alignment; go_board.cuh agz_store / extract_agz_row): element alignment only -- the base one element
    past a 16-byte boundary and an odd stride, so fp32 rows start at every 4-byte offset of a 16-byte line and fp16 rows alternate
    between 4-byte aligned starts (fast path) and odd 2-byte starts (staged path).  The padding keeps its sentinel."""
    import torch
    ld, recs = small
    rec, mt, d4 = small_samples(9)
    got = abi_extract(torch, elf, ld, rec, mt, d4, 2, fmt, stride=18 * 81 + pad, base_off=1)
    assert_rows_equal(got, small_want(recs, rec, mt, d4, 2), fmt)


def test_empty_launch_writes_nothing(elf, small):
    import torch
    ld, recs = small
    rec, mt, d4 = small_samples(3)
    got = abi_extract(torch, elf, ld, rec, mt, d4, 2, "f32_nchw", n_launch=0)      # rc == 0 and every buffer keeps its sentinel
    assert got["s"].shape[0] == 0
