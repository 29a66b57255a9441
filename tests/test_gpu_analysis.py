"""GPU: search analysis (elfmcts_analyze, elfsp_analyze / set_analysis / last_analysis, GTP lz-genmove_analyze / elf-analysis).

Every expectation is computed at test time from entry points that existed before the feature -- elfmcts_root, elfmcts_advance,
elfsp_last_moves, the search log -- never from the code under test, and every comparison is exact (integers, float bits).
The searches are driven by the oracle's deterministic stub net (peaky priors, quantised values), without Dirichlet noise, with
the most-visited pick, policy_distri_cutoff 0 and resigning off; contexts are stopped mid-move (rollouts_per_thread larger than
what is run) so that the trees are what a search in progress holds."""
import ctypes as C
import io
import re

import numpy as np
import pytest

from pyoracle import stub_net

pytestmark = pytest.mark.gpu

M_PASS = 0
GUARD = 16                       # words after each output array that must keep the sentinel
SENT = 0x5A5A5A5A
FIELDS = ("info", "coord", "orig", "visits", "reward", "prior", "pv_len", "pv")
SALT = 7


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def make_sp(elf, n, games, **kw):
    opts = dict(board_size=n, num_games=games, mcts_rollout_per_thread=1 << 13, mcts_rollout_per_batch=16, mcts_puct=1.5,
                mcts_epsilon=0.0, mcts_alpha=0.0, policy_distri_cutoff=0, resign_thres=0.0, mcts_pick_method="most_visited",
                seed=11, nodes_per_game=4096)
    opts.update(kw)
    return elf.SelfPlay(**opts)


def run_steps(sp, k, salt=SALT):
    import torch
    for _ in range(k):
        rows = sp.begin_step()
        if not rows:
            sp.end_step(None, None)
            continue
        pi, v = stub_net(sp.n, sp.s[:rows].cpu().numpy(), salt)
        sp.end_step(torch.from_numpy(pi).to(sp.device), torch.from_numpy(v).to(sp.device))


def stub_actor(n, salt=SALT):
    import torch

    def actor(batch):
        s = batch["s"]
        pi, v = stub_net(n, s.cpu().numpy(), salt)
        return dict(pi=torch.from_numpy(pi).to(s.device), V=torch.from_numpy(v).to(s.device))
    return actor


def mcts_of(sp):
    return C.c_void_p(sp.L.elfsp_mcts(sp._h))


def root_of(sp):
    """elfmcts_root: the root's edges in the reference's iteration order"""
    import torch
    from elf_amd._lib import check
    G, NE = sp.num_games, sp.edge_stride
    i32 = dict(dtype=torch.int32, device=sp.device)
    f32 = dict(dtype=torch.float32, device=sp.device)
    t = dict(info=torch.zeros((G, 8), **i32), coord=torch.zeros((G, NE), **i32), visits=torch.zeros((G, NE), **i32),
             prior=torch.zeros((G, NE), **f32), reward=torch.zeros((G, NE), **f32), child=torch.zeros((G, NE), **i32))
    check(sp.L.elfmcts_root(mcts_of(sp), *(C.c_void_p(t[k].data_ptr()) for k in ("info", "coord", "visits", "prior", "reward", "child")),
                            sp._stream()))
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in t.items()}


def ranked(rt, g):
    """the visited root edges of game g by (visits descending, iteration index ascending): MOST_VISITED's order"""
    ne = int(rt["info"][g, 0])
    vis = rt["visits"][g, :ne]
    return sorted((i for i in range(ne) if vis[i] > 0), key=lambda i: (-int(vis[i]), i))


def analyze_raw(sp, mm, mp, drop=(), expect=0):
    """elfmcts_analyze on the raw handle into arrays followed by guard words; `drop` = outputs passed as NULL"""
    import torch
    G = sp.num_games
    size = dict(info=G * 8, coord=G * mm, orig=G * mm, visits=G * mm, reward=G * mm, prior=G * mm, pv_len=G * mm, pv=G * mm * mp)
    buf = {k: torch.full((max(size[k], 0) + GUARD,), SENT, dtype=torch.int32, device=sp.device) for k in FIELDS}
    rc = sp.L.elfmcts_analyze(mcts_of(sp), mm, mp, *(None if k in drop else C.c_void_p(buf[k].data_ptr()) for k in FIELDS), sp._stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    host = {k: b.cpu().numpy() for k, b in buf.items()}
    for k in FIELDS:
        assert (host[k][max(size[k], 0):] == SENT).all(), "guard words after %s were written" % k
        if k in drop or rc != 0:
            assert (host[k] == SENT).all(), "%s was written" % k
    if rc != 0:
        return None
    out = {k: host[k][:size[k]] for k in FIELDS if k not in drop}
    shape = dict(info=(G, 8), pv=(G, mm, mp))
    out = {k: a.reshape(shape.get(k, (G, mm))) for k, a in out.items()}
    for k in ("reward", "prior"):
        if k in out:
            out[k] = out[k].view(np.float32)
    return out


def check_against_root(an, rt, mm, mp, flip=None):
    """candidates == the ranked root edges, info == RootInfo, unused entries padded, PV heads and tails well-formed"""
    G = rt["info"].shape[0]
    counts = []
    for g in range(G):
        idx = ranked(rt, g)
        k = min(mm, len(idx))
        counts.append(len(idx))
        inf = an["info"][g]
        assert (int(inf[0]), int(inf[1])) == (k, len(idx)), (g, inf, len(idx))
        assert int(inf[2]) == int(rt["info"][g, 1])                      # num_visits
        assert int(inf[4]) == int(rt["info"][g, 4])                      # V bits
        assert int(inf[5]) == int(rt["info"][g, 6]) == 0                 # error bits
        assert int(inf[7]) == 0
        if flip is not None:
            assert int(inf[3]) == int(flip[g]), (g, inf[3], flip[g])
        top = idx[:k]
        assert an["orig"][g, :k].tolist() == top, (g, an["orig"][g], top)
        assert an["coord"][g, :k].tolist() == rt["coord"][g, top].tolist()
        assert an["visits"][g, :k].tolist() == rt["visits"][g, top].tolist()
        assert an["reward"][g, :k].view(np.uint32).tolist() == rt["reward"][g, top].view(np.uint32).tolist()
        assert an["prior"][g, :k].view(np.uint32).tolist() == rt["prior"][g, top].view(np.uint32).tolist()
        # unused entries
        assert (an["coord"][g, k:] == -1).all() and (an["orig"][g, k:] == -1).all() and (an["visits"][g, k:] == 0).all()
        assert (an["reward"][g, k:].view(np.uint32) == 0).all() and (an["prior"][g, k:].view(np.uint32) == 0).all()
        assert (an["pv_len"][g, k:] == 0).all() and (an["pv"][g, k:] == -1).all()
        # variations: own coord first, -1 after the end
        for j in range(k):
            ln = int(an["pv_len"][g, j])
            assert 1 <= ln <= mp and int(an["pv"][g, j, 0]) == int(an["coord"][g, j])
            assert (an["pv"][g, j, :ln] >= 0).all() and (an["pv"][g, j, ln:] == -1).all()
        assert int(inf[6]) == (int(an["pv_len"][g].max()) if k else 0)
    return counts


def root_flips(sp):
    be = sp.board_engine()
    try:
        return (be.info_host()["next_player"] == 2).astype(np.int32)
    finally:
        be.close()


# ---- 1. candidates equal the root -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,games,steps,puct", [(9, 8, 19, 1.5), (19, 4, 63, 2.5)])
def test_candidates_equal_the_root(elf, n, games, steps, puct):
    sp = make_sp(elf, n, games, mcts_puct=puct)
    try:
        flip = root_flips(sp)
        followed, counts_end = [], None
        for upto in (2, steps):                      # after the first batch below the root (small records) and at the end
            run_steps(sp, upto - (0 if upto == 2 else 2))
            rt = root_of(sp)
            followed.append((rt["child"] >= 0).sum(axis=1))
            for mm, mp in ((4, 16), (10, 16), (64, 5)):
                an = analyze_raw(sp, mm, mp)
                counts = check_against_root(an, rt, mm, mp, flip)
            counts_end = counts
            hi = sp.analyze(10, 16)                  # the Python surface returns the same arrays
            an = analyze_raw(sp, 10, 16)
            for k in FIELDS:
                assert np.array_equal(hi[k].view(np.int32), an[k].view(np.int32)), k
            assert hi["winrate"].shape == (games, 10)
        print("n=%d followed root edges after 2 steps %s, at the end %s; visited root edges %s" % (n, followed[0], followed[1], counts_end))
        assert (followed[0] <= 16).any() and (followed[0] >= 1).all()       # small records
        assert (followed[1] > 16).any()                                      # big records
        assert max(counts_end) > 4                                           # max_moves = 4 cut something off
        if n == 9:
            assert min(counts_end) < 64                                      # max_moves = 64 padded
        else:
            assert max(counts_end) > 64                                      # more than one scan round of the root's prefix
        assert sp.validate_trees()[0] == 0
    finally:
        sp.close()


# ---- 2 / 3. PV equals a walk with elfmcts_advance + elfmcts_root ------------------------------------------------------------------
def walk(sp, mm, mp):
    """After one elfmcts_analyze game g follows candidate g mod n_moves[g]: advance along the PV coord by coord and look at every
    new root with elfmcts_root.  Returns (the walked PVs, n_edges of the root each finished walk ended on or None).
    The trees are advanced behind the context's back: the context is good for nothing but close() afterwards."""
    import torch
    from elf_amd._lib import check
    G = sp.num_games
    an = analyze_raw(sp, mm, mp)
    check_against_root(an, root_of(sp), mm, mp)
    nm = an["info"][:, 0]
    assert (nm >= 1).all()
    pvs = [an["pv"][g, g % nm[g], :an["pv_len"][g, g % nm[g]]].tolist() for g in range(G)]
    end_edges = [None] * G
    mv_t = torch.zeros(G, dtype=torch.int32, device=sp.device)
    for d in range(mp):
        mv = np.array([pvs[g][d] if d < len(pvs[g]) else -1 for g in range(G)], np.int32)     # -1: this game does not move
        if (mv < 0).all():
            break
        mv_t.copy_(torch.from_numpy(mv))
        check(sp.L.elfmcts_advance(mcts_of(sp), C.c_void_p(mv_t.data_ptr()), sp._stream()))
        rt = root_of(sp)
        for g in range(G):
            if mv[g] < 0:
                continue
            assert int(rt["info"][g, 6]) == 0
            idx = ranked(rt, g)
            if d + 1 < len(pvs[g]):                  # the PV goes on: the new root's most-visited edge is its next coord
                assert idx and int(rt["visits"][g, idx[0]]) > 0, (g, d, pvs[g])
                assert int(rt["coord"][g, idx[0]]) == pvs[g][d + 1], (g, d, pvs[g], int(rt["coord"][g, idx[0]]))
            elif len(pvs[g]) < mp:                   # it stopped before max_pv: nothing visited below
                assert not idx, (g, d, pvs[g], idx)
                end_edges[g] = int(rt["info"][g, 0])
    return an, pvs, end_edges


@pytest.mark.parametrize("n,games,steps,puct", [(9, 8, 19, 1.5), (19, 4, 63, 2.5)])
def test_pv_equals_a_walk_with_advance_and_root(elf, n, games, steps, puct):
    sp = make_sp(elf, n, games, mcts_puct=puct)
    try:
        run_steps(sp, steps)
        an, pvs, _ = walk(sp, 10, 16)
        print("n=%d candidates %s, walked PV lengths %s" % (n, an["info"][:, 0].tolist(), [len(p) for p in pvs]))
        assert (an["info"][:, 0] >= 2).all()
        assert 2 * sum(len(p) >= 3 for p in pvs) >= games
        assert sp.validate_trees()[0] == 0
    finally:
        sp.close()


def test_a_terminal_node_ends_a_pv(elf):
    """Black has passed: White's pass at the root leads to a terminated position (a node with no edges), and it wins the empty
    board by komi, so a search that tries it once stays with it.  The input is chosen so that it is tried: without the random
    D4 transform the stub net sees the root as the oracle's extractor writes it, and under salt 1238 it gives the pass a prior
    of 0.17 there (the largest among salts 1 .. 1999; computed with pyoracle.Port + stub_net on the CPU)."""
    n, games, salt = 9, 8, 1238
    sp = make_sp(elf, n, games, ply_pass_enabled=0, remove_pass_if_dangerous=False, rotation_flip=False)
    try:
        sp.play([M_PASS] * games)
        run_steps(sp, 19, salt)
        an, pvs, end_edges = walk(sp, 10, 16)
        print("PVs %s end on roots with n_edges %s" % (pvs, end_edges))
        assert (an["info"][:, 3] == 1).all()         # White to move at the root
        assert any(e == 0 and p[-1] == M_PASS for p, e in zip(pvs, end_edges))
    finally:
        sp.close()


# ---- 4. read-only ------------------------------------------------------------------------------------------------------------------
def test_analyze_is_read_only(elf):
    n, games = 9, 8
    a, b = make_sp(elf, n, games), make_sp(elf, n, games)
    try:
        for _ in range(40):
            run_steps(a, 1)
            run_steps(b, 1)
            analyze_raw(b, 10, 16)
            b.analyze(64, 32)
        ra, rb = root_of(a), root_of(b)
        # node ids are internal: which big record a promoted node receives depends on the order in which the waves of a launch
        # reach the pool's atomic (mcts.cuh), so the root's id (info word 3) and the child ids are compared as "has a child"
        for r in (ra, rb):
            r["info"][:, 3] = 0
            r["child"] = (r["child"] >= 0).astype(np.int32)
        for k in ra:
            assert np.array_equal(ra[k].view(np.int32), rb[k].view(np.int32)), k
        assert (ra["child"].sum(axis=1) > 16).any()                       # roots that moved to big records are among them
        assert np.array_equal(a.count_live(), b.count_live()) and a.count_live().sum() > 40 * 8
        assert a.validate_trees()[0] == 0 and b.validate_trees()[0] == 0
        assert a.pool_info() == b.pool_info()
    finally:
        a.close()
        b.close()


# ---- 5. edges of the argument space ----------------------------------------------------------------------------------------------
def test_edges_of_the_argument_space(elf):
    n, games = 9, 8
    sp = make_sp(elf, n, games)
    try:
        # a fresh context: no candidates, padding everywhere
        for mm, mp in ((10, 16), (1, 1), (64, 32)):
            an = analyze_raw(sp, mm, mp)
            assert (an["info"][:, [0, 1, 2, 5, 6, 7]] == 0).all()
            assert (an["coord"] == -1).all() and (an["orig"] == -1).all() and (an["visits"] == 0).all() and (an["pv_len"] == 0).all()
            assert (an["reward"].view(np.uint32) == 0).all() and (an["prior"].view(np.uint32) == 0).all() and (an["pv"] == -1).all()
        # refused calls launch nothing: no output word changes
        for mm, mp in ((0, 16), (65, 16), (10, 0), (10, 33), (-1, -1)):
            assert analyze_raw(sp, mm, mp, expect=-1) is None
        assert analyze_raw(sp, 10, 16, drop=("info",), expect=-1) is None
        run_steps(sp, 19)
        rt = root_of(sp)
        # the best move only
        an = analyze_raw(sp, 1, 1)
        check_against_root(an, rt, 1, 1)
        for g in range(games):
            assert an["pv_len"][g, 0] == 1 and an["pv"][g, 0, 0] == an["coord"][g, 0] == rt["coord"][g, ranked(rt, g)[0]]
        # deeper than any line
        an = analyze_raw(sp, 10, 32)
        check_against_root(an, rt, 10, 32)
        assert 1 < an["pv_len"].max() < 32 and (an["pv"][:, :, -1] == -1).all()
        full = an
        # every optional pointer NULL in turn: the others are unchanged
        for d in FIELDS[1:]:
            an = analyze_raw(sp, 10, 32, drop=(d,))
            for k in FIELDS:
                if k != d:
                    assert np.array_equal(an[k].view(np.int32), full[k].view(np.int32)), (d, k)
        an = analyze_raw(sp, 10, 32, drop=FIELDS[1:])
        assert np.array_equal(an["info"], full["info"])
        # the self-play entry point: actor 0 is this pool, actor 1 does not exist in a self-play context
        info = np.zeros((games, 8), np.int32)
        import torch
        t = torch.zeros((games, 8), dtype=torch.int32, device=sp.device)
        nul = [None] * 7
        assert sp.L.elfsp_analyze(sp._h, 1, 10, 16, C.c_void_p(t.data_ptr()), *nul, None) == -1
        assert sp.L.elfsp_analyze(sp._h, 2, 10, 16, C.c_void_p(t.data_ptr()), *nul, None) == -1
        assert sp.L.elfsp_analyze(sp._h, 0, 10, 32, C.c_void_p(t.data_ptr()), *nul, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), full["info"]) and not info.any()
        assert sp.L.elfsp_set_analysis(sp._h, 65, 16) == -1 and sp.L.elfsp_set_analysis(sp._h, 8, 0) == -1
        assert sp.L.elfsp_set_analysis(sp._h, 0, 4) == -1
    finally:
        sp.close()


# ---- 6. the snapshot of the move boundary ---------------------------------------------------------------------------------------
def test_boundary_snapshot(elf):
    n, games, moves = 9, 4, 6
    kw = dict(mcts_rollout_per_thread=64, log_searches=64, ply_pass_enabled=60, nodes_per_game=2048)
    on, off, never = make_sp(elf, n, games, **kw), make_sp(elf, n, games, **kw), make_sp(elf, n, games, **kw)
    try:
        on.set_analysis(8, 12)
        off.set_analysis(8, 12)
        off.set_analysis(0, 0)
        la = on.last_analysis()
        assert la["coord"].shape == (games, 8) and la["pv"].shape == (games, 8, 12)
        assert (la["info"] == 0).all() and (la["coord"] == -1).all() and (la["pv"] == -1).all()       # no search has finished yet
        played = {id(s): [] for s in (on, off, never)}
        for mvno in range(moves):
            for s in (on, off, never):
                while s.stats()["moves"] < games * (mvno + 1):
                    run_steps(s, 1)
                played[id(s)].append(s.last_moves().copy())
            la = on.last_analysis()
            lm = on.last_moves()
            rec, coord, visits, prior, reward = on.search_log()
            assert len(rec) == games * (mvno + 1)
            assert (la["info"][:, 0] >= 1).all() and (la["info"][:, 5] == 0).all()
            assert la["coord"][:, 0].tolist() == lm.tolist()                       # rank 0 is the move the search played
            for j in range(len(rec) - games, len(rec)):
                g = rec[j].game
                assert rec[j].best_action == la["coord"][g, 0] == rec[j].move_played
                assert int(visits[j].max()) == int(la["visits"][g, 0]) and rec[j].total_visits == int(la["info"][g, 2])
                i = int(la["orig"][g, 0])
                assert int(coord[j, i]) == int(la["coord"][g, 0]) and int(visits[j, i]) == int(la["visits"][g, 0])
                assert reward[j, i:i + 1].view(np.uint32)[0] == la["reward"][g, 0:1].view(np.uint32)[0]
                assert prior[j, i:i + 1].view(np.uint32)[0] == la["prior"][g, 0:1].view(np.uint32)[0]
            # the move re-rooted the tree on the candidate's child: its most-visited edge is the PV's second coord
            rt = root_of(on)
            deep = 0
            for g in range(games):
                if la["pv_len"][g, 0] >= 2:
                    deep += 1
                    idx = ranked(rt, g)
                    assert idx and int(rt["coord"][g, idx[0]]) == int(la["pv"][g, 0, 1]), (mvno, g)
            assert deep >= 1
            lo = off.last_analysis()
            assert lo["coord"].shape == (games, 0) and (lo["info"] == 0).all()      # analysis off: no candidates
        # analysis changes nothing about play: the three contexts played the same moves and logged the same searches
        for s in (off, on):
            assert np.array_equal(np.array(played[id(s)]), np.array(played[id(never)]))
            ra, rn = s.search_log(), never.search_log()
            assert [bytes(r) for r in ra[0]] == [bytes(r) for r in rn[0]]
            for x, y in zip(ra[1:], rn[1:]):
                assert np.array_equal(x.view(np.int32), y.view(np.int32))
        assert on.validate_trees()[0] == 0
    finally:
        on.close()
        off.close()
        never.close()


# ---- 7. GTP ----------------------------------------------------------------------------------------------------------------------
INFO_RE = r"info move \S+ visits \d+ winrate \d+ prior \d+ order 0 pv \S+( \S+)*"


def test_gtp_genmove_analyze(elf):
    from elf_amd.gtp import GtpEngine
    n = 9
    kw = dict(board_size=n, mcts_rollout_per_thread=128, nodes_per_game=2048, ply_pass_enabled=60)
    eng, twin = GtpEngine(stub_actor(n), **kw), GtpEngine(stub_actor(n), **kw)
    try:
        lc = eng.command("list_commands").split()
        assert "lz-genmove_analyze" in lc and "elf-analysis" in lc and "genmove" in lc
        assert eng.command("known_command lz-genmove_analyze") == "= true\n\n"
        assert eng.command("elf-analysis") == "= \n\n"                             # no search has finished yet
        r = eng.command("lz-genmove_analyze b 10")
        assert r.startswith("= \n") and r.endswith("\n\n")
        lines = r[3:-2].split("\n")
        assert len(lines) >= 2 and all(re.fullmatch(INFO_RE, x) for x in lines[:-1]), r
        m = re.fullmatch(r"play (\S+)", lines[-1])
        assert m, r
        assert twin.command("genmove b") == "= %s\n\n" % m.group(1)
        assert re.match(r"info move %s " % re.escape(m.group(1)), lines[-2])      # the final line leads with the move played
        assert eng.command("elf-analysis") == "= %s\n\n" % lines[-2]
        assert eng.command("lz-genmove_analyze b").startswith("? Specified next player")
        # interval 0: a line after every step of the search, each well-formed; streamed by loop() as they come
        r = eng.command("lz-genmove_analyze w 0")
        lines = r[3:-2].split("\n")
        assert len(lines) >= 4 and all(re.fullmatch(INFO_RE, x) for x in lines[:-1]), r
        fout = io.StringIO()
        twin.loop(io.StringIO("lz-genmove_analyze w 0\nelf-analysis\n"), fout)
        assert fout.getvalue() == "=\n" + "\n".join(lines) + "\n\n" + "= %s\n\n" % lines[-2]
        assert eng.command("elf-analysis") == "= %s\n\n" % lines[-2]
        assert eng.command("genmove b").startswith("= ")                           # the plain command is as it was
    finally:
        eng.close()
        twin.close()
