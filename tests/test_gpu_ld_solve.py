"""GPU: elfgo_ld_solve / GoEngine.ld_solve / GTP elf-ld_solve against a plain minimax with no pruning over the reference's own
board functions (region_expected: FindAllCandidateMovesInRegion, bare-board play, OneGroupLives, the stones in the box), on the
straight three, a simple ko, a position whose side to move has no move in the box, and late positions of seeded playouts."""
import numpy as np
import pytest

import ladder_positions as LP
import ownership_expected as OE
import region_expected as RE

pytestmark = pytest.mark.gpu

M_PASS, THRES = 0, RE.S3_THRES


def minimax(rg, h, box, attacker, depth, thres=THRES):
    """the semantics of include/elf_amd.h, literally -> (info [8], value [NP + 1], nodes [NP + 1]) of Board handle h"""
    RB, NP = rg.RB, rg.n * rg.n
    bx, att, dfn = rg.frame(h, box, attacker)
    inb = rg.inbox(bx)

    def verdict(b):
        if rg.lf.one_group_lives(b, dfn, bx):
            return 2
        return 1 if ((RB.board(b)[0] == dfn) & inb).any() else 0

    def children(b):
        for c in rg.cand_in(b, bx, int(RB.info(b)[1]), thres) or [M_PASS]:
            ch = RB.clone(b)
            assert RB.play(ch, c) == 1
            yield c, ch
            RB.free(ch)

    def node(b, d, passes):
        v = verdict(b)
        if v != 1 or d == depth or passes == 2:
            return v, 1
        got = [node(ch, d + 1, passes + 1 if c == M_PASS else 0) for c, ch in children(b)]
        return (max if int(RB.info(b)[1]) == dfn else min)(g[0] for g in got), 1 + sum(g[1] for g in got)

    v0 = verdict(h)
    info = np.array(list(bx) + [att, dfn, int(RB.info(h)[1]), v0], np.int32)
    value, nodes = np.full(NP + 1, -1, np.int8), np.zeros(NP + 1, np.int32)
    if v0 == 1 and depth > 0:
        for c, ch in children(h):
            a = NP if c == M_PASS else rg.action[c]
            value[a], nodes[a] = node(ch, 1, 1 if c == M_PASS else 0)
    return info, value, nodes


def rows_of(n):
    """-> list of dict(src, box, att, depth, ...): move-list rows first (they are played into slots 0 ..), set-up rows after"""
    rg = RE.reg(n)
    s3 = [dict(r, att=0, depth=5) for r in RE.s3_rows(n)]
    moves, _, k = LP.ko_cases(n)   # the last move of the list takes the ko: asked before it (the ban comes up at depth 2) and after
    kx, ky = k // n, k % n
    kbox = (max(kx - 1, 0), max(ky - 2, 0), min(kx + 2, n), min(ky + 2, n))
    ko = [dict(src=[int(c) for c in mv], box=kbox, att=0, depth=3) for mv in (moves[:-1], moves)]
    late = []
    for r in RE.ld_rows(n)[:8]:    # late positions of the seeded playouts, each with the largest corner box that holds 2 .. 8 candidates
        h = LP.play_list(rg.RB, r["moves"])
        fit = [s for s in range(7, 1, -1) if 2 <= len(rg.cand_in(h, (0, 0, s, s), int(rg.RB.info(h)[1]), THRES)) <= 8]
        if fit and len(late) < 4:
            late.append(dict(src=r["moves"], box=(0, 0, fit[0], fit[0]), att=0, depth=3))
        rg.RB.free(h)
    # a 1x1 box on a Black stone of the straight three: nobody has a move in it, so pass, pass and the static verdict
    nomove = dict(src=dict(stones=RE.straight_three(n), mover=1), box=(3, 0, 4, 1), att=2, depth=3)
    return s3[:2] + ko + late + s3[2:] + [nomove]


@pytest.fixture(scope="module", params=[9, 19])
def solved(built, request):
    """the engine with every row in its slot, the rows, and the reference's answer per row (computed once)"""
    import elf_amd
    n = request.param
    rg, rows = RE.reg(n), rows_of(n)
    nl = sum(isinstance(r["src"], list) for r in rows)
    eng = elf_amd.GoEngine(n, len(rows))
    OE.play_all(eng, [r["src"] for r in rows[:nl]])
    ok = eng.setup(np.array([r["src"]["stones"] for r in rows[nl:]]), ids=list(range(nl, len(rows))),
                   next_player=[r["src"]["mover"] for r in rows[nl:]])
    assert (ok.cpu().numpy() == 1).all()
    want = []
    for r in rows:
        h = LP.play_list(rg.RB, r["src"]) if isinstance(r["src"], list) else LP.build(rg.RB, r["src"]["stones"], r["src"]["mover"])
        want.append(minimax(rg, h, r["box"], r["att"], r["depth"]))
        rg.RB.free(h)
    assert sum(int(w[2].sum()) for w in want) <= 20000, "the reference search is sized to stay small"
    yield n, eng, rows, want
    eng.close()


def call(eng, rows, sel, depth, **kw):
    return eng.ld_solve(ids=sel, regions=[rows[j]["box"] for j in sel], attackers=[rows[j]["att"] for j in sel], max_depth=depth,
                        self_atari_thres=THRES, **kw)


def test_values_equal_plain_minimax(solved):
    n, eng, rows, want = solved
    NP = n * n
    for depth in sorted({r["depth"] for r in rows}):
        sel = [j for j, r in enumerate(rows) if r["depth"] == depth]
        sol = call(eng, rows, sel, depth)
        info, value, nodes = sol.info.cpu().numpy(), sol.value.cpu().numpy(), sol.nodes.cpu().numpy()
        for i, j in enumerate(sel):
            w_info, w_value, w_nodes = want[j]
            assert (info[i] == w_info).all() and (value[i] == w_value).all(), (j, info[i], w_info, value[i], w_value)
            assert ((nodes[i] >= (w_value >= 0)) & (nodes[i] <= w_nodes)).all(), (j, nodes[i], w_nodes)
        # known answers, on the reference first: the vital point of the straight three
        for i, j in enumerate(sel):
            r = rows[j]
            if "vital" not in r:
                continue
            for val, root, best in ((want[j][1], None, None), (value[i], sol.root_value()[i], sol.best_move()[i])):
                others = [a for a in range(NP + 1) if val[a] >= 0 and a != r["vital"]]
                if r["defends"]:
                    assert val[r["vital"]] == 2 and all(val[a] < 2 for a in others), (j, val)
                    assert root in (None, 2) and best in (None, r["vital"])
                else:
                    assert val[r["vital"]] < 2 and all(val[a] == 2 for a in others), (j, val)
            assert sol.proved()[i] == (sol.root_value()[i] in (0, 2))
    # the ko is banned where it was just taken, and the side with no move in the box passes twice
    ko_after, nomove = [j for j, r in enumerate(rows) if "vital" not in r and isinstance(r["src"], list)][1], len(rows) - 1
    assert want[ko_after][1][LP.ko_cases(n)[2]] == -1
    assert (np.nonzero(want[nomove][1] >= 0)[0] == [NP]).all() and want[nomove][2][NP] == 2


def test_edges(solved):
    n, eng, rows, want = solved
    NP = n * n
    sel = [j for j, r in enumerate(rows) if r["depth"] == 5]
    ref = call(eng, rows, sel, 5)
    value, nodes, info = ref.value.cpu().numpy(), ref.nodes.cpu().numpy(), ref.info.cpu().numpy()
    # max_depth = 0: the static verdict, nothing searched
    s0 = call(eng, rows, sel, 0)
    assert (s0.value.cpu().numpy() == -1).all() and (s0.nodes.cpu().numpy() == 0).all() and (s0.info.cpu().numpy() == info).all()
    assert s0.root_value() == [int(v) for v in info[:, 7]] and s0.best_move() == [None] * len(sel)
    # max_nodes = 1: every first move with children is cut, the others keep their value; the call returns
    s1 = call(eng, rows, sel, 5, max_nodes=1)
    v1 = s1.value.cpu().numpy()
    assert ((v1 == -2) == (nodes > 1)).all() and (v1[nodes <= 1] == value[nodes <= 1]).all() and (nodes > 1).any()
    assert (s1.nodes.cpu().numpy() == np.minimum(nodes, 1)).all() and None in s1.root_value()
    # a slot id outside the pool, a slot named twice, the rows permuted, a second call
    ids = [sel[0], len(rows) + 5, sel[0], -1] + sel[::-1]
    boxes = [rows[sel[0]]["box"]] * 4 + [rows[j]["box"] for j in sel[::-1]]
    for _ in range(2):
        s2 = eng.ld_solve(ids=ids, regions=boxes, max_depth=5, self_atari_thres=THRES)
        v2, n2, i2 = s2.value.cpu().numpy(), s2.nodes.cpu().numpy(), s2.info.cpu().numpy()
        for bad in (1, 3):
            assert (i2[bad] == 0).all() and (v2[bad] == -1).all() and (n2[bad] == 0).all()
        assert (v2[0] == v2[2]).all() and (n2[0] == n2[2]).all() and (i2[0] == i2[2]).all() and (v2[0] == value[0]).all()
        assert (v2[4:] == value[::-1]).all() and (n2[4:] == nodes[::-1]).all() and (i2[4:] == info[::-1]).all()
    # regions=None: the bounding box, ld_read's
    rd = eng.ld_read(np.ones(len(sel), np.uint64), sel, playouts=1)
    assert (eng.ld_solve(ids=sel, max_depth=1).info.cpu().numpy()[:, :6] == rd.info.cpu().numpy()[:, :6]).all()
    # bad arguments are refused by the library: nothing is launched, the outputs keep their bytes
    import ctypes as C
    deep, out = eng.ld_solve_max_depth(), ref.value.clone()
    p = C.c_void_p(out.data_ptr())
    for k, vp, depth, budget in ((0, p, 5, 16), (len(rows) + 1, p, 5, 16), (1, None, 5, 16), (1, p, -1, 16), (1, p, deep + 1, 16), (1, p, 5, 0)):
        assert eng.L.elfgo_ld_solve(eng._h, None, k, None, None, depth, budget, THRES, None, vp, None, None) == -1
    eng.sync()
    assert (out.cpu().numpy() == value).all()
    with pytest.raises(Exception):
        eng.ld_solve(ids=sel, max_depth=deep + 1)


def test_gtp(built):
    import torch
    from elf_amd.gtp import GtpEngine
    n = 9

    def actor(batch):
        b = batch["s"].shape[0]
        return dict(pi=torch.full((b, n * n + 1), 1.0 / (n * n + 1), device="cuda"), V=torch.zeros(b, device="cuda"))

    eng = GtpEngine(actor, board_size=n, mcts_rollout_per_thread=16, nodes_per_game=1024)
    assert "elf-ld_solve" in eng.command("list_commands").split()
    eng.sp.setup(RE.straight_three(n), [0], 1)
    lines = eng.command("elf-ld_solve A1 E3 5").split("\n")
    assert lines[0] == "= attacker w defender b to_move b status alive best B1", lines
    assert [ln.split()[:2] for ln in lines[1:4]] == [["A1", "dead"], ["B1", "alive"], ["C1", "dead"]], lines
    eng.sp.restart([0])
    eng.sp.setup(RE.straight_three(n), [0], 2)
    assert eng.command("elf-ld_solve e3 a1 5").split("\n")[0] == "= attacker w defender b to_move w status unsettled best B1"
    assert eng.command("elf-ld_solve A1 K9").startswith("?") and eng.command("elf-ld_solve 99").startswith("?")
    eng.close()
