"""GPU: positional superko INSIDE the search tree.  k_mcts_leafstate rebuilds the record map the reference copies into every tree
node (go_state.h:117-124) from three sources that share no code with the board engine's own rule -- the game's Bloom words plus the
path hashes of the descent, an all-ones filter below MCTS_PATH_LV = 64 levels, and TreeSK::exact_hit's walk over the ancestors and
then the game's records up to root_sk_len -- and a node that repeats a position is terminal with value +-1 by the side to move
(go_state.h:194-203), never a net leaf.

The searches here are walked down two games that end on a repetition by a scripted net (tests/superko_lines.py); the expectations
are a closed form derived by hand there and the live checker (the compiled reference stack where oracle/_ref is built, its CPU
restatement otherwise), both confirmed on the CPU by tests/test_superko_lines_cpu.py.  The roots t = 75, 74, 73, 72, 68 with 24
rollouts (and the colours swapped) run as engine-agnostic cases of tests/mcts_known_answers.py in tests/test_gpu_mcts.py."""
import numpy as np
import pytest

import superko_lines as sl
from sp_drive import sp_from_fixture_cfg

pytestmark = pytest.mark.gpu

G9 = sl.SUPERKO_GAME


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def gpu_searches(elf, n, preload, move_to, cfg, net, total, analysis=None, on_step=None):
    """elf.SelfPlay under cfg (pyoracle.MCTS_DEFAULTS keys) after preloading, the net served through begin_step / end_step until
    `total` searches are logged -> ({game: [search rows]}, last analysis or None)"""
    import torch
    sp = sp_from_fixture_cfg(elf, n, cfg, log_searches=total, nodes_per_game=4096)
    try:
        if analysis:
            sp.set_analysis(*analysis)
        sp.preload(np.asarray(preload, np.uint16), move_to)
        while sp.stats()["logged"] < total:
            rows = sp.begin_step()
            if rows:
                pi, v = net(sp.s[:rows].cpu().numpy())
                sp.end_step(torch.from_numpy(pi).to(sp.device), torch.from_numpy(v).to(sp.device))
            else:
                sp.end_step(None, None)
            if on_step:
                on_step(sp)
        rec, coord, visits, prior, reward = sp.search_log()
        got = sl._rows(dict(search=rec[:total], coord=coord, visits=visits, prior=prior, reward=reward), cfg["num_games"])
        return got, (sp.last_analysis() if analysis else None)
    finally:
        sp.close()


def line_edge(s, game, t):
    """(visits, reward, visits on every other edge) of the root edge game[t] in a search row"""
    i = {int(c): i for i, c in enumerate(s["coord"])}[int(game[t])]
    return int(s["visits"][i]), np.float32(s["reward"][i]), int(s["visits"].sum()) - int(s["visits"][i])


def assert_closed_form(s, game, t, R, net):
    want_n, want_r = sl.expected_line_edge(t, R, len(game) - 1)
    n, r, others = line_edge(s, game, t)
    print("root after move %d, %d rollouts: edge %d visits %d reward %r (closed form %d, %r), other edges %d visits, net rows %d"
          % (t, R, game[t], n, float(r), want_n, float(want_r), others, len(net.seen)))
    assert n == want_n and r.view(np.uint32) == want_r.view(np.uint32), (t, n, r, want_n, want_r)
    assert others == 0                                                 # every other root edge unvisited
    assert not s["reward"][s["visits"] == 0].any()
    assert len(net.seen) == sl.line_rows(t, len(game) - 1), len(net.seen)     # the repeated position never reached the net
    assert s["best_action"] == int(game[t])


# ---- deep lines across MCTS_PATH_LV ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,depth", [(12, 64), (11, 65), (8, 68)])
def test_deep_line_across_the_path_row(elf, t, depth):
    """The terminal at depth 64 (the last depth the path's Bloom row serves), 65 (the first on the all-ones filter, where every probe
    goes to the exact check) and 68 (a walk over 67 ancestors): 100 rollouts, one per batch, against the closed form.  A false exact
    hit anywhere on the way down shows as an early +-1 in the reward and as fewer net rows; a miss at the end as a 0.125 (or a 0 and
    a subtree) where +1 belongs."""
    assert len(G9) - t == depth
    net = sl.line_net(9, [], G9, t)
    got, _ = gpu_searches(elf, 9, G9, t, sl.search_cfg(100, 1), net, 1)
    assert_closed_form(got[0][0], G9, t, 100, net)


# ---- live differentials ----------------------------------------------------------------------------------------------------------
def run_live(elf, name):
    n, game, t, cfg, per_game = sl.live_case(name)
    want = sl.run_checker(name)
    sl.assert_repetition_reached(want, name)       # on the checker's own answer
    net = sl.line_net(n, [], game, t)
    got, _ = gpu_searches(elf, n, game, t, cfg, net, cfg["num_games"] * per_game)
    for g in want:
        print("%s game %d: line edge (visits, reward, others) %s" % (name, g, [line_edge(s, game, t + k) for k, s in
                                                                              enumerate(got[g][:len(game) - t])]))
    sl.assert_same_searches(got, want, name)
    return got, net


@pytest.mark.parametrize("name", [k for k in sl.LIVE if not k.startswith("19_")])
def test_live_differential_on_the_line(elf, name):
    """Every root statistic of every search, bit for bit, against the live checker (superko_lines.LIVE): a 68-deep line in batches of
    8; the repetition below an interior node in batches of 4 and 16, with two search threads, and in three games of one context;
    and a game that plays the last six moves itself and ends on the repetition, with the persistent tree (the terminal node found
    by the first search survives every treeAdvance while the repeated position migrates from ancestor to root to game record) and
    with fresh trees (every search finds it again in the records)."""
    run_live(elf, name)


# ---- 19x19 -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def game19_ends_on_the_repetition(built):
    """the checker's board engine ends the 19x19 game after move 12 and nowhere before, with value +1"""
    from pyoracle import Port, Ref
    E = Ref(19) if Ref.available(19) else Port(19)
    s = E.new()
    for c in sl.SUPERKO_GAME_19:
        assert not E.terminated(s) and E.forward(s, int(c)) == 1
    assert E.terminated(s) and E.evaluate(s, 7.5) == 1.0
    E.free(s)
    return True


@pytest.mark.parametrize("name", ["19_t11", "19_t10", "19_t9", "19_t7"])
def test_19x19_repetition(elf, game19_ends_on_the_repetition, name):
    """Geo<19>: 6 bitboard words per colour, 13-word records -- the `lane < G::R` compares and the record layout differ from 9x9.
    The repeated position is the newest game record but one (root after move 11), the newest (10), the root (9), an interior
    node (7); 24 rollouts, one per batch, against the closed form AND the live checker."""
    n, game, t, cfg, _ = sl.live_case(name)
    want = sl.run_checker(name)
    sl.assert_repetition_reached(want, name)
    net = sl.line_net(n, [], game, t)
    got, _ = gpu_searches(elf, n, game, t, cfg, net, 1)
    assert_closed_form(got[0][0], game, t, cfg["rollouts_per_thread"], net)
    sl.assert_same_searches(got, want, name)


# ---- tree shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [75, 74, 73, 72, 68])
def test_nothing_grows_below_the_terminal_node(elf, t):
    """The first candidate's principal variation is exactly the rest of the game and stops on the terminal node; the node records'
    invariants hold after every step; and once every descent ends on the terminal node (batch 76 - t + 2 at the latest, of 24) the
    tree stops growing: the node count does not rise over the last ten batches."""
    net = sl.line_net(9, [], G9, t)
    live, bad = [], []

    def watch(sp):
        bad.append(sp.validate_trees())
        live.append(int(sp.count_live()[0]))

    got, an = gpu_searches(elf, 9, G9, t, sl.search_cfg(24, 1), net, 1, analysis=(4, 16), on_step=watch)
    print("root after move %d: live nodes per step %s, pv %s" % (t, live, an["pv"][0, 0, :an["pv_len"][0, 0]].tolist()))
    assert all(b[0] == 0 for b in bad), bad
    assert len(live) == 24                                       # one batch per step
    assert int(an["pv_len"][0, 0]) == len(G9) - t
    assert an["pv"][0, 0, :len(G9) - t].tolist() == G9[t:] and (an["pv"][0, 0, len(G9) - t:] == -1).all()
    assert int(an["coord"][0, 0]) == G9[t] and int(an["visits"][0, 0]) == 23
    assert all(b <= a for a, b in zip(live[-11:-1], live[-10:])), live
    assert live[-11] > live[0]                                   # it did grow while the line was being built
    assert_closed_form(got[0][0], G9, t, 24, net)
