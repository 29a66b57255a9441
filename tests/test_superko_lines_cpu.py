"""CPU: the inputs of tests/test_gpu_mcts_superko.py are known-good before a GPU is involved.  Every configuration of that file
(tests/superko_lines.py: the deep lines, the live differentials, the 19x19 game) runs on the CPU restatement of the search and --
where oracle/_ref is present -- on the reference's self-play stack; the two must agree bit for bit, equal the closed form where
there is one, and reach the repetition."""
import numpy as np
import pytest

import mcts_known_answers as mka
import superko_lines as sl
from pyoracle import Port, Ref, RefSelfPlay

DEEP = [(12, 100), (11, 100), (8, 100)]      # terminal at depth 64, 65, 68


def need_ref(ok):
    if not ok:
        pytest.skip("oracle/_ref is not built: make -C oracle ref")


@pytest.mark.parametrize("n", [9, 19])
def test_the_games_end_on_the_repetition_and_nowhere_else(built, n):
    """both board engines accept every move, report `terminated` only after the last one, and value the final position +1; the
    final position equals exactly the one earlier position the helper names"""
    game = sl.GAMES[n]
    for E in [Port(n)] + ([Ref(n)] if Ref.available(n) else []):
        s = E.new()
        boards = [E.board(s)[0].copy()]
        for c in game:
            assert not E.terminated(s) and E.forward(s, int(c)) == 1
            boards.append(E.board(s)[0].copy())
        assert E.terminated(s) and E.evaluate(s, 7.5) == 1.0 and int(E.info(s)[1]) == 1       # Black to move, +1
        assert [k for k in range(len(game)) if np.array_equal(boards[k], boards[-1])] == [sl.REPEATS[n]]
        E.free(s)


def _deep(engine, t, R):
    G = sl.SUPERKO_GAME
    net = sl.line_net(9, [], G, t)
    log = engine(G[:t], mka.config(R, 1), net)
    c = G[t]
    mka._only(log, {(c % 11 - 1, c // 11 - 1): sl.expected_line_edge(t, R, len(G) - 1)})
    assert len(net.seen) == sl.line_rows(t, len(G) - 1) and log["best_action"] == c


@pytest.mark.parametrize("t,R", DEEP)
def test_deep_lines_equal_the_closed_form_on_the_restatement(built, t, R):
    _deep(mka.port_engine, t, R)


@pytest.mark.parametrize("t,R", DEEP)
def test_deep_lines_equal_the_closed_form_on_the_reference_stack(built, t, R):
    need_ref(RefSelfPlay.available(9))
    _deep(mka.ref_engine, t, R)


def _closed_form_19(rows, name):
    n, game, t, cfg, _ = sl.live_case(name)
    s = rows[0][0]
    want_n, want_r = sl.expected_line_edge(t, cfg["rollouts_per_thread"], len(game) - 1)
    i = {int(c): i for i, c in enumerate(s["coord"])}[int(game[t])]
    assert int(s["visits"][i]) == want_n and s["reward"][i].view(np.uint32) == want_r.view(np.uint32), (name, s["visits"][i], s["reward"][i])
    assert int(s["visits"].sum()) == want_n and s["best_action"] == int(game[t])


@pytest.mark.parametrize("name", list(sl.LIVE))
def test_live_configurations_on_the_restatement(built, name):
    rows = sl.run_port(name)
    sl.assert_repetition_reached(rows, name)
    if name.startswith("19_"):
        _closed_form_19(rows, name)


@pytest.mark.parametrize("name", list(sl.LIVE))
def test_live_configurations_reference_stack_equals_the_restatement(built, name):
    need_ref(sl.ref_available(name))
    rows = sl.run_ref(name)
    sl.assert_repetition_reached(rows, name)
    if name.startswith("19_"):
        _closed_form_19(rows, name)
    sl.assert_same_searches(sl.run_port(name), rows, name)
