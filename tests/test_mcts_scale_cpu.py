"""CPU: the condition that keeps the thousand-game search tests (test_gpu_mcts_scale.py) discriminating.  Those tests compare
game g of a G-game context with the CPU restatement's game seeded seed + g; handing game A the rows of game B can only show
if A's and B's search logs differ.  So, on the oracle alone and for every configuration used there: every game yields the
requested searches, and at least 99 % of the per-game logs are pairwise distinct."""
import pytest

from mcts_scale_cases import LOCKSTEP, UNEVEN_FORCED, UNEVEN_G, UNEVEN_N, UNEVEN_SEARCHES, lockstep_cfg, uneven_cfg
from sp_drive import oracle_per_game


def _distinct_share(logs, G):
    return len(set(tuple(logs[g]) for g in range(G))) / G


@pytest.mark.parametrize("n,G,roll,bs,searches,nodes", LOCKSTEP)
def test_lockstep_games_are_pairwise_distinct(built, n, G, roll, bs, searches, nodes):
    want = oracle_per_game(n, lockstep_cfg(G, roll, bs), G, searches)
    assert all(len(want[g]) == searches for g in range(G))
    share = _distinct_share(want, G)
    print("distinct logs: %.4f" % share)
    assert share >= 0.99


def test_out_of_phase_evaluation_games_are_pairwise_distinct(built):
    """both populations of the uneven case: the games that start with Black's search, and the first search (White's) of the games
    that start one forced move ahead -- the part of them that is taken from the oracle"""
    n, G = UNEVEN_N, UNEVEN_G
    want = oracle_per_game(n, uneven_cfg(), G, UNEVEN_SEARCHES)
    assert all(len(want[g]) == UNEVEN_SEARCHES for g in range(G))
    ahead = oracle_per_game(n, uneven_cfg(), G, 1, preload=(UNEVEN_FORCED,))
    assert all(len(ahead[g]) == 1 for g in range(G))
    even, odd = _distinct_share(want, G), _distinct_share(ahead, G)
    print("distinct logs: %.4f from the empty board, %.4f first search after the forced move" % (even, odd))
    assert even >= 0.99 and odd >= 0.99
    # the two AIs are different players: White's first search after the forced move is not Black's first search
    assert sum(ahead[g][0] == want[g][0] for g in range(G)) == 0
