"""The search answers the reference itself holds (elfgames/go/mcts/mcts_test.cc), as engine-agnostic cases.

mcts_test.cc pokes NodeT directly (insertAction, updateEdgeStats, findMove); no engine here exposes a node, so each case reaches the
same situation through the normal entry point -- one search of a self-play game from a preloaded position, with a net callback that
answers every position of the case with a chosen `pi` row and `V` -- and asserts on the search log (root edge coords, visit counts,
priors, accumulated rewards, most-visited action, move played).  Every expected number below was written down by hand from
elf/ai/tree_search/tree_search_node.h (findMove :205-231, updateEdgeStats :253-278, UCT :361-397), tree_search_base.h
(EdgeInfo::getScore :132-157) and tree_search.h (batch_rollouts :200-262, single_rollout :264-322) BEFORE any engine was run; none
is copied from an engine's output.

Order of events of one search with R rollouts in batches of K (one search thread):
  * batch 1: the root is not visited, so all K descents stop at the root; it is evaluated once; no edge is touched.
  * every later batch: K descents (findMove at every visited node, virtual loss added to the edge taken), then the UNIQUE leaves of
    the batch are evaluated and backed up ONCE each, whatever the number of descents that ended there (tree_search.h:216-258:
    updateEdgeStats(reward, virtual_loss * count) -> num_visits + 1, virtual_loss back to 0).
  * a leaf's value V goes up unchanged (MCTSActor::reward, go/mcts/mcts.h:162-164): it is Black's value; a node with White to move
    negates Q when it scores its edges (q_flip, mcts.h:186; getScore :136-139).
  * score(edge) = c_puct * prior / (1 + n) * sqrt(N + 1) + q,  N = backups through the node, q = (+-reward - vl) / (n + vl) or, for an
    edge with n + vl == 0, +-unsignedMeanQ (0 at a fresh root; after each findMove (parentQ + sum of visited edges' reward / n) /
    (visited edges + 1)).
  * priors: pi2response (mcts.h:256-332) keeps the legal moves and divides by their sum (+ 1e-10).

The position is the 9x9 board of mcts_test.cc:141-151 loaded with load_board (known_answers.py; its move list interleaves passes,
never two in a row); after it Black is to move, one more pass gives White the move.  The callback sees only feature rows under the
search's random D4 code: it undoes each of the 8 codes and looks the stones + side to move up among the case's positions (the board
has no symmetry, so exactly one code matches).

engine(moves, cfg, net) -> dict(coord, visits, prior, reward: arrays over the root's edges; best_action, move_played) runs ONE search
after preloading `moves`; cfg uses the keys of pyoracle.MCTS_DEFAULTS; net(s [b,18,9,9]) -> (pi [b,82], v [b])."""
import numpy as np

from known_answers import N, flat, load_board
from pyoracle import Port, coord2action

NA = N * N + 1
BOARD = [".XO.XO.OO",          # mcts_test.cc:142-150
         "X.XXOOOO.",
         "XXXXXOOOO",
         "XXXXXOOOO",
         ".XXXXOOO.",
         "XXXXXOOOO",
         ".XXXXOOO.",
         "XXXXXOOOO",
         "XXXXOOOOO"]
# permutation of the 81 board actions under each D4 code: PERM[d4][canonical action x*9+y] = action in the transformed frame
PERM = np.array([[coord2action(N, flat(a // N, a % N), d4) for a in range(N * N)] for d4 in range(8)])


class _Recorder:
    """the part of the known_answers adapter load_board needs: records the moves it plays"""

    def __init__(self):
        self.moves = []

    def ply(self):
        return len(self.moves) + 1

    def forward(self, c):
        self.moves.append(int(c))
        return True


def position_moves(white_to_move):
    r = _Recorder()
    load_board(r, BOARD)
    assert not any(a == 0 and b == 0 for a, b in zip(r.moves, r.moves[1:]))      # never two passes in a row
    return r.moves + ([0] if white_to_move else [])


def act(xy):
    return xy[0] * N + xy[1]


def pi_row(weights, rest):
    """canonical pi row: weights {(x, y): p}; `rest` is shared equally by all other board points; pass gets 0"""
    p = np.full(NA, 0.0, np.float64)
    p[: N * N] = rest / (N * N - len(weights))
    for xy, w in weights.items():
        p[act(xy)] = w
    p[N * N] = 0.0
    return p.astype(np.float32)


class Net:
    """replies: list of (moves after the root position, pi row (canonical) or None for uniform, V); everything else gets the uniform
    row and V = 0"""

    def __init__(self, root_moves, replies):
        P = Port(N)
        self.table = {}
        self.legal = {}
        for extra, pi, v in replies:
            s = P.new()
            for c in list(root_moves) + [flat(*xy) for xy in extra]:
                assert P.forward(s, c) == 1
            assert not P.terminated(s)
            col, mover = P.board(s)[0], int(P.info(s)[1])
            key = ((col == mover).tobytes(), (col == 3 - mover).tobytes(), mover)
            assert key not in self.table
            self.table[key] = (pi if pi is not None else pi_row({}, 1.0), np.float32(v))
            self.legal[tuple(extra)] = P.legal_mask(s)
            P.free(s)
        self.seen = []

    def __call__(self, s):
        b = s.shape[0]
        pi = np.zeros((b, NA), np.float32)
        v = np.zeros(b, np.float32)
        for i in range(b):
            mover = 1 if s[i, 16, 0, 0] == 1.0 else 2
            assert s[i, 16 if mover == 1 else 17].all() and not s[i, 17 if mover == 1 else 16].any()
            hits = []
            for d4 in range(8):
                mine, theirs = (s[i, k].reshape(-1)[PERM[d4]] == 1.0 for k in (0, 1))
                hit = self.table.get((mine.tobytes(), theirs.tobytes(), mover))
                if hit is not None:
                    hits.append((d4, hit))
            assert len(hits) <= 1
            if hits:
                d4, (row, val) = hits[0]
                pi[i, PERM[d4]] = row[: N * N]
                pi[i, N * N] = row[N * N]
                v[i] = val
                self.seen.append(val)
            else:
                pi[i, : N * N] = 1.0 / (N * N)
        return pi, v


def config(rollouts, batch, virtual_loss=1):
    return dict(num_games=1, batchsize=max(batch, 1), mcts_threads=1, rollouts_per_thread=rollouts, rollouts_per_batch=batch, virtual_loss=virtual_loss,
                persistent_tree=1, use_prior=1, unexplored_q_zero=0, root_unexplored_q_zero=0, c_puct=5.0,        # tree_search_options.h:25
                root_epsilon=0.0, root_alpha=0.03, seed=11, komi=7.5, ply_pass_enabled=0, policy_distri_cutoff=0, max_searches=1)


def _edges(log):
    return {int(c): i for i, c in enumerate(log["coord"])}


def _expect_priors(log, net, row, extra=()):
    """pi2response: the legal moves' pi over their sum; the pass edge (present or not: remove_pass_if_dangerous) carries 0 here"""
    legal = net.legal[tuple(extra)]
    e = _edges(log)
    tot = float(sum(np.float64(row[a]) for a in range(N * N) if legal[a]))
    for a in range(N * N):
        c = flat(a // N, a % N)
        assert (c in e) == bool(legal[a]), (a, sorted(e))
        if legal[a]:
            assert abs(float(log["prior"][e[c]]) - float(row[a]) / tot) <= 2e-7 * float(row[a]) / tot + 1e-12, (a, log["prior"][e[c]], row[a] / tot)
    assert set(e) - {0} == {flat(a // N, a % N) for a in range(N * N) if legal[a]}
    if 0 in e:
        assert log["prior"][e[0]] == 0.0


def _only(log, want):
    """want {(x, y): (visits, reward as np.float32 or None)}; every other root edge has no visit and no reward"""
    e = _edges(log)
    want = {flat(*xy): w for xy, w in want.items()}
    for c, i in e.items():
        n, r = want.get(c, (0, np.float32(0)))
        assert int(log["visits"][i]) == n, (c, log["visits"][i], n)
        if r is not None:
            assert np.float32(log["reward"][i]).view(np.uint32) == np.float32(r).view(np.uint32), (c, log["reward"][i], r)
    assert set(want) <= set(e)


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# W root: legal (3,0) (6,0) (8,1) (8,4) (8,6) + pass;  B root: legal (0,0) (0,4) (0,6) (1,1) (3,0), pass removed as dangerous
W_A, W_C, B_A, B_C = (8, 4), (8, 6), (0, 4), (0, 6)


def case_select_the_high_prior(engine):
    """mcts_test.cc:119-136 testSelectLeaf: one prior of 0.4 among equal small ones is the edge findMove takes.
    Root reply: 0.4 on (8,4), the other 80 points 0.0075 each; c_puct 5, no noise, one rollout per batch, R = 2: rollout 1 expands
    the root, rollout 2 is its first findMove -- every edge has n = 0, vl = 0, q = -unsignedMeanQ = 0, so score = 5 * prior and the
    0.4 edge wins (2.0 / S against 0.0375 / S, S = legal mass).  Its child is evaluated (V = 0.5) and backed up once.
    Expected: edge (8,4) visits 1 reward 0.5, every other edge visits 0 reward 0; most-visited action (8,4).
    Fails if the argmax runs over the wrong array (q, visits or the unscaled edge order instead of the score: all of those tie at 0 and
    give the first edge in iteration order, which is not the first-inserted 0.4 edge)."""
    moves = position_moves(white_to_move=True)
    row = pi_row({W_A: 0.4}, 0.6)
    net = Net(moves, [((), row, 0.0), ((W_A,), None, 0.5)])
    log = engine(moves, config(2, 1), net)
    _expect_priors(log, net, row)
    _only(log, {W_A: (1, np.float32(0.5))})
    assert log["best_action"] == flat(*W_A) and log["move_played"] == flat(*W_A)
    assert net.seen == [np.float32(0.0), np.float32(0.5)]


def _backup_case(engine, white_root):
    """Hand derivation (sign s = -1 for a White root, +1 for a Black root; leaf values v1 = s * 1, v2 = s * 0.2, so that the mover at
    the root sees two WINS on edge A; root reply A 0.48, C 0.16 = A / 3, rest 0.36 / 79 each; leaf reply B 0.9; c_puct 5):
      rollout 1: root expanded (V = 0).
      rollout 2: all edges unvisited, q = 0: A by prior.  Child L evaluated, V = v1; A: n 1, reward v1.  root meanQ -> 0.
      rollout 3: N + 1 = 2.  A: q = s * v1 / 1 = +1, score 1 + 5 * a / 2 * 1.414;  C: 0 + 5 * (a / 3) * 1.414: A.  root meanQ ->
                 (0 + v1) / 2 = s * 0.5.  L: B by prior; child L2 evaluated, V = v2; B: n 1, reward v2;  A: n 2, reward v1 + v2.
         => R = 3: A visits 2, reward fl32(v1 + v2) = -+1.2f, Q = -+0.6 (mcts_test.cc:207 EXPECT_FLOAT_EQ(leaf.Q(), -0.6)).
      rollout 4: N + 1 = 3.  A: q = s * (v1 + v2) / 2 = +0.6, score 0.6 + 5 * a / 3 * 1.732 = 0.6 + 2.887 a;
                 C: unvisited, q = s * meanQ = +0.5, score 0.5 + 5 * (a / 3) * 1.732 = 0.5 + 2.887 a: A again, by 0.1.
                 WITHOUT the flip for White (or with a flip for Black) the two q are -0.6 and -0.5 and C wins by 0.1 (and rollout 3
                 already scores A -1 + 3.54 a against 2.36 a for C: C for a < 0.85; a = 0.48 / S ~ 0.74).
                 L: B again (q = -0.2 for L's mover, prior 0.9 dominates); L2: any edge; new leaf V = 0.
         => R = 4: A visits 3, reward unchanged (+ 0), every other root edge 0 visits."""
    s = np.float32(-1.0 if white_root else 1.0)
    A, C, B = (W_A, W_C, B_A) if white_root else (B_A, B_C, W_A)
    moves = position_moves(white_to_move=white_root)
    row = pi_row({A: 0.48, C: 0.16}, 0.36)
    v1, v2 = np.float32(s * np.float32(1.0)), np.float32(s * np.float32(0.2))
    replies = [((), row, 0.0), ((A,), pi_row({B: 0.9}, 0.1), v1), ((A, B), None, v2)]
    want = np.float32(v1 + v2)                                   # the fp32 sum in backup order
    assert _ulps(want / np.float32(2), s * np.float32(0.6)) <= 4      # EXPECT_FLOAT_EQ: within 4 ulp
    net = Net(moves, replies)
    log = engine(moves, config(3, 1), net)
    _expect_priors(log, net, row)
    _only(log, {A: (2, want)})
    i = _edges(log)[flat(*A)]
    assert _ulps(np.float32(log["reward"][i]) / np.float32(log["visits"][i]), s * np.float32(0.6)) <= 4
    assert log["best_action"] == flat(*A) and log["move_played"] == flat(*A)
    assert net.seen == [np.float32(0.0), v1, v2]
    net = Net(moves, replies)
    log = engine(moves, config(4, 1), net)
    _only(log, {A: (3, want)})                                   # the next descent from the root took the same edge again
    assert log["best_action"] == flat(*A)


def case_backup_arithmetic_and_sign_white_root(engine):
    """mcts_test.cc:138-208 testBackupIncorporateResults, White to move at the root: backups of -1 and -0.2 (Black's value: two White
    wins) on one root edge give visits 2, reward fl32(-1 + -0.2), Q = -0.6 within 4 ulp; the next descent takes that edge again.
    Derivation: _backup_case.  Fails if the sign flip for White is missing (C is taken instead, A ends with fewer visits), if a
    backup adds -V or |V|, or if the reward is not accumulated in fp32 in backup order."""
    _backup_case(engine, white_root=True)


def case_backup_arithmetic_and_sign_black_root(engine):
    """the mirror of the case above with Black to move at the root and backups of +1 and +0.2: a flip applied to Black, or a flip
    that is wrong twice along the path, cannot cancel out in both cases."""
    _backup_case(engine, white_root=False)


def case_virtual_loss_keeps_a_dominant_prior(engine):
    """mcts_test.cc:270-296 testDontPickUnexpandedChild: a 0.999 prior is taken again although the edge carries a virtual loss.
    Changed from the reference's test: it adds a virtual loss of -0.5 by hand, which the integer option virtual_loss cannot express;
    here virtual_loss = 1, two rollouts per batch, c_puct 5, White root, root reply 0.999 on (8,4), the rest sharing 0.001.
    Second descent of batch 2, in float64 (tree_search_node.h:361-397, N + 1 = 1, a = 0.999 / S >= 0.999):
        score(A) = 5 * a / (1 + 0) * sqrt(1) + (-0 - 1) / (0 + 1) = 5 a - 1 >= 3.995
        score(other) = 5 * (0.001 / 80 / S) + 0 <= 6.3e-5 / S < 1e-3          gap > 3.99 (>> 1e-3: fp32 cannot reorder them)
    so both descents end in A's child.  The batch backs a unique leaf up ONCE (tree_search.h:216-258): the edge has 1 visit, not 2,
    reward V(child) = 0.25, virtual loss back to 0 -- the observable "both in the same leaf" is: exactly one root edge was visited.
    Third batch (R = 6): descent 1: A (n 1, vl 0: q = -0.25, score 5 a / 2 * 1.414 - 0.25 ~ 3.3), then B in L (0.999); descent 2:
    A: q = (-0.25 - 1) / 2 = -0.625, score ~ 2.9 against < 0.01 - 0.125; L: B: 5 b - 1 ~ 4: the same leaf again -> A visits 2,
    reward 0.25 + -0.5 = -0.25.
    Fails if a virtual loss weighs more than about 4 visits' worth (it unseats A), if the selection ignores the prior term, or if
    the duplicate leaf is backed up twice (visits 2 after R = 4).  Like the reference's own test it does NOT notice a missing or
    wrong-signed virtual loss -- 0.999 wins either way; the next case does, and a loss that is never taken back fails the two
    backup cases."""
    moves = position_moves(white_to_move=True)
    row = pi_row({W_A: 0.999}, 0.001)
    replies = [((), row, 0.0), ((W_A,), pi_row({B_A: 0.999}, 0.001), 0.25), ((W_A, B_A), None, -0.5)]
    net = Net(moves, replies)
    log = engine(moves, config(4, 2), net)
    _expect_priors(log, net, row)
    _only(log, {W_A: (1, np.float32(0.25))})
    assert log["best_action"] == flat(*W_A)
    net = Net(moves, replies)
    log = engine(moves, config(6, 2), net)
    _only(log, {W_A: (2, np.float32(-0.25))})
    assert net.seen == [np.float32(0.0), np.float32(0.25), np.float32(-0.5)]


def case_virtual_loss_unseats_a_narrow_lead(engine):
    """Not in mcts_test.cc: the complement that makes the virtual-loss bookkeeping observable (with a 0.999 prior neither a missing
    nor a wrong-signed loss changes the pick).  White root, root reply A (8,4) 0.5, C (8,6) 0.4, rest 0.1 / 79 each; c_puct 5,
    virtual_loss 1, two rollouts per batch, R = 4.  Second descent of batch 2 in float64 (S = legal mass ~ 0.904, a = 0.5 / S,
    c = 0.4 / S, N + 1 = 1):
        score(A) = 5 a + (-0 - 1) / (0 + 1) = 5 a - 1 = 1.766        score(C) = 5 c + 0 = 2.213        gap 0.447 >= 1e-3
    so the second descent takes C.  Without a virtual loss (or with it added instead of subtracted: r = +1, or n + vl = -1 -> the
    unvisited branch) A scores 5 a = 2.766 > 2.213 and both descents share A's child.
    Expected: A visits 1 reward V(A's child) = 0.5;  C visits 1 reward V(C's child) = -0.25;  every other edge 0.
    Fails if the virtual loss is not applied within a batch, or applied with the wrong sign."""
    moves = position_moves(white_to_move=True)
    row = pi_row({W_A: 0.5, W_C: 0.4}, 0.1)
    net = Net(moves, [((), row, 0.0), ((W_A,), None, 0.5), ((W_C,), None, -0.25)])
    log = engine(moves, config(4, 2), net)
    _expect_priors(log, net, row)
    _only(log, {W_A: (1, np.float32(0.5)), W_C: (1, np.float32(-0.25))})
    assert sorted(net.seen) == sorted([np.float32(0.0), np.float32(0.5), np.float32(-0.25)])


ALL_CASES = [case_select_the_high_prior, case_backup_arithmetic_and_sign_white_root, case_backup_arithmetic_and_sign_black_root,
             case_virtual_loss_keeps_a_dominant_prior, case_virtual_loss_unseats_a_narrow_lead]


# ---- positional superko inside the tree (not in mcts_test.cc; go_state.h:117-124,194-203) ----------------------------------------
def _superko_case(engine, t, pre=()):
    """One search of 24 rollouts (one per batch) from pre + SUPERKO_GAME[:t] with superko_lines.line_net: the search walks down the
    game, the node after move 76 repeats the position after move 73 and is terminal with value +1 (-1 with the colours swapped by a
    leading pass), never sent to the net.  Expectation: superko_lines.expected_line_edge, a closed form derived there by hand.
    Fails if the repetition is missed (the node goes to the net: one more row in net.seen, V = 0 instead of +-1 in the reward, and a
    subtree grows below it), if it is scored by Tromp-Taylor or with the wrong sign, or if a live node of the line is taken for a
    repetition (an early +-1 in the reward, fewer net rows)."""
    import superko_lines as sl
    G = sl.SUPERKO_GAME
    last, R, sign = len(G) - 1, 24, -1 if len(pre) % 2 else 1
    net = sl.line_net(N, list(pre), G, t)
    log = engine(list(pre) + G[:t], config(R, 1), net)
    c = G[t]
    _only(log, {(c % (N + 2) - 1, c // (N + 2) - 1): sl.expected_line_edge(t, R, last, 0.125, sign)})
    assert len(net.seen) == sl.line_rows(t, last) and all(v == np.float32(0.125) for v in net.seen), net.seen
    assert log["best_action"] == c


def case_superko_repeats_the_second_newest_game_record(engine):
    """root after move 75: the repeated position (after move 73) is the game's second-newest record; the terminal is the root's child"""
    _superko_case(engine, 75)


def case_superko_repeats_the_newest_game_record(engine):
    """root after move 74: the repeated position is the newest record that precedes the root -- the boundary of the records the
    game contributes"""
    _superko_case(engine, 74)


def case_superko_repeats_the_root_itself(engine):
    """root after move 73: the repeated position is the root node's own"""
    _superko_case(engine, 73)


def case_superko_repeats_an_interior_tree_node(engine):
    """root after move 72: the repeated position is a tree node between the root and the terminal"""
    _superko_case(engine, 72)


def case_superko_repeats_a_deeper_interior_node(engine):
    """root after move 68: terminal at depth 8, the repeated position five nodes below the root"""
    _superko_case(engine, 68)


def case_superko_colours_swapped_game_record(engine):
    """a leading pass swaps the colours: Black makes the repetition, White is to move in it, value -1; root after move 75"""
    _superko_case(engine, 75, pre=(0,))


def case_superko_colours_swapped_interior_node(engine):
    """colours swapped, root after move 72: value -1 backed up through White and Black nodes alike"""
    _superko_case(engine, 72, pre=(0,))


ALL_CASES += [case_superko_repeats_the_second_newest_game_record, case_superko_repeats_the_newest_game_record,
              case_superko_repeats_the_root_itself, case_superko_repeats_an_interior_tree_node,
              case_superko_repeats_a_deeper_interior_node, case_superko_colours_swapped_game_record,
              case_superko_colours_swapped_interior_node]


# ---- the two CPU engines -------------------------------------------------------------------------------------------------------
def _first_search(r):
    assert len(r["search"]) == 1
    S = r["search"][0]
    ne = S.n_edges
    return dict(coord=r["coord"][0, :ne], visits=r["visits"][0, :ne], prior=r["prior"][0, :ne], reward=r["reward"][0, :ne],
                best_action=int(S.best_action), move_played=int(S.move_played))


def port_engine(moves, cfg, net):
    from pyoracle import PortSelfPlay
    P = PortSelfPlay(N)
    P.set_preload(moves, len(moves))
    try:
        return _first_search(P.run(net=net, **cfg))
    finally:
        P.set_preload([], -1)


def ref_engine(moves, cfg, net):
    """the reference's own self-play stack (the stand-in build, oracle/_ref/libelfsp9.so); preload through an SGF text"""
    import os
    import tempfile
    from pyoracle import RefSelfPlay
    R = RefSelfPlay(N)
    fd, path = tempfile.mkstemp(suffix=".sgf")
    with os.fdopen(fd, "w") as fh:
        fh.write("(;GM[1]FF[4]SZ[%d]KM[7.5]" % N + R.coords2sgfstr(moves)[1:])
    R.set_preload(path, len(moves))
    try:
        return _first_search(R.run(net=net, **cfg))
    finally:
        R.set_preload("", -1)
        os.unlink(path)
