"""Positional superko INSIDE a search tree: two games that end on a repetition, a scripted net that walks the search down the game,
and the closed form of what the root must then hold.  No tests here; tests/mcts_known_answers.py (the engine-agnostic cases),
tests/test_superko_lines_cpu.py, tests/test_gpu_mcts_superko.py and tests/test_gpu_setup.py import it.

The reference scores a node whose position repeats an earlier one as TERMINAL with value nextPlayer() == S_BLACK ? +1 : -1
(go_state.h:194-203) -- not with Tromp-Taylor, not with the net -- and every tree node carries the whole record map of its game
(go_state.h:117-124).  An engine that rebuilds that map from other sources (ancestors' boards, the game's records, a Bloom filter)
is checked here at every place the repeated position can sit relative to the root of the search."""
import numpy as np

from pyoracle import Port, coord2action

# 9x9, 76 moves, no pass: moves 74-76 are a send-two-return-one cycle on the right edge; the position after move 76 is the position
# after move 73 (and no other).  White plays move 76: Black is to move in the repeated position, its value is +1.  Reference Coords.
SUPERKO_GAME = [41, 45, 96, 67, 83, 15, 24, 75, 101, 42, 26, 73, 37, 71, 31, 90, 16, 70, 91, 48, 86, 19, 36, 62, 81, 17, 25, 50, 58,
                38, 84, 69, 47, 23, 12, 60, 57, 20, 89, 27, 18, 107, 52, 13, 108, 102, 14, 28, 85, 95, 104, 51, 106, 92, 103, 46, 78,
                30, 102, 80, 105, 79, 82, 39, 68, 16, 72, 59, 107, 34, 93, 100, 64, 53, 31, 42]

# 19x19, 12 moves: W (18,0) (17,0) (17,1) (18,2) and B (17,2) (17,3) (18,4) with two tenuki moves; then W (18,3), B takes two at
# (18,1), W retakes at (18,2): the position after move 12 is the position after move 9, Black to move, value +1.  Reference Coords.
SUPERKO_GAME_19 = [81, 39, 102, 60, 124, 40, 88, 82, 340, 103, 61, 82]

GAMES = {9: SUPERKO_GAME, 19: SUPERKO_GAME_19}
REPEATS = {9: 73, 19: 9}          # the ply whose position the last move repeats


def perm(n):
    """PERM[d4][canonical action x*n+y] = action in the frame transformed by the D4 code"""
    S = n + 2
    return np.array([[coord2action(n, (a % n + 1) * S + a // n + 1, d4) for a in range(n * n)] for d4 in range(8)])


class line_net:
    """The scripted net of a line: for every k in [t, len(game) - 1] the position after pre + game[:k] answers prior `p` on game[k],
    1 - p shared by the other board points, pass 0, and V = v; every other position gets the uniform row and V = 0.  `pre` goes in
    front of the game ([0], a pass, swaps the colours).  The method is mcts_known_answers.Net's: the callback sees feature rows under
    the search's random D4 code, undoes each of the 8 codes and looks stones + side to move up; at most one code may match.
    seen: the V of every scripted position that was asked for, in order."""

    def __init__(self, n, pre, game, t, v=0.125, p=0.97):
        self.n, self.na, self.PERM = n, n * n + 1, perm(n)
        P = Port(n)
        S = n + 2
        self.table = {}
        s = P.new()
        for c in list(pre) + list(game[:t]):
            assert P.forward(s, int(c)) == 1
        for k in range(t, len(game)):
            assert not P.terminated(s)
            col, mover = P.board(s)[0], int(P.info(s)[1])
            key = ((col == mover).tobytes(), (col == 3 - mover).tobytes(), mover)
            assert key not in self.table
            c = int(game[k])
            row = np.full(self.na, (1.0 - p) / (n * n - 1), np.float64)
            row[(c % S - 1) * n + (c // S - 1)] = p
            row[n * n] = 0.0
            self.table[key] = (row.astype(np.float32), np.float32(v))
            assert P.forward(s, c) == 1
        assert P.terminated(s)                     # the line ends on the repetition
        P.free(s)
        self.seen = []

    def __call__(self, s):
        n, na, PERM = self.n, self.na, self.PERM
        b = s.shape[0]
        pi = np.zeros((b, na), np.float32)
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
                pi[i, PERM[d4]] = row[: n * n]
                pi[i, n * n] = row[n * n]
                v[i] = val
                self.seen.append(val)
            else:
                pi[i, : n * n] = 1.0 / (n * n)
        return pi, v


def expected_line_edge(t, R, last, v=0.125, sign=1):
    """(visits, reward as np.float32) of the root edge game[t] after ONE search of R rollouts, one per batch, one thread, on a fresh
    tree, from the position after game[:t], with line_net; `last` is the index of the move that makes the repetition and sign the
    repeated position's value (+1: Black to move in it).
    Derivation (order of events: mcts_known_answers.py; c_puct 5, no noise):
      * batch 1 evaluates the root; no edge is touched.
      * every descent follows the line.  At a node of the line with N backups the scripted edge (n <= N visits) scores
        5 * (0.97 / S) * sqrt(N + 1) / (1 + n) + q >= 4.85 / sqrt(N + 1) + q, any other edge is unvisited and scores
        5 * (0.03 / (n*n - 1) / S) * sqrt(N + 1) + q' (S: the legal mass, near 1); with N <= 99 and n*n - 1 >= 80 the prior terms
        differ by >= 0.485 - 0.019 = 0.466.  Only one edge is ever visited, so q' = +-unsignedMeanQ = +-(parentQ + Q) / 2 with Q the
        edge's mean backup and parentQ the mean the node was created with; for sign +1 both lie in [0.125, 1], so an unvisited edge
        gains at most |Q - parentQ| / 2 <= 0.4375 < 0.466 on the scripted one.  For sign -1 they lie in [-1, 0.125] and the gain can
        reach 0.5625, but those cases run 24 rollouts: N <= 23, the prior terms differ by >= 0.98.  The two CPU engines confirm
        every figure the tests use (tests/test_superko_lines_cpu.py, tests/test_mcts_known_answers.py) before any GPU is asked.
      * so batches 2 .. last - t + 1 each create ONE new node, the positions after game[:t+1] .. game[:last]: last - t net leaves,
        each backed up with V = v through the root edge;
      * the next batch creates the node after game[:last + 1]: the repetition, terminal, value `sign`, never sent to the net; it has no
        edges, so every later descent ends on it again and backs `sign` up: R - 1 - (last - t) times in all.
    visits = R - 1; reward = the fp32 sum in backup order.  The net is asked for last - t + 1 positions (the root and the line)."""
    assert R - 1 > last - t
    r = np.float32(0)
    for _ in range(last - t):
        r = np.float32(r + np.float32(v))
    for _ in range(R - 1 - (last - t)):
        r = np.float32(r + np.float32(sign))
    return R - 1, r


def line_rows(t, last):
    """positions line_net is asked for in a search that reaches the repetition: the root and the line below it"""
    return last - t + 1


# ---- the live differentials: configurations shared by the CPU twin and the GPU file ----------------------------------------------
def search_cfg(R, K, **over):
    """mcts_known_answers.config (c_puct 5, no noise, one thread, one search) over pyoracle.MCTS_DEFAULTS, then `over`"""
    from mcts_known_answers import config
    from pyoracle import MCTS_DEFAULTS
    cfg = dict(MCTS_DEFAULTS)
    cfg.update(config(R, K))
    cfg.update(over)
    return cfg


# name -> (board size, root t, configuration, searches compared per game)
LIVE = {
    # (a) a deep line in wide batches: 8 descents share every new leaf, about 69 batches reach the repetition, 100 are run
    "deep_K8": (9, 8, dict(R=800, K=8), 1),
    # (b) the repetition below an interior node, batches of 4 and of 16
    "t72_K4": (9, 72, dict(R=96, K=4), 1),
    "t72_K16": (9, 72, dict(R=96, K=16), 1),
    # (c) two search threads on the shared tree (the reference under its turnstile schedule)
    "t72_T2": (9, 72, dict(R=48, K=4, mcts_threads=2), 1),
    # (d) three games in one context, each with its own records, Bloom words and path rows; two searches each
    "t72_G3": (9, 72, dict(R=48, K=4, num_games=3), 2),
    # (e) the game itself plays moves 71 .. 76 and ends on the repetition, restarts, and searches twice more: with the persistent tree
    #     the terminal node found by the first search survives every treeAdvance while the repeated position migrates from tree
    #     ancestor to root to game record; with fresh trees every search finds the repetition again in the records
    "t70_game_persistent": (9, 70, dict(R=24, K=1, persistent_tree=1), 8),
    "t70_game_fresh": (9, 70, dict(R=24, K=1, persistent_tree=0), 8),
    # 19x19 (6 bitboard words, 13-word records): the root at the newest record, the second newest, the repeated position, above it
    "19_t11": (19, 11, dict(R=24, K=1), 1),
    "19_t10": (19, 10, dict(R=24, K=1), 1),
    "19_t9": (19, 9, dict(R=24, K=1), 1),
    "19_t7": (19, 7, dict(R=24, K=1), 1),
}


def live_case(name):
    """-> (n, game, t, cfg with max_searches for ONE game's worth of searches, per_game)"""
    n, t, kw, per_game = LIVE[name]
    kw = dict(kw)
    cfg = search_cfg(kw.pop("R"), kw.pop("K"), max_searches=per_game, **kw)
    return n, GAMES[n], t, cfg, per_game


def _rows(r, games):
    """search log -> {game: [(n_edges, move_played, best_action, total_visits, root value bits, coord, visits, prior, reward)]}"""
    out = {g: [] for g in range(games)}
    for i, s in enumerate(r["search"]):
        ne = s.n_edges
        out[s.game].append(dict(n_edges=ne, move_played=int(s.move_played), best_action=int(s.best_action), total_visits=int(s.total_visits),
                                root_value=np.float32(s.root_value), coord=r["coord"][i, :ne].astype(np.int32).copy(),
                                visits=r["visits"][i, :ne].astype(np.int32).copy(), prior=r["prior"][i, :ne].astype(np.float32).copy(),
                                reward=r["reward"][i, :ne].astype(np.float32).copy()))
    return out


def run_port(name):
    """the CPU restatement on a live case -> {game: [search rows]}; G games are played one by one with seed + g"""
    from pyoracle import PortSelfPlay
    n, game, t, cfg, per_game = live_case(name)
    P = PortSelfPlay(n)
    P.set_preload(game, t)                  # the whole game: the moves after the root are the ones the searches must find anyway
    out = {}
    try:
        for g in range(cfg["num_games"]):
            r = P.run(net=line_net(n, [], game, t), **dict(cfg, num_games=1, seed=cfg["seed"] + g))
            assert len(r["search"]) == per_game
            out[g] = _rows(r, 1)[0]
    finally:
        P.set_preload([], -1)
    return out


def ref_available(name):
    from pyoracle import RefSelfPlay
    n, _, _, cfg, _ = live_case(name)
    return RefSelfPlay.available(n, turnstile=cfg["mcts_threads"] > 1)


def run_ref(name):
    """the reference's own self-play stack on a live case (its turnstile build for mcts_threads > 1) -> {game: [search rows]}; its G
    game threads finish searches at their own pace, so it runs until every game has logged per_game searches"""
    import os
    import tempfile
    from pyoracle import RefSelfPlay
    n, game, t, cfg, per_game = live_case(name)
    G = cfg["num_games"]
    R = RefSelfPlay(n, turnstile=cfg["mcts_threads"] > 1)
    fd, path = tempfile.mkstemp(suffix=".sgf")
    with os.fdopen(fd, "w") as fh:
        fh.write("(;GM[1]FF[4]SZ[%d]KM[7.5]" % n + R.coords2sgfstr(game)[1:])
    R.set_preload(path, t)
    try:
        r = R.run(net=line_net(n, [], game, t), **dict(cfg, max_searches=per_game if G == 1 else G * per_game * 3))
    finally:
        R.set_preload("", -1)
        os.unlink(path)
    out = _rows(r, G)
    assert all(len(out[g]) >= per_game for g in range(G)), [len(out[g]) for g in range(G)]
    return {g: out[g][:per_game] for g in range(G)}


def run_checker(name):
    """the checker of a GPU test: the compiled reference where it is built, its CPU restatement (with a warning that says so) where
    it is not -- the test never skips"""
    if ref_available(name):
        return run_ref(name)
    import warnings
    warnings.warn("oracle/_ref is absent: '%s' is compared with the CPU restatement (oracle/mcts_oracle.cc), not with the compiled "
                  "reference" % name)
    return run_port(name)


def assert_same_searches(got, want, ctx):
    """every root statistic of every search, bit for bit"""
    assert sorted(got) == sorted(want), ctx
    for g in want:
        assert len(got[g]) == len(want[g]), (ctx, g, len(got[g]), len(want[g]))
        for k, (a, b) in enumerate(zip(got[g], want[g])):
            where = "%s: game %d search %d" % (ctx, g, k)
            assert a["n_edges"] == b["n_edges"], where
            assert np.array_equal(a["coord"], b["coord"]), where + ": edge order"
            assert np.array_equal(a["visits"], b["visits"]), where + ": visits %s / %s" % (a["visits"][a["visits"] > 0], b["visits"][b["visits"] > 0])
            assert np.array_equal(a["prior"].view(np.uint32), b["prior"].view(np.uint32)), where + ": priors"
            assert np.array_equal(a["reward"].view(np.uint32), b["reward"].view(np.uint32)), \
                where + ": rewards %s / %s" % (a["reward"][a["visits"] > 0], b["reward"][b["visits"] > 0])
            assert (a["move_played"], a["best_action"], a["total_visits"]) == (b["move_played"], b["best_action"], b["total_visits"]), where
            assert a["root_value"].view(np.uint32) == b["root_value"].view(np.uint32), where


def assert_repetition_reached(rows, name):
    """on the CHECKER's own answer: in every search on the line (search k of a game starts after move t + k: the game plays the
    line's moves) the edge of the game's next move holds more than 0.125 a visit, which only backups of the repetition's +1 can give
    it (every net value on the line is 0.125).  A run that never reaches the repetition proves nothing.  Where more searches are
    compared than the line has moves, the game has ended on the repetition and the later ones belong to the next game."""
    n, game, t, cfg, per_game = live_case(name)
    for g, searches in rows.items():
        assert len(searches) == per_game
        for k, s in enumerate(searches[:len(game) - t]):
            e = {int(c): i for i, c in enumerate(s["coord"])}
            i = e[int(game[t + k])]
            assert s["visits"][i] > 0 and s["reward"][i] > np.float32(0.125) * s["visits"][i], (name, g, k, s["visits"][i], s["reward"][i])
            assert s["move_played"] == int(game[t + k]), (name, g, k)
        for s in searches[len(game) - t:]:
            assert s["n_edges"] > n * n - 2, name         # a fresh game: the previous one ended with the repetition
