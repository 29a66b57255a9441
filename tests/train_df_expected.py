"""What ReplayLoader(feature_format="df_f32_nchw") / elftrain_extract with ELFGO_FEAT_DF_F32_NCHW must write into `s`, taken
from the reference: a record's first move_to moves are replayed with pyoracle.Ref (the reference's own GoState) and the row is
df_expected.Df.planes(state, d4) -- BoardFeature::extract through the stand-in object tests/test_df_cpu.py proves.  A move the
reference refuses is skipped and M_INVALID is never handed to it (GoState::forward throws there): the rule k_replay_extract
documents.  Nothing here calls into elf_amd's kernels.

Also the instrument for the store's placement plies: `place_plies` states, from the reference's replay, what
k_replay_checkpoint_df writes per move, and `placed_from` restates in numpy how a sample rebuilds Info::last_placed from them
(placed[point of move t] = max over t < move_to of place_ply[t])."""
import numpy as np

import df_expected as DE
from pyoracle import M_INVALID, M_PASS, M_RESIGN, coord

PLANES = DE.PLANES
CK = 16   # CK_INTERVAL of train.cuh


def action_of(n, c):
    """reference Coord -> action id a = x*n + y (board.h:183-184 read backwards)"""
    c = np.asarray(c, np.int64)
    return (c % (n + 2) - 1) * n + (c // (n + 2) - 1)


def record(n, moves, seed=0, black_ver=7, reward=1.0):
    """a parse_record()-shaped dict for ReplayLoader.put: the moves, a random quantised policy and a value for every ply"""
    rng = np.random.default_rng(seed)
    moves = np.asarray(moves, np.uint16)
    pol = rng.integers(0, 256, (len(moves), (n + 2) ** 2), dtype=np.uint8)
    pol[:, 0] |= 1                               # the pass entry: no row sums to zero
    return dict(moves=moves, reward=float(reward), black_ver=int(black_ver), policies=pol,
                values=rng.uniform(-1, 1, len(moves)).astype(np.float32), seq=0)


def walk(n, moves, visit):
    """the reference's replay with the skip rule: visit(t, state) at every t in [0, len(moves)] (state = after the first t
    moves), -> (played [len] bool, ply_before [len])"""
    E = DE.df(n).E
    s = E.new()
    played, before = np.zeros(len(moves), bool), np.zeros(len(moves), np.int64)
    for t in range(len(moves) + 1):
        visit(t, s)
        if t < len(moves):
            c = int(moves[t])
            before[t] = int(E.info(s)[0])
            played[t] = c != M_INVALID and E.forward(s, c) == 1
    E.free(s)
    return played, before


def rows(n, moves, move_to, d4):
    """-> float32 [k, 25, n, n]: the reference's DarkForest row after the first min(move_to[i], len(moves)) moves under d4[i]"""
    D = DE.df(n)
    at = {}
    for i, mt in enumerate(move_to):
        at.setdefault(min(int(mt), len(moves)), []).append(i)
    out = np.zeros((len(move_to), PLANES, n, n), np.float32)

    def visit(t, s):
        for i in at.get(t, ()):
            out[i] = D.planes(s, int(d4[i]))
    walk(n, moves, visit)
    return out


_every = {}


def every_ply(name, g):
    """game g of df_expected.game_set(name) -> (n, moves, rows [len + 1, 25, n, n] under code (g + ply) % 8), once per process"""
    if (name, g) not in _every:
        n, games = DE.game_set(name)
        mv = np.asarray(games[g], np.int64)
        mt = np.arange(len(mv) + 1)
        _every[name, g] = (n, mv, rows(n, mv, mt, [DE.code_of(g, int(t)) for t in mt]))
    return _every[name, g]


EVERY_PLY_GAMES = [("nine", 0), ("nine", 1), ("nine", 2), ("ladder16", 0), ("playout19", 0)]


def place_plies(n, moves):
    """uint16 [len(moves)]: the ply an accepted placement at move t wrote into Info::last_placed (the board's ply before the move;
    _ply starts at 1), 0 for a pass, a resignation, a refused move and M_INVALID"""
    played, before = walk(n, moves, lambda t, s: None)
    mv = np.asarray(moves, np.int64)
    return np.where(played & (mv != M_PASS) & (mv != M_RESIGN), before, 0).astype(np.uint16)


def placed_from(n, moves, pp, move_to):
    """numpy restatement of the sample's rule: int64 [n*n], placed[point of move t] = max(place_ply[t]) over t < move_to"""
    mv, pp = np.asarray(moves[:move_to], np.int64), np.asarray(pp[:move_to], np.int64)
    tab = np.zeros(n * n, np.int64)
    on = pp != 0
    np.maximum.at(tab, action_of(n, mv[on]), pp[on])
    return tab


def replays(n, moves):
    """moves onto a point an earlier move of the game was played on (its stone has been captured since): -> (count, index t of the
    first one or -1, number of distinct such points, passes)"""
    seen, again, first = set(), [], -1
    for t, c in enumerate(moves):
        c = int(c)
        if c in (M_PASS, M_RESIGN, M_INVALID):
            continue
        if c in seen:
            again.append(c)
            if first < 0:
                first = t
        seen.add(c)
    return len(again), first, len(set(again)), int(sum(1 for c in moves if int(c) == M_PASS))


def refused_record_moves():
    """9x9, 32 entries: a legal opening, then among further legal moves a move onto an occupied point (index 5), M_INVALID
    (index 9), a second occupied point right behind a checkpoint boundary (index 17) and a pass (index 20).  The refused entries
    do not advance the ply, so every later placement carries a ply below its index + 1."""
    n = 9
    pts = [(x, y) for x in range(1, 8) for y in range(1, 8, 2)]          # never adjacent along y: no captures, no suicides
    legal = [coord(n, x, y) for x, y in pts]
    mv = legal[:5] + [legal[2]] + legal[5:8] + [M_INVALID] + legal[8:15] + [legal[0]] + legal[15:17] + [M_PASS] + legal[17:28]
    assert len(mv) == 32 and mv[5] == legal[2] and mv[9] == M_INVALID and mv[17] == legal[0] and mv[20] == M_PASS
    return n, np.asarray(mv, np.int64)
