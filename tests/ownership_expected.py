"""What elfgo_area_map / elfgo_own_run must return, computed on the CPU: a numpy restatement of the Tromp-Taylor area map and
the playout sums taken from an oracle engine (pyoracle.Ref or pyoracle.Port).  Integers only."""
import numpy as np

GOLDEN64 = 0x9E3779B97F4A7C15


def seed_of(seed, k):
    """seed(i, k) = seeds[i] + k * 0x9E3779B97F4A7C15 (mod 2^64)"""
    return (int(seed) + k * GOLDEN64) & 0xFFFFFFFFFFFFFFFF


def area_map(col, n):
    """col: stone colours uint8 [n*n] in action order (a = x*n + y; 0 empty, 1 black, 2 white) -> uint8 [n*n], 0 neutral,
    1 black area, 2 white area: simple_flood_fill per colour (a colour's stones spread through empty points) as a masked
    dilation to its fixed point, then black && !white / white && !black."""
    g = np.asarray(col).reshape(n, n)
    empty = g == 0

    def fill(c):
        r = g == c
        while True:
            d = r.copy()
            d[1:] |= r[:-1]
            d[:-1] |= r[1:]
            d[:, 1:] |= r[:, :-1]
            d[:, :-1] |= r[:, 1:]
            nr = r | (d & empty)
            if np.array_equal(nr, r):
                return r
            r = nr

    b, w = fill(1), fill(2)
    out = np.zeros((n, n), np.uint8)
    out[b & ~w] = 1
    out[w & ~b] = 2
    return out.reshape(-1)


def area_diff(am):
    return int((am == 1).sum()) - int((am == 2).sum())


def ended_by_superko(E, state):
    """GoState::evaluate answers +-1 whatever the komi exactly when the position repeats an earlier one"""
    return E.evaluate(state, 0.0) == E.evaluate(state, 1000.0)


def expected(E, state, seed, K, komi, max_steps=100000, ends=None):
    """counts int32 [2, n*n] and stats int64 [4] of K playouts from `state` (left untouched); `ends`, if a list, receives
    the end states (the caller frees them)"""
    n = E.n
    counts = np.zeros((2, n * n), np.int32)
    stats = np.zeros(4, np.int64)
    for k in range(K):
        c = E.clone(state)
        mv = E.playout_moves(c, seed_of(seed, k), max_steps)
        am = area_map(E.board(c)[0], n)
        counts[0] += am == 1
        counts[1] += am == 2
        diff = area_diff(am)
        stats[0] += diff
        stats[1] += int(np.float32(diff) - np.float32(komi) > 0)
        stats[2] += int(ended_by_superko(E, c))
        stats[3] += len(mv)
        if ends is not None:
            ends.append(c)
        else:
            E.free(c)
    return counts, stats


def prefix(E, seed, plies):
    """the position after `plies` plies of the config-2 policy from the empty board, and its moves"""
    s = E.new()
    mv = E.playout_moves(s, int(seed), plies)
    return s, [int(c) for c in mv]


def ko_moves(n):
    """five moves after which White faces a live simple ko in the corner: B (2,0) W (1,0) B (1,1) W (0,1) B (0,0) takes (1,0)"""
    return [(y + 1) * (n + 2) + (x + 1) for x, y in ((2, 0), (1, 0), (1, 1), (0, 1), (0, 0))]
