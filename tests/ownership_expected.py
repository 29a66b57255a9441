"""What elfgo_area_map / elfgo_own_run must return, computed on the CPU: a numpy restatement of the Tromp-Taylor area map and
the playout sums taken from an oracle engine (pyoracle.Ref or pyoracle.Port); for the edge battery, constructed shapes, a second
area map by component labelling, the trip count of the kernel's fill loop and the rows both test files share.  Integers only."""
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


# ---- the edge battery: constructed shapes, a second area map, the kernel's trip count, shared rows ---------------------------------
def oracle(n):
    from pyoracle import Port, Ref
    return Ref(n) if Ref.available(n) else Port(n)


def play_all(eng, move_lists):
    """slot i <- move_lists[i] from the empty board, one ply of every slot per launch"""
    for t in range(max(len(m) for m in move_lists)):
        live = [i for i, m in enumerate(move_lists) if t < len(m)]
        ok = eng.forward(live, [int(move_lists[i][t]) for i in live]).cpu().numpy()
        assert (ok == 1).all()


def states_of(E, move_lists):
    out = []
    for mv in move_lists:
        s = E.new()
        for c in mv:
            assert E.forward(s, int(c)) == 1
        out.append(s)
    return out


def mixed_rows(E, n):
    """empty board, mid game, late game, a live simple ko, a finished game"""
    from pyoracle import playout_seeds
    sd = playout_seeds(3, base=31)
    early, late = (20, 60) if n == 9 else (60, 300)
    lists = [[], prefix(E, sd[0], early)[1], prefix(E, sd[1], late)[1], ko_moves(n), prefix(E, sd[2], 100000)[1]]
    return lists


def area_test_lists(E, n, plies):
    """the move lists of test_gpu_ownership.test_area_map: the empty board, config-2 prefixes of four seeds and, at 19x19, every
    10th ply of one ladder-suite game"""
    import os
    from pyoracle import playout_seeds
    lists = [[]] + [prefix(E, sd, pl)[1] for sd in playout_seeds(4) for pl in plies]
    if n == 19:
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ladder_suite.npz"))
        game = [int(c) for c in g["moves"][g["offsets"][0]:g["offsets"][1]]]
        lists += [game[:t] for t in range(10, len(game) + 1, 10)]
    return lists


def _neighbours(a, n):
    x, y = divmod(a, n)
    if x > 0:
        yield a - n
    if x < n - 1:
        yield a + n
    if y > 0:
        yield a - 1
    if y < n - 1:
        yield a + 1


def area_map_bfs(col, n):
    """The Tromp-Taylor map a second way: the connected components of the empty points, each labelled with an explicit queue; a
    component belongs to a colour iff stones of exactly that colour border it; a stone is its own colour's."""
    from collections import deque
    col = np.asarray(col).reshape(-1)
    out = col.astype(np.uint8).copy()
    seen = np.zeros(n * n, bool)
    for a0 in range(n * n):
        if col[a0] != 0 or seen[a0]:
            continue
        comp, border, queue = [], set(), deque([a0])
        seen[a0] = True
        while queue:
            a = queue.popleft()
            comp.append(a)
            for b in _neighbours(a, n):
                if col[b] != 0:
                    border.add(int(col[b]))
                elif not seen[b]:
                    seen[b] = True
                    queue.append(b)
        out[comp] = border.pop() if len(border) == 1 else 0
    return out


def groups_have_liberties(col, n):
    """every connected group of stones touches an empty point"""
    col = np.asarray(col).reshape(-1)
    seen = np.zeros(n * n, bool)
    for a0 in range(n * n):
        if col[a0] == 0 or seen[a0]:
            continue
        stack, free = [a0], False
        seen[a0] = True
        while stack:
            a = stack.pop()
            for b in _neighbours(a, n):
                if col[b] == 0:
                    free = True
                elif col[b] == col[a0] and not seen[b]:
                    seen[b] = True
                    stack.append(b)
        if not free:
            return False
    return True


def word_rows(n):
    """the rows x whose n points [x*n, x*n + n) straddle a 64-bit word of the action-order bitboard"""
    return [x for x in range(n) if (x * n) // 64 != (x * n + n - 1) // 64]


def shapes(n):
    """Named constructed positions, colour arrays uint8 [n*n] with a = x*n + y (g[x, y] below); every group has a liberty.  The
    long fills end neutral by necessity: a colour that has to travel far travels between the other colour's walls."""
    def swap(g):
        return np.where(g == 0, 0, 3 - g).astype(np.uint8)

    out = {}
    g = np.zeros((n, n), np.uint8)
    out["empty"] = g.copy()
    g[0, 0] = 1
    out["black_corner"] = g.copy()
    g[:] = 0
    g[n // 2, n // 2] = 2
    out["white_centre"] = g.copy()
    # snake: every odd row full of black but for a gap at alternating ends; White at the head of the corridor
    g[:] = 0
    for i, x in enumerate(range(1, n, 2)):
        g[x, :] = 1
        g[x, n - 1 if i % 2 == 0 else 0] = 0
    g[0, 0] = 2
    out["snake"] = g.copy()
    out["snake_T"] = g.T.copy()
    out["snake_swapped"] = swap(g)
    out["snake_T_swapped"] = swap(g.T)
    # spiral: a one-wide corridor wound inwards from (0, 0) between one-wide black walls, White at its mouth
    g[:] = 1
    x, y, dx, dy = 0, 0, 0, 1
    g[0, 0] = 0
    while True:
        for _ in range(4):
            x2, y2 = x + 2 * dx, y + 2 * dy
            if 0 <= x + dx < n and 0 <= y + dy < n and not (0 <= x2 < n and 0 <= y2 < n and g[x2, y2] == 0):
                break
            dx, dy = dy, -dx
        else:
            break
        x, y = x + dx, y + dy
        g[x, y] = 0
    g[0, 0] = 2
    out["spiral"] = g.copy()
    out["spiral_T"] = g.T.copy()
    # comb: black teeth on even y, open along x = 0; the same with a white stone at the bottom of the first gap
    g[:] = 0
    g[1:, 0::2] = 1
    out["comb"] = g.copy()
    g[n - 1, 1] = 2
    out["comb_white"] = g.copy()
    out["comb_white_T"] = g.T.copy()
    # two halves and a dame line that both colours reach
    g[:] = 0
    g[:n // 2] = 1
    g[n // 2 + 1:] = 2
    out["dame_x"] = g.copy()
    out["dame_y"] = g.T.copy()
    g[:] = 1
    g[n - 1, n - 1] = 0
    out["full_but_one"] = g.copy()
    g[:] = 0
    g[0, :] = 1
    g[:, 0] = 1
    g[n - 1, 1:] = 2
    g[1:, n - 1] = 2
    out["borders"] = g.copy()
    for x in word_rows(n)[:2]:
        g[:] = 0
        g[x, 0::3] = 1
        g[x, 2::3] = 2
        out["word_row%d" % x] = g.copy()
    return {k: v.reshape(-1) for k, v in out.items()}


def kernel_trips(col, n):
    """How many trips area_rows' loop makes on this position: one vertical exchange plus five in-row steps per trip, counted up to
    and including the trip that changes nothing.  Says how hard a position is; never an expected value."""
    g = np.asarray(col).reshape(n, n)
    empty = g == 0

    def inrow(r):
        d = np.zeros_like(r)
        d[:, 1:] |= r[:, :-1]
        d[:, :-1] |= r[:, 1:]
        return d

    rb, rw = g == 1, g == 2
    trips = 0
    while True:
        trips += 1
        new = []
        for r in (rb, rw):
            d = inrow(r)
            d[1:] |= r[:-1]
            d[:-1] |= r[1:]
            nr = r | (d & empty)
            for _ in range(5):
                nr = nr | (inrow(nr) & empty)
            new.append(nr)
        same = np.array_equal(new[0], rb) and np.array_equal(new[1], rw)
        rb, rw = new
        if same:
            return trips


def moves_for(col, n):
    """A move list (reference Coords) that builds `col` from the empty board: the black stones and the white stones in action
    order, taken in turn, and the side that has run out passes.  Two passes in a row never occur; a pass as the last move is
    dropped."""
    g = np.asarray(col).reshape(n, n)
    pts = [[(y + 1) * (n + 2) + (x + 1) for x in range(n) for y in range(n) if g[x, y] == c] for c in (1, 2)]
    mv = []
    for t in range(2 * max(len(pts[0]), len(pts[1]))):
        side, i = t % 2, t // 2
        mv.append(pts[side][i] if i < len(pts[side]) else 0)
    while mv and mv[-1] == 0:
        mv.pop()
    return mv


def replay(E, moves):
    """the oracle state after `moves`, every one of them accepted"""
    s = E.new()
    for c in moves:
        assert E.forward(s, int(c)) == 1, c
    return s


# the rows that the CPU tests qualify and the GPU tests run, 9x9
STEP_ROW = dict(prefix=(12345, 30), seed=777, K=16, max_steps=60)
TIE_ROW = dict(prefix=(12345, 30), seed=4242, K=64)
# the geometry sweep: seven rows over the slots of mixed_rows (late game and mid game twice, each time with another seed)
GEOMETRY_IDS = [0, 1, 2, 3, 4, 2, 1]
GEOMETRY_K = (1, 2, 3, 5, 6, 7, 9)
GEOMETRY_LANES = (1, 8, 12, 0)


def geometry_seeds(rows=len(GEOMETRY_IDS)):
    from pyoracle import playout_seeds
    return playout_seeds(rows, base=2000)


def row_source(E, row):
    return prefix(E, *row["prefix"])


def playout_diffs(E, state, seed, K, max_steps=100000):
    """area difference and move count of each of the K playouts of a row"""
    out = []
    for k in range(K):
        c = E.clone(state)
        mv = E.playout_moves(c, seed_of(seed, k), max_steps)
        out.append((area_diff(area_map(E.board(c)[0], E.n)), len(mv)))
        E.free(c)
    return out


def superko_source(E, limit=256):
    """The first playout among the mixed rows' mid- and late-game sources (row seed 1000 + row) that ends on a super-ko repeat:
    the whole game's moves from the empty board."""
    lists = mixed_rows(E, E.n)
    for r in (2, 1):
        for k in range(limit):
            s = replay(E, lists[r])
            mv = E.playout_moves(s, seed_of(1000 + r, k))
            hit = ended_by_superko(E, s)
            E.free(s)
            if hit:
                return [int(c) for c in lists[r]] + [int(c) for c in mv]
    raise AssertionError("no playout ended by super-ko")
