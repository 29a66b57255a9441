"""Benson's unconditional life over sets of points, as include/elf_amd.h states it for elfgo_pass_alive, and the constructed 9x9
positions of tests/test_gpu_pass_alive.py with their maps stated by hand.  Plain Python; not a test module."""
import numpy as np


def _nbrs(n, a):
    return [bx * n + by for bx, by in ((a // n - 1, a % n), (a // n + 1, a % n), (a // n, a % n - 1), (a // n, a % n + 1)) if 0 <= bx < n and 0 <= by < n]


def _components(n, members):
    """the 4-connected components of a set of points, breadth first -> list of sets"""
    left, out = set(members), []
    while left:
        comp, queue = set(), [left.pop()]
        while queue:
            a = queue.pop(0)
            comp.add(a)
            for b in _nbrs(n, a):
                if b in left:
                    left.discard(b)
                    queue.append(b)
        out.append(comp)
    return out


def pass_alive(n, colours):
    """colours: N*N values 0 / 1 / 2 in export_board's order (a = x*N + y) -> (map uint8 [N*N], summary int32 [8])"""
    col = [int(v) for v in colours]
    out, summary = np.zeros(n * n, np.uint8), []
    for c in (1, 2):
        chains = _components(n, [a for a in range(n * n) if col[a] == c])
        regions = _components(n, [a for a in range(n * n) if col[a] != c])
        touches = lambda pts, chain: {a for a in pts if any(b in chain for b in _nbrs(n, a))}
        borders = [[bool(touches(r, ch)) for ch in chains] for r in regions]
        empties = [{a for a in r if col[a] == 0} for r in regions]
        vital = [[bool(e) and touches(e, ch) == e for ch in chains] for e in empties]
        cs, rs, rounds = set(range(len(chains))), set(range(len(regions))), 0
        while True:
            rounds += 1
            cs2 = {i for i in cs if sum(1 for j in rs if vital[j][i]) >= 2}
            rs2 = {j for j in rs if not any(borders[j][i] for i in range(len(chains)) if i not in cs2)}
            changed, cs, rs = (cs2, rs2) != (cs, rs), cs2, rs2
            if not changed:
                break
        safe = [j for j in rs if any(vital[j][i] for i in cs)]
        for i in cs:
            out[list(chains[i])] |= 1 << (c - 1)
        for j in safe:
            out[list(regions[j])] |= 4 << (c - 1)
        summary += [len(cs), sum(len(chains[i]) for i in cs), sum(len(regions[j]) for j in safe), rounds]
    return out, np.array(summary, np.int32)


# Row = y, column = x.  Board: X Black, O White.  Black's answer, stated by hand: A a pass-alive stone, s a safe point; White has
# nothing in any of them.  Rows that are left out are empty.  Last: Black's chains, stones, safe points and rounds, White's rounds.
POSITIONS = {
    # a corner group with two one-point eyes
    "two_eyes": ([".X.X", "XXXX"], ["sAsA", "AAAA"], (1, 6, 2, 1), 1),
    # the same with one eye filled by its owner
    "one_eye": (["XX.X", "XXXX"], [], (0, 0, 0, 2), 1),
    # two chains, (1,0) (2,0) (2,1) and (0,1) (0,2) (1,2), that share the eyes (0,0) and (1,1)
    "shared_eyes": ([".XX", "X.X", "XX."], ["sAA", "AsA", "AA."], (2, 6, 2, 1), 1),
    # walls A (x = 1), B (x = 3) and the block D (x >= 5).  A: column 0 and column 2.  B: column 2 and column 4 with the White
    # stone; (4,4) does not touch D, so that region is not vital to D, whose one eye is (8,0).  D goes, then column 4, then B, then
    # column 2, then A: four rounds, the last one idle
    "cascade": ([".X.X.XXX.", ".X.X.XXXX", ".X.X.XXXX", ".X.X.XXXX", ".X.X.OXXX", ".X.X.XXXX", ".X.X.XXXX", ".X.X.XXXX", ".X.X.XXXX"],
                [], (0, 0, 0, 4), 2),
    # the eye (0,0) (1,0) holds a White stone; its one empty point touches the chain
    "stone_in_eye": ([".OX.X", "XXXXX"], ["ssAsA", "AAAAA"], (1, 7, 3, 1), 2),
    # a 2x2 corner eye whose corner point does not touch the chain, and one real eye
    "big_eye": (["..X.X", "..XXX", "XXX.."], [], (0, 0, 0, 2), 1),
    "empty": ([], [], (0, 0, 0, 1), 1),
    "one_colour": (["....", ".X..", "...X", "..X."], [], (0, 0, 0, 2), 1),
}


def constructed(n, name, d4, swap):
    """-> (stones uint8 [N*N], map uint8 [N*N], summary int32 [8]) of a position under a D4 code and, swap, with colours exchanged"""
    from elf_amd.engine import d4_transform
    rows, marks, black, white_rounds = POSITIONS[name]
    stones, exp = np.zeros(n * n, np.uint8), np.zeros(n * n, np.uint8)
    for src, dst, code in ((rows, stones, {"X": 1, "O": 2}), (marks, exp, {"A": 1, "s": 4})):
        for y, line in enumerate(src):
            for x, ch in enumerate(line):
                tx, ty = d4_transform(n, d4, x, y)
                dst[tx * n + ty] = code.get(ch, 0)
    summary = np.array(list(black) + [0, 0, 0, white_rounds], np.int32)
    if swap:
        stones = np.array([0, 2, 1], np.uint8)[stones]
        exp = (exp << 1).astype(np.uint8)
        summary = np.concatenate([summary[4:], summary[:4]])
    return stones, exp, summary
