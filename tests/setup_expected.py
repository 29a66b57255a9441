"""What elfgo_setup must build from a stones row, computed on the CPU, and the positions the setup tests use.

restate() is a numpy / Python restatement (flood fill + XOR of Zobrist words); test_setup_cpu.py pins it on the reference's own
board engine (pyoracle.RefBoard), and the GPU tests take their positions -- and what every field must be -- from RefBoard.replay."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ZOBRIST = os.path.join(os.path.dirname(HERE), "elf_amd", "data", "zobrist21.bin")
GOLDEN = os.path.join(HERE, "golden")
M64 = 0xFFFFFFFFFFFFFFFF

_zob = None


def zobrist():
    global _zob
    if _zob is None:
        _zob = np.fromfile(ZOBRIST, dtype="<u8")
        assert _zob.size == 441
    return _zob


def swap_halves(h):
    h = int(h)
    return ((h >> 32) | ((h & 0xFFFFFFFF) << 32)) & M64


def restate(colour, n=None):
    """colour uint8 [n*n] in action order (a = x*n + y; 0 empty, 1 black, 2 white) -> (liberties of the group on every point
    int16 [n*n] (0 on empty points), Zobrist hash of the stones (words indexed by the reference Coord (y+1)*(n+2) + (x+1); a
    white stone's word has its 32-bit halves swapped), whether some group has no liberty)"""
    colour = np.asarray(colour)
    if n is None:
        n = int(round(colour.size ** 0.5))
    z = zobrist()
    c = colour.reshape(n, n)
    seen = np.zeros((n, n), bool)
    libs = np.zeros((n, n), np.int16)
    h, zero = 0, False
    for x in range(n):
        for y in range(n):
            s = int(c[x, y])
            if not s:
                continue
            w = int(z[(y + 1) * (n + 2) + (x + 1)])
            h ^= w if s == 1 else swap_halves(w)
            if seen[x, y]:
                continue
            seen[x, y] = True
            stack, group, lb = [(x, y)], [], set()
            while stack:
                px, py = stack.pop()
                group.append((px, py))
                for qx, qy in ((px - 1, py), (px + 1, py), (px, py - 1), (px, py + 1)):
                    if 0 <= qx < n and 0 <= qy < n:
                        if c[qx, qy] == 0:
                            lb.add((qx, qy))
                        elif c[qx, qy] == s and not seen[qx, qy]:
                            seen[qx, qy] = True
                            stack.append((qx, qy))
            zero = zero or not lb
            for p in group:
                libs[p] = len(lb)
    return libs.reshape(-1), h, zero


def ko_pending(info):
    """rows of RefBoard info [k, 10] -> bool [k]: a simple ko is live (a point is recorded and its age is 0)"""
    return (info[:, 5] != 0) & (info[:, 4] == 0)


def first_no_ko(pend, t):
    """the first ply >= t with no simple ko pending, None if it would lie past the game's end"""
    while t < len(pend) and pend[t]:
        t += 1
    return t if t < len(pend) else None


def chosen_plies(rep, step=10):
    """every step-th ply (t = step, 2 step, ... <= number of moves), moved forward to the next one with no ko pending;
    -> (plies, how many were moved, number of positions with a ko pending)"""
    pend = ko_pending(rep["info"])
    out, moved = [], 0
    for t in range(step, len(pend), step):
        u = first_no_ko(pend, t)
        if u is None:
            continue
        moved += u != t
        out.append(u)
    return out, moved, int(pend.sum())


def ladder_games():
    g = np.load(os.path.join(GOLDEN, "ladder_suite.npz"))
    return [g["moves"][g["offsets"][i]:g["offsets"][i + 1]].astype(np.int32) for i in range(len(g["offsets"]) - 1)]


def nine_games(E, count=64):
    """move lists of `count` seeded config-2 playouts on 9x9 from oracle engine E (pyoracle.Port / Ref)"""
    from ownership_expected import prefix
    from pyoracle import playout_seeds
    games = []
    for sd in playout_seeds(count):
        s, mv = prefix(E, int(sd), 1 << 20)
        E.free(s)
        games.append(np.asarray(mv, np.int32))
    return games


def cases(RB, games):
    """-> list of (game index, ply, RefBoard.replay dict of that game) for the chosen plies of every game, and the counters
    (positions, ko pending, chosen, moved)"""
    out, positions, ko, moved = [], 0, 0, 0
    for gi, mv in enumerate(games):
        rep = RB.replay(mv)
        assert rep["ok"].all()
        plies, m, k = chosen_plies(rep)
        positions += len(mv) + 1
        ko += k
        moved += m
        out += [(gi, u, rep) for u in plies]
    return out, dict(positions=positions, ko=ko, chosen=len(out), moved=moved)
