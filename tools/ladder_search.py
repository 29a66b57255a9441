#!/usr/bin/env python3
"""Finds board layouts on which the reference's ladder search works hard, for tests/golden/ladder_constructed.npz.

    python tools/ladder_search.py climb  --n 19 --seed 1 --seconds 330 --out run1.npz
    python tools/ladder_search.py climb  --n 19 --seed 1 --seconds 300 --resume run1.npz --out run1b.npz
    python tools/ladder_search.py select --runs run1b.npz run2.npz ... --budget S19 S9 [--out tests/golden/ladder_constructed.npz]

The committed fixture: seeds 1 to 5 for 330 s each at 19x19, seeds 1, 2 and 5 resumed for 300 s, seeds 2 and 5 resumed again for
300 s and seed 6 started from seed 5's second file for 300 s (3450 s in all; num_call passed 1024 in the third round); seeds 1
and 2 for 150 s at 9x9, seed 2 resumed for 200 s (500 s).  A climb ends on the clock, so another machine finds other layouts.

climb:  a seeded, time-boxed hill-climb on the CPU.  It starts from random stones, toggles 1 to 3 random points per step and
        keeps a layout whose (largest num_call, largest depth) over all points does not get worse; every layout it accepts with
        a large num_call goes into the run's archive.  Black is the side to move.  Expected values come from the reference's own
        reader through oracle/_ref (tests/ladder_expected.py); nothing else is read.
select: counts, with the restated kernel loop (tests/ladder_restated.py), the device plays and the open forks of every archived
        layout and writes the layouts with the largest num_call, the most plays, the most open forks and the answers that
        differ most between the board's symmetries: stones and movers only.

The tests read the fixture and never run this tool."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ladder_expected as LE          # noqa: E402
import ladder_positions as LP         # noqa: E402
import ladder_restated as LR          # noqa: E402


def score(lad, stones, objective="calls"):
    """-> (largest num_call, largest depth) for Black to move, None if the stones cannot stand.  Objective "work" puts their
    product in front: a stand-in for the device plays, which grow with the nodes and with the length of the lines replayed"""
    h = LP.build(lad.RB, stones, LP.BLACK)
    if h is None:
        return None
    d, c = lad.expected(h)
    lad.RB.free(h)
    sc = int(c.max()), int(d.max())
    return (sc[0] * sc[1],) + sc if objective == "work" else sc


def climb(a):
    n = a.n
    lad = LE.Ladder(n)
    rng = np.random.RandomState(a.seed)
    start = a.stones if a.stones else (80 if n == 19 else 24)
    keep_from = a.keep_from if a.keep_from else (60 if n == 19 else 12)
    cur = best = None
    spent = 0
    if a.resume:                          # go on from the best layout of an earlier run; its budget is added to this one's
        with np.load(a.resume) as f:
            assert int(f["n"]) == n
            cur, spent = f["stones"][0].copy(), int(f["seconds"])
        best = score(lad, cur, a.objective)
    while cur is None:
        st = np.zeros(n * n, np.uint8)
        st[rng.choice(n * n, start, replace=False)] = rng.randint(1, 3, start)
        best = score(lad, st, a.objective)
        cur = st if best is not None else None
    archive, t0, steps = {}, time.time(), 0
    while time.time() - t0 < a.seconds:
        steps += 1
        st = cur.copy()
        for p in rng.choice(n * n, rng.randint(1, 4), replace=False):
            st[p] = rng.randint(1, 3) if st[p] == 0 else 0
        sc = score(lad, st, a.objective)
        if sc is None or sc < best:
            continue
        cur, best = st, sc
        if sc[-2] >= keep_from:
            archive[st.tobytes()] = sc
            if len(archive) > 50 * a.archive:
                archive = {k: archive[k] for k in sorted(archive, key=lambda k: archive[k], reverse=True)[:a.archive]}
    print("seed %d, %dx%d: %d steps in %.0f s, best (..., num_call, depth) = %s, %d layouts archived"
          % (a.seed, n, n, steps, time.time() - t0, best, len(archive)))
    keys = sorted(archive, key=lambda k: archive[k], reverse=True)[:a.archive]
    np.savez_compressed(a.out, n=n, seed=a.seed, seconds=int(a.seconds) + spent, steps=steps,
                        stones=np.array([np.frombuffer(k, np.uint8) for k in keys]).reshape(-1, n * n))


def measure(lad, rs, stones):
    h = LP.build(lad.RB, stones, LP.BLACK)
    d, c = lad.expected(h)
    rd, rc, res = rs.maps(h)
    lad.RB.free(h)
    assert np.array_equal(d, rd) and np.array_equal(c, rc), "the restated loop disagrees with the reference"
    # the reference's answer is not symmetric: how many different largest depths / num_calls the 8 board symmetries give
    sd, sc = set(), set()
    for s in range(8):
        h = LP.build(lad.RB, LP.sym(lad.n, stones, s), LP.BLACK)
        di, ci = lad.expected(h)
        lad.RB.free(h)
        sd.add(int(di.max()))
        sc.add(int(ci.max()))
    return dict(calls=int(c.max()), depth=int(d.max()), plays=max(r.plays for _, r in res), forks=max(r.forks for _, r in res),
                longest=max(r.longest for _, r in res), asym=min(len(sd), len(sc)))


def select(a):
    out, budget = {}, {}
    for n in (19, 9):
        lad = LE.Ladder(n)
        rs = LR.Restated(lad.RB, stack=1 << 20, max_plays=1 << 30)      # count past the kernel's bounds: the tests judge them
        rows = []
        for path in a.runs:
            with np.load(path) as f:
                if int(f["n"]) != n:
                    continue
                budget[n] = budget.get(n, 0) + int(f["seconds"])
                for st in f["stones"][:a.per_run]:
                    rows.append((int(f["seed"]), st.copy(), measure(lad, rs, st)))
        chosen = []
        for key in ("calls", "plays", "forks", "asym"):
            for row in sorted(rows, key=lambda r: (r[2][key], r[2]["calls"]), reverse=True):
                if len([1 for c in chosen if c[3] == key]) == a.each:
                    break
                # one layout per climb: the layouts of one seed are neighbours of each other
                if any(c[0] == row[0] for c in chosen):
                    continue
                chosen.append(row + (key,))
        for i, (seed, st, m, key) in enumerate(chosen):
            print("%dx%d searched_seed%d (chosen for %s): %s" % (n, n, seed, key, m))
        out["names%d" % n] = np.array(["searched_seed%d" % seed for seed, _, _, _ in chosen])
        out["stones%d" % n] = np.array([c[1] for c in chosen], np.uint8).reshape(-1, n * n)
        out["mover%d" % n] = np.full(len(chosen), LP.BLACK, np.uint8)
        out["budget_seconds%d" % n] = np.int32(a.budget[n == 9] if a.budget else budget.get(n, 0))
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("climb")
    c.add_argument("--n", type=int, default=19, choices=(19, 9))
    c.add_argument("--seed", type=int, default=1)
    c.add_argument("--seconds", type=float, default=330)
    c.add_argument("--stones", type=int, default=0, help="stones of the random start (0: 80 at 19x19, 24 at 9x9)")
    c.add_argument("--keep-from", type=int, default=0, help="archive accepted layouts from this num_call on")
    c.add_argument("--archive", type=int, default=400, help="layouts kept in the run's file")
    c.add_argument("--objective", default="calls", choices=("calls", "work"), help="what the climb keeps from getting worse")
    c.add_argument("--resume", help="a run's file: start from its best layout instead of random stones")
    c.add_argument("--out", required=True)
    s = sub.add_parser("select")
    s.add_argument("--runs", nargs="+", required=True)
    s.add_argument("--per-run", type=int, default=60, help="layouts measured per run, best first")
    s.add_argument("--each", type=int, default=2, help="layouts kept per criterion and board size")
    s.add_argument("--budget", type=int, nargs=2, metavar=("S19", "S9"),
                   help="seconds of search behind the runs (default: the sum over the files, which counts a resumed run's start twice)")
    s.add_argument("--out", default=LP.FIXTURE)
    a = ap.parse_args()
    assert LE.RefBoard.available(19) and LE.RefBoard.available(9), "oracle/_ref has to be built first"
    (climb if a.cmd == "climb" else select)(a)


if __name__ == "__main__":
    main()
