"""GPU: time of GoEngine.ladder_map on mid-game positions, beside legal_mask on the same boards and the reference's own reader.

Positions are taken the way tools/ownership_bench.py takes its rows: config-2 playouts from the empty board, cut at a mid-game
ply (19x19: 4096 boards at ply 120; 9x9: 65 536 boards at ply 40).  Per size: time per ladder_map call (device events, after a
warm-up), boards/s, points searched per board, total num_call, and in the same process the time of legal_mask on the same boards
as a yardstick.  Where oracle/_ref's board library is present, the first REF_BOARDS positions are rebuilt on it from the
oracle's move lists and the reference's maps are timed through ctypes: that figure INCLUDES one Python call per point (TryPlay2,
checkLadder, and a clone + play + search where a search runs) and is labelled so; the device maps of those boards are checked
against it.  Writes profiles/ladder_bench.json (or the path given as the first argument) and prints the same JSON."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import elf_amd
from pyoracle import Port, RefBoard, playout_seeds

REPS, REF_BOARDS = 24, 64
SIZES = ((19, 4096, 120), (9, 65536, 40))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, r


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def one_size(n, boards, ply):
    eng = elf_amd.GoEngine(n, boards, 0)
    seeds = playout_seeds(boards)
    eng.playout(seeds, max_steps=ply)
    lad, leg = [], []
    for rep in range(REPS + 3):
        dt_l, (depth, calls) = timed(lambda: eng.ladder_map(with_calls=True))
        dt_m, _ = timed(lambda: eng.legal_mask())
        if rep >= 3:
            lad.append(dt_l * 1e3)
            leg.append(dt_m * 1e3)
    depth, calls = depth.cpu().numpy(), calls.cpu().numpy()
    res = dict(boards=boards, ply=ply, reps=REPS, ladder_map_ms_per_call=spread(lad), legal_mask_ms_per_call=spread(leg),
               boards_per_s=boards / (spread(lad)["median"] * 1e-3),
               ladder_over_legal_mask=spread(lad)["median"] / spread(leg)["median"],
               points_searched_per_board=float((calls != 0).sum()) / boards, total_calls=int(calls[calls > 0].sum()),
               largest_calls=int(calls.max()), overflowed_points=int((calls == -1).sum()),
               nonzero_points=int((depth > 0).sum()), largest_depth=int(depth.max()))
    if RefBoard.available(n):
        import ladder_expected as LE
        ref = LE.Ladder(n)
        port = Port(n)
        hs = []
        for sd in seeds[:REF_BOARDS]:
            s = port.new()
            h = ref.RB.new()
            for m in port.playout_moves(s, int(sd), ply):
                assert ref.RB.play(h, int(m)) == 1
            port.free(s)
            hs.append(h)
        t0 = time.perf_counter()
        want = [ref.expected(h) for h in hs]
        dt = time.perf_counter() - t0
        for h in hs:
            ref.RB.free(h)
        for j, (wd, wc) in enumerate(want):
            assert np.array_equal(depth[j], wd) and np.array_equal(calls[j], wc), (n, j)
        res["reference_ctypes"] = dict(boards=REF_BOARDS, ms_per_board=dt * 1e3 / REF_BOARDS, boards_per_s=REF_BOARDS / dt,
                                       note="includes one Python/ctypes call per point; not the reference's native speed")
    eng.close()
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ladder_bench.json")
    res = {"%dx%d" % (n, n): one_size(n, boards, ply) for n, boards, ply in SIZES}
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
