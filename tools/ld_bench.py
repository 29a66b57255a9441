"""GPU: the life-and-death reader beside the ownership playouts it shares a harness with, and the region lists beside the
whole-board list, in one process with the kernels alternating.

eng.ld_read (k_playout_ld) and eng.ownership(self_atari_thres=3) (k_playout_own<CandPolicy>) on 16 19x19 positions at ply 120 of
the seeded playouts x 256 playouts, in three settings:
  whole_board   the box is the whole board: both kernels play the same games, so the ratio is the cost of the box, the two verdicts
                and the counters
  corner_8x8    8x8 corner boxes: the reader's own workload (short local fights); ownership still plays whole games
  rows_4096     4096 rows x 1 playout (8x8 corner boxes for the reader)
and eng.region_moves beside eng.candidates on 4096 boards at ply 150 (a sample there is INNER back-to-back calls).  Medians of 12
samples after a warm-up.  Writes profiles/ld_bench.json (or the path given as the first argument) and prints the same JSON.
Not measured: 9x9, thresholds other than 3, max_lanes other than the default."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import elf_amd

REPS, WARM, INNER = 12, 2, 20
N, THRES = 19, 3


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner, r


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def seeds_of(k):
    return torch.from_numpy((np.arange(k, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(1)).view(np.int64)).cuda()


def alternate(calls, inner=1):
    """calls: name -> fn; -> (name -> list of seconds per call, name -> last result)"""
    t, last = {k: [] for k in calls}, {}
    for rep in range(REPS + WARM):
        for k, fn in calls.items():
            dt, last[k] = timed(fn, inner)
            if rep >= WARM:
                t[k].append(dt)
    return t, last


def playouts(eng, rows, K, box):
    seeds = seeds_of(rows)
    boxes = torch.tensor([box] * rows, dtype=torch.int32, device="cuda")   # on the device: no host work inside the timed window
    t, last = alternate(dict(ownership=lambda: eng.ownership(seeds, playouts=K, self_atari_thres=THRES),
                             ld_read=lambda: eng.ld_read(seeds, regions=boxes, playouts=K, self_atari_thres=THRES)))
    res = dict(rows=rows, playouts=K, box=list(box), reps=REPS)
    steps = dict(ownership=int(last["ownership"]["stats"][:, 3].sum()), ld_read=int(last["ld_read"].stats[:, 5].sum()))
    for k in t:
        s = spread([x * 1e3 for x in t[k]])
        res[k] = dict(ms_per_call=s, steps=steps[k], steps_per_s=steps[k] / (s["median"] * 1e-3), playouts_per_s=rows * K / (s["median"] * 1e-3))
    res["ld_read"]["time_ratio_to_ownership"] = res["ld_read"]["ms_per_call"]["median"] / res["ownership"]["ms_per_call"]["median"]
    res["ld_read"]["steps_per_s_ratio_to_ownership"] = res["ld_read"]["steps_per_s"] / res["ownership"]["steps_per_s"]
    res["ld_read"]["lived"] = int(last["ld_read"].stats[:, 0].sum())
    res["ld_read"]["survived"] = int(last["ld_read"].stats[:, 1].sum())
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ld_bench.json")
    res = dict(device=torch.cuda.get_device_name(0), self_atari_thres=THRES)
    eng = elf_amd.GoEngine(N, 4096, 0)
    eng.playout(seeds_of(4096), max_steps=120)
    res["mean_ply"] = float(eng.info()[:, 0].to(torch.float64).mean())
    small = elf_amd.GoEngine(N, 16, 0)
    small.setup(eng.export_board(n=16)[0], next_player=eng.info(n=16)[:, 1].to(torch.uint8))   # the stones of the first 16 boards
    res["whole_board"] = playouts(small, 16, 256, (0, 0, N, N))
    res["corner_8x8"] = playouts(small, 16, 256, (0, 0, 8, 8))
    small.close()
    res["rows_4096"] = playouts(eng, 4096, 1, (0, 0, 8, 8))
    # the lists, on the same pool played on to ply 150
    eng.playout(seeds_of(4096), max_steps=30)
    boxes = torch.tensor([(0, 0, 8, 8)] * 4096, dtype=torch.int32, device="cuda")
    t, _ = alternate(dict(candidates=lambda: eng.candidates(self_atari_thres=THRES),
                          region_moves_whole=lambda: eng.region_moves(self_atari_thres=THRES),
                          region_moves_8x8=lambda: eng.region_moves(regions=boxes, self_atari_thres=THRES)), INNER)
    lists = dict(boards=4096, reps=REPS, calls_per_sample=INNER, mean_ply=float(eng.info()[:, 0].to(torch.float64).mean()))
    for k in t:
        s = spread([x * 1e6 for x in t[k]])
        lists[k] = dict(us_per_call=s, boards_per_s=4096 / (s["median"] * 1e-6))
    for k in ("region_moves_whole", "region_moves_8x8"):
        lists[k]["ratio_to_candidates"] = lists[k]["us_per_call"]["median"] / lists["candidates"]["us_per_call"]["median"]
    res["lists"] = lists
    eng.close()
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
