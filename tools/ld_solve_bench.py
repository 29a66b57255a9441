"""GPU: the exact life-and-death search beside the playout reader, in one process with the kernels alternating.

eng.ld_solve (k_ld_solve) at depths 4 / 6 / 8 beside eng.ld_read(playouts=256) (k_playout_ld), both at threshold 3, on
  corner_8x8       tools/ld_bench.py's rows: 16 19x19 positions at ply 120 of the seeded playouts, 8x8 corner boxes
  straight_three   16 copies of the straight three in the corner on 9x9, Black to move, box (0, 0, 5, 3)
Medians of 12 samples after a warm-up.  Per depth: time per call, nodes entered, nodes per second, nodes per row and the share of
first moves cut at max_nodes = 1 << 16.  Writes profiles/ld_solve_bench.json (or the path given as the first argument) and prints
the same JSON.  Not measured: other thresholds, other budgets, depths above 8."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import elf_amd

REPS, WARM = 12, 2
THRES, PLAYOUTS, BUDGET, DEPTHS = 3, 256, 1 << 16, (4, 6, 8)
STRAIGHT_THREE = ("...XO....", "XXXXO....", "OOOOO....")   # row = y, column = x, X Black, O White


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


def seeds_of(k):
    return torch.from_numpy((np.arange(k, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(1)).view(np.int64)).cuda()


def measure(eng, rows, box):
    seeds = seeds_of(rows)
    boxes = torch.tensor([box] * rows, dtype=torch.int32, device="cuda")   # on the device: no host work inside the timed window
    calls = dict(ld_read=lambda: eng.ld_read(seeds, regions=boxes, playouts=PLAYOUTS, self_atari_thres=THRES))
    for d in DEPTHS:
        calls["ld_solve_depth%d" % d] = lambda d=d: eng.ld_solve(n=rows, regions=boxes, max_depth=d, max_nodes=BUDGET, self_atari_thres=THRES)
    t, last = {k: [] for k in calls}, {}
    for rep in range(REPS + WARM):
        for k, fn in calls.items():
            dt, last[k] = timed(fn)
            if rep >= WARM:
                t[k].append(dt)
    res = dict(rows=rows, box=list(box), reps=REPS)
    ms = spread([x * 1e3 for x in t["ld_read"]])
    steps = int(last["ld_read"].stats[:, 5].sum())
    res["ld_read"] = dict(ms_per_call=ms, playouts=PLAYOUTS, steps=steps, steps_per_s=steps / (ms["median"] * 1e-3))
    for d in DEPTHS:
        k = "ld_solve_depth%d" % d
        ms = spread([x * 1e3 for x in t[k]])
        value, nodes = last[k].value.cpu().numpy(), last[k].nodes.cpu().numpy().astype(np.int64)
        first = int((value != -1).sum())
        res[k] = dict(ms_per_call=ms, nodes=int(nodes.sum()), nodes_per_s=int(nodes.sum()) / (ms["median"] * 1e-3),
                      nodes_per_row=int(nodes.sum()) / rows, first_moves=first, cut_share=float((value == -2).sum()) / max(first, 1),
                      rows_proved=int(sum(last[k].proved())), time_ratio_to_ld_read=ms["median"] / res["ld_read"]["ms_per_call"]["median"])
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ld_solve_bench.json")
    res = dict(device=torch.cuda.get_device_name(0), self_atari_thres=THRES, max_nodes=BUDGET, max_depth_limit=int(elf_amd.lib().elfgo_ld_solve_max_depth()))
    big = elf_amd.GoEngine(19, 16, 0)
    big.playout(seeds_of(16), max_steps=120)
    res["corner_8x8"] = measure(big, 16, (0, 0, 8, 8))
    big.close()
    n = 9
    stones = np.zeros((n, n), np.uint8)   # [x, y]
    for y, row in enumerate(STRAIGHT_THREE):
        for x, ch in enumerate(row):
            stones[x, y] = 1 if ch == "X" else 2 if ch == "O" else 0
    small = elf_amd.GoEngine(n, 16, 0)
    small.setup(np.tile(stones.reshape(1, -1), (16, 1)), next_player=[1] * 16)
    res["straight_three"] = measure(small, 16, (0, 0, 5, 3))
    small.close()
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
