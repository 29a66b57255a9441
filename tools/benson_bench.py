"""GPU: Benson's pass-alive reading beside the two per-point status maps the engine already had, in one process.

eng.pass_alive (k_pass_alive), eng.life_map (k_life_map) and eng.area_map on the same boards, alternating, on three board sets: 4096
19x19 boards at ply 150 of the seeded playouts, the same 4096 boards at the end of the playouts, and 65 536 9x9 boards at the end
of theirs.  A sample is INNER back-to-back calls between two device events (one call is tens of microseconds: too short a window
on its own), reported per call; medians of 12 samples after a warm-up.  Per set: time per call and boards per second of each
kernel, pass_alive's ratios to the other two, what pass_alive finds per board (chains, stones, safe points, removal rounds) and,
counted on the host over the first SAMPLE boards, the chains and regions per board it works on.
Writes profiles/benson_bench.json (or the path given as the first argument) and prints the same JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import elf_amd

REPS, WARM, INNER, SAMPLE = 12, 2, 20, 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / INNER, r


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def seeds_of(k):
    return torch.from_numpy((np.arange(k, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(1)).view(np.int64)).cuda()


def components(n, member):
    """number of 4-connected components of the points a = x*N + y with member[a]"""
    seen, count = set(), 0
    for s in np.nonzero(member)[0]:
        if int(s) in seen:
            continue
        count += 1
        seen.add(int(s))
        stack = [int(s)]
        while stack:
            x, y = divmod(stack.pop(), n)
            for bx, by in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                b = bx * n + by
                if 0 <= bx < n and 0 <= by < n and member[b] and b not in seen:
                    seen.add(b)
                    stack.append(b)
    return count


def maps(eng, boards):
    calls = dict(area_map=lambda: eng.area_map(), life_map=lambda: eng.life_map(), pass_alive=lambda: eng.pass_alive())
    us = {k: [] for k in calls}
    pa = None
    for rep in range(REPS + WARM):
        for k, fn in calls.items():
            dt, r = timed(fn)
            if k == "pass_alive":
                pa = r
            if rep >= WARM:
                us[k].append(dt * 1e6)
    res = dict(boards=boards, reps=REPS, calls_per_sample=INNER)
    for k in calls:
        s = spread(us[k])
        res[k] = dict(us_per_call=s, boards_per_s=boards / (s["median"] * 1e-6))
    med = lambda k: res[k]["us_per_call"]["median"]
    res["pass_alive"]["ratio_to_life_map"] = med("pass_alive") / med("life_map")
    res["pass_alive"]["ratio_to_area_map"] = med("pass_alive") / med("area_map")
    s = pa.summary.to(torch.int64)
    res["bound_hits"] = int((s[:, [3, 7]] < 0).sum())
    for j, name in enumerate(("pass_alive_chains", "pass_alive_stones", "safe_points", "removal_rounds")):
        res[name + "_per_board"] = float((s[:, j] + s[:, 4 + j]).sum()) / boards
    res["removal_rounds_max"] = int(s[:, [3, 7]].max())
    col = eng.export_board(n=SAMPLE)[0].cpu().numpy()
    res["chains_per_board"] = sum(components(eng.n, col[i] == c) for i in range(SAMPLE) for c in (1, 2)) / SAMPLE
    res["regions_per_board"] = sum(components(eng.n, col[i] != c) for i in range(SAMPLE) for c in (1, 2)) / SAMPLE
    res["mean_ply"] = float(eng.info()[:, 0].to(torch.float64).mean())
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "benson_bench.json")
    res = dict(device=torch.cuda.get_device_name(0))
    eng = elf_amd.GoEngine(19, 4096, 0)
    seeds = seeds_of(4096)
    eng.playout(seeds, max_steps=150)
    res["ply150_19"] = maps(eng, 4096)
    eng.playout(seeds)   # on from ply 150 to the end of the games
    res["end_19"] = maps(eng, 4096)
    eng.close()
    eng = elf_amd.GoEngine(9, 65536, 0)
    eng.playout(seeds_of(65536))
    res["end_9"] = maps(eng, 65536)
    eng.close()
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
