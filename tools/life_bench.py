"""GPU: the life reading beside the per-point maps it was modelled on, in one process.

eng.life_map (k_life_map), eng.legal_mask and eng.candidates (k_candidates) on the same boards, alternating, on three board sets:
4096 19x19 boards at ply 150 of the seeded playouts, the same 4096 boards at the end of the playouts, and 65 536 9x9 boards at the
end of the playouts.  A sample is INNER back-to-back calls between two device events (one call is tens of microseconds: too short
a window on its own), reported per call; medians of 12 samples after a warm-up.  Per set: time per call and boards per second of
each kernel, life_map's ratios to the other two, and living groups and true eyes per board as life_map counts them.
Writes profiles/life_bench.json (or the path given as the first argument) and prints the same JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import elf_amd

REPS, WARM, INNER = 12, 2, 20


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


def maps(eng, boards):
    calls = dict(legal_mask=lambda: eng.legal_mask(), candidates=lambda: eng.candidates(self_atari_thres=1), life_map=lambda: eng.life_map())
    us = {k: [] for k in calls}
    lm = None
    for rep in range(REPS + WARM):
        for k, fn in calls.items():
            dt, r = timed(fn)
            if k == "life_map":
                lm = r
            if rep >= WARM:
                us[k].append(dt * 1e6)
    res = dict(boards=boards, reps=REPS, calls_per_sample=INNER)
    for k in calls:
        s = spread(us[k])
        res[k] = dict(us_per_call=s, boards_per_s=boards / (s["median"] * 1e-6))
    med = lambda k: res[k]["us_per_call"]["median"]
    res["life_map"]["ratio_to_legal_mask"] = med("life_map") / med("legal_mask")
    res["life_map"]["ratio_to_candidates"] = med("life_map") / med("candidates")
    eye = lm.eye
    res["true_eyes_per_board"] = float(((eye & 4) != 0).sum() + ((eye & 64) != 0).sum()) / boards
    res["semi_eyes_per_board"] = float(((eye & 8) != 0).sum() + ((eye & 128) != 0).sum()) / boards
    res["living_groups_per_board"] = float(lm.summary[:, 9:11].sum()) / boards
    res["living_stones_per_board"] = float(lm.alive.sum()) / boards
    res["mean_ply"] = float(eng.info()[:, 0].to(torch.float64).mean())
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "life_bench.json")
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
