"""GPU: the candidate-move playouts and the self-atari map beside the kernels they were modelled on, in one process.

(a) 4096 19x19 and 65 536 9x9 playouts from the empty board with playout_seeds: eng.playout (k_playout) and
    eng.playout(self_atari_thres=1 / 5) (k_playout_cand) on the same slots and seeds, alternating: board steps per second and
    mean steps per game of each;
(b) eng.ownership at 16 ply-120 19x19 positions x 256 playouts, with no threshold (k_playout_own<N, EyePolicy>) and with
    thres 1 / 5 (k_playout_own<N, CandPolicy>);
(c) eng.candidates beside eng.legal_mask on 4096 19x19 boards at ply 150.
Times are device events around each call, after a warm-up.  Writes profiles/candidates_bench.json (or the path given as the
first argument) and prints the same JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import elf_amd

REPS, WARM = 12, 2
THRESHOLDS = (1, 5)


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


def playouts(n, boards):
    eng = elf_amd.GoEngine(n, boards, 0)
    seeds = seeds_of(boards)
    rate = {t: [] for t in (None,) + THRESHOLDS}
    steps = {}
    for rep in range(REPS + WARM):
        for t in rate:
            eng.reset()
            dt, out = timed(lambda: eng.playout(seeds, self_atari_thres=t))
            steps[t] = int(out[:, 3].to(torch.int64).sum())
            if rep >= WARM:
                rate[t].append(steps[t] / dt)
    eng.close()
    key = lambda t: "playout" if t is None else "thres%d" % t
    res = dict(boards=boards, reps=REPS)
    for t in rate:
        res[key(t)] = dict(steps_per_s=spread(rate[t]), mean_steps_per_game=steps[t] / boards,
                           games_per_s=spread(rate[t])["median"] / (steps[t] / boards))
    for t in THRESHOLDS:
        res[key(t)]["steps_per_s_ratio_to_playout"] = res[key(t)]["steps_per_s"]["median"] / res["playout"]["steps_per_s"]["median"]
        res[key(t)]["games_per_s_ratio_to_playout"] = res[key(t)]["games_per_s"] / res["playout"]["games_per_s"]
    return res


def ownership(rows=16, K=256, ply=120):
    eng = elf_amd.GoEngine(19, rows, 0)
    seeds = seeds_of(rows)
    eng.playout(seeds, max_steps=ply)
    res = dict(rows=rows, playouts=K, ply=ply)
    for t in (None,) + THRESHOLDS:
        ms = []
        for rep in range(REPS + WARM):
            dt, own = timed(lambda: eng.ownership(seeds, ids=list(range(rows)), playouts=K, self_atari_thres=t))
            if rep >= WARM:
                ms.append(dt * 1e3)
        res["playout" if t is None else "thres%d" % t] = dict(ms_per_call=spread(ms), steps_per_playout=float(own["stats"][:, 3].sum()) / (rows * K))
    for t in THRESHOLDS:
        res["thres%d" % t]["ms_ratio_to_playout"] = res["thres%d" % t]["ms_per_call"]["median"] / res["playout"]["ms_per_call"]["median"]
    eng.close()
    return res


def maps(boards=4096, ply=150):
    eng = elf_amd.GoEngine(19, boards, 0)
    eng.playout(seeds_of(boards), max_steps=ply)
    us_c, us_l = [], []
    for rep in range(REPS + WARM):
        dt_l, _ = timed(lambda: eng.legal_mask())
        dt_c, (mask, stones) = timed(lambda: eng.candidates(self_atari_thres=1))
        if rep >= WARM:
            us_c.append(dt_c * 1e6)
            us_l.append(dt_l * 1e6)
    res = dict(boards=boards, ply=ply, candidates_us=spread(us_c), legal_mask_us=spread(us_l),
               ratio_median=spread(us_c)["median"] / spread(us_l)["median"],
               self_atari_points_per_board=float((stones > 0).sum()) / boards, candidates_per_board=float(mask.sum()) / boards)
    eng.close()
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "candidates_bench.json")
    res = dict(device=torch.cuda.get_device_name(0), playout_19=playouts(19, 4096), playout_9=playouts(9, 65536), ownership_19=ownership(),
               candidates_19=maps())
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
