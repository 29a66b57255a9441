"""GPU: k_playout_own beside k_playout on the same 4096 games, then the user-shaped ownership call.

(a) eng.playout on 4096 slots from the empty 19x19 board with playout_seeds(4096): benchmark config 2;
(b) eng.ownership(playouts=1) on the same slots and seeds: the same 4096 games through the ownership kernel;
(c) 16 rows x 256 playouts from ply-120 positions.
(a) and (b) alternate inside one process; times are device events around each call, after a warm-up.  Writes
profiles/ownership_bench.json (or the path given as the first argument) and prints the same JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import elf_amd

REPS, BOARDS = 24, 4096


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


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ownership_bench.json")
    eng = elf_amd.GoEngine(19, BOARDS, 0)
    seeds = torch.from_numpy((np.arange(BOARDS, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(1)).view(np.int64)).cuda()
    rate_a, rate_b = [], []
    for rep in range(REPS + 3):
        eng.reset()
        dt_b, own = timed(lambda: eng.ownership(seeds, playouts=1))
        steps_b = int(own["stats"][:, 3].sum())
        dt_a, out = timed(lambda: eng.playout(seeds))
        steps_a = int(out[:, 3].to(torch.int64).sum())
        assert steps_a == steps_b, (steps_a, steps_b)          # the same games
        if rep >= 3:
            rate_a.append(steps_a / dt_a)
            rate_b.append(steps_b / dt_b)
    res = dict(boards=BOARDS, reps=REPS, board_steps=steps_a,
               playout_steps_per_s=spread(rate_a), ownership_k1_steps_per_s=spread(rate_b),
               ratio_median=spread(rate_b)["median"] / spread(rate_a)["median"],
               scratch_bytes=int(eng.L.elfgo_own_scratch_bytes(eng._own[1])))
    # the user-shaped call: 16 positions at ply 120, 256 playouts each
    rows, K = 16, 256
    eng.reset()
    eng.playout(seeds[:rows], ids=list(range(rows)), max_steps=120)
    ms = []
    for rep in range(REPS + 3):
        dt, own = timed(lambda: eng.ownership(seeds[:rows], ids=list(range(rows)), playouts=K))
        if rep >= 3:
            ms.append(dt * 1e3)
    res["rows16_k256"] = dict(ms_per_call=spread(ms), playouts_per_s=rows * K / (spread(ms)["median"] * 1e-3),
                              steps_per_playout=float(own["stats"][:, 3].sum()) / (rows * K))
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
