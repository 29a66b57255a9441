"""GPU: elfgo_setup beside the only other way to reach a position, elfgo_reset + one elfgo_forward launch per move.

4096 19x19 positions at ply 200 of seeded random games (the config-2 policy; the move lists come from the CPU oracle, which
plays the same games):
(a) eng.setup of all 4096 from their stones, one launch;
(b) eng.reset + 199 eng.forward launches over the same 4096 slots (ids and moves already on the device).
(a) and (b) alternate inside one process; times are device events around windows of LAUNCHES back-to-back setup calls and of
REPLAYS back-to-back replays (a tenth of a second or more each), after a warm-up.  Both go through the Python methods, so these
are times per CALL (kernel + whatever the host and the launch path add) and bound the kernel from above.  Also calls for
1 board (19x19) and for 65 536 9x9 boards (ply 60).  Writes profiles/setup_bench.json (or the path given as the first argument)
and prints the same JSON.  No threshold: the file records what was measured.

Kernel durations come from a run of their own under the profiler:
    rocprofv3 --kernel-trace -d DIR -- python tools/setup_bench.py OUT.json
    python tools/setup_bench.py --trace DIR/.../*_kernel_trace.csv profiles/setup_bench.json
The second command adds `kernel_us` (per kernel and grid size: launches, min / median / max of end - start) to the JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
import elf_amd
from pyoracle import Port, playout_seeds

REPS, BOARDS, PLY, LAUNCHES, REPLAYS = 12, 4096, 200, 1000, 50


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


def hashes(eng, ids):
    i = eng.info(ids).cpu().numpy()
    return i[:, 13].astype(np.uint32).astype(np.uint64) | (i[:, 14].astype(np.uint32).astype(np.uint64) << np.uint64(32))


def setup_window(eng, stones, ids, players, launches):
    """seconds per launch over a window of back-to-back launches"""
    def run():
        for _ in range(launches):
            ok = eng.setup(stones, ids, players)
        return ok
    dt, ok = timed(run)
    assert bool((ok == 1).all())
    return dt / launches


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "setup_bench.json")
    n = 19
    seeds = playout_seeds(BOARDS)
    P = Port(n)
    moves = np.zeros((BOARDS, PLY - 1), np.int32)
    for g, sd in enumerate(seeds):
        s = P.new()
        mv = P.playout_moves(s, int(sd), PLY - 1)
        P.free(s)
        assert len(mv) == PLY - 1, "a seeded game ended before ply %d" % PLY
        moves[g] = mv
    eng = elf_amd.GoEngine(n, 2 * BOARDS, 0)
    src = torch.arange(BOARDS, dtype=torch.int32, device="cuda")
    dst = src + BOARDS
    eng.playout(seeds, ids=src, max_steps=PLY - 1)
    want = hashes(eng, src)
    stones = eng.export_board(src)[0]
    players = eng.info(src)[:, 1].to(torch.uint8).contiguous()
    mv_dev = torch.from_numpy(np.ascontiguousarray(moves.T)).cuda()          # [PLY - 1, BOARDS]

    def replay():
        for _ in range(REPLAYS):
            eng.reset(dst)
            for t in range(PLY - 1):
                ok = eng.forward(dst, mv_dev[t])
        return ok

    t_a, t_b = [], []
    for rep in range(REPS + 2):
        a = setup_window(eng, stones, dst, players, LAUNCHES)
        assert np.array_equal(hashes(eng, dst), want)
        b, ok = timed(replay)
        b /= REPLAYS
        assert bool((ok == 1).all()) and np.array_equal(hashes(eng, dst), want)   # both ways reach the same positions
        if rep >= 2:
            t_a.append(a)
            t_b.append(b)
    res = dict(boards=BOARDS, ply=PLY, reps=REPS, launches_per_window=LAUNCHES, replays_per_window=REPLAYS,
               stones_per_board=float((stones != 0).sum().item()) / BOARDS,
               setup_s=spread(t_a), reset_forward_s=spread(t_b),
               setup_boards_per_s=BOARDS / spread(t_a)["median"], reset_forward_boards_per_s=BOARDS / spread(t_b)["median"],
               ratio_median=spread(t_b)["median"] / spread(t_a)["median"])
    one = [setup_window(eng, stones[:1], dst[:1], players[:1], 2 * LAUNCHES) for _ in range(REPS + 2)][2:]
    res["one_board_us_per_launch"] = {k: v * 1e6 for k, v in spread(one).items()}
    eng.close()
    # 65 536 9x9 boards at ply 60
    n9, B9 = 9, 65536
    e9 = elf_amd.GoEngine(n9, B9, 0)
    e9.playout(playout_seeds(B9), max_steps=59)
    st9 = e9.export_board()[0]
    pl9 = e9.info()[:, 1].to(torch.uint8).contiguous()
    w9 = hashes(e9, None)
    t9 = [setup_window(e9, st9, None, pl9, LAUNCHES // 2) for _ in range(REPS + 2)][2:]
    assert np.array_equal(hashes(e9, None), w9)
    res["boards9_65536"] = dict(ply=60, stones_per_board=float((st9 != 0).sum().item()) / B9, setup_s=spread(t9),
                                boards_per_s=B9 / spread(t9)["median"])
    e9.close()
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


def add_trace(csv_path, json_path):
    """kernel durations of the setup / reset / forward kernels from a rocprofv3 kernel trace, grouped by grid size"""
    import csv
    import re
    groups = {}
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"k_(setup|reset|forward)<(\d+)>", row["Kernel_Name"])
            if not m:
                continue
            boards = int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"])
            key = "k_%s<%s> x %d boards" % (m.group(1), m.group(2), boards)
            groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    with open(json_path) as f:
        res = json.load(f)
    res["kernel_us"] = {k: dict(launches=len(v), **spread(v)) for k, v in sorted(groups.items())}
    text = json.dumps(res, indent=1)
    with open(json_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--trace":
        add_trace(sys.argv[2], sys.argv[3])
    else:
        main()
