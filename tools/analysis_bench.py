"""GPU: time of elfmcts_analyze (candidate moves + principal variations), beside elfmcts_root on the same trees, and what the
analysis snapshot adds to a self-play move boundary.

19x19 trees of 1, 256 and 2048 games after ROLLOUTS rollouts each (a net that costs nothing: random peaky policies and quantised
values drawn on the GPU), stopped mid-move.  Per size: time per elfmcts_analyze call with max_moves 10 and max_pv 16 and per
elfmcts_root call with every output (device events around one launch, after a warm-up; REPS repetitions, median and spread), and
how many candidates and how long the lines were.  Then one SelfPlay of 2048 games, 64 rollouts per move: wall time per move (all
steps + the boundary) with the snapshot on and off, alternating move by move, and the boundary's own host time from
SelfPlay.stats().  Writes profiles/analysis_bench.json (or the path given as the first argument) and prints the same JSON."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
import elf_amd
from elf_amd._lib import check

N, REPS, ROLLOUTS, BATCH = 19, 24, 256, 16
GAMES = (1, 256, 2048)
MAX_MOVES, MAX_PV = 10, 16
MOVE_GAMES, MOVE_ROLLOUTS, MOVE_PAIRS = 2048, 64, 6


def make_actor(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def actor(batch):
        b = batch["s"].shape[0]
        pi = torch.softmax(2.0 * torch.randn((b, n * n + 1), device="cuda", generator=g), dim=1)
        v = torch.round(torch.tanh(torch.randn((b,), device="cuda", generator=g)) * 64) / 64
        return dict(pi=pi, V=v)
    return actor


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def trees(games):
    sp = elf_amd.SelfPlay(board_size=N, num_games=games, mcts_rollout_per_thread=1 << 13, mcts_rollout_per_batch=BATCH, seed=5,
                          nodes_per_game=1024, resign_thres=0.0)
    sp.reg_callback("actor_black", make_actor(N))
    for _ in range(ROLLOUTS // BATCH):
        sp.run()
    m = C.c_void_p(sp.L.elfsp_mcts(sp._h))
    i32 = dict(dtype=torch.int32, device=sp.device)
    f32 = dict(dtype=torch.float32, device=sp.device)
    G, NE = games, sp.edge_stride
    a = dict(info=torch.zeros((G, 8), **i32), coord=torch.zeros((G, MAX_MOVES), **i32), orig=torch.zeros((G, MAX_MOVES), **i32),
             visits=torch.zeros((G, MAX_MOVES), **i32), reward=torch.zeros((G, MAX_MOVES), **f32), prior=torch.zeros((G, MAX_MOVES), **f32),
             pv_len=torch.zeros((G, MAX_MOVES), **i32), pv=torch.zeros((G, MAX_MOVES, MAX_PV), **i32))
    r = dict(info=torch.zeros((G, 8), **i32), coord=torch.zeros((G, NE), **i32), visits=torch.zeros((G, NE), **i32),
             prior=torch.zeros((G, NE), **f32), reward=torch.zeros((G, NE), **f32), child=torch.zeros((G, NE), **i32))
    ap = [C.c_void_p(a[k].data_ptr()) for k in ("info", "coord", "orig", "visits", "reward", "prior", "pv_len", "pv")]
    rp = [C.c_void_p(r[k].data_ptr()) for k in ("info", "coord", "visits", "prior", "reward", "child")]
    st = sp._stream()
    an, ro = [], []
    for rep in range(REPS + 3):
        dt_a = timed(lambda: check(sp.L.elfmcts_analyze(m, MAX_MOVES, MAX_PV, *ap, st)))
        dt_r = timed(lambda: check(sp.L.elfmcts_root(m, *rp, st)))
        if rep >= 3:
            an.append(dt_a * 1e6)
            ro.append(dt_r * 1e6)
    info, pv_len = a["info"].cpu().numpy(), a["pv_len"].cpu().numpy()
    res = dict(games=games, rollouts=ROLLOUTS, reps=REPS, max_moves=MAX_MOVES, max_pv=MAX_PV, analyze_us_per_call=spread(an),
               root_us_per_call=spread(ro), analyze_over_root=spread(an)["median"] / spread(ro)["median"],
               candidates_per_game=float(info[:, 0].mean()), visited_root_edges_per_game=float(info[:, 1].mean()),
               mean_pv_len=float(pv_len[pv_len > 0].mean()) if (pv_len > 0).any() else 0.0, longest_pv=int(info[:, 6].max()),
               error_bits=int(np.bitwise_or.reduce(info[:, 5])))
    sp.close()
    return res


def moves():
    sp = elf_amd.SelfPlay(board_size=N, num_games=MOVE_GAMES, mcts_rollout_per_thread=MOVE_ROLLOUTS, mcts_rollout_per_batch=BATCH, seed=5,
                          nodes_per_game=1024, resign_thres=0.0)
    sp.reg_callback("actor_black", make_actor(N))

    def one_move():
        before = sp.stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(MOVE_ROLLOUTS // BATCH):
            sp.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        after = sp.stats()
        assert after["moves"] - before["moves"] == MOVE_GAMES
        return dt * 1e3, (after["boundary_ns"] - before["boundary_ns"]) * 1e-6
    one_move()                                   # warm-up: first move, one-off set-up
    t = {True: [], False: []}
    b = {True: [], False: []}
    for _ in range(MOVE_PAIRS):
        for on in (True, False):
            sp.set_analysis(MAX_MOVES, MAX_PV) if on else sp.set_analysis(0, 0)
            dt, bd = one_move()
            t[on].append(dt)
            b[on].append(bd)
    sp.close()
    return dict(games=MOVE_GAMES, rollouts_per_move=MOVE_ROLLOUTS, moves_each=MOVE_PAIRS,
                move_ms_snapshot_on=spread(t[True]), move_ms_snapshot_off=spread(t[False]),
                boundary_host_ms_snapshot_on=spread(b[True]), boundary_host_ms_snapshot_off=spread(b[False]))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "analysis_bench.json")
    res = {"analyze_19x19": [trees(g) for g in GAMES], "selfplay_move_19x19": moves()}
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
