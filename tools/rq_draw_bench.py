"""GPU: the trainer's samples drawn on the host (elfrq_draw, the default ReplayBuffer) beside the same samples drawn on the device
(k_rq_draw, ReplayBuffer(device_draws=True)), in one process on the same records and seeds.

Shapes: bench.py --workload train's (19x19, 16 batches of 2048 per launch = 512 acts over 32 game threads, 256 records,
num_reader 4) and the same with the reference's 50 queues.  Every repetition runs both paths, alternating which goes first:
  end to end  -- LAUNCHES ReplayBuffer.sample() calls, wall time from the first call to the stream's end;
  the stages  -- one more launch taken apart: the draws (the host path: wall time of draw_into on the host, then its copy; the
                 device path: device events around elfrq_dev_draw) and the extraction kernel between events.
The two buffers stay in step (the same number of draws each), so the rows of every repetition's last launch are compared too.
Medians of 12 after a warm-up, with minimum and maximum.  Writes profiles/rq_draw_bench.json (or the path given as the first
argument) and prints it."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import elf_amd
from train_df_bench import random_games, spread

REPS, WARM, LAUNCHES = 12, 2, 400
N, RECORDS, PLIES, BATCH, BATCHES, NFA = 19, 256, 320, 2048, 16, 1


def stages(rb, acts, out):
    """one launch taken apart -> (seconds for the draws, seconds for the extraction kernel)"""
    k, ld = 64 * acts, rb.loader
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    if rb.device_draws:
        dev = ld._draw
        a.record()
        rb.queues.draw_device(acts, NFA, out=dev)
        b.record()
    else:
        host, dev, done = rb._ring[0]
        done.synchronize()
        t0 = time.perf_counter()
        rb.queues.draw_into(host, acts, NFA)
        t_host = time.perf_counter() - t0
        dev[:, :k].copy_(host[:, :k], non_blocking=True)
        done.record(torch.cuda.current_stream(ld.device))
        b.record()
    ld.extract(dev[0, :k], dev[1, :k], dev[2, :k], out=out)
    c.record()
    c.synchronize()
    return (a.elapsed_time(b) * 1e-3 if rb.device_draws else t_host), b.elapsed_time(c) * 1e-3


def measure(moves, num_reader):
    rng = np.random.default_rng(7)
    P = (N + 2) ** 2
    kw = dict(board_size=N, num_reader=num_reader, queue_min_size=max(1, min(10, RECORDS // (4 * num_reader))), queue_max_size=1000,
              batchsize=BATCH, batches_per_launch=BATCHES, insert_seed=77, seed=1234, num_future_actions=NFA, feature_format="f16_nhwc")
    rbs = dict(host=elf_amd.ReplayBuffer(**kw), device=elf_amd.ReplayBuffer(device_draws=True, **kw))
    for r in range(RECORDS):
        pol = np.zeros((PLIES, P), np.uint8)
        np.put_along_axis(pol, rng.integers(0, P, size=(PLIES, 24)), rng.integers(1, 256, size=(PLIES, 24)).astype(np.uint8), axis=1)
        pol[np.arange(PLIES), moves[r]] = 255
        rec = dict(moves=moves[r], reward=float(rng.choice([-1.0, 1.0])), black_ver=0, policies=pol,
                   values=np.tanh(rng.standard_normal(PLIES)).astype(np.float32))
        for rb in rbs.values():
            rb.insert(rec)
    B, acts = BATCH * BATCHES, BATCH * BATCHES // 64
    out = {k: rb.loader._alloc(B) for k, rb in rbs.items()}
    t = {k: dict(end_to_end=[], draw=[], extract=[]) for k in rbs}
    for rep in range(REPS + WARM):
        for k in (("host", "device") if rep % 2 == 0 else ("device", "host")):
            rb = rbs[k]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(LAUNCHES):
                rb.sample(acts, out=out[k])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            dr, ex = stages(rb, acts, out[k])
            if rep >= WARM:
                t[k]["end_to_end"].append(dt / LAUNCHES)
                t[k]["draw"].append(dr)
                t[k]["extract"].append(ex)
        for f in ("move_idx", "aug_code", "offline_a", "winner", "s"):
            assert torch.equal(out["host"][f], out["device"][f]), f
    assert rbs["device"].queues.device_status() == 0
    res = dict(num_reader=num_reader, queue_sizes=[int(s) for s in rbs["host"].queues.sizes()])
    for k, rb in rbs.items():
        e = spread(t[k]["end_to_end"])
        res[k] = dict(samples_per_s=dict(median=B / e["median"], min=B / e["max"], max=B / e["min"]),
                      ms_per_launch=spread([x * 1e3 for x in t[k]["end_to_end"]]),
                      draw_ms=spread([x * 1e3 for x in t[k]["draw"]]), extract_kernel_ms=spread([x * 1e3 for x in t[k]["extract"]]))
        rb.close()
    h, d = res["host"]["samples_per_s"], res["device"]["samples_per_s"]
    res["device_over_host"] = dict(samples_per_s=d["median"] / h["median"],
                                   beyond_spread=bool(d["min"] > h["max"]) if d["median"] >= h["median"] else bool(d["max"] < h["min"]))
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rq_draw_bench.json")
    moves = random_games(RECORDS, PLIES)
    res = dict(device=torch.cuda.get_device_name(0), board_size=N, records=RECORDS, plies=PLIES, samples_per_launch=BATCH * BATCHES,
               acts_per_launch=BATCH * BATCHES // 64, game_threads=BATCH // 64, num_future_actions=NFA, feature_format="f16_nhwc",
               reps=REPS, launches_per_end_to_end_sample=LAUNCHES,
               draw_ms_is="host: wall time of elfrq_draw on the host (its copy not included); device: events around elfrq_dev_draw")
    for nr in (4, 50):
        res["num_reader_%d" % nr] = measure(moves, nr)
    text = json.dumps(res, indent=1)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
