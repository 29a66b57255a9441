"""Times ONE bf16 trunk convolution (19 x 19, 256 -> 256 channels, NHWC) at 1, 16, 64, 128 and 2048 rows, without and with the skip:
    tile64 / tile128  elfnet_conv3x3_bf16_tile with the narrow (64 x 64) / wide (128 x 128) tile of net_conv3x3_bf16.hip; bias, skip
                      and ReLU in the convolution's epilogue
    pair              what a bf16 net ran before: F.conv2d (MIOpen, the solver its find step picks, as in bench.py) followed by
                      elfnet_bias_act_bf16
The three alternate inside one process: a round is `--launches` back-to-back launches of each variant in turn between HIP events,
after a warm-up of every variant at that shape, and there are `--rounds` rounds; per variant the median of the rounds and their
spread (min, max) in µs per convolution.  `pick` is the tile elfnet_conv3x3_bf16 itself takes at the shape on this device.
One process; run it under a time limit:
    timeout -k 10 300 python tools/conv_bf16_probe.py [--rows 1,16,64,128,2048] [--out profiles/conv_bf16_probe.json]
A variant the library refuses (a non-zero status) is recorded with its status and not timed."""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,16,64,128,2048")
    ap.add_argument("--board-size", type=int, default=19)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bf16_probe.json"))
    a = ap.parse_args()
    # the pair runs the convolution MIOpen's tuned database names for a shape where it has one, as the benchmark does: the committed
    # entries go into the user database directory where no file of that name is there yet (bench.py's seed_miopen_db)
    src = os.path.join(ROOT, "elf_amd", "data", "miopen_db")
    dst = os.environ.get("MIOPEN_USER_DB_PATH") or os.path.join(os.path.expanduser("~"), ".config", "miopen")
    os.makedirs(dst, exist_ok=True)
    for name in sorted(os.listdir(src)):
        if not os.path.exists(os.path.join(dst, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
    import torch
    import elf_amd
    torch.backends.cudnn.benchmark = True   # as bench.py: the pair runs the solver MIOpen's find step picks, not immediate mode's
    L = elf_amd.lib()
    n, ch = a.board_size, a.dim
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    res = dict(what="one bf16 trunk convolution, %d -> %d channels, %d x %d, NHWC: elfnet_conv3x3_bf16_tile at tile 64 and tile 128 "
                    "(net_conv3x3_bf16.hip) against F.conv2d (MIOpen) + elfnet_bias_act_bf16; without and with skip" % (ch, ch, n, n),
               method="HIP events around back-to-back launches, the variants alternating round by round in one process; µs per "
                      "convolution, median / min / max of the rounds",
               launches=a.launches, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0), cus=cus, shapes=[])
    g = torch.Generator(device="cuda").manual_seed(7)
    w = (torch.randn((ch, 3, 3, ch), device="cuda", generator=g) * (9 * ch) ** -0.5).bfloat16()
    b = torch.randn((ch,), device="cuda", generator=g).bfloat16()
    wv = w.permute(0, 3, 1, 2)
    for rows in [int(v) for v in a.rows.split(",") if v != ""]:
        x = torch.randn((rows, n, n, ch), device="cuda", generator=g).bfloat16()
        r = torch.randn((rows, n, n, ch), device="cuda", generator=g).bfloat16()
        y = torch.empty_like(x)
        xv = x.permute(0, 3, 1, 2)
        for skip, rr in (("noskip", None), ("skip", r)):
            def tiled(tile, rr=rr):
                return lambda: L.elfnet_conv3x3_bf16_tile(p(x), p(w), p(b), p(rr), p(y), rows, n, n, ch, ch, 1, tile, st)

            def pair(rr=rr):
                o = torch.nn.functional.conv2d(xv, wv, None, 1, 1)
                return L.elfnet_bias_act_bf16(p(o), p(b), p(rr), rows * n * n, ch, 1, st)

            variants = dict(tile64=tiled(64), tile128=tiled(128), pair=pair)
            out = dict(rows=rows, positions=rows * n * n, skip=skip == "skip", pick=int(L.elfnet_conv3x3_bf16_pick(rows * n * n, ch, cus)))
            us = {}
            with torch.no_grad():
                for name, fn in variants.items():
                    rc = fn()
                    torch.cuda.synchronize()
                    if rc != 0:
                        out[name] = dict(status=int(rc))
                        continue
                    for _ in range(a.warmup):
                        fn()
                    us[name] = []
                for _ in range(a.rounds):
                    for name in us:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.launches):
                            variants[name]()
                        e1.record()
                        e1.synchronize()
                        us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
            for name, v in us.items():
                out[name] = dict(status=0, median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))
            print(json.dumps(out), flush=True)
            res["shapes"].append(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
