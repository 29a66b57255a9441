"""Times ONE bf16 trunk convolution (256 -> 256 channels, NHWC), without and with the skip, at 19 x 19 and 128, 182, 256, 512, 1024,
2048 and 2304 rows and at 9 x 9 and 4096 rows:
    tile128  elfnet_conv3x3_bf16_tile pinned to the wide (128 x 128) tile of net_conv3x3_bf16.hip: what elfnet_conv3x3_bf16 takes
             at every one of these sizes
    big      elfnet_conv3x3_bf16_big, the 256 x 256 tile of net_conv3x3_bf16_big.hip
The two alternate inside one process: a round is `--launches` back-to-back launches of each variant in turn between HIP events,
after a warm-up of both at that shape, and there are `--rounds` rounds; per variant the median of the rounds and their spread
(min, max) in µs per convolution.  `same_bits` says whether the two outputs of the shape were equal bit for bit.
FusedInferenceNet.bf16_big_min_positions comes from this table.  One process; run it under a time limit:
    timeout -k 10 300 python tools/conv_bf16_big_probe.py [--shapes 19x128,...,9x4096] [--out profiles/conv_bf16_big_probe.json]
A variant the library refuses (a non-zero status) is recorded with its status and not timed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="19x128,19x182,19x256,19x512,19x1024,19x2048,19x2304,9x4096", help="board size x rows")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bf16_big_probe.json"))
    a = ap.parse_args()
    import torch
    import elf_amd
    L = elf_amd.lib()
    ch = a.dim
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    res = dict(what="one bf16 trunk convolution, %d -> %d channels, NHWC: elfnet_conv3x3_bf16_tile at tile 128 (net_conv3x3_bf16.hip) "
                    "against elfnet_conv3x3_bf16_big (the 256 x 256 tile, net_conv3x3_bf16_big.hip); without and with skip" % (ch, ch),
               method="HIP events around back-to-back launches, the variants alternating round by round in one process; µs per "
                      "convolution, median / min / max of the rounds",
               launches=a.launches, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0), cus=cus, shapes=[])
    g = torch.Generator(device="cuda").manual_seed(7)
    w = (torch.randn((ch, 3, 3, ch), device="cuda", generator=g) * (9 * ch) ** -0.5).bfloat16()
    b = torch.randn((ch,), device="cuda", generator=g).bfloat16()
    for n, rows in [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",") if s != ""]:
        x = torch.randn((rows, n, n, ch), device="cuda", generator=g).bfloat16()
        r = torch.randn((rows, n, n, ch), device="cuda", generator=g).bfloat16()
        y = {name: torch.empty_like(x) for name in ("tile128", "big")}
        for skip, rr in (("noskip", None), ("skip", r)):
            variants = dict(
                tile128=lambda rr=rr: L.elfnet_conv3x3_bf16_tile(p(x), p(w), p(b), p(rr), p(y["tile128"]), rows, n, n, ch, ch, 1, 128, st),
                big=lambda rr=rr: L.elfnet_conv3x3_bf16_big(p(x), p(w), p(b), p(rr), p(y["big"]), rows, n, n, ch, ch, 1, st))
            out = dict(board=n, rows=rows, positions=rows * n * n, skip=skip == "skip", big_tiles=(rows * n * n + 255) // 256 * (ch // 256))
            us = {}
            for name, fn in variants.items():
                rc = fn()
                torch.cuda.synchronize()
                if rc != 0:
                    out[name] = dict(status=int(rc))
                    continue
                for _ in range(a.warmup):
                    fn()
                us[name] = []
            if len(us) == 2:
                out["same_bits"] = bool(torch.equal(y["tile128"].view(torch.int16), y["big"].view(torch.int16)))
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
        del x, r, y
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
