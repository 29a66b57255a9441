"""Times the two ends of the bf16 net (elf_amd/csrc/net_io.hip, the bf16 instances) against what a bf16 net ran before them, 19 x 19, 18 -> 256
planes and 256-channel heads, at 1, 16, 128 and 2048 rows:
    in_conv   native  elfnet_conv3x3_in_bf16 from the fp16 feature rows (x_is_f16 = 1)
              pair    s.to(bfloat16), F.conv2d (MIOpen, the solver its find step picks, as in bench.py), elfnet_bias_act_bf16
    heads     native  elfnet_heads_bf16
              eager   the head ops of FusedInferenceNet.__call__ (two 1x1 convolutions, three Linear layers, softmax, tanh)
    net       native  GraphedNet(NativeBf16InferenceNet)      } the whole call of the --blocks x 256 net on fp16 rows, at the
              fused   GraphedNet(FusedInferenceNet), bf16     } --net-rows sizes only
The two variants of a comparison alternate inside one process: a round is `--launches` back-to-back launches of each in turn between
HIP events, after a warm-up of both at that shape, and there are `--rounds` rounds; per variant the median of the rounds and their
spread (min, max) in µs per call.  One process; run it under a time limit:
    timeout -k 10 600 python tools/net_io_bf16_probe.py [--rows 1,16,128,2048] [--net-rows 16,2048] [--out profiles/net_io_bf16_probe.json]
The floor of the heads is one pass over the [rows,19,19,256] bf16 activation, of the input convolution one write of it (378 MB at
2048 rows: about 75 µs at 5 TB/s)."""
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
    ap.add_argument("--rows", default="1,16,128,2048")
    ap.add_argument("--net-rows", default="16,2048")
    ap.add_argument("--board-size", type=int, default=19)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_io_bf16_probe.json"))
    a = ap.parse_args()
    # the MIOpen side runs what the tuned database names, as the benchmark does (bench.py's seed_miopen_db)
    src = os.path.join(ROOT, "elf_amd", "data", "miopen_db")
    dst = os.environ.get("MIOPEN_USER_DB_PATH") or os.path.join(os.path.expanduser("~"), ".config", "miopen")
    os.makedirs(dst, exist_ok=True)
    for name in sorted(os.listdir(src)):
        if not os.path.exists(os.path.join(dst, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
    import torch
    import elf_amd
    from elf_amd.net import FusedInferenceNet, GraphedNet, NativeBf16InferenceNet, make_net
    torch.backends.cudnn.benchmark = True   # as bench.py: the pair runs the solver MIOpen's find step picks, not immediate mode's
    L = elf_amd.lib()
    n, dim = a.board_size, a.dim
    d = n * n
    net = make_net(board_size=n, num_block=a.blocks, dim=dim, dtype=torch.bfloat16, fold_bn=True)
    native = NativeBf16InferenceNet(net)
    first = net.init_conv[0]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    g = torch.Generator(device="cuda").manual_seed(7)

    def alternate(variants):
        """{name: fn} -> {name: dict(status, median_us, min_us, max_us)}; a variant with a non-zero status is recorded and not timed"""
        out, us = {}, {}
        for name, fn in variants.items():
            rc = fn()
            torch.cuda.synchronize()
            if rc:
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
        return out

    res = dict(what="the ends of a bf16 net, %d x %d, 18 -> %d planes and %d-channel heads: net_io.hip's bf16 entries against the ops a bf16 "
                    "FusedInferenceNet runs; the whole %d-block net under GraphedNet" % (n, n, dim, dim, a.blocks),
               method="HIP events around back-to-back launches, the two variants of a comparison alternating round by round in one "
                      "process; µs per call, median / min / max of the rounds",
               launches=a.launches, warmup=a.warmup, rounds=a.rounds, device=torch.cuda.get_device_name(0), shapes=[])
    net_rows = [int(v) for v in a.net_rows.split(",") if v != ""]
    with torch.no_grad():
        for rows in [int(v) for v in a.rows.split(",") if v != ""]:
            s = (torch.rand((rows, n, n, 18), device="cuda", generator=g) < 0.3).half().permute(0, 3, 1, 2)   # fp16 rows, channels_last
            act = torch.relu(torch.randn((rows, n, n, dim), device="cuda", generator=g)).bfloat16().permute(0, 3, 1, 2)
            y = torch.empty((rows, dim, n, n), device="cuda", dtype=torch.bfloat16, memory_format=torch.channels_last)
            pi = torch.empty((rows, d + 1), device="cuda", dtype=torch.float32)
            v = torch.empty((rows,), device="cuda", dtype=torch.float32)
            nb = L.elfnet_heads_workspace(rows, n, n)
            ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)

            def in_native():
                return L.elfnet_conv3x3_in_bf16(p(s), 1, p(first.weight), p(first.bias), p(y), rows, n, n, 18, dim, 1, st)

            def in_pair():
                o = torch.nn.functional.conv2d(s.to(torch.bfloat16), first.weight, None, 1, 1)
                return L.elfnet_bias_act_bf16(p(o), p(first.bias), None, rows * d, dim, 1, st)

            def heads_native():
                return L.elfnet_heads_bf16(p(act), C.byref(native.heads), rows, n, n, p(pi), d + 1, p(v), None, p(ws), nb, st)

            def heads_eager():
                a_pi = net.pi_linear(net.pi_final_conv(act).reshape(-1, 2 * d))
                torch.softmax(a_pi.float(), dim=1)
                a_v = torch.relu(net.value_linear1(net.value_final_conv(act).reshape(-1, d)))
                torch.tanh(net.value_linear2(a_v)).float().reshape(-1)
                return 0

            out = dict(rows=rows, floor_us_one_pass_at_5TBs=round(rows * d * dim * 2 / 5e12 * 1e6, 1),
                       in_conv=alternate(dict(native=in_native, pair=in_pair)), heads=alternate(dict(native=heads_native, eager=heads_eager)))
            if rows in net_rows:
                gn, gf = GraphedNet(native, s), GraphedNet(FusedInferenceNet(net), s)
                out["net"] = alternate(dict(native=lambda: gn() and 0, fused=lambda: gf() and 0))
                del gn, gf
            print(json.dumps(out), flush=True)
            res["shapes"].append(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
