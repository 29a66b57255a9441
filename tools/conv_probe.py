"""Times ONE trunk convolution of the benchmark net (rows = 2048, 19 x 19, 256 -> 256, fp16 NHWC), with and without the skip:
    fused0 / fused1   elfnet_conv3x3_f16 with algo 0 (CK's main loop) / 1 (the hand-written kernel of net_conv3x3.hip); bias, skip
                      and ReLU in the convolution's epilogue
    fusedsmall        elfnet_conv3x3_small_f16, the 64 x 64 x 64 kernel of net_conv3x3_small.hip for calls of a few thousand positions
                      (`--algos 0,small`; for the single game's call: --rows 16 --no-pair)
    pair              what ran before: F.conv2d (MIOpen) followed by elfnet_bias_act_f16
HIP events around `--launches` back-to-back launches after a warm-up, `--repeats` times; mean / min / max of the repeats in µs per
convolution.  One process; run it under a time limit:
    timeout -k 10 300 python tools/conv_probe.py [--algos 0,1] [--rows 2048] [--out profiles/conv_fused_probe.json]
For a counter pass (rocprofv3 --pmc, which replays every dispatch once per counter group) run one variant and nothing else:
    ... python tools/conv_probe.py --algos 1 --no-pair --launches 4 --warmup 1 --repeats 1 --out /dev/null
A variant the library refuses (a non-zero status, e.g. CK's IsSupportedArgument saying no on this device) is recorded with its
status and not timed.  --round-width W runs algo 1 through elfnet_conv3x3_f16_width: W work items at a time instead of the device's CU
count, which decides whether the last round is split into half tiles and how many workgroups the launch has: min(W, work ids),
each running every W-th id one after the other with the next item's prologue issued in front of its epilogue.  -1 (or any W above
the number of tiles) never splits and gives every work id a workgroup of its own, which is the A/B of the split and of the chains
inside one build.  The rule needs one whole round in front of the split one, so at most a third of the
tiles can be split: W = 2 * tiles / 3 gives one round of W full tiles and one of W half tiles.  FusedInferenceNet routes to algo 1 only where its mean is below algo 0's by more than the spread
(max - min over the repeats) of either.
--order linear|board pins algo 1's row order, which elfnet_conv3x3_f16 otherwise chooses by shape (elfnet_conv3x3_f16_order):
linear is elfnet_conv3x3_f16_width at the device's CU count named as the round width (or at --round-width), board is
elfnet_conv3x3_f16_boards; the same build, the same process: the A/B of the two orders."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--board-size", type=int, default=19)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--algos", default="0,1", help="comma-separated: 0, 1 (elfnet_conv3x3_f16's algos) and small (elfnet_conv3x3_small_f16)")
    ap.add_argument("--round-width", type=int, default=None,
                    help="algo 1's round width (elfnet_conv3x3_f16_width): 0 = the CU count, -1 = never split the last round")
    ap.add_argument("--order", choices=["linear", "board"], default=None, help="algo 1's row order; default: the library's own choice")
    ap.add_argument("--no-pair", action="store_true", help="leave F.conv2d + elfnet_bias_act_f16 out: only the fused variants run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_fused_probe.json"))
    a = ap.parse_args()
    # the pair runs the convolution MIOpen's tuned database names for this shape, as the benchmark does: the committed entries go
    # into the user database directory where no file of that name is there yet (bench.py's seed_miopen_db)
    src = os.path.join(ROOT, "elf_amd", "data", "miopen_db")
    dst = os.environ.get("MIOPEN_USER_DB_PATH") or os.path.join(os.path.expanduser("~"), ".config", "miopen")
    os.makedirs(dst, exist_ok=True)
    for name in sorted(os.listdir(src)):
        if not os.path.exists(os.path.join(dst, name)):
            shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
    import torch
    import elf_amd
    L = elf_amd.lib()
    rows, n, ch = a.rows, a.board_size, a.dim
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((rows, n, n, ch), device="cuda", generator=g).half()
    w = (torch.randn((ch, 3, 3, ch), device="cuda", generator=g) * (9 * ch) ** -0.5).half()
    b = torch.randn((ch,), device="cuda", generator=g).half()
    r = torch.randn((rows, n, n, ch), device="cuda", generator=g).half()
    y = torch.empty_like(x)
    xv, wv = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    width = None if a.round_width is None else (1 << 30) if a.round_width < 0 else a.round_width
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def fused(algo, res):
        if algo == "small":
            return lambda: L.elfnet_conv3x3_small_f16(p(x), p(w), p(b), p(res), p(y), rows, n, n, ch, ch, 1, st)
        if algo == 1 and a.order == "board":
            return lambda: L.elfnet_conv3x3_f16_boards(p(x), p(w), p(b), p(res), p(y), rows, n, n, ch, ch, 1, width or 0, st)
        if algo == 1 and a.order == "linear":
            return lambda: L.elfnet_conv3x3_f16_width(p(x), p(w), p(b), p(res), p(y), rows, n, n, ch, ch, 1, 1, width or cus, st)
        if width is not None:
            return lambda: L.elfnet_conv3x3_f16_width(p(x), p(w), p(b), p(res), p(y), rows, n, n, ch, ch, 1, algo, width, st)
        return lambda: L.elfnet_conv3x3_f16(p(x), p(w), p(b), p(res), p(y), rows, n, n, ch, ch, 1, algo, st)

    def pair(res):
        def f():
            o = torch.nn.functional.conv2d(xv, wv, None, 1, 1)
            return L.elfnet_bias_act_f16(p(o), p(b), p(res), rows * n * n, ch, 1, st)
        return f

    def timed(fn):
        rc = fn()
        torch.cuda.synchronize()
        if rc != 0:
            return dict(status=int(rc))
        for _ in range(a.warmup):
            fn()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        return dict(status=0, us=[round(u, 2) for u in us], mean_us=round(sum(us) / len(us), 2), min_us=round(min(us), 2),
                    max_us=round(max(us), 2))

    res = dict(shape=dict(rows=rows, board_size=n, channels=ch), round_width=a.round_width, order=a.order,
               order_chosen=int(L.elfnet_conv3x3_f16_order(rows, n, n, ch, ch, 0)), launches=a.launches, warmup=a.warmup, repeats=a.repeats,
               device=torch.cuda.get_device_name(0), method="HIP events around back-to-back launches, µs per convolution")
    with torch.no_grad():
        for skip, rr in (("noskip", None), ("skip", r)):
            if not a.no_pair:
                res["pair_" + skip] = timed(pair(rr))
            for algo in [v if v == "small" else int(v) for v in a.algos.split(",") if v != ""]:
                res["fused%s_%s" % (algo, skip)] = timed(fused(algo, rr))
                print(skip, "algo", algo, res["fused%s_%s" % (algo, skip)], flush=True)
            if not a.no_pair:
                print(skip, "pair", res["pair_" + skip], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
