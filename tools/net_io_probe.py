"""Times the two ends of the fp16 net (elf_amd/csrc/net_io.hip) against what ran before, at one batch size, in ONE process:
    in_conv   the 18 -> dim input convolution with bias and ReLU:
                pair    F.conv2d (MIOpen) followed by elfnet_bias_act_f16
                native  elfnet_conv3x3_in_f16
    heads     trunk activation -> pi, V:
                eager   the op sequence of FusedInferenceNet.__call__ (two 1x1 convolutions, three Linear layers, softmax, tanh)
                native  elfnet_heads_f16
    net       the whole call of a --blocks x --dim net captured into a graph:
                fused   GraphedNet(FusedInferenceNet)
                native  GraphedNet(NativeInferenceNet)
HIP events around `--launches` back-to-back launches after a warm-up, `--repeats` times; mean / min / max of the repeats in µs per
call.  One process per shape; run it under a time limit and give each shape its own --key in the one output file:
    timeout -k 10 300 python tools/net_io_probe.py --rows 2048 --key rows2048 [--out profiles/net_native_io.json]
    timeout -k 10 300 python tools/net_io_probe.py --rows 16 --key rows16
The floor of either kernel is one pass over the [rows,19,19,256] fp16 activation (378 MB at 2048 rows: about 75 µs at 5 TB/s)."""
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
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-net", action="store_true", help="leave the whole-net comparison out")
    ap.add_argument("--key", default=None, help="store the result under this key of --out (other keys are kept)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_native_io.json"))
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
    from elf_amd.net import FusedInferenceNet, GraphedNet, NativeInferenceNet, make_net
    L = elf_amd.lib()
    rows, n, dim = a.rows, a.board_size, a.dim
    d = n * n
    net = make_net(board_size=n, num_block=a.blocks, dim=dim, fold_bn=True)
    native = NativeInferenceNet(net)
    g = torch.Generator(device="cuda").manual_seed(7)
    s = (torch.rand((rows, n, n, 18), device="cuda", generator=g) < 0.3).half().permute(0, 3, 1, 2)   # binary planes, channels_last
    act = torch.relu(torch.randn((rows, n, n, dim), device="cuda", generator=g)).half().permute(0, 3, 1, 2)
    first = net.init_conv[0]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    y = torch.empty((rows, dim, n, n), device="cuda", dtype=torch.float16, memory_format=torch.channels_last)
    pi = torch.empty((rows, d + 1), device="cuda", dtype=torch.float32)
    v = torch.empty((rows,), device="cuda", dtype=torch.float32)
    nb = L.elfnet_heads_workspace(rows, n, n)
    ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)

    def in_pair():
        o = torch.nn.functional.conv2d(s, first.weight, None, 1, 1)
        return L.elfnet_bias_act_f16(p(o), p(first.bias), None, rows * d, dim, 1, st)

    def in_native():
        return L.elfnet_conv3x3_in_f16(p(s), p(first.weight), p(first.bias), p(y), rows, n, n, 18, dim, 1, st)

    def heads_eager():
        a_pi = net.pi_linear(net.pi_final_conv(act).reshape(-1, 2 * d))
        torch.softmax(a_pi.float(), dim=1)
        a_v = torch.relu(net.value_linear1(net.value_final_conv(act).reshape(-1, d)))
        torch.tanh(net.value_linear2(a_v)).float().reshape(-1)
        return 0

    def heads_native():
        return L.elfnet_heads_f16(p(act), C.byref(native.heads), rows, n, n, p(pi), d + 1, p(v), None, p(ws), nb, st)

    def timed(fn):
        rc = fn()
        torch.cuda.synchronize()
        if rc:
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

    res = dict(shape=dict(rows=rows, board_size=n, channels=dim, blocks=a.blocks), launches=a.launches, warmup=a.warmup,
               repeats=a.repeats, device=torch.cuda.get_device_name(0), method="HIP events around back-to-back launches, µs per call",
               floor_us_one_pass_at_5TBs=round(rows * d * dim * 2 / 5e12 * 1e6, 1))
    with torch.no_grad():
        for name, fn in (("in_conv_pair", in_pair), ("in_conv_native", in_native), ("heads_eager", heads_eager),
                         ("heads_native", heads_native)):
            res[name] = timed(fn)
            print(name, res[name], flush=True)
        if not a.no_net:
            for name, cls in (("net_fused_graphed", FusedInferenceNet), ("net_native_graphed", NativeInferenceNet)):
                gn = GraphedNet(cls(net), s)
                res[name] = timed(lambda: gn() and 0)
                print(name, res[name], flush=True)
                del gn
    out = {}
    if a.key and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    if a.key:
        out[a.key] = res
    else:
        out = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
