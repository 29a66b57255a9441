"""GPU: the small-tile trunk convolution (elfnet_conv3x3_small_f16, elf_amd/csrc/net_conv3x3_small.hip: 64 positions x 64 channels
per workgroup, for a single game's net call) on inputs whose result is exact -- small integers, so every partial sum is an integer
fp32 and fp16 hold exactly and any differing element is a wrong halo, layout, swizzle or pipeline timing, never rounding -- then bit
for bit against algo 0 (same K order, same MFMA), a race screen (repeated launches return the bits of the first), batch
invariance, the calls it refuses, and whole nets routed through it and past it.  Then what only this kernel has: a grid larger
than one residency, tail tiles on either side of the wave split, poison beside the tail, the skip's clamped rows behind M, both
size limits and one launch at the top of the accepted range (its 32-bit byte offsets at their largest), and a single game's search
served through it.  The battery it shares with algos 0 and 1 is sections B and C of test_gpu_net_edges.py."""
import ctypes as C

import pytest

import conv_cases as cc
from conv_cases import NAN, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 77 + rows + 1000 * h + 31 * wd + c + 7 * k


def _rseed(rows, h, wd, c, k):
    return 4242 + rows + h + c + k


def _small(L, x, w, b, r, y, rows, h, wd, relu, c, k):
    return cc.launch(L, "small", x, w, b, r, y, relu, shape=(rows, h, wd, c, k))


def _algo0(L, x, w, b, r, y, rows, h, wd, relu, c, k):
    return cc.launch(L, "algo0", x, w, b, r, y, relu, shape=(rows, h, wd, c, k))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("rows,h,wd,c,k", [(1, 19, 19, 256, 256),   # M = 361: five full 64-tiles and a 41-row tail; four channel columns
                                           (5, 9, 9, 256, 256),     # M = 405: tiles straddle boards
                                           (64, 1, 1, 64, 64),      # M = 64 exactly, no tail; every tap but the centre is off-board; 9 K tiles
                                           (3, 9, 9, 192, 128),     # 27 K tiles (an odd count), two channel columns
                                           (2, 3, 7, 64, 192),      # h != wd
                                           (1, 1, 19, 64, 64),      # a one-line board
                                           (1, 2, 2, 64, 64),       # M = 4: a single tile that is almost all tail
                                           (5, 9, 9, 128, 256),     # two K chunks per tap: the prologue's K tile 2 is (tap 1, chunk 0)
                                           (1, 5, 7, 64, 64),       # M = 35: the tail spills 3 rows into the second wave row
                                           (1, 19, 19, 64, 512),    # eight channel columns
                                           (1, 3, 11, 64, 64)])     # M = 33: a second wave row with one valid position
def test_exact_integers(elf, rows, h, wd, c, k, use_res, relu):
    """equality with the nine-tap fp32 form; y is prefilled with NaN, and one guard row of NaN behind y's last row stays NaN (the
    tail tile's stores are masked)"""
    import torch
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    ref = d["conv"] + d["b"].float()
    if use_res:
        ref = ref + d["r"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = cc.guarded(rows, h, wd, k)
    rc = _small(elf.lib(), d["x"], d["w"], d["b"], d["r"] if use_res else None, y, rows, h, wd, relu, c, k)
    assert rc == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("rows %d h %d wd %d c %d k %d res %d relu %d: %d of %d differ" % (rows, h, wd, c, k, use_res, relu, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("n", [19, 9])
def test_all_ones_halo(elf, n):
    """x = 1, w = 1, bias = 0: every output is 256 x the number of on-board taps: 1024 at corners, 1536 on edges, 2304 inside"""
    import torch
    rows, ch = 2, 256
    x = torch.ones((rows, n, n, ch), device="cuda", dtype=torch.float16)
    w = torch.ones((ch, 3, 3, ch), device="cuda", dtype=torch.float16)
    b = torch.zeros((ch,), device="cuda", dtype=torch.float16)
    y = torch.full((rows, n, n, ch), float("nan"), device="cuda", dtype=torch.float16)
    assert _small(elf.lib(), x, w, b, None, y, rows, n, n, 0, ch, ch) == 0
    torch.cuda.synchronize()
    i = torch.arange(n, device="cuda")
    on = 3 - ((i == 0) | (i == n - 1)).long()           # taps on the board along one axis
    want = (256 * on[:, None] * on[None, :]).float()    # [n, n]
    assert want[0, 0] == 1024 and want[0, 1] == 1536 and want[1, 1] == 2304
    assert bool((y.float() == want[None, :, :, None]).all())


_first = {}


def _first_launch(rows, n, c, k):
    """cc.rand_case's operands and y, the first launch of the small entry on them, with skip and ReLU; nobody writes it again"""
    import torch
    key = (rows, n, c, k)
    if key not in _first:
        x, w, b, r = cc.rand_case(_rseed(rows, n, n, c, k), rows, n, n, c, k)
        y = torch.full((rows, n, n, k), float("nan"), device="cuda", dtype=torch.float16)
        assert _small(__import__("elf_amd").lib(), x, w, b, r, y, rows, n, n, 1, c, k) == 0
        torch.cuda.synchronize()
        _first[key] = (x, w, b, r, y)
    return _first[key]


@pytest.mark.parametrize("rows,n,c,k", [(16, 19, 256, 256), (3, 9, 128, 64)])
def test_bit_equal_with_algo_0(elf, rows, n, c, k):
    """the single game's own call, and a smaller one, with skip and ReLU: algo 0's accumulation chain (tap-major K; in every
    32-channel block one 32x32x16 MFMA over channels {0..7, 16..23}, the next over {8..15, 24..31}) and its epilogue sequence, so
    the two outputs are the same bits"""
    import torch
    x, w, b, r, got = _first_launch(rows, n, c, k)
    y0 = torch.full((rows, n, n, k), float("nan"), device="cuda", dtype=torch.float16)
    assert _algo0(elf.lib(), x, w, b, r, y0, rows, n, n, 1, c, k) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(y0).any())
    print("%d of %d elements differ between the small kernel and algo 0" % (int((got != y0).sum().item()), y0.numel()))
    assert torch.equal(got, y0)


def test_repeated_launches_return_the_same_bits(elf):
    """A staged buffer read before its data has landed, or restaged before its last read, gives wrong tiles that come and go.  The
    same 16-row inputs launched 20 times return the bits of the first launch."""
    import torch
    rows = 16
    x, w, b, r, first = _first_launch(rows, 19, 256, 256)
    assert not bool(torch.isnan(first).any())
    for i in range(1, 20):
        y = torch.full((rows, 19, 19, 256), float("nan"), device="cuda", dtype=torch.float16)
        assert _small(elf.lib(), x, w, b, r, y, rows, 19, 19, 1, 256, 256) == 0
        torch.cuda.synchronize()
        assert torch.equal(y, first), "launch %d differs from the first" % i


@pytest.mark.parametrize("row", [0, 7, 15])
def test_a_row_does_not_depend_on_its_batch(elf, row):
    """a row of the 16-row call, run as a 1-row call (other tiles, other tails), returns the bits it has in the batch"""
    import torch
    x, w, b, r, batch = _first_launch(16, 19, 256, 256)
    x1, r1 = x[row:row + 1].contiguous(), r[row:row + 1].contiguous()
    y = torch.full((1, 19, 19, 256), float("nan"), device="cuda", dtype=torch.float16)
    assert _small(elf.lib(), x1, w, b, r1, y, 1, 19, 19, 1, 256, 256) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[0], batch[row])


@pytest.mark.parametrize("case", ["c72", "k72", "c32", "x_off_by_8", "y_is_x", "y_is_res"])
def test_refusals_leave_y_alone(elf, case):
    """a negative status, nothing launched, y keeps its bytes"""
    import torch
    rows, n = 2, 9
    c = dict(c72=72, c32=32).get(case, 64)
    k = 72 if case == "k72" else 64
    z = lambda *shape: torch.zeros(shape, device="cuda", dtype=torch.float16)
    x, w, b, r = z(rows * n * n * c + 8), z(k, 3, 3, c), z(k), z(rows, n, n, k)
    y = torch.full((rows, n, n, k), 7.0, device="cuda", dtype=torch.float16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, pr, py = x.data_ptr(), r.data_ptr(), y.data_ptr()
    if case == "x_off_by_8":
        px += 8
    elif case == "y_is_x":
        px = py          # c == k == 64: y's buffer is large enough to be read as x
    elif case == "y_is_res":
        pr = py
    rc = elf.lib().elfnet_conv3x3_small_f16(C.c_void_p(px), cc.ptr(w), cc.ptr(b), C.c_void_p(pr), C.c_void_p(py), rows, n, n, c, k, 1,
                                            st)
    assert rc < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_no_rows_is_accepted_and_launches_nothing(elf):
    import torch
    n, ch = 9, 64
    x = torch.zeros((1, n, n, ch), device="cuda", dtype=torch.float16)
    w = torch.zeros((ch, 3, 3, ch), device="cuda", dtype=torch.float16)
    b = torch.zeros((ch,), device="cuda", dtype=torch.float16)
    y = torch.full((1, n, n, ch), 7.0, device="cuda", dtype=torch.float16)
    assert _small(elf.lib(), x, w, b, None, y, 0, n, n, 1, ch, ch) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------ whole nets

_net = {}


def _net_case():
    import torch
    from elf_amd.net import make_net
    if not _net:
        net = make_net(9, num_block=2, dim=64, fold_bn=True)
        g = torch.Generator(device="cuda").manual_seed(99)
        s = torch.randint(0, 2, (16, 18, 9, 9), device="cuda", generator=g).half().contiguous(memory_format=torch.channels_last)
        _net["v"] = (net, s)
    return _net["v"]


class _Calls:
    """counts the calls of the small entry that go through a net's library handle"""

    def __init__(self, L):
        self.L, self.small = L, 0

    def __getattr__(self, name):
        f = getattr(self.L, name)
        if name != "elfnet_conv3x3_small_f16":
            return f

        def counted(*a):
            self.small += 1
            return f(*a)
        return counted


@pytest.mark.parametrize("cls", ["FusedInferenceNet", "NativeInferenceNet"])
def test_whole_net_routed_through_the_small_kernel_returns_the_same_bits(elf, cls):
    """9 x 9, 2 blocks of 64 channels, 16 rows (1 296 positions): small_max_positions = 0 sends every trunk convolution to algo 0,
    32768 sends all four to the small kernel; pi and V are the same bits"""
    import torch
    import elf_amd.net as N
    net, s = _net_case()
    outs, calls = [], []
    for limit in (0, 32768):
        f = getattr(N, cls)(net)
        f.small_max_positions = limit
        f.L = _Calls(f.L)
        outs.append(f({"s": s}))
        torch.cuda.synchronize()
        calls.append(f.L.small)
    assert calls == [0, 4]
    assert torch.equal(outs[0]["pi"], outs[1]["pi"]) and torch.equal(outs[0]["V"], outs[1]["V"])
    assert not bool(torch.isnan(outs[1]["pi"]).any()) and not bool(torch.isnan(outs[1]["V"]).any())


def test_whole_net_replays_from_a_graph_to_the_same_bits(elf):
    """the small kernel's launch is capturable: GraphedNet's replay equals the eager call"""
    import torch
    from elf_amd.net import GraphedNet, NativeInferenceNet
    net, s = _net_case()
    native = NativeInferenceNet(net)
    native.small_max_positions = 32768
    eager = native({"s": s})
    torch.cuda.synchronize()
    s_static = s.clone(memory_format=torch.preserve_format)
    out = GraphedNet(native, s_static)()
    torch.cuda.synchronize()
    assert torch.equal(out["pi"], eager["pi"]) and torch.equal(out["V"], eager["V"])


# ------------------------------------------------------------------------------------------------ what only this kernel has

def test_more_workgroups_than_are_resident(elf):
    """Three workgroups of 48 KiB LDS fit a CU, 768 on the chip's 256 CUs.  200 rows of 9 x 9 are 16 200 positions = 254 tiles x
    4 channel columns = 1 016 workgroups: with and without skip, with and without ReLU, the result is the integer nine-tap form and
    algo 0's output bit for bit; the guard row behind y stays NaN (test_gpu_net_edges.test_algo_1_beyond_one_round_of_workgroups)."""
    import torch
    rows, h, wd, c, k = 200, 9, 9, 64, 256
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    assert (rows * h * wd + 63) // 64 == 254 and 254 * (k // 64) == 1016 > 3 * 256
    for use_res in (False, True):
        for relu in (0, 1):
            r = d["r"] if use_res else None
            ref = d["conv"] + d["b"].float()
            if use_res:
                ref = ref + r.float()
            if relu:
                ref = torch.relu(ref)
            buf, y = cc.guarded(rows, h, wd, k)
            assert _small(elf.lib(), d["x"], d["w"], d["b"], r, y, rows, h, wd, relu, c, k) == 0
            buf0, y0 = cc.guarded(rows, h, wd, k)
            assert _algo0(elf.lib(), d["x"], d["w"], d["b"], r, y0, rows, h, wd, relu, c, k) == 0
            torch.cuda.synchronize()
            bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
            bits = int((y.view(torch.int16) != y0.view(torch.int16)).sum().item())
            print("res %d relu %d: %d of %d differ from the integer form, %d from algo 0's bits" % (use_res, relu, bad, y.numel(), bits))
            assert bad == 0
            assert bits == 0
            assert bool(torch.isnan(buf[-1]).all()) and bool(torch.isnan(buf0[-1]).all())


@pytest.mark.parametrize("pos", [360, 351, 352])
def test_one_nan_next_to_the_tail(elf, pos):
    """1 x 19 x 19 is M = 361: five full tiles and a tail tile of 41 rows, positions 320 .. 360, whose wave split lies between 351
    and 352.  One x element at position 360 (the last valid row: the rows behind it are staged from the zero line), 351 or 352 set
    to NaN, no ReLU, no skip: the output is NaN at exactly the 3 x 3 neighbourhood of that cell on the board, in all K channels,
    and the clean result everywhere else (test_gpu_net_edges.test_one_poisoned_input_element); the guard row stays NaN."""
    import torch
    rows, h, wd, c, k = 1, 19, 19, 256, 256
    assert rows * h * wd == 5 * 64 + 41 and 5 * 64 + 32 == 352
    i, j = divmod(pos, wd)
    assert (i, j) in ((18, 18), (18, 9), (18, 10))
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    clean = d["conv"] + d["b"].float()
    x = d["x"].clone()
    touched = torch.zeros((rows, h, wd), device="cuda", dtype=torch.bool)
    touched[0, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = True
    assert int(touched.sum().item()) == (4 if pos == 360 else 6)
    for ch in (0, 100, c - 1):
        keep = x[0, i, j, ch].item()
        x[0, i, j, ch] = NAN
        buf, y = cc.guarded(rows, h, wd, k)
        assert _small(elf.lib(), x, d["w"], d["b"], None, y, rows, h, wd, 0, c, k) == 0
        torch.cuda.synchronize()
        yf = y.float()
        assert bool(torch.isfinite(yf[~touched]).all()), ch
        assert bool((yf[~touched] == clean[~touched]).all()), ch
        assert bool(torch.isnan(yf[touched]).all()), ch
        assert bool(torch.isnan(buf[-1]).all())
        x[0, i, j, ch] = keep
    assert torch.equal(x, d["x"])


@pytest.mark.parametrize("rows,h,wd,c,k", [(1, 5, 7, 64, 64),        # M = 35: 29 rows of the one tile lie behind M
                                           (5, 9, 9, 256, 256)])     # M = 405: 43 rows of the tail tile do
def test_res_behind_the_last_row(elf, rows, h, wd, c, k):
    """For a row at or beyond M the kernel loads the skip of row M - 1 and stores nothing.  res and y lie between NaN guards
    (16-byte, not 32-byte aligned); no ReLU, so a skip value taken from behind res would reach the result as NaN: the result is
    the integer form exactly and both guards of y are still all NaN."""
    import torch
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    guard = (wd + 2) * max(c, k)
    assert rows * h * wd % 64 != 0    # there are rows behind M in the last tile
    r, _, _ = cc.carve(d["r"], guard)
    y, front, back = cc.carve(torch.full((rows, h, wd, k), NAN, device="cuda", dtype=torch.float16), guard)
    ref = d["conv"] + d["b"].float() + d["r"].float()
    assert _small(elf.lib(), d["x"], d["w"], d["b"], r, y, rows, h, wd, 0, c, k) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())
    print("%s: %d of %d differ" % ((rows, h, wd, c, k), bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())


def test_the_first_refused_weight_size(elf):
    """k * 9 * c >= 2^30 elements is refused (the weight's byte offsets are 32-bit): c = k = 10 944 = 171 x 64 is the first square
    size at or above it, 10 880 = 170 x 64 the last below.  A negative status, nothing launched, y keeps its bytes (the buffers
    here are tiny: the call must not touch them).  The accepted side is not launched."""
    import torch
    ck = 10944
    assert ck % 64 == 0 and ck * ck * 9 == 1077940224 >= 2 ** 30 > (ck - 64) * (ck - 64) * 9
    z = lambda *shape: torch.zeros(shape, device="cuda", dtype=torch.float16)
    x, w, b = z(1, 1, 1, ck), z(64, 3, 3, 64), z(ck)
    y = torch.full((1, 1, 1, ck), 7.0, device="cuda", dtype=torch.float16)
    assert _small(elf.lib(), x, w, b, None, y, 1, 1, 1, 1, ck, ck) < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


def test_the_top_of_the_accepted_range(elf):
    """The largest call the entry takes at c = k = 64 on 19 x 19: rows * 361 * 64 < 2^30 elements, x and y just below 2^31 bytes
    each, so the kernel's 32-bit byte offsets (position * 128 plus a tap's distance) are as large as they get.  One more row is
    refused.  x in {-1, 0, 1}, the integer weights and bias of cc.int_case; one launch, no skip, no ReLU.  Three slices of two boards
    each -- the first two, the two around byte offset 2^30 of x, the last two -- equal the integer nine-tap form of those boards
    alone; no row of y is left NaN and the guard row behind y still is."""
    import time
    import torch
    h = wd = 19
    c = k = 64
    rows = (2 ** 30 - 1) // (h * wd * c)
    assert rows * h * wd * c < 2 ** 30 <= (rows + 1) * h * wd * c and rows == 46474
    m = rows * h * wd
    assert 2 ** 31 - 2 * h * wd * c <= m * c * 2 < 2 ** 31
    d = cc.int_case(_seed(2, h, wd, c, k), 2, h, wd, c, k)
    w, b = d["w"], d["b"]
    g = torch.Generator(device="cuda").manual_seed(2 ** 30)
    x = torch.randint(-1, 2, (rows, h, wd, c), device="cuda", dtype=torch.int8, generator=g).half()
    buf = torch.full((m + 1, k), NAN, device="cuda", dtype=torch.float16)
    y = buf[:m].view(rows, h, wd, k)
    assert _small(elf.lib(), x, w, b, None, y, rows + 1, h, wd, 0, c, k) < 0      # refused: nothing is launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-2]).all())
    t0 = time.perf_counter()
    assert _small(elf.lib(), x, w, b, None, y, rows, h, wd, 0, c, k) == 0
    torch.cuda.synchronize()
    print("the launch of %d rows (%d tiles): %.1f ms" % (rows, (m + 63) // 64, 1e3 * (time.perf_counter() - t0)))
    mid = 2 ** 30 // (h * wd * c * 2)            # the board that holds byte 2^30 of x, or begins there
    assert (mid - 1) * h * wd * c * 2 < 2 ** 30 < (mid + 1) * h * wd * c * 2 and 2 < mid - 1 and mid + 1 < rows - 2
    for lo in (0, mid - 1, rows - 2):
        xs = x[lo:lo + 2]
        assert bool((xs != 0).any())
        ref = cc.conv_fp32(xs.float(), w.float()) + b.float()
        bad = int((y[lo:lo + 2].float() != ref).sum().item())
        print("boards %d and %d: %d of %d differ" % (lo, lo + 1, bad, ref.numel()))
        assert bad == 0
    assert not bool(torch.isnan(y).any())
    assert bool(torch.isnan(buf[-1]).all())


def test_a_single_games_search_through_the_small_kernel(elf):
    """What the kernel is for: one 9 x 9 game searched with 32 rollouts per move in batches of at most 8, every net call evaluated
    twice -- NativeInferenceNet with small_max_positions = 0 (algo 0) and with 23 104 (the small kernel, four calls per
    evaluation) -- on the feature rows the search really produces, at the row counts it really produces.  pi and V are the same
    bits at every step; the search is fed the small kernel's; four searches are logged and the trees keep their invariants."""
    import torch
    from elf_amd.net import NativeInferenceNet
    net, _ = _net_case()
    base, small = NativeInferenceNet(net), NativeInferenceNet(net)
    base.small_max_positions = 0
    small.small_max_positions = 23104
    base.L, small.L = _Calls(base.L), _Calls(small.L)
    sp = elf.SelfPlay(board_size=9, num_games=1, mcts_rollout_per_thread=32, mcts_rollout_per_batch=8, feature_format="f16_nhwc",
                      seed=5, log_searches=4)
    steps, evals, seen = 0, 0, set()
    try:
        while sp.stats()["logged"] < 4 and steps < 200:
            rows = sp.begin_step()
            if rows:
                s = sp.s[:rows]
                a, o = base({"s": s}), small({"s": s})
                torch.cuda.synchronize()
                assert torch.equal(a["pi"], o["pi"]) and torch.equal(a["V"], o["V"]), (steps, rows)
                assert bool(torch.isfinite(o["pi"]).all()) and bool(torch.isfinite(o["V"]).all())
                seen.add(int(rows))
                evals += 1
                sp.end_step(o["pi"], o["V"])
            else:
                sp.end_step(None, None)
            steps += 1
        assert sp.stats()["logged"] >= 4
        assert sp.validate_trees()[0] == 0
    finally:
        sp.close()
    print("%d steps, %d evaluations, row counts %s" % (steps, evals, sorted(seen)))
    assert base.L.small == 0 and small.L.small == 4 * evals and evals > 0
    assert len(seen) > 1
