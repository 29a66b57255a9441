"""GPU: the edges of the four net kernels (k_bias_act of net_epilogue.hip and the three trunk convolution entries: elfnet_conv3x3_f16's
algo 0 of net_conv.hip and algo 1 of net_conv3x3.hip, and elfnet_conv3x3_small_f16 of net_conv3x3_small.hip) that the other
test_gpu_net*.py files do not reach, every comparison exact (equal as values, NaN in the same places; no tolerance anywhere).
Sections B and C run every convolution case through all three entries (algo 0, algo 1, "small"), and their poison sites sit on
the seams of both tilings: 256 positions for algos 0 and 1; 64 (tile), 32 (wave split) and 8 (staging piece) for the small kernel:
  A  algo 1 with more workgroups than the chip has CUs (a second and a third round), against the integer nine-tap form and,
     bit for bit, against algo 0;
  B  which cells a cell influences (one poisoned input element, one poisoned weight), operands that lie between NaN guards at
     an address that is 16-byte and not 32-byte aligned, res == x;
  C  the two roundings of the convolution's epilogue told apart, fp16 subnormals in and out, what the ReLU does to NaN,
     k_bias_act (f16 and bf16, all four variants) over a grid-stride loop that runs more than once and over a table of special
     values, and the size limit;
  D  algo 0 at the channel counts FusedInferenceNet._fusable sends it (8, 40, 72, 264);
  E  FusedInferenceNet's trunk routed to algo 1 by size, a chunked call's mix of the two algos (algo 1 and algo 0 by default, algo 1
     and the small kernel with small_max_positions set), and algo 1 inside a captured graph.
References are plain torch fp32 formulas written out here, or algo 0 where bit equality is the claim."""
import ctypes as C

import pytest

import conv_cases as cc
from conv_cases import NAN, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu

INF = float("inf")

ENTRIES = [0, 1, "small"]   # elfnet_conv3x3_f16's two algos and elfnet_conv3x3_small_f16
HOW = {0: "algo0", 1: "plain", "small": "small"}     # conv_cases.launch's names of them


def _seed(rows, h, wd, c, k):
    return 77 + rows + 1000 * h + 31 * wd + c + 7 * k


# ---------------------------------------------------------------------------------------------------------------------------------
# A. algo 1 beyond one round of workgroups

@pytest.mark.parametrize("rows,h,wd,c,k", [(810, 9, 9, 64, 256),     # M = 65 610: 256 full tiles and a 74-row tail, 257 workgroups
                                           (406, 9, 9, 64, 512),     # 129 tiles x 2 channel tiles = 258; the tail tile has 118 rows
                                           (1620, 9, 9, 64, 256),    # 513 tiles: a third round
                                           (810, 9, 9, 128, 256)])   # the 257 tiles with 18 K tiles
def test_algo_1_beyond_one_round_of_workgroups(elf, rows, h, wd, c, k):
    """More workgroups than the 256 CUs: with and without skip, with and without ReLU, algo 1 equals the integer nine-tap form and
    is algo 0's output bit for bit; the guard row behind y stays NaN."""
    import torch
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    assert (rows * h * wd + 255) // 256 * (k // 256) > 256
    for use_res in (False, True):
        for relu in (0, 1):
            r = d["r"] if use_res else None
            ref = d["conv"] + d["b"].float()
            if use_res:
                ref = ref + r.float()
            if relu:
                ref = torch.relu(ref)
            buf, y = cc.guarded(rows, h, wd, k)
            assert cc.launch(elf.lib(), "plain", d["x"], d["w"], d["b"], r, y, relu) == 0
            buf0, y0 = cc.guarded(rows, h, wd, k)
            assert cc.launch(elf.lib(), "algo0", d["x"], d["w"], d["b"], r, y0, relu) == 0
            torch.cuda.synchronize()
            bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
            bits = int((y.view(torch.int16) != y0.view(torch.int16)).sum().item())
            print("%s res %d relu %d: %d of %d differ from the integer form, %d from algo 0's bits"
                  % ((rows, h, wd, c, k), use_res, relu, bad, y.numel(), bits))
            assert bad == 0
            assert bits == 0
            assert bool(torch.isnan(buf[-1]).all()) and bool(torch.isnan(buf0[-1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# B. locality, bounds and alignment

@pytest.mark.parametrize("algo", ENTRIES)
@pytest.mark.parametrize("rows,h,wd,c,k,res", [(5, 9, 9, 256, 256, None), (5, 9, 9, 256, 256, "r"), (5, 9, 9, 256, 256, "x"),
                                               (11, 5, 7, 64, 256, None), (11, 5, 7, 64, 256, "r")])
def test_guarded_operands_at_16_byte_alignment(elf, rows, h, wd, c, k, res, algo):
    """x, w, bias, res and y each between guards of NaN ((w + 2) * max(c, k) elements or more) and each 16-byte, not 32-byte,
    aligned; no ReLU, so a NaN read from outside an operand reaches the result.  The result is the integer nine-tap form
    exactly, and both guards of y are still all NaN.  res == "x" passes x itself as the skip (c == k), which the ABI allows."""
    import torch
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    guard = (wd + 2) * max(c, k)
    x, _, _ = cc.carve(d["x"], guard)
    w, _, _ = cc.carve(d["w"], guard)
    b, _, _ = cc.carve(d["b"], guard)
    r = None
    ref = d["conv"] + d["b"].float()
    if res == "r":
        r, _, _ = cc.carve(d["r"], guard)
        ref = ref + d["r"].float()
    elif res == "x":
        assert c == k
        r = x
        ref = ref + d["x"].float()
    y, front, back = cc.carve(torch.full((rows, h, wd, k), NAN, device="cuda", dtype=torch.float16), guard)
    for t in (x, w, b, y) + ((r,) if r is not None else ()):
        assert t.data_ptr() % 32 == 16
    assert cc.launch(elf.lib(), HOW[algo], x, w, b, r, y, 0) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())
    print("%s res %s algo %s: %d of %d differ" % ((rows, h, wd, c, k), res, algo, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())


# (board, row, column) on 5 boards of 9 x 9, M = 405
POISON_SITES = [(0, 0, 0), (0, 0, 8), (0, 8, 0), (0, 8, 8),   # the four corners of one board
                (1, 8, 8), (2, 0, 0),                         # neighbours in memory and not on the board
                (3, 1, 3), (3, 1, 4),                         # positions 255 and 256: the tile seam
                (4, 8, 8),                                    # position 404: the last valid row of the tail tile
                # the small kernel's seams (64-position tiles, two wave rows of 32, staging pieces of 8 rows)
                (0, 0, 7),                                    # position 7: with the corner (0, 0, 8) above, a staging-piece seam
                (0, 3, 4), (0, 3, 5),                         # positions 31 and 32: the wave split
                (0, 7, 0), (0, 7, 1),                         # positions 63 and 64: the 64-tile seam
                (4, 6, 5), (4, 6, 6)]                         # positions 383 and 384: the last row of the last full 64-tile and the
                                                              # first of its 21-row tail tile


@pytest.mark.parametrize("algo", ENTRIES)
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("poison", [NAN, INF])
def test_one_poisoned_input_element(elf, poison, c, algo):
    """One x[b, i, j, ch] set to NaN (or +Inf), no ReLU, no skip: the output is not finite at exactly the cells (b, i', j') with
    |i - i'| <= 1 and |j - j'| <= 1 of board b, in all K channels (NaN x 0 is NaN: the weights do not matter), and everywhere else
    it is the unpoisoned result.  With +Inf the affected cells are NaN, +Inf or -Inf as the nine-tap fp32 form of the poisoned input
    has them."""
    import torch
    rows, h, wd, k = 5, 9, 9, 256
    assert [(b * h + i) * wd + j for b, i, j in POISON_SITES[6:]] == [255, 256, 404, 7, 31, 32, 63, 64, 383, 384]
    assert (0 * h + 0) * wd + 8 == 8 and (0, 0, 8) in POISON_SITES and rows * h * wd == 6 * 64 + 21
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    clean = d["conv"] + d["b"].float()
    x = d["x"].clone()
    for (b, i, j) in POISON_SITES:
        for ch in (0, c - 1):
            keep = x[b, i, j, ch].item()
            x[b, i, j, ch] = poison
            touched = torch.zeros((rows, h, wd), device="cuda", dtype=torch.bool)
            touched[b, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = True
            buf, y = cc.guarded(rows, h, wd, k)
            assert cc.launch(elf.lib(), HOW[algo], x, d["w"], d["b"], None, y, 0) == 0
            torch.cuda.synchronize()
            yf = y.float()
            assert bool(torch.isfinite(yf[~touched]).all()), (b, i, j, ch)
            assert bool((yf[~touched] == clean[~touched]).all()), (b, i, j, ch)
            assert not bool(torch.isfinite(yf[touched]).any()), (b, i, j, ch)
            if poison != poison:
                assert bool(torch.isnan(yf[touched]).all()), (b, i, j, ch)
            else:
                ref = cc.conv_fp32(x.float(), d["w"].float()) + d["b"].float()
                assert cc.differing(y, ref) == 0, (b, i, j, ch)
            assert bool(torch.isnan(buf[-1]).all())
            x[b, i, j, ch] = keep
    assert torch.equal(x, d["x"])


@pytest.mark.parametrize("algo", ENTRIES)
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("k0,ky,kx,last_ch", [(0, 0, 0, False), (255, 2, 1, True), (77, 1, 1, True), (130, 1, 2, False)])
def test_one_poisoned_weight(elf, k0, ky, kx, last_ch, c, algo):
    """One w[k0, ky, kx, ch] set to +Inf, no ReLU, no skip: every channel but k0 is the unpoisoned result, and channel k0 is the
    nine-tap fp32 form of the same inputs -- +Inf, -Inf or NaN (x = 0) where the tap is on the board, NaN where it is off the
    board, because zero padding times Inf is NaN."""
    _one_poisoned_weight(elf, k0, ky, kx, c - 1 if last_ch else 0, c, algo)


@pytest.mark.parametrize("algo", ENTRIES)
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("k0,ky,kx,where", [(31, 0, 2, "mid"), (32, 2, 0, "mid"), (63, 1, 0, "mid"), (64, 0, 1, "mid"),
                                            (31, 2, 2, "last"), (32, 0, 0, "first"), (63, 1, 1, "first"), (64, 2, 1, "last")])
def test_one_poisoned_weight_at_the_k_seams(elf, k0, ky, kx, where, c, algo):
    """test_one_poisoned_weight on the output-channel seams of the small kernel: k0 = 31 | 32 is the split between its two wave
    columns, 63 | 64 the edge of its first channel column.  "mid" is an input channel other than 0 and C - 1 that the second MFMA
    of a 32-channel block takes ({8..15, 24..31}): channel 72 for C = 256, in the second 64-channel K chunk of its tap, and
    channel 40 for C = 64, which has one chunk per tap.  The sign of channel k0 follows x[..., ch] at the tap's source cell, so a
    weight channel multiplied with another activation channel (the two operands' swizzles or MFMA halves disagreeing) shows."""
    ch = {"first": 0, "last": c - 1, "mid": 72 if c == 256 else 40}[where]
    assert 0 < ch < c - 1 or where != "mid"
    assert where != "mid" or ((ch % 32) // 8 in (1, 3) and (c == 64 or ch // 64 >= 1))
    _one_poisoned_weight(elf, k0, ky, kx, ch, c, algo)


def _one_poisoned_weight(elf, k0, ky, kx, ch, c, algo):
    import torch
    rows, h, wd, k = 5, 9, 9, 256
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    w = d["w"].clone()
    w[k0, ky, kx, ch] = INF
    ref = cc.conv_fp32(d["x"].float(), w.float()) + d["b"].float()
    clean = d["conv"] + d["b"].float()
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), HOW[algo], d["x"], w, d["b"], None, y, 0) == 0
    torch.cuda.synchronize()
    yf = y.float()
    others = torch.arange(k, device="cuda") != k0
    assert bool((yf[..., others] == clean[..., others]).all())
    assert cc.differing(y, ref) == 0
    # stated directly, not through the reference: the source cell of output (i, j) is (i + ky - 1, j + kx - 1)
    i = torch.arange(h, device="cuda")[:, None] + (ky - 1)
    j = torch.arange(wd, device="cuda")[None, :] + (kx - 1)
    on = ((i >= 0) & (i < h) & (j >= 0) & (j < wd))[None].expand(rows, h, wd)
    assert not bool(torch.isfinite(yf[..., k0]).any())
    assert bool(torch.isnan(yf[..., k0][~on]).all())
    src = torch.nn.functional.pad(d["x"][..., ch].float(), (1, 1, 1, 1))[:, ky:ky + h, kx:kx + wd]
    assert bool((yf[..., k0][on & (src > 0)] == INF).all()) and bool((yf[..., k0][on & (src < 0)] == -INF).all())
    assert bool(torch.isnan(yf[..., k0][on & (src == 0)]).all())
    assert bool(torch.isnan(buf[-1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# C. the two roundings and the value edges

def _cell_kinds(n):
    """[n, n] long: the number of 3 x 3 taps on the board at each cell: 4 at corners, 6 on edges, 9 inside"""
    import torch
    i = torch.arange(n, device="cuda")
    on = 3 - ((i == 0) | (i == n - 1)).long()
    return on[:, None] * on[None, :]


@pytest.mark.parametrize("algo", ENTRIES)
def test_two_roundings_not_one_at_a_tie(elf, algo):
    """x = 1, w = 1 but for the centre tap of one input channel per output channel, which is 2; bias = 1; no skip.  A cell sums
    256 per tap on the board and 1 more: 2305 inside, 1537 on an edge, 1025 at a corner.  The header's sequence gives
    half(2305) = 2304 (a tie, to even), then 2304 + 1 = 2305, which rounds to 2304 again; one rounding of 2306 would give 2306.
    Edge and corner sums stay below 2048, where every integer is an fp16: 1537 + 1 and 1025 + 1."""
    import torch
    rows, n, ch = 2, 9, 256
    x = torch.ones((rows, n, n, ch), device="cuda", dtype=torch.float16)
    w = torch.ones((ch, 3, 3, ch), device="cuda", dtype=torch.float16)
    ko = torch.arange(ch, device="cuda")
    w[ko, 1, 1, (ko * 37 + 5) % ch] = 2.0
    b = torch.ones((ch,), device="cuda", dtype=torch.float16)
    kinds = _cell_kinds(n)
    acc = (256 * kinds + 1).float()
    assert acc[1, 1] == 2305 and acc[0, 1] == 1537 and acc[0, 0] == 1025
    want = torch.where(kinds == 9, 2304.0, torch.where(kinds == 6, 1538.0, 1026.0))
    assert torch.equal((acc.half().float() + 1).half().float(), want) and (acc + 1).half()[1, 1] == 2306   # the two sequences
    for relu in (0, 1):
        buf, y = cc.guarded(rows, n, n, ch)
        assert cc.launch(elf.lib(), HOW[algo], x, w, b, None, y, relu) == 0
        torch.cuda.synchronize()
        print("algo %s relu %d: interior %s edge %s corner %s" % (algo, relu, y[0, 4, 4, 0].item(), y[0, 0, 4, 0].item(), y[0, 0, 0, 0].item()))
        assert bool((y.float() == want[None, :, :, None]).all())
        assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("algo", ENTRIES)
def test_the_first_rounding_overflows_to_inf(elf, algo):
    """x = 32, w = 1, bias = -16384: a cell sums 8192 per tap on the board, 73 728 inside, 49 152 on an edge, 32 768 at a corner.
    half(73 728) is Inf before the bias is added, so the interior is +Inf (one rounding of 73 728 - 16 384 = 57 344 would be
    finite); edges are 49 152 - 16 384 = 32 768 and corners 16 384."""
    import torch
    rows, n, ch = 2, 9, 256
    x = torch.full((rows, n, n, ch), 32.0, device="cuda", dtype=torch.float16)
    w = torch.ones((ch, 3, 3, ch), device="cuda", dtype=torch.float16)
    b = torch.full((ch,), -16384.0, device="cuda", dtype=torch.float16)
    kinds = _cell_kinds(n)
    want = torch.where(kinds == 9, INF, torch.where(kinds == 6, 32768.0, 16384.0))
    assert torch.equal(((8192 * kinds).float().half().float() - 16384).half().float(), want)
    for relu in (0, 1):
        buf, y = cc.guarded(rows, n, n, ch)
        assert cc.launch(elf.lib(), HOW[algo], x, w, b, None, y, relu) == 0
        torch.cuda.synchronize()
        assert bool((y.float() == want[None, :, :, None]).all())
        assert bool(torch.isnan(buf[-1]).all())


def _scaled(ints, shift):
    """fp16 ints * 2^-shift for small integers, built from bit patterns where the values are subnormal (shift 24: the integer IS
    the bit pattern's magnitude) so that no conversion of this test's own can flush them; checked on the device by the caller"""
    import torch
    i = ints.to(torch.int32)
    if shift == 24:
        assert int(i.abs().max().item()) < 1024
        bits = i.abs() | ((i < 0).to(torch.int32) << 15)
        return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.float16)
    return (i.double() * 2.0 ** -shift).half()


@pytest.mark.parametrize("algo", ENTRIES)
@pytest.mark.parametrize("wshift,oshift", [(10, 14), (0, 24)])
def test_subnormal_inputs_and_outputs(elf, wshift, oshift, algo):
    """The integer case scaled by powers of two: x = xi * 2^-24 (every nonzero x is the smallest fp16 subnormal), w = wi * 2^10,
    bias = bi * 2^-14, res = ri * 2^-14; the result is (integer result) * 2^-14 exactly.  The second scaling (w = wi, bias and
    res * 2^-24) gives (integer result) * 2^-24: every input but w and every output is subnormal or zero.  Nothing may be
    flushed at the MFMA's inputs, at either rounding or in between.  The expected values are made on the host."""
    import torch
    rows, n, ch = 2, 9, 256
    d = cc.int_case(_seed(rows, n, n, ch, ch), rows, n, n, ch, ch)
    xi, wi, bi, ri = (d[key].float() for key in ("x", "w", "b", "r"))
    x = _scaled(xi, 24)
    w = (wi * 2.0 ** wshift).half()
    b, r = _scaled(bi, oshift), _scaled(ri, oshift)
    assert torch.equal(x.float() * 2.0 ** 24, xi) and torch.equal(w.float() * 2.0 ** -wshift, wi)
    assert torch.equal(b.float() * 2.0 ** oshift, bi) and torch.equal(r.float() * 2.0 ** oshift, ri)
    assert bool(((x.view(torch.int16)[xi != 0] & 0x7FFF) == 1).all())
    for use_res in (False, True):
        for relu in (0, 1):
            ints = d["conv"] + bi
            if use_res:
                ints = ints + ri
            if relu:
                ints = torch.relu(ints)
            assert float(ints.abs().max().item()) < 1024
            want = (ints.cpu().double() * 2.0 ** -oshift).half()      # exact: |ints| < 2^10, so ints * 2^-24 is an fp16 subnormal
            assert torch.equal(want.double() * 2.0 ** oshift, ints.cpu().double())
            buf, y = cc.guarded(rows, n, n, ch)
            assert cc.launch(elf.lib(), HOW[algo], x, w, b, r if use_res else None, y, relu) == 0
            torch.cuda.synchronize()
            got = y.cpu()
            bad = int((got.double() != want.double()).sum().item())
            sub = int(((want != 0) & (want.abs() < 2.0 ** -14)).sum().item())
            print("algo %s shifts %d/%d res %d relu %d: %d of %d differ; %d expected values are subnormal"
                  % (algo, wshift, oshift, use_res, relu, bad, got.numel(), sub))
            assert bad == 0
            assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("algo", ENTRIES)
@pytest.mark.parametrize("use_res", [False, True])
def test_relu_turns_nan_into_zero(elf, use_res, algo):
    """Pins what the three epilogues do: max(v, 0) is fmaxf, so with relu = 1 a NaN before the activation comes out as +0 (the
    eager net's torch.relu would keep it).  NaN enters through one x element (its 3 x 3 cells, all channels), one bias channel and,
    with skip, one res element; the reference is torch.fmax(v, 0).  With relu = 0 the same NaNs come through."""
    import torch
    rows, n, ch = 2, 9, 256
    d = cc.int_case(_seed(rows, n, n, ch, ch), rows, n, n, ch, ch)
    x, b, r = d["x"].clone(), d["b"].clone(), d["r"].clone()
    x[1, 4, 4, 17] = NAN
    b[200] = NAN
    r[0, 2, 3, 5] = NAN
    v = cc.conv_fp32(x.float(), d["w"].float()) + b.float()
    if use_res:
        v = v + r.float()
    nan = torch.isnan(v)
    expect = torch.zeros_like(nan)
    expect[1, 3:6, 3:6, :] = True
    expect[..., 200] = True
    if use_res:
        expect[0, 2, 3, 5] = True
    assert torch.equal(nan, expect)
    for relu in (1, 0):
        buf, y = cc.guarded(rows, n, n, ch)
        assert cc.launch(elf.lib(), HOW[algo], x, d["w"], b, r if use_res else None, y, relu) == 0
        torch.cuda.synchronize()
        if relu:
            want = torch.fmax(v, torch.zeros((), device="cuda"))
            assert not bool(torch.isnan(want).any())
            assert bool((y.float() == want).all())
            assert bool((y.view(torch.int16)[nan] == 0).all())      # +0, not -0
        else:
            assert cc.differing(y, v) == 0 and torch.equal(torch.isnan(y), nan)
        assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("algo", ENTRIES)
def test_the_first_refused_size(elf, algo):
    """rows * h * w * max(c, k) = 4096 * 32 * 32 * 256 = 2^30 elements is the first size refused: a negative status from every
    entry, nothing launched, y keeps its bytes (the buffers here are small: the call must not touch them)"""
    import torch
    ch = 256
    x = torch.zeros((1, 32, 32, ch), device="cuda", dtype=torch.float16)
    w = torch.zeros((ch, 3, 3, ch), device="cuda", dtype=torch.float16)
    b = torch.zeros((ch,), device="cuda", dtype=torch.float16)
    y = torch.full((1, 32, 32, ch), 7.0, device="cuda", dtype=torch.float16)
    assert 4096 * 32 * 32 * ch == 2 ** 30
    assert cc.launch(elf.lib(), HOW[algo], x, w, b, None, y, 1, shape=(4096, 32, 32, ch, ch)) < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---- k_bias_act

def _bias_act(L, dtype, y, b, r, rows, ch, relu):
    import torch
    fn = L.elfnet_bias_act_f16 if dtype == torch.float16 else L.elfnet_bias_act_bf16
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return fn(p(y), p(b), p(r), rows, ch, int(relu), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _bias_act_ref(x, b, r, relu, dtype):
    """((x + bias) + res) in fp32 in that association, fmax(., 0), one conversion to the storage type; on x's device"""
    import torch
    v = x.float()
    if b is not None:
        v = v + b.float()
    if r is not None:
        v = v + r.float()
    if relu:
        v = torch.fmax(v, torch.zeros((), device=v.device))
    return v.to(dtype)


def _dtype(name):
    import torch
    return {"f16": torch.float16, "bf16": torch.bfloat16}[name]


@pytest.mark.parametrize("rows,ch", [(2 * 65536 + 77, 256),   # 4 196 768 lanes of 8: the capped grid (2 097 152 threads) runs its loop
                                                              # two or three times, and the last pass is ragged
                                     (2 ** 21 + 5, 8)])       # one lane per row (c8 = 1), 5 lanes into a second pass
@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_bias_act_grid_stride_loop_exact(elf, name, rows, ch):
    """All four variants (bias x res), each with and without ReLU, where the grid-stride loop runs more than once: equal to the
    fp32 formula in the kernel's own association -- exactly, the three-addend variants included (there is no fast-math and an
    add chain cannot be contracted)."""
    import torch
    dtype = _dtype(name)
    assert rows * (ch // 8) > 8192 * 256
    g = torch.Generator(device="cuda").manual_seed(rows + ch)
    x = torch.randn((rows, ch), device="cuda", generator=g).to(dtype)
    b = torch.randn((ch,), device="cuda", generator=g).to(dtype)
    r = torch.randn((rows, ch), device="cuda", generator=g).to(dtype)
    for use_bias in (False, True):
        for use_res in (False, True):
            for relu in (0, 1):
                bb, rr = b if use_bias else None, r if use_res else None
                want = _bias_act_ref(x, bb, rr, relu, dtype)
                y = x.clone()
                assert _bias_act(elf.lib(), dtype, y, bb, rr, rows, ch, relu) == 0
                torch.cuda.synchronize()
                bad = int((y != want).sum().item())
                print("%s %s bias %d res %d relu %d: %d of %d differ" % (name, (rows, ch), use_bias, use_res, relu, bad, y.numel()))
                assert bad == 0


def _special_table(name):
    """(x, res) pairs as bit patterns, one case per row: -> (x [64, 8], res [64, 8], bias [8]) on the host, every row one case in all
    eight lanes of an H8; the bias differs by lane (lane 0 is +0, which leaves a row's case as it is)."""
    import numpy as np
    import torch
    if name == "f16":
        nan, inf, ninf, one, zero, nzero = 0x7E00, 0x7C00, 0xFC00, 0x3C00, 0x0000, 0x8000
        min_sub, max_sub, min_norm, big = 0x0001, 0x03FF, 0x0400, 0x7BFF
        pairs = [(0x6800, one),        # 2048 + 1: a tie between 2048 and 2050, to the even neighbour below
                 (0x6801, one),        # 2050 + 1: a tie between 2050 and 2052, to the even neighbour above
                 (big, 0x4C00),        # 65504 + 16 = 65520: a tie between 65504 and 2^16, which is even: Inf
                 (big, 0x4B80),        # 65504 + 15: stays 65504
                 (0xFBFF, 0xCC00),     # -65504 - 16: -Inf
                 (0x0600, 0x8400)]     # 1.5 * 2^-14 - 2^-14 = 2^-15: cancels to a subnormal
        bias = [zero, nzero, one, 0xBC00, min_sub, big, min_norm, 0x8001]
    else:
        nan, inf, ninf, one, zero, nzero = 0x7FC0, 0x7F80, 0xFF80, 0x3F80, 0x0000, 0x8000
        min_sub, max_sub, min_norm, big = 0x0001, 0x007F, 0x0080, 0x7F7F
        pairs = [(0x4380, one),        # 256 + 1: a tie between 256 and 258, to the even neighbour below
                 (0x4381, one),        # 258 + 1: a tie between 258 and 260, to the even neighbour above
                 (big, 0x7B00),        # the largest finite bf16 + 2^119 (half its ulp): a tie, to 2^128: Inf
                 (big, 0x7A80),        # + 2^118: stays
                 (0xFF7F, 0xFB00),     # -Inf
                 (0x00C0, 0x8080)]     # 1.5 * 2^-126 - 2^-126 = 2^-127: cancels to a subnormal (an fp32 subnormal too)
        bias = [zero, nzero, one, 0xBF80, min_sub, big, min_norm, 0x8001]
    pairs += [(nan, one), (one, nan), (nan, nan), (inf, one), (ninf, one), (one, inf), (inf, ninf), (inf, inf), (ninf, ninf),
              (zero, zero), (zero, nzero), (nzero, zero), (nzero, nzero),
              (min_sub, zero), (min_sub, min_sub), (min_sub, min_sub | 0x8000), (max_sub, zero), (max_sub, min_sub),
              (max_sub | 0x8000, zero), (min_norm, min_sub | 0x8000), (big, zero), (big | 0x8000, zero), (big, big),
              (big, big | 0x8000), (one, one | 0x8000)]
    assert len(pairs) <= 64
    pairs += [(one, one)] * (64 - len(pairs))
    t = lambda bits: torch.from_numpy(np.array(bits, dtype=np.uint16).view(np.int16).copy()).view(_dtype(name))
    x = t([p[0] for p in pairs])[:, None].repeat(1, 8).contiguous()
    r = t([p[1] for p in pairs])[:, None].repeat(1, 8).contiguous()
    return x, r, t(bias)


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_bias_act_special_values(elf, name):
    """A table of NaN, +-Inf, +-0, the smallest and the largest subnormal, the largest finite value, sums that are exact ties
    between two storage values (to the even neighbour below, and above), sums that round to Inf and a sum that cancels to a
    subnormal, through all four variants with and without ReLU.  The reference is the fp32 formula evaluated on the host;
    NaN is compared by position, everything else as values.  With ReLU a NaN becomes 0 (fmax)."""
    import torch
    dtype = _dtype(name)
    x, r, b = _special_table(name)
    assert x.shape == (64, 8) and bool(torch.isnan(x[:, 0]).any()) and bool(torch.isinf(x[:, 0]).any())
    # the table does what its comments say, by the host's arithmetic
    s = _bias_act_ref(x[:, 0], None, r[:, 0], 0, dtype).float()
    if name == "f16":
        assert s[:6].tolist() == [2048.0, 2052.0, INF, 65504.0, -INF, 2.0 ** -15]
    else:
        assert s[:6].tolist() == [256.0, 260.0, INF, x[3, 0].float().item(), -INF, 2.0 ** -127]
    xd, rd, bd = x.cuda(), r.cuda(), b.cuda()
    assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))
    for use_bias in (False, True):
        for use_res in (False, True):
            for relu in (0, 1):
                want = _bias_act_ref(x, b if use_bias else None, r if use_res else None, relu, dtype)
                y = xd.clone()
                assert _bias_act(elf.lib(), dtype, y, bd if use_bias else None, rd if use_res else None, 64, 8, relu) == 0
                torch.cuda.synchronize()
                got = y.cpu()
                bad = cc.differing(got, want)
                if relu and not use_bias and not use_res:
                    assert x.view(torch.int16)[18, 0].item() == -32768 and bool(torch.isnan(x[6, 0]))
                    print("%s relu(-0) has the bits 0x%04x, relu(NaN) 0x%04x"
                          % (name, got.view(torch.int16)[18, 0].item() & 0xFFFF, got.view(torch.int16)[6, 0].item() & 0xFFFF))
                print("%s bias %d res %d relu %d: %d of %d differ" % (name, use_bias, use_res, relu, bad, got.numel()))
                assert bad == 0, [(i, l, got[i, l].item(), want[i, l].item()) for i in range(64) for l in range(8)
                                  if not (got[i, l] == want[i, l] or (got[i, l] != got[i, l] and want[i, l] != want[i, l]))][:8]
                if relu:
                    assert not bool(torch.isnan(got).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# D. algo 0 at the channel counts _fusable sends it

@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c,k", [(8, 8), (72, 40), (64, 64), (40, 264)])
def test_algo_0_at_channel_counts_that_need_padding(elf, c, k, use_res):
    """FusedInferenceNet._fusable sends every C and K that are multiples of 8 to algo 0, which rests on CK's MNK padding where
    they are no multiple of its 128-channel and 32-deep tiles: the integer nine-tap form exactly, with and without ReLU"""
    import torch
    rows, h, wd = 3, 9, 9
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    for relu in (0, 1):
        ref = d["conv"] + d["b"].float()
        if use_res:
            ref = ref + d["r"].float()
        if relu:
            ref = torch.relu(ref)
        buf, y = cc.guarded(rows, h, wd, k)
        assert cc.launch(elf.lib(), "algo0", d["x"], d["w"], d["b"], d["r"] if use_res else None, y, relu) == 0
        torch.cuda.synchronize()
        bad = int((y.float() != ref).sum().item())
        print("c %d k %d res %d relu %d: %d of %d differ" % (c, k, use_res, relu, bad, y.numel()))
        assert bad == 0
        assert bool(torch.isnan(buf[-1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# E. the routed path

class _Recording:
    """forwards everything to libelf_amd.so, keeps the algo argument of every elfnet_conv3x3_f16 call and counts the
    elfnet_conv3x3_small_f16 calls"""

    def __init__(self, lib):
        self._lib, self.algos, self.small = lib, [], 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "elfnet_conv3x3_small_f16":
            def small(*args):
                self.small += 1
                return fn(*args)
            return small
        if name != "elfnet_conv3x3_f16":
            return fn

        def conv(*args):
            self.algos.append(args[11])
            return fn(*args)
        return conv


_routed = {}


def _routed_net():
    """test_gpu_net_conv._nets' 2-block, 256-channel fp16 net at 100 rows of 19 x 19, and h0 = the input convolution's output,
    computed once: what is compared below is the residual blocks alone, four elfnet_conv3x3_f16 calls and no MIOpen kernel"""
    import torch
    from elf_amd.net import FusedInferenceNet, make_net
    if not _routed:
        n, blocks, ch, bs = 19, 2, 256, 100
        net16 = make_net(n, blocks, ch, "cuda", torch.float16, channels_last=True, seed=3, fold_bn=True)
        s = (torch.rand((bs, 18, n, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) < 0.3).float()
        f = FusedInferenceNet(net16)
        f.L = _Recording(f.L)
        s16 = s.half().contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            h0 = f._conv(s16, f.first)
        torch.cuda.synchronize()
        assert f.L.algos == [] and f.L.small == 0 and h0.shape == (bs, ch, n, n) and bool(torch.isfinite(h0).all())
        _routed.update(f=f, h0=h0)
    return _routed["f"], _routed["h0"]


def _trunk(f, h, conv_algo=None, small_max_positions=None):
    """the residual blocks of f on h with f.conv_algo (and, where given, f.small_max_positions) set for the call -> (output, the
    algos of its elfnet_conv3x3_f16 calls); f.L.small is the number of its elfnet_conv3x3_small_f16 calls"""
    import torch
    f.L.algos.clear()
    f.L.small = 0
    f.conv_algo = conv_algo
    if small_max_positions is not None:
        f.small_max_positions = small_max_positions
    try:
        with torch.no_grad():
            for lo, up in f.blocks:
                h = f._conv(f._conv(h, lo), up, res=h)
    finally:
        del f.conv_algo
        if small_max_positions is not None:
            del f.small_max_positions
    return h, list(f.L.algos)


def test_fused_net_routes_by_size(elf):
    """91 rows of 19 x 19 are 32 851 positions, the first row count at or above native_min_positions: four algo 1 calls; 90 rows
    (32 490): four algo 0 calls.  And the whole 100 rows give the same bits routed, pinned to algo 0 and pinned to algo 1."""
    import torch
    f, h0 = _routed_net()
    assert 90 * 361 < f.native_min_positions <= 91 * 361
    _, algos = _trunk(f, h0[:91])
    assert algos == [1, 1, 1, 1]
    _, algos = _trunk(f, h0[:90])
    assert algos == [0, 0, 0, 0]
    routed, algos = _trunk(f, h0)
    assert algos == [1, 1, 1, 1]
    for pinned in (0, 1):
        out, algos = _trunk(f, h0, pinned)
        assert algos == [pinned] * 4
        assert torch.equal(out, routed), pinned
    assert bool(torch.isfinite(routed).all()) and float(routed.float().abs().max().item()) > 0


def test_fused_net_chunks_through_both_algos(elf):
    """What a chunked call does with a short last chunk: 91 rows through algo 1 and the 9 that remain through algo 0 are, row for
    row, the bits of all 100 at once"""
    import torch
    f, h0 = _routed_net()
    whole, _ = _trunk(f, h0)
    head, algos = _trunk(f, h0[:91])
    assert algos == [1, 1, 1, 1]
    tail, algos = _trunk(f, h0[91:])
    assert algos == [0, 0, 0, 0]
    assert torch.equal(whole[:91], head)
    assert torch.equal(whole[91:], tail)


def test_fused_net_chunks_through_algo_1_and_the_small_kernel(elf):
    """The same chunked call with small_max_positions = 23 104, the value the default is meant to move to: 91 rows still go through
    four algo 1 calls, and the 9 that remain (3 249 positions) through four elfnet_conv3x3_small_f16 calls and no
    elfnet_conv3x3_f16 call; both are, row for row, the bits of all 100 at once"""
    import torch
    f, h0 = _routed_net()
    assert type(f).small_max_positions == 0 and 9 * 361 == 3249 <= 23104 < f.native_min_positions
    whole, algos = _trunk(f, h0)
    assert algos == [1, 1, 1, 1] and f.L.small == 0
    head, algos = _trunk(f, h0[:91], small_max_positions=23104)
    assert algos == [1, 1, 1, 1] and f.L.small == 0
    tail, algos = _trunk(f, h0[91:], small_max_positions=23104)
    assert algos == [] and f.L.small == 4
    assert f.small_max_positions == 0      # the instance attribute is gone: the class default shows again
    assert torch.equal(whole[:91], head)
    assert torch.equal(whole[91:], tail)
    assert bool(torch.isfinite(tail).all()) and float(tail.float().abs().max().item()) > 0


def test_algo_1_captured_equals_uncaptured(elf):
    """The residual blocks pinned to algo 1 at 16 rows, captured into a graph after a warm-up on a side stream (as
    test_gpu_net_conv.test_fused_net_captured_equals_uncaptured does): two replays return the bits of the uncaptured call"""
    import torch
    f, h0 = _routed_net()
    x = h0[:16]
    plain, algos = _trunk(f, x, 1)
    assert algos == [1, 1, 1, 1]
    plain = plain.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _trunk(f, x, 1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        hg, algos = _trunk(f, x, 1)
    assert algos == [1, 1, 1, 1]
    for replay in range(2):
        hg.fill_(NAN)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(hg, plain), replay
