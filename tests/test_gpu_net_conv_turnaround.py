"""GPU: what the hand-written trunk convolution (algo 1, elf_amd/csrc/net_conv3x3.hip) does between two main loops, after that
block was cut down: the decode of a staging lane's rows (position -> board row and column by a host-made multiplier and shift, the
9-bit tap mask as the product of a row mask and a column mask) and the epilogue's arithmetic (v_fma_mix_f32 for conversion +
addition, the ReLU as v_pk_max_f16 behind the last rounding, under a uniform branch).

A. Decode: all-ones x and w, zero bias: an output is Cin x (taps on the board), so a wrong quotient or mask is a wrong integer.
   Boards 19 x 19, 9 x 9, 16 x 16, 2 x 2, 5 x 37, 37 x 5, 1 x 19 with 5 - 9 tiles each.  M = rows * H * W = 1 (mod 256) has no
   solution with 5 - 9 tiles for any of these boards, so the rows are those with the fewest valid rows in the last tile (13, 3, 4,
   15, 15, 2; 16 x 16 has no partial tile: every tile starts on a board), and two more boards give the one valid row: 1 x 1281 and
   1281 boards of 1 x 1 (the divisor 1).  Round widths 1, 2, 3 and 0 (the device's: one item per workgroup).
B. Epilogue values: one board of 19 x 19, C = 64, K = 256, width 1 (both tiles in one workgroup), centre-tap weights that hand
   chosen input channels to the output channels 0, 63, 64, 127, 128 and 255, so that the accumulator there is an exact chosen value,
   at positions of both tiles.  Skip on / off x ReLU on / off.
The reference is algo 0 on the same inputs, bit for bit; in A the nine-tap integers and in B a numpy float32 model of the contract
(include/elf_amd.h: float(half(acc)) + float(bias), + float(res), fmaxf(., 0), one rounding to fp16) are a second one.  y is
prefilled with NaN and has a NaN guard row behind it."""
import numpy as np
import pytest

import conv_cases as cc
from conv_cases import RES_RELU, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 8191 + rows + 31 * h + 977 * wd + c + 7 * k


def _both(elf, x, w, b, r, rows, h, wd, c, k, relu, width):
    """algo 1 at `width` and algo 0 on the same inputs; asserts the guard row and returns (y1, y0)"""
    import torch
    buf1, y1 = cc.guarded(rows, h, wd, k)
    buf0, y0 = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", x, w, b, r, y1, relu, width) == 0
    assert cc.launch(elf.lib(), "algo0", x, w, b, r, y0, relu) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf1[-1]).all()) and bool(torch.isnan(buf0[-1]).all())
    return y1, y0


# ---------------------------------------------------------------------------------------------------------------- A. decode

# rows, H, W, K: 5 - 9 tiles of 256 positions (per channel column)
DECODE = [(5, 19, 19, 256),      # M = 1805: 8 tiles, 13 valid rows in the last
          (19, 9, 9, 256),       # 1539: 7 tiles, 3
          (7, 16, 16, 256),      # 1792: 7 full tiles, every tile starts on a board
          (257, 2, 2, 256),      # 1028: 5 tiles, 4
          (7, 5, 37, 256),       # 1295: 6 tiles, 15
          (7, 37, 5, 256),       # 1295: 6 tiles, 15
          (54, 1, 19, 256),      # 1026: 5 tiles, 2
          (1, 1, 1281, 256),     # 1281: 6 tiles, one valid row in the last
          (1281, 1, 1, 256),     # the same M on boards of one point: both divisors are 1
          (5, 19, 19, 512)]      # two channel columns: 16 items, a column change inside a chain
_ones = {}


def _ones_case(elf, rows, h, wd, k):
    """all-ones operands, algo 0's output and the nine-tap integers; made once per case"""
    import torch
    key = (rows, h, wd, k)
    if key not in _ones:
        c = 64
        x = torch.ones((rows, h, wd, c), device="cuda", dtype=torch.float16)
        w = torch.ones((k, 3, 3, c), device="cuda", dtype=torch.float16)
        b = torch.zeros((k,), device="cuda", dtype=torch.float16)
        y0 = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.launch(elf.lib(), "algo0", x, w, b, None, y0, 0) == 0
        torch.cuda.synchronize()
        rowc = np.array([(i > 0) + 1 + (i < h - 1) for i in range(h)])
        colc = np.array([(j > 0) + 1 + (j < wd - 1) for j in range(wd)])
        taps = torch.from_numpy((c * rowc[:, None] * colc[None, :]).astype(np.float32)).cuda()   # at most 576: exact in fp16
        _ones[key] = (x, w, b, y0, taps[None, :, :, None].expand(rows, h, wd, k))
    return _ones[key]


@pytest.mark.parametrize("width", [1, 2, 3, 0])
@pytest.mark.parametrize("rows,h,wd,k", DECODE)
def test_decode_counts_the_taps_on_the_board(elf, rows, h, wd, k, width):
    import torch
    x, w, b, y0, taps = _ones_case(elf, rows, h, wd, k)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "linear", x, w, b, None, y, 0, width) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != taps).sum().item())   # a NaN left in y differs from everything
    print("%s width %d: %d of %d differ from the nine-tap integers, %d from algo 0"
          % ((rows, h, wd, k), width, bad, y.numel(), int((cc.bits(y) != cc.bits(y0)).sum().item())))
    assert bad == 0
    assert torch.equal(cc.bits(y), cc.bits(y0))
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("rows,h,wd,k,width", [(5, 19, 19, 256, 1), (7, 5, 37, 256, 3)])
def test_repeated_launches_of_two_chains(elf, rows, h, wd, k, width):
    """eight full items in one workgroup; six items at width 3 (two per workgroup).  20 launches into fresh NaN-filled outputs,
    every one the first's, which is algo 0's"""
    import torch
    x, w, b, y0, _ = _ones_case(elf, rows, h, wd, k)
    first = None
    for i in range(20):
        y = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.launch(elf.lib(), "linear", x, w, b, None, y, 0, width) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert torch.equal(cc.bits(y), cc.bits(y0)), "the first launch differs from algo 0"
        else:
            assert torch.equal(cc.bits(y), cc.bits(first)), "launch %d differs from the first" % i


# ------------------------------------------------------------------------------------------------------- B. epilogue values

H = W = 19
CIN, K = 64, 256
CH = [0, 63, 64, 127, 128, 255]                        # the output channels the probes sit in
S1 = {0: 0, 63: 63, 64: 1, 127: 62, 128: 2, 255: 61}   # their two input channels: acc = wt * (x[s1] + x[s2]), exactly
S2 = {0: 32, 63: 33, 64: 34, 127: 35, 128: 36, 255: 37}
POS = [0, 40, 255, 258, 300, 360]                      # positions of both tiles (256 positions each), no two of them neighbours
NAN = float("nan")


def _model(x, w, b, r, relu):
    """the contract in numpy, from the tensors themselves.  acc: the centre tap's products in float64 (at most two non-zero per
    output, chosen so that their sum is exact in float32); a NaN anywhere in x makes every output of its 3 x 3 neighbourhood
    NaN (0 * NaN), as it does in the MFMA chain."""
    xs = x.reshape(H * W, CIN).astype(np.float64)
    nan_at = np.isnan(xs).any(axis=1).reshape(H, W)
    near = np.zeros((H, W), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)] |= nan_at[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]
    assert not np.isinf(xs).any()
    acc = (np.nan_to_num(xs) @ w[:, 1, 1, :].astype(np.float64).T)
    acc[near.reshape(-1)] = np.nan
    acc32 = acc.astype(np.float32)
    assert np.array_equal(acc32.astype(np.float64), acc, equal_nan=True), "the chosen accumulators are not exact in float32"
    with np.errstate(over="ignore", invalid="ignore"):
        v = acc32.astype(np.float16).astype(np.float32) + b.astype(np.float32)[None, :]
        if r is not None:
            v = v + r.reshape(H * W, K).astype(np.float32)
        if relu:
            v = np.fmax(v, np.float32(0))
        return v.astype(np.float16)


def _case(probes, rot, seed):
    """x, w, bias, res (numpy fp16) with probe j = (x1, x2, wt, bias, res) in the channels CH[(j + rot) % n :: n] at every position
    of POS; everything else is background: multiples of 2^-6 (sums of two are exact), every output channel k a copy of input
    channel k % 64"""
    rng = np.random.default_rng(seed)
    bg = lambda shape: (rng.integers(-128, 129, shape) / 64.0).astype(np.float16)
    x = bg((H * W, CIN))
    w = np.zeros((K, 3, 3, CIN), dtype=np.float16)
    w[np.arange(K), 1, 1, np.arange(K) % CIN] = 1
    b = bg((K,))
    r = bg((H * W, K))
    n = len(probes)
    where = []
    for j, (x1, x2, wt, pb, pr) in enumerate(probes):
        for k in CH[(j + rot) % n::n]:
            w[k] = 0
            w[k, 1, 1, S1[k]] = wt
            w[k, 1, 1, S2[k]] = wt
            b[k] = pb
            for p in POS:
                x[p, S1[k]], x[p, S2[k]], r[p, k] = x1, x2, pr
                where.append((j, p, k))
    return x.reshape(1, H, W, CIN), w, b, r.reshape(1, H, W, K), where


def _epilogue_case(elf, probes, use_res, relu, expect=None, zero_sign_is_algo0s=False):
    """every rotation of the probes over the six channels; algo 1 against algo 0 bit for bit, against the model, and the probes'
    own expected fp16 bit patterns (expect[j], None = whatever the model says) at every place they sit.  Returns algo 0's bits at
    the probes, for the tests that pin them."""
    import torch
    seen = {}
    for rot in range(len(probes)):
        x, w, b, r, where = _case(probes, rot, 99 + rot)
        t = lambda a: torch.from_numpy(a).cuda()
        y1, y0 = _both(elf, t(x), t(w), t(b), t(r) if use_res else None, 1, H, W, CIN, K, relu, 1)
        g1, g0 = cc.bits(y1).cpu().numpy().reshape(H * W, K), cc.bits(y0).cpu().numpy().reshape(H * W, K)
        m = _model(x, w, b, r if use_res else None, relu)
        mb = m.view(np.int16)
        print("res %d relu %d rot %d: %d of %d elements differ from algo 0" % (use_res, relu, rot, int((g1 != g0).sum()), g1.size))
        for j, p, k in where:
            seen.setdefault(j, set()).update([(int(g1[p, k]) & 0xFFFF, int(g0[p, k]) & 0xFFFF)])
            if expect is not None and expect[j] is not None:
                assert int(g1[p, k]) & 0xFFFF == expect[j], "probe %d at position %d channel %d: 0x%04x, expected 0x%04x" % (
                    j, p, k, int(g1[p, k]) & 0xFFFF, expect[j])
        assert np.array_equal(g1, g0), "algo 1 differs from algo 0"
        # the model: NaN is NaN whatever its payload; behind the ReLU the header leaves a zero's sign open (algo 0's is pinned above)
        y1f = g1.view(np.float16)
        same = (g1 == mb) | (np.isnan(y1f) & np.isnan(m))
        if relu or zero_sign_is_algo0s:
            same |= (y1f == 0) & (m == 0)
        assert same.all(), "%d elements differ from the model, first at %s" % (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    return seen


ONE, MONE, INF, MINF, PZ, MZ = 0x3C00, 0xBC00, 0x7C00, 0xFC00, 0x0000, 0x8000


@pytest.mark.parametrize("use_res,relu", RES_RELU)
def test_two_roundings_not_one(elf, use_res, relu):
    """acc 1.0, bias 2^-11, res 2^-24: float(half(acc)) + bias + res is 1 + 2^-11 + 2^-24 in fp32, above the tie, so one rounding
    of it gives 1.00098 (0x3C01).  The contract is that sum as fp32 arithmetic computes it, and fp32 arithmetic drops the 2^-24:
    (1 + 2^-11) + 2^-24 is itself a tie in fp32 and goes to the even 1 + 2^-11, which is fp16's tie and goes to 1.0.  Mirrored for
    -1.0, and a third probe whose res is large enough (2^-22) to survive the fp32 addition: that one is above the tie."""
    probes = [(1.0, 0.0, 1.0, 2.0 ** -11, 2.0 ** -24), (-1.0, 0.0, 1.0, -2.0 ** -11, -2.0 ** -24), (1.0, 0.0, 1.0, 2.0 ** -11, 2.0 ** -22)]
    if use_res:
        expect = [ONE, PZ if relu else MONE, 0x3C01]
    else:
        expect = [ONE, PZ if relu else MONE, ONE]        # 1 + 2^-11 alone is fp16's tie: to even
    _epilogue_case(elf, probes, use_res, relu, expect)


@pytest.mark.parametrize("use_res,relu", RES_RELU)
def test_the_first_rounding_overflows(elf, use_res, relu):
    """acc = 40000 + 40000 is beyond 65 504: Inf after the first rounding, which no bias or res brings back; -Inf behind the ReLU
    is 0.  A third probe stays finite: 65 504 with bias -4 is 65 500, which rounds back to 65 504."""
    probes = [(40000.0, 40000.0, 1.0, -30000.0, -30000.0), (-40000.0, -40000.0, 1.0, 30000.0, 30000.0), (32768.0, 32736.0, 1.0, -4.0, 0.0)]
    _epilogue_case(elf, probes, use_res, relu, [INF, PZ if relu else MINF, 0x7BFF])


@pytest.mark.parametrize("use_res,relu", RES_RELU)
def test_nan_in_x_res_and_bias(elf, use_res, relu):
    """a NaN in x (every output of its 3 x 3 neighbourhood is NaN, so that probe runs alone), in res and in bias: +0 behind the ReLU,
    NaN without it"""
    in_x = _epilogue_case(elf, [(NAN, 0.0, 1.0, 0.5, 0.25)], use_res, relu)
    seen = _epilogue_case(elf, [(1.5, 0.0, 1.0, 0.5, NAN), (1.5, 0.0, 1.0, NAN, 0.25)], use_res, relu)
    for name, bits, plain in (("x", in_x[0], False), ("res", seen[0], not use_res), ("bias", seen[1], False)):
        for got, _ in bits:
            if plain:
                assert got == 0x4000            # no res: 1.5 + 0.5
            elif relu:
                assert got == PZ, "NaN in %s: 0x%04x behind the ReLU" % (name, got)
            else:
                assert (got & 0x7C00) == 0x7C00 and (got & 0x3FF) != 0, "NaN in %s: 0x%04x is not NaN" % (name, got)


@pytest.mark.parametrize("use_res,relu", RES_RELU)
def test_the_sign_of_zero_is_algo_0s(elf, use_res, relu):
    """sums that are exactly -0 and +0.  The accumulator itself is never -0 (it starts at +0), but -2^-26 rounds to fp16's -0:
    x = -2^-24 with weight 1/4.  Probes: (-0) + (-0) + (-0) = -0; 1 + (-1) + (+0) = +0; (-0) + (+0) + (-0) = +0.  Without the ReLU
    the sign is arithmetic's and asserted; behind it the header allows either and algo 0's is pinned: +0 here, for all three."""
    tiny = -2.0 ** -24
    probes = [(tiny, 0.0, 0.25, -0.0, -0.0), (1.0, 0.0, 1.0, -1.0, 0.0), (tiny, 0.0, 0.25, 0.0, -0.0)]
    expect = [PZ, PZ, PZ] if relu else [MZ, PZ, PZ]
    seen = _epilogue_case(elf, probes, use_res, relu, expect, zero_sign_is_algo0s=True)
    for j in range(3):
        assert seen[j] == {(expect[j], expect[j])}, "probe %d (algo 1, algo 0): %s" % (j, sorted(seen[j]))


@pytest.mark.parametrize("use_res", [False, True])
def test_negative_and_subnormal_results_without_relu(elf, use_res):
    """relu = 0 passes negative values through; fp16 subnormals of both signs as results (2^-14 - 2^-15, 3 2^-24 - 2^-24) and as
    the rounded accumulator itself (2^-24 + 2^-24)"""
    s = 2.0 ** -24
    probes = [(-1.5, 0.0, 1.0, 0.25, 0.0), (2.0 ** -14, 0.0, 1.0, -2.0 ** -15, 0.0), (-2.0 ** -14, 0.0, 1.0, 2.0 ** -15, 0.0),
              (3 * s, 0.0, 1.0, -s, 0.0), (-3 * s, 0.0, 1.0, s, 0.0), (s, 0.0, 1.0, s, 0.0)]
    expect = [0xBD00, 0x0200, 0x8200, 0x0002, 0x8002, 0x0002]
    _epilogue_case(elf, probes, use_res, 0, expect)
    # and the same values behind the ReLU: the negative ones are +0
    _epilogue_case(elf, probes, use_res, 1, [PZ, 0x0200, PZ, 0x0002, PZ, 0x0002])


# rows, H, W, round width: M = 81 (one tile), 257 (one valid row in the second), 1620 (seven tiles at width 2: three full items and a
# half item per workgroup)
RANDOM = [(1, 9, 9, 0), (1, 1, 257, 0), (20, 9, 9, 2)]


@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("k", [256, 512])
@pytest.mark.parametrize("c", [64, 192, 256])
def test_random_data_is_bit_equal_with_algo_0(elf, c, k, use_res, relu):
    import torch
    for rows, h, wd, width in RANDOM:
        x, w, b, r = cc.rand_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
        y1, y0 = _both(elf, x, w, b, r if use_res else None, rows, h, wd, c, k, relu, width)
        print("%s width %d res %d relu %d: %d of %d elements differ from algo 0"
              % ((rows, h, wd, c, k), width, use_res, relu, int((cc.bits(y1) != cc.bits(y0)).sum().item()), y1.numel()))
        assert not bool(torch.isnan(y0).any())
        assert torch.equal(cc.bits(y1), cc.bits(y0))
