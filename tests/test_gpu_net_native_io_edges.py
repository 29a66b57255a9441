"""GPU: the edges of the two ends of the native fp16 net (elfnet_conv3x3_in_f16 and elfnet_heads_f16, elf_amd/csrc/net_io.hip) that
test_gpu_net_native_io.py does not reach, by test_gpu_net_edges.py's method.  Every comparison is exact (equal as values, NaN in
the same places) except what follows an expf or a tanhf, which keeps test_heads_exact's three bounds (relative 1e-4 on pi, 1e-5 on
|sum pi - 1|, 2^-20 on V):
  A  input convolution: non-square, one-cell and one-line boards, the channel counts around the two instances' limits, and two
     workgroup columns with a tile loop that goes round;
  B  which cells one input element or one weight influences, and operands between NaN guards at the weakest alignment the ABI allows;
  C  the input convolution's two roundings told apart, fp16 subnormals in and out, what the ReLU does to NaN, Inf and -0;
  D  heads: the workload's own launch (2048 rows of 19 x 19: eight rows and 54 KiB of LDS per workgroup), the LDS-bound reduction of
     the rows per workgroup, partially filled lane groups, a position loop that goes round, value_hidden of 1 / 65 / 300,
     non-square boards and d = 1;
  E  heads: operands between NaN guards at the weakest alignment, a workspace of exactly the documented size;
  F  heads: softmax with a large offset, with entries that underflow and with equal logits, tanh at its ends, one NaN and one +Inf
     activation;
  G  a row's bits do not depend on the batch it is in: heads, input convolution, NativeInferenceNet.
Every reference helper asserts its own preconditions (exact representability of every partial sum, a case that is not degenerate) on
the reference alone, on the host."""
import ctypes as C

import numpy as np
import pytest

import conv_cases as cc
from conv_cases import NAN, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu

INF = float("inf")
PI_REL, PI_SUM, V_ABS = 1e-4, 1e-5, 2.0 ** -20      # test_heads_exact's bounds


# test_gpu_net_native_io's integer recipe (no res, |sum| <= 9 * 32 = 288) on an h x wd board, and not degenerate: the convolution is
# not all zero and on a non-square board the nine-tap form of the same memory read as wd x h differs
INTS = dict(res=False, limit=288, not_degenerate=True)


def _seed(rows, h, wd, c, k):
    return 4242 + rows + 1000 * h + 31 * wd + c + 7 * k


# ---------------------------------------------------------------------------------------------------------------------------------
# A. input convolution: shapes

@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,h,wd,c,k", [(3, 5, 7, 18, 64), (3, 7, 5, 18, 64),      # non-square: h and wd must not be swapped
                                           (70, 1, 1, 18, 32),                        # one cell: eight of nine taps off the board
                                           (9, 1, 5, 18, 32), (9, 5, 1, 18, 32),      # one line
                                           (17, 2, 2, 18, 32),                        # every cell a corner; a tile holds 16 boards
                                           (2, 9, 9, 4, 64),
                                           (2, 9, 9, 16, 64),                         # 9 C = 144: two whole MFMA steps of K padding
                                           (2, 9, 9, 20, 64),                         # the first C of the 18-step instance
                                           (2, 9, 9, 30, 64),
                                           (410, 9, 9, 18, 288)])                     # two workgroup columns, 519 tiles on 256 each
def test_input_conv_shapes_exact_integers(elf, rows, h, wd, c, k, relu):
    """equality with the nine-tap fp32 form; y is prefilled with NaN, and the guard row of NaN behind y's last row stays NaN"""
    import torch
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k, **INTS)
    ref = d["conv"] + d["b"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.conv_in(elf.lib(), d["x"], d["w"], d["b"], y, rows, h, wd, c, k, relu) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("%s relu %d: %d of %d differ" % ((rows, h, wd, c, k), relu, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# B. input convolution: influence and guards

@pytest.mark.parametrize("poison", [NAN, INF])
@pytest.mark.parametrize("rows,n,b,i,j", [(2, 9, 0, 8, 8),      # the last cell of board 0: board 1 lies behind it in memory
                                          (2, 9, 1, 0, 0),      # the first cell of board 1
                                          (1, 19, 0, 3, 7)])    # position 64, interior: its 3 x 3 cells lie in tiles 0 and 1
def test_input_conv_one_poisoned_input_element(elf, rows, n, b, i, j, poison):
    """All-ones weights, the integer case's x with one element (the first, then the last channel of the cell) set to NaN or +Inf,
    no ReLU: the output is not finite at exactly the on-board cells within one step of (i, j) on board b, over all k, and
    everywhere else it is the unpoisoned run's.  The affected cells equal the nine-tap fp32 form of the poisoned input (NaN, or
    +Inf: a finite sum plus Inf)."""
    import torch
    c, k = 18, 64
    d = cc.int_case(_seed(rows, n, n, c, k), rows, n, n, c, k, **INTS)
    w = torch.ones((k, 3, 3, c), device="cuda", dtype=torch.float16)
    if n == 19:
        assert (i * n + j) == 64 and 0 < i < n - 1 and 0 < j < n - 1 and ((i - 1) * n + j - 1) // 64 != ((i + 1) * n + j + 1) // 64
    L = elf.lib()
    _, clean = cc.guarded(rows, n, n, k)
    assert cc.conv_in(L, d["x"], w, d["b"], clean, rows, n, n, c, k, 0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(clean).all())
    assert bool((clean.float() == cc.conv_fp32(d["x"].float(), w.float()) + d["b"].float()).all())
    touched = torch.zeros((rows, n, n), device="cuda", dtype=torch.bool)
    touched[b, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = True
    assert int(touched.sum().item()) == (4 if n == 9 else 9)
    for ch in (0, c - 1):
        x = d["x"].clone()
        x[b, i, j, ch] = poison
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(L, x, w, d["b"], y, rows, n, n, c, k, 0) == 0
        torch.cuda.synchronize()
        assert torch.equal(y[~touched].view(torch.int16), clean[~touched].view(torch.int16)), ch
        assert not bool(torch.isfinite(y[touched]).any()), ch
        assert cc.differing(y, cc.conv_fp32(x.float(), w.float()) + d["b"].float()) == 0, ch
        if poison != poison:
            assert bool(torch.isnan(y[touched]).all()), ch
        else:
            assert bool((y[touched].float() == INF).all()), ch
        assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("ky,kx", [(0, 0), (1, 1)])
@pytest.mark.parametrize("k0", [0, 31, 32, 255])
def test_input_conv_one_nan_weight(elf, k0, ky, kx):
    """One w[k0, ky, kx, 17] (the last channel of C = 18) set to NaN.  Without the ReLU channel k0 is NaN at EVERY position, also
    where the tap is off the board: an off-board tap is staged as zeros and 0 x NaN is NaN in the MFMA.  The nine-tap torch
    reference agrees, because its zero padding is multiplied by the same NaN.  Every other channel is the unpoisoned run's.  With
    the ReLU channel k0 is 0 (fmaxf) and the others are unchanged."""
    import torch
    rows, n, c, k = 2, 9, 18, 256
    d = cc.int_case(_seed(rows, n, n, c, k), rows, n, n, c, k, **INTS)
    w = d["w"].clone()
    w[k0, ky, kx, c - 1] = NAN
    others = torch.arange(k, device="cuda") != k0
    L = elf.lib()
    for relu in (0, 1):
        _, clean = cc.guarded(rows, n, n, k)
        assert cc.conv_in(L, d["x"], d["w"], d["b"], clean, rows, n, n, c, k, relu) == 0
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(L, d["x"], w, d["b"], y, rows, n, n, c, k, relu) == 0
        torch.cuda.synchronize()
        ref = cc.conv_fp32(d["x"].float(), w.float()) + d["b"].float()
        assert bool(torch.isnan(ref[..., k0]).all()) and bool(torch.isfinite(ref[..., others]).all())
        assert bool(torch.isfinite(clean).all())
        assert torch.equal(y[..., others].view(torch.int16), clean[..., others].view(torch.int16)), relu
        if relu:
            assert bool((y[..., k0].view(torch.int16) == 0).all())
        else:
            assert bool(torch.isnan(y[..., k0]).all())
            assert cc.differing(y, ref) == 0
        assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("rows,h,wd,c,k", [(5, 9, 9, 18, 64), (3, 5, 7, 30, 32)])
def test_input_conv_guarded_operands_at_the_weakest_alignment(elf, rows, h, wd, c, k):
    """x, w, bias and y each a view inside a larger NaN-filled buffer ((wd + 2) * max(c, k) elements of NaN or more on either
    side): x at an address that is 4 modulo 16 (the header: "x needs 4-B alignment only"), w, bias and y at 16 modulo 32.  No
    ReLU, so a NaN read from outside an operand would reach the result.  The result is the unguarded run's bit for bit and the
    integer nine-tap form; y's guards stay NaN."""
    import torch
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k, **INTS)
    guard = (wd + 2) * max(c, k)
    x, _, _ = cc.carve(d["x"], guard, 16, 4)
    w, _, _ = cc.carve(d["w"], guard, 32, 16)
    b, _, _ = cc.carve(d["b"], guard, 32, 16)
    y, front, back = cc.carve(torch.full((rows, h, wd, k), NAN, device="cuda", dtype=torch.float16), guard, 32, 16)
    assert x.data_ptr() % 16 == 4 and w.data_ptr() % 32 == 16 and b.data_ptr() % 32 == 16
    _, plain = cc.guarded(rows, h, wd, k)
    assert cc.conv_in(elf.lib(), d["x"], d["w"], d["b"], plain, rows, h, wd, c, k, 0) == 0
    assert cc.conv_in(elf.lib(), x, w, b, y, rows, h, wd, c, k, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), plain.view(torch.int16))
    assert bool((y.float() == d["conv"] + d["b"].float()).all())
    assert bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# C. input convolution: values

def _cell_kinds(n):
    """[n, n] long: the number of 3 x 3 taps on the board at each cell: 4 at corners, 6 on edges, 9 inside"""
    import torch
    i = torch.arange(n, device="cuda")
    on = 3 - ((i == 0) | (i == n - 1)).long()
    return on[:, None] * on[None, :]


@pytest.mark.parametrize("c,xv", [(18, 16.0), (32, 8.0)])
def test_input_conv_two_roundings_not_one_at_a_tie(elf, c, xv):
    """test_gpu_net_edges' tie with 9 C terms: x = xv, w = 1 but for the centre tap of one input channel per output channel, which
    is 1 + 1 / xv; bias = 1.  A cell sums T = C xv per tap on the board and 1 more (T = 288 for C = 18, 256 for C = 32): 9 T + 1
    inside is odd and above 2048, a tie between two fp16 values.  The header's sequence rounds it to the even neighbour 9 T, adds 1
    and rounds to 9 T again; one rounding of 9 T + 2 would keep 9 T + 2.  Edges (6 T + 2) and corners (4 T + 2) are below 2048,
    where every integer is an fp16."""
    import torch
    rows, n, k = 2, 9, 64
    t = int(c * xv)
    x = torch.full((rows, n, n, c), xv, device="cuda", dtype=torch.float16)
    w = torch.ones((k, 3, 3, c), device="cuda", dtype=torch.float16)
    ko = torch.arange(k, device="cuda")
    w[ko, 1, 1, (ko * 5 + 3) % c] = 1.0 + 1.0 / xv
    assert bool((w[ko, 1, 1, (ko * 5 + 3) % c].double() * xv == xv + 1).all())       # the fp16 weight is exact
    b = torch.ones((k,), device="cuda", dtype=torch.float16)
    kinds = _cell_kinds(n)
    acc = (t * kinds + 1).float()
    assert 2048 < acc[1, 1] < 4096 and acc[1, 1] % 2 == 1 and acc[0, 1] + 1 < 2048
    want = cc.epilogue_fp32(acc, b[0], None, 0).float()
    assert want[1, 1] == 9 * t and (acc + 1).half()[1, 1] == 9 * t + 2 and want[0, 1] == 6 * t + 2 and want[0, 0] == 4 * t + 2
    for relu in (0, 1):
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(elf.lib(), x, w, b, y, rows, n, n, c, k, relu) == 0
        torch.cuda.synchronize()
        print("c %d relu %d: interior %s edge %s corner %s" % (c, relu, y[0, 4, 4, 0].item(), y[0, 0, 4, 0].item(), y[0, 0, 0, 0].item()))
        assert bool((y.float() == want[None, :, :, None]).all())
        assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("c,xv,wv,bv", [(18, 32.0, 16.0, -32768.0), (32, 16.0, 16.0, -16384.0)])
def test_input_conv_first_rounding_overflows_to_inf(elf, c, xv, wv, bv):
    """x = xv, w = wv, a negative bias: a cell sums T = C xv wv per tap on the board (9216 for C = 18, 8192 for C = 32).  9 T is
    beyond 65 520, so half(9 T) is Inf before the bias is added and the interior is +Inf, where one rounding of 9 T + bias would
    be finite; edges are 6 T + bias and corners 4 T + bias, all fp16 values."""
    import torch
    rows, n, k = 2, 9, 64
    t = int(c * xv * wv)
    x = torch.full((rows, n, n, c), xv, device="cuda", dtype=torch.float16)
    w = torch.full((k, 3, 3, c), wv, device="cuda", dtype=torch.float16)
    b = torch.full((k,), bv, device="cuda", dtype=torch.float16)
    kinds = _cell_kinds(n)
    acc = (t * kinds).float()
    want = cc.epilogue_fp32(acc, b[0], None, 0).float()
    assert want[1, 1] == INF and bool(torch.isfinite((acc + bv).half()[1, 1])) and acc[1, 1] < 2.0 ** 24
    assert want[0, 1] == 6 * t + bv and want[0, 0] == 4 * t + bv
    for relu in (0, 1):
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(elf.lib(), x, w, b, y, rows, n, n, c, k, relu) == 0
        torch.cuda.synchronize()
        assert bool((y.float() == want[None, :, :, None]).all())
        assert bool(torch.isnan(buf[-1]).all())


def _scaled(ints, shift):
    """fp16 ints * 2^-shift for small integers, built from bit patterns where the values are subnormal (shift 24: the integer IS
    the bit pattern's magnitude) so that no conversion of this test's own can flush them"""
    import torch
    i = ints.to(torch.int32)
    if shift == 24:
        assert int(i.abs().max().item()) < 1024
        bits = i.abs() | ((i < 0).to(torch.int32) << 15)
        return torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(torch.float16)
    return (i.double() * 2.0 ** -shift).half()


@pytest.mark.parametrize("wshift,oshift", [(10, 14), (0, 24)])
def test_input_conv_subnormal_inputs_and_outputs(elf, wshift, oshift):
    """The integer case scaled by powers of two: x = xi * 2^-24 (every nonzero x is the smallest fp16 subnormal), w = wi * 2^10,
    bias = bi * 2^-14: the result is (integer result) * 2^-14 exactly, normal numbers from subnormal inputs.  The second scaling
    (w = wi, bias * 2^-24) gives (integer result) * 2^-24: every input but w and every output is subnormal or zero.  Nothing may
    be flushed at the MFMA's inputs, at either rounding or in between.  The expected values are made on the host."""
    import torch
    rows, n, c, k = 2, 9, 18, 64
    d = cc.int_case(_seed(rows, n, n, c, k), rows, n, n, c, k, **INTS)
    xi, wi, bi = (d[key].float() for key in ("x", "w", "b"))
    x = _scaled(xi, 24)
    w = (wi * 2.0 ** wshift).half()
    b = _scaled(bi, oshift)
    assert torch.equal(x.float() * 2.0 ** 24, xi) and torch.equal(w.float() * 2.0 ** -wshift, wi) and torch.equal(b.float() * 2.0 ** oshift, bi)
    assert bool(((x.view(torch.int16)[xi != 0] & 0x7FFF) == 1).all())
    for relu in (0, 1):
        ints = d["conv"] + bi
        if relu:
            ints = torch.relu(ints)
        assert float(ints.abs().max().item()) < 1024
        want = (ints.cpu().double() * 2.0 ** -oshift).half()      # exact: |ints| < 2^10
        assert torch.equal(want.double() * 2.0 ** oshift, ints.cpu().double())
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(elf.lib(), x, w, b, y, rows, n, n, c, k, relu) == 0
        torch.cuda.synchronize()
        got = y.cpu()
        bad = int((got.double() != want.double()).sum().item())
        sub = int(((want != 0) & (want.abs() < 2.0 ** -14)).sum().item())
        print("shifts %d/%d relu %d: %d of %d differ; %d expected values are subnormal" % (wshift, oshift, relu, bad, got.numel(), sub))
        assert sub == (0 if oshift == 14 else int((want != 0).sum().item())) and int((want != 0).sum().item()) > got.numel() // 4   # the ReLU zeroes about half
        assert bad == 0
        assert bool(torch.isnan(buf[-1]).all())


def test_input_conv_relu_turns_nan_into_zero(elf):
    """max(v, 0) is fmaxf: with relu = 1 a NaN before the activation comes out as +0 (torch.relu would keep it) and +Inf stays.
    NaN enters through one x element (its 3 x 3 cells, all channels: 0 x NaN) and one bias channel, Inf through another x element
    (+Inf, -Inf or NaN by the weights' signs); the reference is the nine-tap fp32 form and torch.fmax.  With relu = 0 the same
    NaN and Inf come through."""
    import torch
    rows, n, c, k = 2, 9, 18, 64
    d = cc.int_case(_seed(rows, n, n, c, k), rows, n, n, c, k, **INTS)
    x, b = d["x"].clone(), d["b"].clone()
    x[1, 4, 4, 7] = NAN
    x[0, 2, 2, 3] = INF
    b[20] = NAN
    v = cc.conv_fp32(x.float(), d["w"].float()) + b.float()
    nan = torch.isnan(v)
    must = torch.zeros_like(nan)
    must[1, 3:6, 3:6, :] = True
    must[..., 20] = True
    may = must.clone()
    may[0, 1:4, 1:4, :] = True
    assert bool(nan[must].all()) and not bool(nan[~may].any())
    assert bool((v == INF).any()) and bool((v == -INF).any()) and bool(torch.isfinite(v[~may]).all())
    for relu in (1, 0):
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(elf.lib(), x, d["w"], b, y, rows, n, n, c, k, relu) == 0
        torch.cuda.synchronize()
        if relu:
            want = torch.fmax(v, torch.zeros((), device="cuda"))
            assert not bool(torch.isnan(want).any())
            assert bool((y.float() == want).all())
            assert bool((y.view(torch.int16)[nan] == 0).all())      # +0, not -0
        else:
            assert cc.differing(y, v) == 0 and torch.equal(torch.isnan(y), nan)
        assert bool(torch.isnan(buf[-1]).all())


def test_input_conv_negative_zero_passes_without_relu(elf):
    """x = 2^-24 everywhere, w = 0 but for the centre tap of one input channel of output channel 5, which is -1/4; bias = -0.  The
    accumulator of channel 5 is -2^-26, less than half the smallest fp16 subnormal: the first rounding gives -0, -0 + -0 is -0, and
    without the ReLU the result has the bits 0x8000.  Every other channel is +0 + -0 = +0.  With the ReLU every result is a zero of
    either sign (the header does not promise which)."""
    import torch
    rows, n, c, k = 1, 9, 18, 32
    x = torch.ones((rows, n, n, c), device="cuda", dtype=torch.int16).view(torch.float16)
    w = torch.zeros((k, 3, 3, c), device="cuda", dtype=torch.float16)
    w[5, 1, 1, 11] = -0.25
    b = torch.full((k,), -0.0, device="cuda", dtype=torch.float16)
    assert float(x[0, 0, 0, 0].double().item()) == 2.0 ** -24 and int(b.view(torch.int16)[0].item()) == -32768
    host = (torch.tensor(-2.0 ** -26, dtype=torch.float32).half().float() + torch.tensor(-0.0)).half()
    assert int(host.view(torch.int16).item()) == -32768
    for relu in (0, 1):
        buf, y = cc.guarded(rows, n, n, k)
        assert cc.conv_in(elf.lib(), x, w, b, y, rows, n, n, c, k, relu) == 0
        torch.cuda.synchronize()
        assert bool((y.float() == 0).all())
        if not relu:
            bits = y.view(torch.int16)
            assert bool((bits[..., 5] == -32768).all())
            assert bool((bits[..., torch.arange(k, device="cuda") != 5] == 0).all())
        assert bool(torch.isnan(buf[-1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# heads: reference and driver

def _upload(a):
    """name -> fp16 device tensor of every array in `a`; every finite value must be an fp16 value"""
    import torch
    out = {}
    for nm, v in a.items():
        h = v.astype(np.float16)
        fin = np.isfinite(v)
        assert np.array_equal(h.astype(np.float64)[fin], v[fin]) and np.array_equal(np.isnan(h), np.isnan(v)), nm
        out[nm] = torch.from_numpy(h).cuda()
    return out


def _heads_ref(a, rows, d, zero=None):
    """fp64: (logits [rows, d+1], pi, V, the value's pre-activation, and the largest sum of absolute terms of the three linear
    layers, in units of their grids 1/64, 1/8 and 1/256).  zero = (row, pos): that position's three head-convolution outputs are 0."""
    act = a["act"].reshape(rows, d, -1)
    p = np.maximum(act @ a["pconv_w"].T + a["pconv_b"], 0)                  # [rows, d, 2]
    v0 = np.maximum(act @ a["vconv_w"].T + a["vconv_b"], 0)[:, :, 0]        # [rows, d]
    if zero is not None:
        p[zero[0], zero[1], :] = 0
        v0[zero[0], zero[1]] = 0
    flat = p.transpose(0, 2, 1).reshape(rows, 2 * d)                       # torch's flattening of [B,2,H,W]: c * d + pos
    logits = flat @ a["pi_w"].T + a["pi_b"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    pi = e / e.sum(axis=1, keepdims=True)
    v1 = np.maximum(v0 @ a["v1_w"].T + a["v1_b"], 0)
    pre = (v1 @ a["v2_w"].T + a["v2_b"])[:, 0]
    mass = (64 * (np.abs(flat) @ np.abs(a["pi_w"]).T + np.abs(a["pi_b"])).max(),
            8 * (np.abs(v0) @ np.abs(a["v1_w"]).T + np.abs(a["v1_b"])).max(),
            256 * (np.abs(v1) @ np.abs(a["v2_w"]).T + np.abs(a["v2_b"])).max())
    return logits, pi, np.tanh(pre), pre, mass


def _assert_exact_in_fp32(a, logits, pre, mass):
    """Every partial sum of the kernels, in any order, is exact in fp32: the head-convolution sums are integers of at most 3 C,
    the terms of a logit are multiples of 1/64, those of v1 multiples of 1/8 and those of the value's pre-activation multiples of
    1/256, and even the
    sum of their absolute values stays below 2^24 units."""
    ch = a["pconv_w"].shape[1]
    for nm, unit in (("pi_w", 64), ("pi_b", 8), ("v1_w", 8), ("v1_b", 8), ("v2_w", 32), ("v2_b", 8)):
        assert np.array_equal(np.round(a[nm] * unit), a[nm] * unit), nm
    for nm in ("pconv_w", "pconv_b", "vconv_w", "vconv_b"):
        assert np.array_equal(np.round(a[nm]), a[nm]), nm
    fin = np.isfinite(a["act"])
    assert np.array_equal(np.round(a["act"][fin]), a["act"][fin]) and np.abs(a["act"][fin]).max() * ch + 2 < 2 ** 24
    assert max(mass) < 2 ** 24
    assert np.array_equal(logits.astype(np.float32).astype(np.float64), logits) and np.array_equal(pre.astype(np.float32).astype(np.float64), pre)


_hexact = {}


def _heads_exact_case(rows, h, wd, ch, vh, keep=True):
    """test_gpu_net_native_io._heads_exact_case's recipe for an h x wd board and any value_hidden: act in {0,1,2} (1/2, 1/4, 1/4);
    head-conv weights in {-1,0,1} with 3/4 zeros, integer biases in [-2,2]; pi_w in {-1,0,1}/8 with 7/8 zeros (/64 from 256
    channels on, where the policy planes' values are an order of magnitude larger and /8 would make the softmax one-hot), v1_w in
    {-1,0,1}/8 with 7/8 zeros, their biases multiples of 1/8; v2_w in {-1,1}/32.
    Not degenerate: both policy planes and the value plane are non-zero somewhere, the softmax has mass on ten entries or more (on
    all of them where there are fewer) and no entry below 2^-100 (the relative bound applies to every entry), the value is off
    tanh's flat ends.  A draw that is degenerate -- this happens on the smallest boards -- is drawn again from the next seed; the
    choice looks at the fp64 reference only.  Host arrays only; the device copies are made by the caller."""
    key = (rows, h, wd, ch, vh)
    if key in _hexact:
        return _hexact[key]
    d = h * wd
    pi_unit = 8 if ch < 256 else 64
    for attempt in range(64):
        rng = np.random.RandomState(7 + 1000 * rows + 10 * h + 3 * wd + ch + 17 * vh + 7919 * attempt)
        tern = lambda shape, pz: rng.choice([-1.0, 0.0, 1.0], size=shape, p=[(1 - pz) / 2, pz, (1 - pz) / 2])
        a = dict(act=rng.choice([0.0, 1.0, 2.0], size=(rows, h, wd, ch), p=[0.5, 0.25, 0.25]),
                 pconv_w=tern((2, ch), 0.75), pconv_b=rng.randint(-2, 3, size=(2,)).astype(np.float64),
                 vconv_w=tern((1, ch), 0.75), vconv_b=rng.randint(-2, 3, size=(1,)).astype(np.float64),
                 pi_w=tern((d + 1, 2 * d), 0.875) / pi_unit, pi_b=rng.randint(-8, 9, size=(d + 1,)) / 8.0,
                 v1_w=tern((vh, d), 0.875) / 8, v1_b=rng.randint(-8, 9, size=(vh,)) / 8.0,
                 v2_w=rng.choice([-1.0, 1.0], size=(1, vh)) / 32, v2_b=rng.randint(-2, 3, size=(1,)) / 8.0)
        logits, pi, v, pre, mass = _heads_ref(a, rows, d)
        act = a["act"].reshape(rows * d, ch)
        planes = all((act @ wr + br > 0).any() for wr, br in ((a["pconv_w"][0], a["pconv_b"][0]), (a["pconv_w"][1], a["pconv_b"][1]),
                                                              (a["vconv_w"][0], a["vconv_b"][0])))
        if planes and ((pi > 1e-6).sum(axis=1) >= min(10, d + 1)).all() and pi.min() >= 2.0 ** -100 and (np.abs(v) < 0.999).all():
            break
    else:
        raise AssertionError("no draw of %s is non-degenerate" % (key,))
    _assert_exact_in_fp32(a, logits, pre, mass)
    cs = dict(a=a, logits=logits, pi=pi, v=v, rows=rows, h=h, wd=wd, ch=ch, vh=vh, attempt=attempt)
    if keep:
        _hexact[key] = cs
    return cs


def _run_heads(L, t, ch, vh, rows, h, wd, stride=None, ws=None, ws_bytes=None):
    """-> (status, pi buffer [rows, stride], value buffer [rows + 1], logits buffer [rows, stride]); all prefilled with NaN"""
    import torch
    d = h * wd
    stride = d + 1 if stride is None else stride
    nan = lambda *shape: torch.full(shape, NAN, device="cuda", dtype=torch.float32)
    pi, value, logits = nan(rows, stride), nan(rows + 1), nan(rows, stride)
    if ws is None:
        ws_bytes = L.elfnet_heads_workspace(rows, h, wd)
        ws = torch.empty((ws_bytes,), device="cuda", dtype=torch.uint8)
    hd = cc.heads_struct(t, ch, vh)
    rc = L.elfnet_heads_f16(cc.ptr(t["act"]), C.byref(hd), rows, h, wd, cc.ptr(pi), stride, cc.ptr(value), cc.ptr(logits), cc.ptr(ws),
                            ws_bytes, cc.stream())
    torch.cuda.synchronize()
    return rc, pi, value, logits


def _check_heads(tag, pi, value, logits, ref_logits, ref_pi, ref_v, rows, d):
    """test_heads_exact's checks on host arrays: logits bit-equal to the fp64 reference, pi within relative 1e-4 and its sum within
    1e-5 of 1, V within 2^-20; the padding of the strided rows and the element behind value still NaN"""
    lg = logits[:, :d + 1]
    bad = int((lg != ref_logits.astype(np.float32)).sum())
    rel = np.abs(pi[:, :d + 1].astype(np.float64) - ref_pi) / ref_pi
    sums = np.abs(pi[:, :d + 1].astype(np.float64).sum(axis=1) - 1)
    verr = np.abs(value[:rows].astype(np.float64) - ref_v)
    print("%s: %d of %d logits differ; pi: max relative error %.3g, max |sum - 1| %.3g; V: max error %.3g (2^-20 = %.3g)"
          % (tag, bad, lg.size, rel.max(), sums.max(), verr.max(), V_ABS))
    assert bad == 0
    assert not np.isnan(pi[:, :d + 1]).any() and not np.isnan(value[:rows]).any()
    assert rel.max() <= PI_REL
    assert sums.max() <= PI_SUM
    assert verr.max() <= V_ABS
    assert np.isnan(pi[:, d + 1:]).all() and np.isnan(logits[:, d + 1:]).all() and np.isnan(value[rows])


# ---------------------------------------------------------------------------------------------------------------------------------
# D. heads: shapes

@pytest.mark.parametrize("rows,h,wd,ch,vh", [(2048, 19, 19, 8, 256),     # the workload's launch: rpb = 8, 54 432 B of dynamic LDS
                                             (2049, 25, 25, 8, 256),     # 11 028 B per row: rpb falls from 8 to 5; the last workgroup holds 4
                                             (3, 9, 9, 24, 256),         # 3 of a group's 8 lanes hold a chunk
                                             (3, 9, 9, 72, 256),         # 9 of 16
                                             (3, 9, 9, 136, 256),        # 17 of 32
                                             (3, 9, 9, 264, 256),        # 33 chunks on 32 lanes: only lane 0 takes a second one
                                             (3, 9, 9, 520, 256),        # 65: lane 0 takes a third
                                             (182, 19, 19, 264, 8),      # 65 702 positions on 2048 x 32: the position loop goes round
                                             (5, 9, 9, 64, 1), (5, 9, 9, 64, 65), (5, 9, 9, 64, 300),
                                             (4, 5, 7, 64, 64), (4, 7, 5, 64, 64),
                                             (2, 1, 1, 8, 1)])           # d = 1: two logits, one value neuron
def test_heads_shapes_exact(elf, rows, h, wd, ch, vh):
    """test_heads_exact's checks, with three floats of NaN padding behind every pi / logits row, at the shapes where
    elfnet_heads_f16 takes another path"""
    d = h * wd
    if (rows, h) == (2048, 19):
        assert min(8, rows // 256) * (4 * d + 1 + vh) * 4 == 54432
    if (rows, h) == (2049, 25):
        per_row = (4 * d + 1 + vh) * 4
        assert per_row == 11028 and 6 * per_row > 65536 >= 5 * per_row and rows % 5 == 4
    if ch == 264 and rows == 182:
        assert rows * d == 65702 > 2048 * (256 // 32) * 4
    cs = _heads_exact_case(rows, h, wd, ch, vh, keep=rows * d * ch < 10 ** 6)
    rc, pi, value, logits = _run_heads(elf.lib(), _upload(cs["a"]), ch, vh, rows, h, wd, d + 1 + 3)
    assert rc == 0
    _check_heads(str((rows, h, wd, ch, vh)), pi.cpu().numpy(), value.cpu().numpy(), logits.cpu().numpy(), cs["logits"], cs["pi"], cs["v"],
                 rows, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# E. heads: guards and alignment

def test_heads_guarded_operands_at_the_weakest_alignment(elf):
    """Every operand a view inside a larger NaN-filled buffer: act and the head-convolution weights at 16 modulo 32 (16-B loads),
    pi_w at 4 modulo 8 (pairs), v1_w, whose rows are d = 81 halves, and the small vectors at 2 modulo 4.  The workspace is exactly
    rows * 3 * d * 4 bytes -- what the header's size check demands -- inside a buffer of a sentinel pattern, which is unchanged
    in front of and behind it after the call.  pi, V and logits are the unguarded run's bit for bit, and pass the exact checks."""
    import torch
    rows, h, wd, ch, vh = 5, 9, 9, 64, 65
    d = h * wd
    cs = _heads_exact_case(rows, h, wd, ch, vh)
    plain = _upload(cs["a"])
    L = elf.lib()
    rc, pi0, v0, lg0 = _run_heads(L, plain, ch, vh, rows, h, wd)
    assert rc == 0
    where = dict(act=(32, 16), pconv_w=(32, 16), vconv_w=(32, 16), pi_w=(8, 4))
    t = {}
    for nm in ("act",) + cc.HEAD_NAMES:
        mod, rem = where.get(nm, (4, 2))
        t[nm], _, _ = cc.carve(plain[nm], 2 * (d + 1) + ch, mod, rem)
        assert t[nm].data_ptr() % mod == rem
    sentinel = 0x5A5A5A5A
    need = rows * 3 * d
    assert need * 4 < L.elfnet_heads_workspace(rows, h, wd)        # the rounded-up size is not what is required
    wbuf = torch.full((256 + need + 256,), sentinel, device="cuda", dtype=torch.int32)
    ws = wbuf[256:256 + need]
    rc, pi, v, lg = _run_heads(L, t, ch, vh, rows, h, wd, ws=ws, ws_bytes=need * 4)
    assert rc == 0
    assert bool((wbuf[:256] == sentinel).all()) and bool((wbuf[256 + need:] == sentinel).all())
    for got, first in ((pi, pi0), (v, v0), (lg, lg0)):
        assert torch.equal(got.view(torch.int32), first.view(torch.int32))
    _check_heads("guarded", pi.cpu().numpy(), v.cpu().numpy(), lg.cpu().numpy(), cs["logits"], cs["pi"], cs["v"], rows, d)


# ---------------------------------------------------------------------------------------------------------------------------------
# F. heads: values

def _softmax_case(pi_b, zero_pi_w=False):
    """4 rows of 9 x 9, C = 8, vh = 8 of the exact recipe with the given pi_b [d + 1] (and pi_w = 0 on request): the logits are
    multiples of 1/8 below 2^15 in magnitude, so the logits, the row maximum and every lg - mx are exact in fp32"""
    rows, h, wd, ch, vh = 4, 9, 9, 8, 8
    d = h * wd
    a = dict(_heads_exact_case(rows, h, wd, ch, vh)["a"])
    a["pi_b"] = np.asarray(pi_b, np.float64)
    if zero_pi_w:
        a["pi_w"] = np.zeros_like(a["pi_w"])
    logits, pi, v, pre, mass = _heads_ref(a, rows, d)
    _assert_exact_in_fp32(a, logits, pre, mass)
    assert np.abs(logits).max() < 2 ** 15 and np.array_equal(np.round(logits * 8), logits * 8)
    diff = logits - logits.max(axis=1, keepdims=True)
    assert np.array_equal(diff.astype(np.float32).astype(np.float64), diff)
    return a, logits, pi, v, (rows, h, wd, ch, vh)


def test_heads_softmax_with_a_large_offset(elf):
    """pi_b = 30 000 everywhere: logits within a few units of 3e4, where expf without the subtraction of the maximum is Inf.  pi
    keeps the relative bound against the fp64 softmax and is not NaN."""
    d = 81
    a, logits, pi64, v64, (rows, h, wd, ch, vh) = _softmax_case(np.full(d + 1, 30000.0))
    spread = logits.max(axis=1) - logits.min(axis=1)
    assert (logits > 29000).all() and (logits < 31000).all() and (spread >= 2).all() and (spread < 40).all()
    rc, pi, value, lg = _run_heads(elf.lib(), _upload(a), ch, vh, rows, h, wd)
    assert rc == 0
    _check_heads("offset 3e4", pi.cpu().numpy(), value.cpu().numpy(), lg.cpu().numpy(), logits, pi64, v64, rows, d)


def test_heads_softmax_with_entries_that_underflow(elf):
    """pi_b cycles through 0, -40, -80, -86, -90, -104 and -250: a spread above 200 in every row.  Entries whose fp64 value is at
    least 2^-126 (fp32's smallest normal number) keep the relative bound; the entries below it -- some of them fp32 subnormals,
    some below 2^-150 -- come out as at most 2^-125 (0 is allowed) and never negative or NaN; the sum bound holds."""
    d = 81
    steps = np.array([0.0, -40.0, -80.0, -86.0, -90.0, -104.0, -250.0])
    a, logits, pi64, v64, (rows, h, wd, ch, vh) = _softmax_case(steps[np.arange(d + 1) % 7])
    big = pi64 >= 2.0 ** -126
    assert ((logits.max(axis=1) - logits.min(axis=1)) > 200).all()
    for r in range(rows):
        assert big[r].sum() >= 20 and (pi64[r] < 2.0 ** -150).sum() >= 5 and ((pi64[r] < 2.0 ** -126) & (pi64[r] > 2.0 ** -149)).sum() >= 5
        assert (big[r] & (pi64[r] < 1e-30)).sum() >= 5                       # small and still bound relatively
    rc, pi, value, lg = _run_heads(elf.lib(), _upload(a), ch, vh, rows, h, wd)
    assert rc == 0
    pi, lg = pi.cpu().numpy(), lg.cpu().numpy()
    assert np.array_equal(lg, logits.astype(np.float32))
    got = pi.astype(np.float64)
    rel = np.abs(got[big] - pi64[big]) / pi64[big]
    print("underflow: max relative error of the %d entries >= 2^-126: %.3g; largest of the %d others %.3g; max |sum - 1| %.3g"
          % (big.sum(), rel.max(), (~big).sum(), got[~big].max(), np.abs(got.sum(axis=1) - 1).max()))
    assert not np.isnan(pi).any()
    assert rel.max() <= PI_REL
    assert (got[~big] >= 0).all() and (got[~big] <= 2.0 ** -125).all()
    assert np.abs(got.sum(axis=1) - 1).max() <= PI_SUM


def test_heads_softmax_of_equal_logits_is_uniform(elf):
    """pi_w = 0 and pi_b = 3.5: every logit is 3.5 and every entry of pi within relative 1e-6 of 1 / (d + 1) (expf(0) = 1, an exact
    sum of d + 1 ones, one division)"""
    d = 81
    a, logits, pi64, v64, (rows, h, wd, ch, vh) = _softmax_case(np.full(d + 1, 3.5), zero_pi_w=True)
    assert (logits == 3.5).all()
    rc, pi, value, lg = _run_heads(elf.lib(), _upload(a), ch, vh, rows, h, wd)
    assert rc == 0
    pi = pi.cpu().numpy().astype(np.float64)
    assert np.array_equal(lg.cpu().numpy(), logits.astype(np.float32))
    rel = np.abs(pi * (d + 1) - 1)
    print("uniform: max relative error %.3g" % rel.max())
    assert rel.max() <= 1e-6


def test_heads_tanh_ends(elf):
    """Three rows whose activation is 0, 1 and 2 in channel 0 and 0 elsewhere; vconv_w picks channel 0, value_linear1 copies
    position 40 into each of its 8 neurons, v2_w = 2.5 and v2_b = -20: the pre-activations are exactly -20, 0 and +20.  V is
    within 2^-20 of -1 and +1 and exactly 0 in the middle."""
    rows, h, wd, ch, vh = 3, 9, 9, 8, 8
    d = h * wd
    a = dict(act=np.zeros((rows, h, wd, ch)), pconv_w=np.zeros((2, ch)), pconv_b=np.zeros(2), vconv_w=np.zeros((1, ch)),
             vconv_b=np.zeros(1), pi_w=np.zeros((d + 1, 2 * d)), pi_b=np.zeros(d + 1), v1_w=np.zeros((vh, d)), v1_b=np.zeros(vh),
             v2_w=np.full((1, vh), 2.5), v2_b=np.full(1, -20.0))
    a["act"][:, :, :, 0] = np.arange(rows)[:, None, None]
    a["vconv_w"][0, 0] = 1.0
    a["v1_w"][:, 40] = 1.0
    logits, pi64, v64, pre, mass = _heads_ref(a, rows, d)
    assert pre.tolist() == [-20.0, 0.0, 20.0] and max(mass) < 2 ** 24
    rc, pi, value, lg = _run_heads(elf.lib(), _upload(a), ch, vh, rows, h, wd)
    assert rc == 0
    v = value.cpu().numpy()
    print("tanh ends: V = %r" % (v[:rows].tolist(),))
    assert abs(float(v[0]) + 1) <= V_ABS and abs(float(v[2]) - 1) <= V_ABS and abs(float(v[0])) <= 1 and abs(float(v[2])) <= 1
    assert v[1] == 0 and np.isnan(v[rows])


def _poison_case():
    """5 rows of 9 x 9, C = 64, vh = 65 of the exact recipe; the cell (row 2, position 40, channel 9) will be poisoned.
    pconv_w[0][9] is set to 1 and pconv_w[1][9] to 0, so that +Inf there makes policy plane 0 +Inf at the position and plane 1 NaN
    before its ReLU, which is 0 behind it."""
    rows, h, wd, ch, vh = 5, 9, 9, 64, 65
    a = {nm: v.copy() for nm, v in _heads_exact_case(rows, h, wd, ch, vh)["a"].items()}
    a["pconv_w"][0, 9], a["pconv_w"][1, 9] = 1.0, 0.0
    return a, (rows, h, wd, ch, vh), (2, 40, 9)


def test_heads_one_nan_activation(elf):
    """The three head convolutions end in fmaxf(sum + bias, 0): a NaN activation makes the sums of its position NaN and the
    outputs 0.  Every other row's pi, V and logits are the clean run's bits; the poisoned row is finite, and is the fp64 reference
    with that position's three head-convolution outputs set to 0: a diverged trunk shows as a finite pi (include/elf_amd.h)."""
    import torch
    a, (rows, h, wd, ch, vh), (r, pos, c0) = _poison_case()
    d = h * wd
    L = elf.lib()
    rc, pi0, v0, lg0 = _run_heads(L, _upload(a), ch, vh, rows, h, wd)
    assert rc == 0
    b = dict(a)
    b["act"] = a["act"].copy()
    b["act"].reshape(rows, d, ch)[r, pos, c0] = NAN
    logits, pi64, v64, pre, mass = _heads_ref(b, rows, d, zero=(r, pos))
    clean = _heads_ref(a, rows, d)
    _assert_exact_in_fp32(b, logits, pre, mass)
    assert np.isfinite(logits).all() and not np.array_equal(logits[r], clean[0][r]) and pre[r] != clean[3][r]   # the position matters
    others = np.arange(rows) != r
    assert np.array_equal(logits[others], clean[0][others])
    rc, pi, v, lg = _run_heads(L, _upload(b), ch, vh, rows, h, wd)
    assert rc == 0
    keep = torch.from_numpy(others).cuda()
    assert torch.equal(pi[keep].view(torch.int32), pi0[keep].view(torch.int32))
    assert torch.equal(lg[keep].view(torch.int32), lg0[keep].view(torch.int32))
    assert torch.equal(v[:rows][keep].view(torch.int32), v0[:rows][keep].view(torch.int32))
    assert bool(torch.isfinite(pi[r]).all()) and bool(torch.isfinite(lg[r]).all()) and bool(torch.isfinite(v[r]))
    _check_heads("one NaN activation", pi.cpu().numpy(), v.cpu().numpy(), lg.cpu().numpy(), logits, pi64, v64, rows, d)


def test_heads_one_inf_activation(elf):
    """+Inf on a channel whose pconv_w[0] is positive: policy plane 0 is +Inf at the position, the row's logits are +Inf, -Inf or
    NaN (0 x Inf) by pi_w's column, and the row's pi is not finite anywhere, as torch.softmax of a row with an infinite logit is
    (exp(Inf - Inf) is NaN and so is the sum).  Every other row's pi, V and logits are the clean run's bits."""
    import torch
    a, (rows, h, wd, ch, vh), (r, pos, c0) = _poison_case()
    d = h * wd
    assert a["pconv_w"][0, c0] > 0 and (a["pi_w"][:, pos] > 0).any()        # plane 0's column `pos` of pi_w: some logit is +Inf
    L = elf.lib()
    rc, pi0, v0, lg0 = _run_heads(L, _upload(a), ch, vh, rows, h, wd)
    assert rc == 0
    b = dict(a)
    b["act"] = a["act"].copy()
    b["act"].reshape(rows, d, ch)[r, pos, c0] = INF
    rc, pi, v, lg = _run_heads(L, _upload(b), ch, vh, rows, h, wd)
    assert rc == 0
    keep = torch.from_numpy(np.arange(rows) != r).cuda()
    assert torch.equal(pi[keep].view(torch.int32), pi0[keep].view(torch.int32))
    assert torch.equal(lg[keep].view(torch.int32), lg0[keep].view(torch.int32))
    assert torch.equal(v[:rows][keep].view(torch.int32), v0[:rows][keep].view(torch.int32))
    assert bool(torch.isfinite(pi0).all())
    col = torch.from_numpy(a["pi_w"][:, pos]).cuda()
    assert bool((lg[r][col > 0] == INF).all()) and bool((lg[r][col < 0] == -INF).all()) and bool(torch.isnan(lg[r][col == 0]).all())
    assert not bool(torch.isfinite(pi[r]).any())
    want = torch.softmax(lg[r], dim=0)
    assert not bool(torch.isfinite(want).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# G. batch invariance

def test_heads_rows_do_not_depend_on_the_batch(elf):
    """Random fp16 operands (sums that do round, so an order that changed with the row count would show): rows 0, 7, 8, 1000, 2051
    and 2052 of a 2053-row 9 x 9 batch (eight rows per workgroup, the last one holds five) each run alone as rows = 1 (one row per
    workgroup, another grid of k_head_convs) give the batch's pi, logits and V bit for bit."""
    import torch
    rows, n, ch, vh = 2053, 9, 64, 256
    d = n * n
    g = torch.Generator(device="cuda").manual_seed(2053)
    rn = lambda shape, scale: (torch.randn(shape, device="cuda", generator=g) * scale).half()
    t = dict(act=torch.relu(rn((rows, n, n, ch), 1.0)), pconv_w=rn((2, ch), ch ** -0.5), pconv_b=rn((2,), 0.1), vconv_w=rn((1, ch), ch ** -0.5),
             vconv_b=rn((1,), 0.1), pi_w=rn((d + 1, 2 * d), (2 * d) ** -0.5), pi_b=rn((d + 1,), 0.1), v1_w=rn((vh, d), d ** -0.5),
             v1_b=rn((vh,), 0.1), v2_w=rn((1, vh), vh ** -0.5), v2_b=rn((1,), 0.1))
    L = elf.lib()
    rc, pi, v, lg = _run_heads(L, t, ch, vh, rows, n, n)
    assert rc == 0
    assert bool(torch.isfinite(pi).all()) and bool(torch.isfinite(v[:rows]).all())
    assert not torch.equal(pi[0], pi[1]) and float(v[:rows].std().item()) > 0
    for i in (0, 7, 8, 1000, 2051, 2052):
        one = dict(t, act=t["act"][i:i + 1])
        assert one["act"].data_ptr() % 16 == 0
        rc, pi1, v1, lg1 = _run_heads(L, one, ch, vh, 1, n, n)
        assert rc == 0
        assert torch.equal(pi1[0].view(torch.int32), pi[i].view(torch.int32)), i
        assert torch.equal(lg1[0].view(torch.int32), lg[i].view(torch.int32)), i
        assert torch.equal(v1[:1].view(torch.int32), v[i:i + 1].view(torch.int32)), i


def test_input_conv_boards_do_not_depend_on_the_batch(elf):
    """Random fp16 operands: boards 0, 1, 205 and 409 of a 410-board 9 x 9 batch (519 tiles on 512 workgroups: a board's positions
    lie anywhere in a tile, and some tiles are a workgroup's second) each run alone give the batch's y rows bit for bit"""
    import torch
    rows, n, c, k = 410, 9, 18, 64
    g = torch.Generator(device="cuda").manual_seed(410)
    x = torch.randn((rows, n, n, c), device="cuda", generator=g).half()
    w = (torch.randn((k, 3, 3, c), device="cuda", generator=g) * (9 * c) ** -0.5).half()
    b = torch.randn((k,), device="cuda", generator=g).half()
    L = elf.lib()
    _, y = cc.guarded(rows, n, n, k)
    assert cc.conv_in(L, x, w, b, y, rows, n, n, c, k, 0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    for i in (0, 1, 205, 409):
        buf, y1 = cc.guarded(1, n, n, k)
        assert x[i].data_ptr() % 4 == 0
        assert cc.conv_in(L, x[i], w, b, y1, 1, n, n, c, k, 0) == 0
        torch.cuda.synchronize()
        assert torch.equal(y1[0].view(torch.int16), y[i].view(torch.int16)), i
        assert bool(torch.isnan(buf[-1]).all())


def test_native_net_rows_do_not_depend_on_the_batch(elf):
    """NativeInferenceNet at 9 x 9, 2 blocks, 64 channels on 37 random binary feature rows: all at once, through
    chunked_forward(chunk_rows=16) (16 + 16 + 5) and one row at a time.  pi and V are bit-equal in all three: what a search sees
    for a position does not depend on how many other positions were evaluated with it."""
    import torch
    from elf_amd.net import NativeInferenceNet, chunked_forward, make_net
    n, rows = 9, 37
    net = NativeInferenceNet(make_net(board_size=n, num_block=2, dim=64, fold_bn=True, seed=11))
    g = torch.Generator(device="cuda").manual_seed(37)
    s = (torch.rand((rows, 18, n, n), device="cuda", generator=g) < 0.3).half().contiguous(memory_format=torch.channels_last)
    whole = net({"s": s})
    chunked = chunked_forward(net, s, chunk_rows=16)
    torch.cuda.synchronize()
    assert tuple(whole["pi"].shape) == (rows, n * n + 1) and bool(torch.isfinite(whole["pi"]).all()) and bool(torch.isfinite(whole["V"]).all())
    assert not torch.equal(whole["pi"][0], whole["pi"][1])
    assert torch.equal(chunked["pi"].view(torch.int32), whole["pi"].view(torch.int32))
    assert torch.equal(chunked["V"].view(torch.int32), whole["V"].view(torch.int32))
    for i in range(rows):
        one = net({"s": s[i:i + 1]})
        torch.cuda.synchronize()
        assert torch.equal(one["pi"][0].view(torch.int32), whole["pi"][i].view(torch.int32)), i
        assert torch.equal(one["V"].view(torch.int32), whole["V"][i:i + 1].view(torch.int32)), i
