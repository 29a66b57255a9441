"""GPU: the bf16 trunk convolution on the 256 x 256 tile (elfnet_conv3x3_bf16_big, elf_amd/csrc/net_conv3x3_bf16_big.hip) against a
plain high-precision reference and, bit for bit, against the 128-tile.  The shapes are the smallest at which it can go wrong:
M = 105 (one partial tile, one K chunk per tap: the 9-K-tile minimum, where the ring's prologue and drain meet), M = 324 (a full
tile and one of 68 rows, three chunks per tap, the skip's M - 1 clamp) and M = 272 on a non-square board with two channel columns."""
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 64, 256), (4, 9, 9, 192, 256), (1, 17, 16, 128, 512)]


def _seed(rows, h, wd, c, k):
    return 7300 + rows + h + wd + c + k


def _run(L, tile, x, w, b, r, relu):
    """one launch (tile None: the big tile) into a NaN-filled bf16 y with one guard row of NaN behind it, which stays NaN"""
    import torch
    rows, h, wd, c = x.shape
    k = w.shape[0]
    buf = torch.full((rows * h * wd + 1, k), cc.NAN, device="cuda", dtype=torch.bfloat16)
    y = buf[:rows * h * wd].view(rows, h, wd, k)
    a = (cc.ptr(x), cc.ptr(w), cc.ptr(b), cc.ptr(r), cc.ptr(y), rows, h, wd, c, k, int(relu))
    rc = L.elfnet_conv3x3_bf16_big(*a, cc.stream()) if tile is None else L.elfnet_conv3x3_bf16_tile(*a, tile, cc.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[-1]).all()), "the guard row behind y was written"
    return y


@pytest.mark.parametrize("use_res,relu", cc.RES_RELU)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_integers_rounded_once(elf, shape, use_res, relu):
    """Integer operands, the bias scaled by 64 (exact in bf16 up to 512): every partial sum is an integer far below 2^24, so fp32 is
    exact, while |conv + b + r| passes 512 and many outputs are not bf16 numbers.  The output is, bit for bit, that fp32 value,
    fmax(., 0), rounded once to nearest even.  x and res lie between NaN guards."""
    import torch
    d = cc.int_case(_seed(*shape), *shape, not_degenerate=True)
    x, w, b = cc.carve(d["x"].bfloat16(), 64)[0], d["w"].bfloat16(), (d["b"].float() * 64).bfloat16()
    r = cc.carve(d["r"].bfloat16(), 64)[0] if use_res else None
    v = d["conv"] + b.float() + (r.float() if use_res else 0)
    if relu:
        v = torch.fmax(v, torch.zeros((), device="cuda"))
    y = _run(elf.lib(), None, x, w, b, r, relu)
    bad = int((cc.bits(y) != cc.bits(v.bfloat16())).sum().item())
    print("%s res %d relu %d: %d of %d differ" % (shape, use_res, relu, bad, y.numel()))
    assert bad == 0


@pytest.mark.parametrize("use_res,relu", cc.RES_RELU)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_within_the_derived_bound_and_the_bits_of_the_128_tile(elf, shape, use_res, relu):
    """|y - v| <= 2^-8 |v| + (9 c + 2) 2^-23 S against the fp64 value v of the bf16 operands, S = conv(|x|, |w|) + |b| + |res|
    (tests/test_gpu_net_conv_bf16.py derives it), and y is elfnet_conv3x3_bf16_tile(..., 128, ...)'s on the same operands, bit for
    bit: same K order, same single rounding.  x and res lie between NaN guards."""
    import torch
    x, w, b, r = (t.bfloat16() for t in cc.rand_case(_seed(*shape), *shape))
    x, r = cc.carve(x, 64)[0], (cc.carve(r, 64)[0] if use_res else None)
    xd, wd_, bd = x.double(), w.double(), b.double()
    v, s = cc.conv_fp32(xd, wd_) + bd, cc.conv_fp32(xd.abs(), wd_.abs()) + bd.abs()
    if use_res:
        v, s = v + r.double(), s + r.double().abs()
    if relu:
        v = v.clamp(min=0)
    L = elf.lib()
    y = _run(L, None, x, w, b, r, relu)
    assert not bool(torch.isnan(y).any())
    err, bound = (y.double() - v).abs(), 2.0 ** -8 * v.abs() + (9 * shape[3] + 2) * 2.0 ** -23 * s
    bad = int((cc.bits(y) != cc.bits(_run(L, 128, x, w, b, r, relu))).sum().item())
    print("%s res %d relu %d: max err / bound %.3f, %d bits off the 128-tile" % (shape, use_res, relu, float((err / bound).max()), bad))
    assert bool((err <= bound).all())
    assert bad == 0


def test_a_net_returns_the_same_bits_through_either_tile(elf):
    """A two-block 256-channel 9 x 9 bf16 net on 4 rows through NativeBf16InferenceNet: with bf16_big_min_positions = 1 every trunk
    convolution is the big tile's, with 0 none is, and pi and V have the same bits."""
    import torch
    from elf_amd.net import NativeBf16InferenceNet, make_net
    net = make_net(board_size=9, num_block=2, dim=256, dtype=torch.bfloat16, fold_bn=True)
    s = (torch.rand((4, 18, 9, 9), device="cuda", generator=torch.Generator(device="cuda").manual_seed(11)) < 0.3).half()
    f = NativeBf16InferenceNet(net)
    f.bf16_big_min_positions = 1
    big = f({"s": s})
    f.bf16_big_min_positions = 0
    small = f({"s": s})
    for key in ("pi", "V"):
        assert not bool(torch.isnan(big[key]).any())
        assert torch.equal(big[key].view(torch.int32), small[key].view(torch.int32)), key
