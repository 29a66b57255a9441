"""GPU: the bf16 trunk convolution (elfnet_conv3x3_bf16, elf_amd/csrc/net_conv3x3_bf16.hip), both workgroup tiles, against a plain
high-precision reference.  The shapes are the smallest that cover M = 105, 162 and 24 (none a multiple of either tile: partial last
tiles and the skip's M - 1 clamp), non-square boards, 1, 3 and 2 K chunks per tap (every prologue, and the 9-K-tile minimum), more
than one tile along K, and K = 64, where only the narrow tile exists."""
import copy

import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 64, 128), (2, 9, 9, 192, 256), (1, 4, 6, 128, 64)]
CASES = [(s, t) for s in SHAPES for t in (64, 128) if s[4] % t == 0]


def _seed(rows, h, wd, c, k):
    return 7100 + rows + h + wd + c + k


def _run(L, tile, x, w, b, r, relu):
    """one launch (tile None: the unpinned entry) into a NaN-filled bf16 y with one guard row of NaN behind it, which stays NaN"""
    import torch
    rows, h, wd, c = x.shape
    k = w.shape[0]
    buf = torch.full((rows * h * wd + 1, k), cc.NAN, device="cuda", dtype=torch.bfloat16)
    y = buf[:rows * h * wd].view(rows, h, wd, k)
    a = (cc.ptr(x), cc.ptr(w), cc.ptr(b), cc.ptr(r), cc.ptr(y), rows, h, wd, c, k, int(relu))
    rc = L.elfnet_conv3x3_bf16(*a, cc.stream()) if tile is None else L.elfnet_conv3x3_bf16_tile(*a, tile, cc.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[-1]).all()), "the guard row behind y was written"
    return y


@pytest.mark.parametrize("use_res,relu", cc.RES_RELU)
@pytest.mark.parametrize("shape,tile", CASES)
def test_exact_integers_rounded_once(elf, shape, tile, use_res, relu):
    """Integer operands, the bias scaled by 64 (exact in bf16 up to 512): every partial sum is an integer far below 2^24, so fp32 is
    exact, while |conv + b + r| passes 512 and a quarter to a third of the outputs are not bf16 numbers, hundreds of them ties.  The
    output is, bit for bit, that fp32 value, fmax(., 0), rounded once to nearest even.  x and res lie between NaN guards."""
    import torch
    d = cc.int_case(_seed(*shape), *shape, not_degenerate=True)
    x, w, b = cc.carve(d["x"].bfloat16(), 64)[0], d["w"].bfloat16(), (d["b"].float() * 64).bfloat16()
    r = cc.carve(d["r"].bfloat16(), 64)[0] if use_res else None
    v = d["conv"] + b.float() + (r.float() if use_res else 0)
    if relu:
        v = torch.fmax(v, torch.zeros((), device="cuda"))
    want = v.bfloat16()
    y = _run(elf.lib(), tile, x, w, b, r, relu)
    bad = int((cc.bits(y) != cc.bits(want)).sum().item())
    print("%s tile %d res %d relu %d: %d of %d differ" % (shape, tile, use_res, relu, bad, y.numel()))
    assert bad == 0


@pytest.mark.parametrize("use_res,relu", cc.RES_RELU)
@pytest.mark.parametrize("shape,tile", CASES)
def test_random_within_the_derived_bound(elf, shape, tile, use_res, relu):
    """|y - v| <= 2^-8 |v| + (9 c + 2) 2^-23 S against the fp64 value v of the bf16 operands, S = conv(|x|, |w|) + |b| + |res|.
    Derived: half a bf16 ulp is at most 2^-8 relative, and an fp32 sum of n = 9 c + 2 terms in any order errs by at most
    n 2^-24 S to first order, doubled here."""
    import torch
    x, w, b, r = (t.bfloat16() for t in cc.rand_case(_seed(*shape), *shape))
    if not use_res:
        r = None
    xd, wd_, bd = x.double(), w.double(), b.double()
    v, s = cc.conv_fp32(xd, wd_) + bd, cc.conv_fp32(xd.abs(), wd_.abs()) + bd.abs()
    if use_res:
        v, s = v + r.double(), s + r.double().abs()
    if relu:
        v = v.clamp(min=0)
    y = _run(elf.lib(), tile, x, w, b, r, relu)
    assert not bool(torch.isnan(y).any())
    err, bound = (y.double() - v).abs(), 2.0 ** -8 * v.abs() + (9 * shape[3] + 2) * 2.0 ** -23 * s
    print("%s tile %d res %d relu %d: max err / bound %.3f" % (shape, tile, use_res, relu, float((err / bound).max())))
    assert bool((err <= bound).all())


def test_the_entry_takes_the_tile_of_its_rule(elf):
    """the unpinned entry returns the bits of the pinned one at elfnet_conv3x3_bf16_pick(M, k, CUs), with skip and ReLU"""
    import torch
    L, shape = elf.lib(), SHAPES[1]
    x, w, b, r = (t.bfloat16() for t in cc.rand_case(_seed(*shape), *shape))
    tile = L.elfnet_conv3x3_bf16_pick(shape[0] * shape[1] * shape[2], shape[4], torch.cuda.get_device_properties(0).multi_processor_count)
    assert tile in (64, 128)
    assert torch.equal(cc.bits(_run(L, None, x, w, b, r, 1)), cc.bits(_run(L, tile, x, w, b, r, 1)))


def test_a_bf16_net_is_no_further_from_fp64_than_eager(elf):
    """A two-block 64-channel 9 x 9 bf16 net on 8 rows: the RMS error of pi and of V against the same weights in fp64 is at most
    twice the eager bf16 net's (the fused route rounds fewer times, so it should be below; 2 is slack for other rounding patterns
    in so small a net), through the kernel and, with bf16_conv = False, through MIOpen and elfnet_bias_act_bf16."""
    import torch
    from elf_amd.net import FusedInferenceNet, make_net
    net = make_net(board_size=9, num_block=2, dim=64, dtype=torch.bfloat16, fold_bn=True)
    s = (torch.rand((8, 18, 9, 9), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) < 0.3).float()
    ref = copy.deepcopy(net).cpu().double().to(memory_format=torch.contiguous_format)
    with torch.no_grad():
        truth, eager = ref({"s": s.cpu()}), net({"s": s})
    fused, pair = FusedInferenceNet(net), FusedInferenceNet(net)
    fused.bf16_conv, pair.bf16_conv = True, False
    rms = lambda o, key: float((o[key].double().cpu() - truth[key].double()).pow(2).mean().sqrt())
    for name, f in (("kernel", fused), ("pair", pair)):
        out = f({"s": s})
        for key in ("pi", "V"):
            print("%s %s: rms error %.3e, eager %.3e, ratio %.3f" % (name, key, rms(out, key), rms(eager, key), rms(out, key) / rms(eager, key)))
            assert rms(out, key) <= 2 * rms(eager, key)
