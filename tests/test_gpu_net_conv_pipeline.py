"""GPU: what the deep pipeline of the hand-written trunk convolution (elfnet_conv3x3_f16 with algo 1, elf_amd/csrc/net_conv3x3.hip)
can break and tests/test_gpu_net_conv_native.py does not reach: K-tile counts as short as the prologue's depth and odd ones
(Cin = 64, 192), two channel tiles, tiles with one valid row, tile counts that are and are not a multiple of the eight XCDs
workgroups are dealt over, and boards with h != w.  Every comparison is exact: bit for bit against algo 0 (same K order, same MFMA,
same epilogue sequence), against the integer nine-tap form, and launch against launch."""
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 77 + rows + 1000 * h + 31 * wd + c + 7 * k


def _rseed(rows, h, wd, c, k):
    return 4242 + rows + 31 * h + 977 * wd + c + 7 * k


SHAPES = [(1, 9, 9, 64, 256),       # Cin = 64: 9 K tiles, barely more than the prologue stages; M = 81: one partial tile
          (3, 19, 19, 128, 256),    # Cin = 128: 18 K tiles; 5 tiles, not a multiple of 8
          (3, 19, 19, 192, 256),    # Cin = 192: 27 K tiles, an odd count
          (1, 9, 9, 256, 512),      # K = 512: two channel tiles
          (1, 1, 257, 256, 256),    # M = 257: the second tile has one valid row
          (25, 9, 9, 256, 256),     # M = 2025: 8 tiles, a multiple of 8
          (3, 19, 19, 256, 256),    # 5 tiles
          (256, 9, 9, 256, 256)]    # 81 tiles: ten workgroups on every XCD and one more


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("rows,h,wd,c,k", SHAPES)
def test_bit_equal_with_algo_0(elf, rows, h, wd, c, k, use_res, relu):
    import torch
    shape = (rows, h, wd, c, k)
    x, w, b, r = cc.rand_case(_rseed(*shape), *shape)
    want = cc.algo0_ref(elf.lib(), _rseed(*shape), shape, use_res, relu)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "plain", x, w, b, r if use_res else None, y, relu) == 0
    torch.cuda.synchronize()
    print("%s res %d relu %d: %d of %d elements differ between algo 1 and algo 0"
          % ((rows, h, wd, c, k), use_res, relu, int((y != want).sum().item()), y.numel()))
    assert torch.equal(y, want)
    assert bool(torch.isnan(buf[-1]).all())


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("h,wd", [(5, 7), (7, 5)])
def test_non_square_boards_exact_integers(elf, h, wd, c, use_res, relu):
    """11 boards of 5 x 7 or 7 x 5 (M = 385: a full tile whose rows straddle boards, and a 129-row tail) against the nine-tap
    fp32 form; a kernel that took one of h, w for the other would put the halo in the wrong places"""
    import torch
    rows, k = 11, 256
    d = cc.int_case(_seed(rows, h, wd, c, k), rows, h, wd, c, k)
    ref = d["conv"] + d["b"].float()
    if use_res:
        ref = ref + d["r"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = cc.guarded(rows, h, wd, k)
    assert cc.launch(elf.lib(), "plain", d["x"], d["w"], d["b"], d["r"] if use_res else None, y, relu) == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("h %d w %d c %d res %d relu %d: %d of %d differ" % (h, wd, c, use_res, relu, bad, y.numel()))
    assert bad == 0
    assert bool(torch.isnan(buf[-1]).all())


def test_repeated_launches_at_an_odd_k_tile_count(elf):
    """48 x 19 x 19 with Cin = 192 (27 K tiles, 68 tiles of positions), with skip: 20 launches return the bits of the first, and
    the first is algo 0's.  A half-tile read before it has landed, or restaged before its last read, gives wrong tiles that come
    and go from launch to launch."""
    import torch
    shape = rows, h, wd, c, k = 48, 19, 19, 192, 256
    x, w, b, r = cc.rand_case(_rseed(*shape), *shape)
    want = cc.algo0_ref(elf.lib(), _rseed(*shape), shape, True, 1)
    first = None
    for i in range(20):
        y = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.launch(elf.lib(), "plain", x, w, b, r, y, 1) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert torch.equal(y, want), "the first launch differs from algo 0"
        else:
            assert torch.equal(y, first), "launch %d differs from the first" % i
