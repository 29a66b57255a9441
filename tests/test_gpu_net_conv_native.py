"""GPU: the hand-written trunk convolution (elfnet_conv3x3_f16 with algo 1, elf_amd/csrc/net_conv3x3.hip) on inputs whose result
is exact -- small integers, so every partial sum is an integer fp32 and fp16 hold exactly and any differing element is a wrong
halo, layout, swizzle or pipeline timing, never rounding -- then bit for bit against algo 0 (same K order, same MFMA), a race
screen (repeated launches return the bits of the first), and the shapes it refuses."""
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _seed(rows, h, wd, c, k):
    return 77 + rows + 1000 * h + c + 7 * k


def _rseed(rows, h, wd, c, k):
    return 4242 + rows


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("rows,n,c,k", [(3, 19, 256, 256),     # M = 1083: four full tiles and a 59-row tail
                                        (5, 9, 256, 256),      # M = 405: a tile straddles several boards
                                        (256, 9, 256, 256),    # M = 81 tiles exactly, no tail
                                        (1, 19, 256, 256),
                                        (3, 9, 128, 256),
                                        (3, 9, 64, 512)])
def test_exact_integers(elf, rows, n, c, k, use_res, relu):
    """equality with the nine-tap fp32 form; y is prefilled with NaN, and one guard row of NaN behind y's last row stays NaN (the
    tail tile's stores are masked)"""
    import torch
    d = cc.int_case(_seed(rows, n, n, c, k), rows, n, n, c, k)
    ref = d["conv"] + d["b"].float()
    if use_res:
        ref = ref + d["r"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = cc.guarded(rows, n, n, k)
    rc = cc.launch(elf.lib(), "plain", d["x"], d["w"], d["b"], d["r"] if use_res else None, y, relu)
    assert rc == 0
    torch.cuda.synchronize()
    bad = int((y.float() != ref).sum().item())   # a NaN left in y differs from everything
    print("rows %d n %d c %d k %d res %d relu %d: %d of %d differ" % (rows, n, c, k, use_res, relu, bad, y.numel()))
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
    assert cc.launch(elf.lib(), "plain", x, w, b, None, y, 0) == 0
    torch.cuda.synchronize()
    i = torch.arange(n, device="cuda")
    on = 3 - ((i == 0) | (i == n - 1)).long()           # taps on the board along one axis
    want = (256 * on[:, None] * on[None, :]).float()    # [n, n]
    assert want[0, 0] == 1024 and want[0, 1] == 1536 and want[1, 1] == 2304
    assert bool((y.float() == want[None, :, :, None]).all())


def test_bit_equal_with_algo_0(elf):
    """rows 48 x 19 x 19 with skip: the shipped kernel keeps algo 0's accumulation chain (tap-major K; in every 32-channel block
    one 32x32x16 MFMA over channels {0..7, 16..23}, the next over {8..15, 24..31}, as CK hands them out) and its epilogue
    sequence, so the two outputs are the same bits"""
    import torch
    rows = 48
    x, w, b, r = cc.rand_case(_rseed(rows, 19, 19, 256, 256), rows, 19, 19, 256, 256)
    ys = []
    for how in ("algo0", "plain"):
        y = torch.full((rows, 19, 19, 256), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.launch(elf.lib(), how, x, w, b, r, y, 1) == 0
        ys.append(y)
    torch.cuda.synchronize()
    print("%d of %d elements differ between algo 1 and algo 0" % (int((ys[0] != ys[1]).sum().item()), ys[0].numel()))
    assert torch.equal(ys[1], ys[0])


@pytest.mark.parametrize("rows,launches", [(48, 20), (2048, 5)])
def test_repeated_launches_return_the_same_bits(elf, rows, launches):
    """A staged buffer read before its data has landed, or restaged before its last read, gives wrong tiles that come and go.  The
    same inputs launched again and again return the bits of the first launch; at 2048 rows every CU is busy for 11 rounds, which
    is where a read placed too early shows."""
    import torch
    x, w, b, r = cc.rand_case(_rseed(rows, 19, 19, 256, 256), rows, 19, 19, 256, 256)
    first = None
    for i in range(launches):
        y = torch.full((rows, 19, 19, 256), float("nan"), device="cuda", dtype=torch.float16)
        assert cc.launch(elf.lib(), "plain", x, w, b, r, y, 1) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert not bool(torch.isnan(y).any())
        else:
            assert torch.equal(y, first), "launch %d differs from the first" % i


@pytest.mark.parametrize("c,k", [(72, 256), (256, 128)])
def test_unsupported_shapes_are_refused(elf, c, k):
    """c % 64 != 0 or k % 256 != 0: a negative status, nothing launched, y keeps its bytes"""
    import torch
    rows, n = 2, 9
    x = torch.zeros((rows, n, n, c), device="cuda", dtype=torch.float16)
    w = torch.zeros((k, 3, 3, c), device="cuda", dtype=torch.float16)
    b = torch.zeros((k,), device="cuda", dtype=torch.float16)
    y = torch.full((rows, n, n, k), 7.0, device="cuda", dtype=torch.float16)
    assert cc.launch(elf.lib(), "plain", x, w, b, None, y, 0) < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
