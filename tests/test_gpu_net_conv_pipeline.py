"""GPU: what the deep pipeline of the hand-written trunk convolution (elfnet_conv3x3_f16 with algo 1, elf_amd/csrc/net_conv3x3.hip)
can break and tests/test_gpu_net_conv_native.py does not reach: K-tile counts as short as the prologue's depth and odd ones
(Cin = 64, 192), two channel tiles, tiles with one valid row, tile counts that are and are not a multiple of the eight XCDs
workgroups are dealt over, and boards with h != w.  Every comparison is exact: bit for bit against algo 0 (same K order, same MFMA,
same epilogue sequence), against the integer nine-tap form, and launch against launch."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def _run(L, x, w, b, r, y, rows, h, wd, c, k, relu, algo):
    import torch
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return L.elfnet_conv3x3_f16(p(x), p(w), p(b), p(r), p(y), rows, h, wd, c, k, int(relu), algo,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _guarded(rows, h, wd, k):
    """y prefilled with NaN, and one guard row of NaN behind its last row"""
    import torch
    buf = torch.full((rows * h * wd + 1, k), float("nan"), device="cuda", dtype=torch.float16)
    return buf, buf[:rows * h * wd].view(rows, h, wd, k)


_rand = {}


def _rand_case(rows, h, wd, c, k):
    """test_gpu_net_conv_native._rand_case's recipe at any shape; drawn once per shape and left unchanged"""
    import torch
    key = (rows, h, wd, c, k)
    if key not in _rand:
        g = torch.Generator(device="cuda").manual_seed(4242 + rows + 31 * h + 977 * wd + c + 7 * k)
        x = torch.randn((rows, h, wd, c), device="cuda", generator=g).half()
        w = (torch.randn((k, 3, 3, c), device="cuda", generator=g) * (9 * c) ** -0.5).half()
        b = torch.randn((k,), device="cuda", generator=g).half()
        r = torch.randn((rows, h, wd, k), device="cuda", generator=g).half()
        _rand[key] = (x, w, b, r)
    return _rand[key]


_algo0 = {}


def _algo0_result(elf, rows, h, wd, c, k, use_res, relu):
    """algo 0's output, computed once per case"""
    import torch
    key = (rows, h, wd, c, k, use_res, relu)
    if key not in _algo0:
        x, w, b, r = _rand_case(rows, h, wd, c, k)
        y = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert _run(elf.lib(), x, w, b, r if use_res else None, y, rows, h, wd, c, k, relu, 0) == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(y).any())
        _algo0[key] = y
    return _algo0[key]


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
    x, w, b, r = _rand_case(rows, h, wd, c, k)
    want = _algo0_result(elf, rows, h, wd, c, k, use_res, relu)
    buf, y = _guarded(rows, h, wd, k)
    assert _run(elf.lib(), x, w, b, r if use_res else None, y, rows, h, wd, c, k, relu, 1) == 0
    torch.cuda.synchronize()
    print("%s res %d relu %d: %d of %d elements differ between algo 1 and algo 0"
          % ((rows, h, wd, c, k), use_res, relu, int((y != want).sum().item()), y.numel()))
    assert torch.equal(y, want)
    assert bool(torch.isnan(buf[-1]).all())


def _conv_fp32(x, w):
    """conv2d(x, w, padding=1) in fp32 for NHWC x [rows,h,w,C] and w [K,3,3,C] as its nine taps"""
    import torch
    rows, h, wd = x.shape[0], x.shape[1], x.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((rows, h, wd, w.shape[0]), device=x.device, dtype=torch.float32)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + wd, :] @ w[:, ky, kx, :].t()
    return out


_ints = {}


def _int_case(rows, h, wd, c, k):
    """test_gpu_net_conv_native._int_case's recipe with h and w apart: x in {-1,0,1}; w in {-1,0,1} with about 3/4 zeros, drawn
    per element so it is asymmetric in (k,c) and in (ky,kx); integer bias and res.  Every partial sum is an integer below 2048 in
    magnitude: exact in fp32 and in fp16."""
    import torch
    key = (rows, h, wd, c, k)
    if key not in _ints:
        g = torch.Generator(device="cuda").manual_seed(77 + rows + 1000 * h + 31 * wd + c + 7 * k)
        ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
        x = ri((rows, h, wd, c), -1, 1).half()
        w = (ri((k, 3, 3, c), -1, 1) * (ri((k, 3, 3, c), 0, 3) == 0)).half()
        b = ri((k,), -8, 8).half()
        r = ri((rows, h, wd, k), -8, 8).half()
        conv = _conv_fp32(x.float(), w.float())
        assert conv.abs().max().item() < 1024 and not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(2))
        _ints[key] = dict(x=x, w=w, b=b, r=r, conv=conv)
    return _ints[key]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("c", [64, 256])
@pytest.mark.parametrize("h,wd", [(5, 7), (7, 5)])
def test_non_square_boards_exact_integers(elf, h, wd, c, use_res, relu):
    """11 boards of 5 x 7 or 7 x 5 (M = 385: a full tile whose rows straddle boards, and a 129-row tail) against the nine-tap
    fp32 form; a kernel that took one of h, w for the other would put the halo in the wrong places"""
    import torch
    rows, k = 11, 256
    d = _int_case(rows, h, wd, c, k)
    ref = d["conv"] + d["b"].float()
    if use_res:
        ref = ref + d["r"].float()
    if relu:
        ref = torch.relu(ref)
    buf, y = _guarded(rows, h, wd, k)
    assert _run(elf.lib(), d["x"], d["w"], d["b"], d["r"] if use_res else None, y, rows, h, wd, c, k, relu, 1) == 0
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
    rows, h, wd, c, k = 48, 19, 19, 192, 256
    x, w, b, r = _rand_case(rows, h, wd, c, k)
    want = _algo0_result(elf, rows, h, wd, c, k, True, 1)
    first = None
    for i in range(20):
        y = torch.full((rows, h, wd, k), float("nan"), device="cuda", dtype=torch.float16)
        assert _run(elf.lib(), x, w, b, r, y, rows, h, wd, c, k, 1, 1) == 0
        torch.cuda.synchronize()
        if first is None:
            first = y
            assert torch.equal(y, want), "the first launch differs from algo 0"
        else:
            assert torch.equal(y, first), "launch %d differs from the first" % i
