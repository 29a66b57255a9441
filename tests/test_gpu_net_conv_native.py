"""GPU: the hand-written trunk convolution (elfnet_conv3x3_f16 with algo 1, elf_amd/csrc/net_conv3x3.hip) on inputs whose result
is exact -- small integers, so every partial sum is an integer fp32 and fp16 hold exactly and any differing element is a wrong
halo, layout, swizzle or pipeline timing, never rounding -- then bit for bit against algo 0 (same K order, same MFMA), a race
screen (repeated launches return the bits of the first), and the shapes it refuses."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

ALGO = 1


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


def _conv_fp32(x, w):
    """conv2d(x, w, padding=1) in fp32 for NHWC x [rows,h,w,C] and w [K,3,3,C] as its nine taps (test_gpu_net_conv._conv_fp32)"""
    import torch
    rows, h, wd = x.shape[0], x.shape[1], x.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((rows, h, wd, w.shape[0]), device=x.device, dtype=torch.float32)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + wd, :] @ w[:, ky, kx, :].t()
    return out


def _run(L, x, w, b, r, y, rows, n, relu, algo, c, k):
    import torch
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return L.elfnet_conv3x3_f16(p(x), p(w), p(b), p(r), p(y), rows, n, n, c, k, int(relu), algo,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))


_ints = {}


def _int_case(rows, n, c, k):
    """x in {-1,0,1}; w in {-1,0,1} with about 3/4 zeros, drawn per element so it is asymmetric in (k,c) and in (ky,kx); integer
    bias and res.  |partial sum| <= 9 c / 4 + spread, far below 2048, |result| below 2048: exact in fp32 and in fp16."""
    import torch
    key = (rows, n, c, k)
    if key not in _ints:
        g = torch.Generator(device="cuda").manual_seed(77 + rows + 1000 * n + c + 7 * k)
        ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, device="cuda", generator=g)
        x = ri((rows, n, n, c), -1, 1).half()
        w = (ri((k, 3, 3, c), -1, 1) * (ri((k, 3, 3, c), 0, 3) == 0)).half()
        b = ri((k,), -8, 8).half()
        r = ri((rows, n, n, k), -8, 8).half()
        conv = _conv_fp32(x.float(), w.float())
        assert conv.abs().max().item() < 1024 and not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(2))
        _ints[key] = dict(x=x, w=w, b=b, r=r, conv=conv)
    return _ints[key]


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
    d = _int_case(rows, n, c, k)
    ref = d["conv"] + d["b"].float()
    if use_res:
        ref = ref + d["r"].float()
    if relu:
        ref = torch.relu(ref)
    buf = torch.full((rows * n * n + 1, k), float("nan"), device="cuda", dtype=torch.float16)
    y = buf[:rows * n * n].view(rows, n, n, k)
    rc = _run(elf.lib(), d["x"], d["w"], d["b"], d["r"] if use_res else None, y, rows, n, relu, ALGO, c, k)
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
    assert _run(elf.lib(), x, w, b, None, y, rows, n, 0, ALGO, ch, ch) == 0
    torch.cuda.synchronize()
    i = torch.arange(n, device="cuda")
    on = 3 - ((i == 0) | (i == n - 1)).long()           # taps on the board along one axis
    want = (256 * on[:, None] * on[None, :]).float()    # [n, n]
    assert want[0, 0] == 1024 and want[0, 1] == 1536 and want[1, 1] == 2304
    assert bool((y.float() == want[None, :, :, None]).all())


_rand = {}


def _rand_case(rows):
    import torch
    if rows not in _rand:
        g = torch.Generator(device="cuda").manual_seed(4242 + rows)
        n, ch = 19, 256
        x = torch.randn((rows, n, n, ch), device="cuda", generator=g).half()
        w = (torch.randn((ch, 3, 3, ch), device="cuda", generator=g) * (9 * ch) ** -0.5).half()
        b = torch.randn((ch,), device="cuda", generator=g).half()
        r = torch.randn((rows, n, n, ch), device="cuda", generator=g).half()
        _rand[rows] = (x, w, b, r)
    return _rand[rows]


def test_bit_equal_with_algo_0(elf):
    """rows 48 x 19 x 19 with skip: the shipped kernel keeps algo 0's accumulation chain (tap-major K; in every 32-channel block
    one 32x32x16 MFMA over channels {0..7, 16..23}, the next over {8..15, 24..31}, as CK hands them out) and its epilogue
    sequence, so the two outputs are the same bits"""
    import torch
    rows = 48
    x, w, b, r = _rand_case(rows)
    ys = []
    for algo in (0, 1):
        y = torch.full((rows, 19, 19, 256), float("nan"), device="cuda", dtype=torch.float16)
        assert _run(elf.lib(), x, w, b, r, y, rows, 19, 1, algo, 256, 256) == 0
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
    x, w, b, r = _rand_case(rows)
    first = None
    for i in range(launches):
        y = torch.full((rows, 19, 19, 256), float("nan"), device="cuda", dtype=torch.float16)
        assert _run(elf.lib(), x, w, b, r, y, rows, 19, 1, ALGO, 256, 256) == 0
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
    assert _run(elf.lib(), x, w, b, None, y, rows, n, 0, ALGO, c, k) < 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
