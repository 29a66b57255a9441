"""CPU: tests/conv_cases.py, the instrument of the tests/test_gpu_net*.py files, proven without a GPU: its references against
torch's own and against hand-written values, its buffers' addresses and guards, the integer case's own caps, and launch's argument
lists against a stub library.  Toy shapes only.  Nothing here compares CPU-drawn operands with CUDA-drawn ones: the generators
differ."""
import pytest
import torch

import conv_cases as cc

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ numerics

@pytest.mark.parametrize("rows,h,wd,c,k", [(2, 5, 7, 3, 4), (2, 7, 5, 3, 4), (3, 1, 5, 2, 3), (1, 4, 4, 5, 2)])
def test_conv_fp32_is_conv2d_on_integers(rows, h, wd, c, k):
    """small integers: every product and partial sum is exact in fp32, so the nine-tap form and F.conv2d agree to the bit"""
    g = torch.Generator().manual_seed(rows + 10 * h + 100 * wd)
    x = torch.randint(-3, 4, (rows, h, wd, c), generator=g).float()
    w = torch.randint(-3, 4, (k, 3, 3, c), generator=g).float()
    assert not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(2))
    want = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    got = cc.conv_fp32(x, w)
    assert got.dtype == torch.float32 and tuple(got.shape) == (rows, h, wd, k)
    assert torch.equal(got, want.contiguous())
    assert cc.conv_fp32(x.double(), w.double()).dtype == torch.float64       # the fp64 truths of the native net's ends


def test_epilogue_fp32_on_hand_written_values():
    """conv rounded to fp16 first (2049 is a tie: to the even 2048), then + bias (+ res) in fp32, fmax, one more rounding"""
    conv = torch.tensor([2049.0, 1.0, -3.0, NAN, -0.0, -0.0])
    b = torch.tensor([1.0, 0.5, 1.0, 1.0, -0.0, 0.0]).half()
    r = torch.tensor([0.0, -2.0, 1.0, 1.0, -0.0, -0.0]).half()
    bits = lambda t: t.view(torch.int16).tolist()
    no_res = cc.epilogue_fp32(conv, b, None, 0)
    assert no_res.dtype == torch.float16
    assert no_res[:3].tolist() == [2048.0, 1.5, -2.0] and bool(torch.isnan(no_res[3]))       # 2048 + 1 = 2049 rounds to 2048 again
    assert bits(no_res[4:]) == [-32768, 0]                                                   # -0 + -0 = -0, -0 + +0 = +0
    with_res = cc.epilogue_fp32(conv, b, r, 0)
    assert with_res[:3].tolist() == [2048.0, -0.5, -1.0] and bool(torch.isnan(with_res[3]))
    assert bits(with_res[4:]) == [-32768, 0]
    relu = cc.epilogue_fp32(conv, b, r, 1)
    assert relu[:4].tolist() == [2048.0, 0.0, 0.0, 0.0]                                      # fmax: ReLU of a NaN is 0
    assert bits(relu[3:4]) == [0]                                                            # and that zero is +0
    assert bool((relu[4:] == 0).all())                                                       # fmax(-0, +0): a zero of either sign
    assert cc.epilogue_fp32(conv, b, None, 1)[:4].tolist() == [2048.0, 1.5, 0.0, 0.0]


def test_differing_counts_values_not_bits():
    y = torch.tensor([NAN, -0.0, 1.0, INF, NAN, 2.0]).half()
    assert cc.differing(y, torch.tensor([NAN, 0.0, 1.0, INF, NAN, 2.0]).half()) == 0        # NaN against NaN, -0 against +0
    assert cc.differing(y, torch.tensor([5.0, 0.0, 1.0, INF, NAN, 2.0]).half()) == 1         # NaN against a number
    assert cc.differing(y, torch.tensor([NAN, 0.0, 1.0, -INF, NAN, 2.5]).half()) == 2
    assert cc.differing(torch.tensor([1.0]), torch.tensor([NAN])) == 1


def test_bits_and_ptr():
    t = torch.tensor([0.0, -0.0, 1.0]).half()
    assert cc.bits(t).tolist() == [0, -32768, 0x3C00]
    assert cc.ptr(None) is None and cc.ptr(t).value == t.data_ptr()
    assert cc.ALONE == 1 << 30 and cc.RES_RELU == [(False, 0), (False, 1), (True, 0), (True, 1)]


# ------------------------------------------------------------------------------------------------ buffers

@pytest.mark.parametrize("dtype,mod,rem", [(torch.float16, 32, 16), (torch.float16, 16, 4), (torch.float16, 8, 4), (torch.float16, 4, 2),
                                           (torch.float32, 32, 16), (torch.float64, 16, 8)])
def test_carve(dtype, mod, rem):
    """the pairs the GPU files use on fp16, and two other floating-point element types"""
    src = torch.arange(35, dtype=torch.float32).reshape(5, 7).to(dtype)
    guard = 19
    v, front, back = cc.carve(src, guard, mod, rem)
    assert v.data_ptr() % mod == rem
    assert v.dtype == dtype and torch.equal(v, src) and v.data_ptr() != src.data_ptr()
    assert front.numel() >= guard and back.numel() >= guard
    assert bool(torch.isnan(front).all()) and bool(torch.isnan(back).all())
    assert front.data_ptr() + front.numel() * src.element_size() == v.data_ptr()
    assert v.data_ptr() + v.numel() * src.element_size() == back.data_ptr()


def test_carve_defaults_to_16_modulo_32():
    v, _, _ = cc.carve(torch.zeros(10, dtype=torch.float16), 8)
    assert v.data_ptr() % 32 == 16


def test_guarded():
    rows, h, wd, k = 3, 2, 5, 8
    buf, y = cc.guarded(rows, h, wd, k, device="cpu")
    assert buf.dtype == torch.float16 and tuple(buf.shape) == (rows * h * wd + 1, k) and tuple(y.shape) == (rows, h, wd, k)
    assert bool(torch.isnan(buf).all())
    assert y.data_ptr() == buf.data_ptr() and buf[-1].data_ptr() == y.data_ptr() + y.numel() * 2     # the guard row is behind the last row
    y.zero_()
    assert bool((buf[:-1] == 0).all()) and bool(torch.isnan(buf[-1]).all())


# ------------------------------------------------------------------------------------------------ operands

def test_int_case_stays_inside_its_caps():
    """the shape of the non-square GPU cases: the reference passes int_case's own magnitude and asymmetry checks where that can be
    checked, and is what the docstring says"""
    rows, h, wd, c, k = 11, 5, 7, 64, 256
    d = cc.int_case(5, rows, h, wd, c, k, device="cpu")
    assert sorted(d) == ["b", "conv", "r", "w", "x"]
    assert tuple(d["x"].shape) == (rows, h, wd, c) and tuple(d["w"].shape) == (k, 3, 3, c) and tuple(d["r"].shape) == (rows, h, wd, k)
    assert all(d[n].dtype == torch.float16 for n in "xwbr") and d["conv"].dtype == torch.float32
    assert set(d["x"].unique().tolist()) == {-1.0, 0.0, 1.0} and set(d["w"].unique().tolist()) == {-1.0, 0.0, 1.0}
    assert 0.70 < float((d["w"] == 0).float().mean()) < 0.86          # 1/3 + 2/3 * 3/4 = 5/6 zeros
    assert float(d["b"].abs().max()) <= 8 and float(d["r"].abs().max()) <= 8
    assert float(d["conv"].abs().max()) < 1024 and torch.equal(d["conv"], d["conv"].round())
    assert cc.int_case(5, rows, h, wd, c, k, device="cpu") is d       # cached by (seed, shape)
    assert not torch.equal(cc.int_case(6, rows, h, wd, c, k, device="cpu")["x"], d["x"])


def test_int_case_keywords():
    d = cc.int_case(7, 2, 3, 5, 18, 32, res=False, limit=288, not_degenerate=True, device="cpu")
    assert "r" not in d and float(d["conv"].abs().max()) <= 288
    with pytest.raises(AssertionError):
        cc.int_case(7, 2, 3, 5, 18, 32, res=False, limit=3, device="cpu")      # the cap is checked, not assumed


def test_rand_case_draws_x_w_b_r_in_that_order():
    seed, rows, h, wd, c, k = 9, 2, 3, 4, 8, 16
    x, w, b, r = cc.rand_case(seed, rows, h, wd, c, k, device="cpu")
    g = torch.Generator().manual_seed(seed)
    assert torch.equal(x, torch.randn((rows, h, wd, c), generator=g).half())
    assert torch.equal(w, (torch.randn((k, 3, 3, c), generator=g) * (9 * c) ** -0.5).half())
    assert torch.equal(b, torch.randn((k,), generator=g).half())
    assert torch.equal(r, torch.randn((rows, h, wd, k), generator=g).half())
    assert cc.rand_case(seed, rows, h, wd, c, k, device="cpu")[0] is x


# ------------------------------------------------------------------------------------------------ launches

class _Stub:
    """records (entry name, arguments) of every call and returns 7"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*a):
            self.calls.append((name, a))
            return 7
        return entry


def test_launch_reaches_the_entry_it_names(monkeypatch):
    monkeypatch.setattr(cc, "stream", lambda: "stream")
    rows, h, wd, c, k = 2, 3, 4, 8, 16
    x, w, b, r = cc.rand_case(1, rows, h, wd, c, k, device="cpu")
    _, y = cc.guarded(rows, h, wd, k, device="cpu")
    L = _Stub()
    for how, kw in (("algo0", {}), ("plain", {}), ("linear", dict(width=5)), ("board", dict(width=3)), ("small", {}),
                    ("linear", dict(width=4, algo=2)), ("algo0", dict(shape=(9, 1, 2, 24, 32)))):
        assert cc.launch(L, how, x, w, b, None if how == "small" else r, y, 1, **kw) == 7
    v = lambda a: [p.value if p is not None else None for p in a[:5]] + list(a[5:])
    ops = [x.data_ptr(), w.data_ptr(), b.data_ptr(), r.data_ptr(), y.data_ptr()]
    dims = [rows, h, wd, c, k, 1]
    assert [(n, v(a)) for n, a in L.calls] == [
        ("elfnet_conv3x3_f16", ops + dims + [0, "stream"]),                     # 'algo0' passes 0
        ("elfnet_conv3x3_f16", ops + dims + [1, "stream"]),
        ("elfnet_conv3x3_f16_width", ops + dims + [1, 5, "stream"]),            # 'linear' passes algo = 1, width
        ("elfnet_conv3x3_f16_boards", ops + dims + [3, "stream"]),              # 'board' passes no algo
        ("elfnet_conv3x3_small_f16", ops[:3] + [None] + ops[4:] + dims + ["stream"]),
        ("elfnet_conv3x3_f16_width", ops + dims + [2, 4, "stream"]),
        ("elfnet_conv3x3_f16", ops + [9, 1, 2, 24, 32, 1] + [0, "stream"])]
    with pytest.raises(ValueError):
        cc.launch(L, "nonesuch", x, w, b, r, y, 0)
    L.calls.clear()
    assert cc.conv_in(L, x, w, b, y, rows, h, wd, c, k, 0) == 7
    name, a = L.calls[0]
    assert name == "elfnet_conv3x3_in_f16" and [p.value for p in a[:4]] == ops[:3] + [y.data_ptr()]
    assert list(a[4:]) == [rows, h, wd, c, k, 0, "stream"]
