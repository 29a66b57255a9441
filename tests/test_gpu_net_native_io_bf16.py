"""GPU: the two ends of the native bf16 net (elf_amd/csrc/net_io.hip, the bf16 entries) and NativeBf16InferenceNet on top of them, against plain
high-precision references: exact operands where any differing bit is a layout, halo, tail or rounding-rule bug, random ones within
a derived bound, and a whole net against its own weights in fp64 with the bf16 FusedInferenceNet as the yardstick."""
import copy
import ctypes as C

import numpy as np
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)
from test_gpu_net_native_io import _feature_rows, _heads_exact_case   # the real feature rows and the exact heads case, shared

pytestmark = pytest.mark.gpu

# (rows, n, c, k).  The grid rule is (min(tiles, 512 / gy), gy) workgroups with gy = ceil(k / 256): at k = 32 that is 512, and
# 410 rows of 9 x 9 are 33 210 positions = 519 tiles of 64, so seven workgroups go round their tile loop a second time.
# k = 288 is two workgroups along k: the second has one wave with channels (256 .. 287) and seven that only stage.
SHAPES = [(3, 19, 18, 256), (5, 9, 18, 64), (2, 9, 2, 32), (3, 9, 32, 64), (2, 9, 18, 288), (410, 9, 18, 32)]


def _seed(rows, n, c, k):
    return 4200 + rows + 1000 * n + c + 7 * k


def _conv_in(L, x, w, b, relu):
    """one launch into a NaN-filled bf16 y with one guard row of NaN behind it, which stays NaN; x is fp16 or bf16"""
    import torch
    rows, h, wd, c = x.shape
    k = w.shape[0]
    buf = torch.full((rows * h * wd + 1, k), cc.NAN, device="cuda", dtype=torch.bfloat16)
    y = buf[:rows * h * wd].view(rows, h, wd, k)
    assert L.elfnet_conv3x3_in_bf16(cc.ptr(x), int(x.dtype == torch.float16), cc.ptr(w), cc.ptr(b), cc.ptr(y), rows, h, wd, c, k,
                                    int(relu), cc.stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[-1]).all()), "the guard row behind y was written"
    return y


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("x_is_f16", [0, 1])
@pytest.mark.parametrize("rows,n,c,k", SHAPES)
def test_input_conv_exact_integers_rounded_once(elf, rows, n, c, k, x_is_f16, relu):
    """Integer operands, the bias scaled by 64 (exact in bf16): fp32 is exact, |conv + b| passes 256 and many outputs are not bf16
    numbers.  The output is, bit for bit, that fp32 value, fmax(., 0), rounded once to nearest even."""
    import torch
    d = cc.int_case(_seed(rows, n, c, k), rows, n, n, c, k, res=False, limit=288)
    b = (d["b"].float() * 64).bfloat16()
    assert torch.equal(b.float(), d["b"].float() * 64)
    v = d["conv"] + b.float()
    inexact = float((v.bfloat16().float() != v).float().mean())
    print("%s: %.3f of conv + b are not bf16 numbers" % ((rows, n, c, k), inexact))
    assert inexact > 0.1
    if relu:
        v = torch.fmax(v, torch.zeros((), device="cuda"))
    y = _conv_in(elf.lib(), d["x"] if x_is_f16 else d["x"].bfloat16(), d["w"].bfloat16(), b, relu)
    bad = int((cc.bits(y) != cc.bits(v.bfloat16())).sum().item())
    print("f16 %d relu %d: %d of %d differ" % (x_is_f16, relu, bad, y.numel()))
    assert bad == 0


@pytest.mark.parametrize("rows,n,c,k", [(3, 19, 18, 256), (5, 9, 18, 64)])
def test_fp16_rows_give_the_bits_of_bf16_rows(elf, rows, n, c, k):
    """random fp16 x (most values are not bf16 numbers): converted inside the kernel as x.bfloat16() converts them"""
    import torch
    x, w, b, _ = cc.rand_case(_seed(rows, n, c, k), rows, n, n, c, k)
    assert float((x.bfloat16().half() != x).float().mean()) > 0.5
    w, b = w.bfloat16(), b.bfloat16()
    y16, ybf = _conv_in(elf.lib(), x, w, b, 1), _conv_in(elf.lib(), x.bfloat16(), w, b, 1)
    assert not bool(torch.isnan(ybf).any()) and torch.equal(cc.bits(y16), cc.bits(ybf))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("rows,n,c,k", [(3, 9, 32, 64), (3, 19, 18, 256)])
def test_input_conv_random_within_the_derived_bound(elf, rows, n, c, k, relu):
    """|y - v| <= 2^-8 |v| + (9 c + 1) 2^-23 S against the fp64 value v of the bf16 operands, S = conv(|x|, |w|) + |b|: half a bf16
    ulp is at most 2^-8 relative, and an fp32 sum of 9 c + 1 terms in any order errs by at most (9 c + 1) 2^-24 S to first order,
    doubled here (the bf16 trunk test's bound without the skip's term)."""
    import torch
    x, w, b = (t.bfloat16() for t in cc.rand_case(_seed(rows, n, c, k), rows, n, n, c, k)[:3])
    xd, wd_, bd = x.double(), w.double(), b.double()
    v, s = cc.conv_fp32(xd, wd_) + bd, cc.conv_fp32(xd.abs(), wd_.abs()) + bd.abs()
    if relu:
        v = v.clamp(min=0)
    y = _conv_in(elf.lib(), x, w, b, relu)
    assert not bool(torch.isnan(y).any())
    err, bound = (y.double() - v).abs(), 2.0 ** -8 * v.abs() + (9 * c + 1) * 2.0 ** -23 * s
    print("%s relu %d: max err / bound %.3f" % ((rows, n, c, k), relu, float((err / bound).max())))
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ heads

def _upload_bf16(a):
    """name -> bf16 device tensor of every array in `a`, each value exactly representable"""
    import torch
    out = {}
    for nm, v in a.items():
        t = torch.from_numpy(v).bfloat16()
        assert np.array_equal(t.double().numpy(), v), nm
        out[nm] = t.cuda()
    return out


def _run_heads(L, t, ch, vh, rows, n, stride, want_logits=True):
    """-> (pi buffer [rows, stride], value buffer [rows + 1], logits buffer or None); all prefilled with NaN"""
    import torch
    nan = lambda *shape: torch.full(shape, cc.NAN, device="cuda", dtype=torch.float32)
    pi, value, logits = nan(rows, stride), nan(rows + 1), nan(rows, stride) if want_logits else None
    nb = L.elfnet_heads_workspace(rows, n, n)
    ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)
    hd = cc.heads_struct(t, ch, vh)
    assert L.elfnet_heads_bf16(cc.ptr(t["act"]), C.byref(hd), rows, n, n, cc.ptr(pi), stride, cc.ptr(value), cc.ptr(logits), cc.ptr(ws),
                               nb, cc.stream()) == 0
    torch.cuda.synchronize()
    return pi.cpu().numpy(), value.cpu().numpy(), logits.cpu().numpy() if want_logits else None


@pytest.mark.parametrize("rows,n,ch,pad,want_logits", [(1, 19, 256, 0, True),
                                                        (3, 19, 256, 6, True),     # pi_stride = d + 1 + 6
                                                        (5, 9, 64, 0, False),      # logits = NULL
                                                        (17, 9, 64, 0, True),      # more rows than one workgroup's share
                                                        (2053, 9, 8, 0, True),     # the smallest C; eight rows per workgroup, the last partial
                                                        (2, 9, 512, 0, True)])     # more 16-B chunks per position than lanes in a group
def test_heads_exact(elf, rows, n, ch, pad, want_logits):
    """test_gpu_net_native_io.py's exact case, uploaded as bf16, and its bounds, which rest on the fp32 arithmetic alone: logits
    bit-equal to fp64, pi within relative 1e-4, |sum pi - 1| <= 1e-5, V within 2^-20; the padding of a strided row and the
    element behind value stay NaN."""
    cs = _heads_exact_case(rows, n, ch)
    d = n * n
    pi, value, lg = _run_heads(elf.lib(), _upload_bf16(cs["a"]), ch, cs["vh"], rows, n, d + 1 + pad, want_logits)
    if want_logits:
        bad = int((lg[:, :d + 1] != cs["logits"].astype(np.float32)).sum())
        print("logits: %d of %d differ" % (bad, rows * (d + 1)))
        assert bad == 0 and np.isnan(lg[:, d + 1:]).all()
    p64 = pi[:, :d + 1].astype(np.float64)
    rel, verr = np.abs(p64 - cs["pi"]) / cs["pi"], np.abs(value[:rows].astype(np.float64) - cs["v"])
    print("pi: max relative error %.3g, max |sum - 1| %.3g; V: max error %.3g" % (rel.max(), np.abs(p64.sum(axis=1) - 1).max(), verr.max()))
    assert not np.isnan(p64).any() and not np.isnan(value[:rows]).any()
    assert rel.max() <= 1e-4 and np.abs(p64.sum(axis=1) - 1).max() <= 1e-5 and verr.max() <= 2.0 ** -20
    assert np.isnan(pi[:, d + 1:]).all() and np.isnan(value[rows])


def test_heads_policy_flattening_is_channel_major(elf):
    """only p[1][pos0] of one row is non-zero (= 1): that row's logits are exactly column d + pos0 of pi_w (pi_b = 0), the other
    row's are 0.  A pos * 2 + c flattening would pick column 2 pos0 + 1."""
    n, ch, row0, pos0 = 9, 64, 1, 23
    rng = np.random.RandomState(n + pos0)
    rows, d, vh = 2, n * n, 8
    a = dict(act=np.zeros((rows, n, n, ch)), pconv_w=np.zeros((2, ch)), pconv_b=np.zeros(2), vconv_w=np.zeros((1, ch)),
             vconv_b=np.zeros(1), pi_w=rng.randint(-64, 65, size=(d + 1, 2 * d)) / 8.0, pi_b=np.zeros(d + 1), v1_w=np.zeros((vh, d)),
             v1_b=np.zeros(vh), v2_w=np.zeros((1, vh)), v2_b=np.zeros(1))
    a["act"].reshape(rows, d, ch)[row0, pos0, 5] = 1.0
    a["pconv_w"][1, 5] = 1.0
    assert not np.array_equal(a["pi_w"][:, d + pos0], a["pi_w"][:, 2 * pos0 + 1])
    pi, value, lg = _run_heads(elf.lib(), _upload_bf16(a), ch, vh, rows, n, d + 1)
    assert np.array_equal(lg[row0], a["pi_w"][:, d + pos0].astype(np.float32))
    assert np.array_equal(lg[1 - row0], np.zeros(d + 1, np.float32))
    assert np.array_equal(value[:rows], np.zeros(rows, np.float32))


# ------------------------------------------------------------------------------------------------ NativeBf16InferenceNet

@pytest.mark.parametrize("n,blocks,dim,rows", [(9, 2, 64, 8), (19, 1, 256, 3)])
def test_native_bf16_net(elf, monkeypatch, n, blocks, dim, rows):
    """On real fp16 feature rows, with F.conv2d, F.linear, torch.softmax and torch.tanh made to raise: pi fp32 [rows, d + 1] and V
    fp32 [rows] whose RMS errors against the same weights in fp64 are at most 2 x the bf16 FusedInferenceNet's (fewer roundings
    must not be less accurate).  On the 9 x 9 net a GraphedNet replay and chunked_forward in slices of 3 return the call's bits."""
    import torch
    from elf_amd.net import FusedInferenceNet, GraphedNet, NativeBf16InferenceNet, chunked_forward, make_net
    net = make_net(board_size=n, num_block=blocks, dim=dim, dtype=torch.bfloat16, fold_bn=True)
    s = _feature_rows(elf, n, rows)
    ref = copy.deepcopy(net).cpu().double().to(memory_format=torch.contiguous_format)
    with torch.no_grad():
        truth = ref({"s": s.cpu().double().contiguous()})
    fused = FusedInferenceNet(net)({"s": s})
    native_net = NativeBf16InferenceNet(net)

    def refuse(name):
        def f(*a, **k):
            raise AssertionError("NativeBf16InferenceNet called " + name)
        return f
    with monkeypatch.context() as m:
        m.setattr(torch.nn.functional, "conv2d", refuse("F.conv2d"))
        m.setattr(torch.nn.functional, "linear", refuse("F.linear"))
        m.setattr(torch, "softmax", refuse("torch.softmax"))
        m.setattr(torch, "tanh", refuse("torch.tanh"))
        native = native_net({"s": s})
        torch.cuda.synchronize()
    assert native["pi"].dtype == torch.float32 and tuple(native["pi"].shape) == (rows, n * n + 1)
    assert native["V"].dtype == torch.float32 and tuple(native["V"].shape) == (rows,)
    rms = lambda o, key: float((o[key].double().cpu() - truth[key].double()).pow(2).mean().sqrt())
    for key in ("pi", "V"):
        print("%s: rms error native %.3e, fused %.3e" % (key, rms(native, key), rms(fused, key)))
        assert rms(native, key) <= 2 * rms(fused, key)
    if n == 9:
        out = GraphedNet(native_net, s.clone(memory_format=torch.preserve_format))()
        ch = chunked_forward(native_net, s, 3)
        torch.cuda.synchronize()
        assert torch.equal(out["pi"], native["pi"]) and torch.equal(out["V"], native["V"])
        assert torch.equal(ch["pi"], native["pi"]) and torch.equal(ch["V"], native["V"])


def test_native_bf16_net_refuses_what_it_cannot_take_completely(elf):
    import torch
    from elf_amd.net import NativeBf16InferenceNet, make_net
    for kw in (dict(dim=64, fold_bn=True), dict(dim=64, dtype=torch.bfloat16, fold_bn=False), dict(dim=32, dtype=torch.bfloat16, fold_bn=True)):
        with pytest.raises(ValueError):
            NativeBf16InferenceNet(make_net(board_size=9, num_block=1, **kw))
