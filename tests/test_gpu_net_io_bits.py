"""GPU: the output bits of the net's ends (elf_amd/csrc/net_io.hip: elfnet_conv3x3_in_f16 / _bf16, elfnet_heads_f16 / _bf16) against
sha256 digests recorded from the library before the fp16 and bf16 kernels became one templated set (tests/net_io_expected.py,
written by tools/net_io_digests.py).  The operands are drawn with numpy's RandomState on the CPU from seeds the shape fixes, so the
digests depend on nothing but the kernels' arithmetic: their rounding and their summation order.  Bits are compared, so there is no
tolerance."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import conv_cases as cc
from conv_cases import elf  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

# (rows, c, k) of 9 x 9 boards: both step counts (c = 18: 11 MFMA steps, c = 32: 18), one workgroup along k and two (k = 288: the
# second has one wave with channels), one partial tile and 519 tiles for at most 512 workgroups
CONV_SHAPES = [(rows, c, k) for rows in (1, 410) for c in (18, 32) for k in (64, 288)]
CONV_KINDS = ("f16", "bf16", "bf16_xf16")   # the entry; _xf16: the bf16 entry on fp16 rows (x_is_f16 = 1)
# (rows, ch): lane groups of 8 / 16 / 32 and, at 512 channels, further chunks from memory; one row, a partial workgroup, one row per
# workgroup, and eight rows per workgroup with a last workgroup of five
HEADS_SHAPES = [(rows, ch) for rows in (1, 5, 8, 2053) for ch in (64, 128, 256, 512)]
N, VH = 9, 256


def _draw(seed, shape, scale):
    """uniform multiples of scale / 32768 in [-scale, scale), fp32, from numpy on the CPU"""
    u = np.frombuffer(np.random.RandomState(seed).bytes(2 * int(np.prod(shape))), dtype="<u2").reshape(shape)
    return (u.astype(np.float32) - np.float32(32768.0)) * np.float32(scale / 32768.0)


def _dev(a, dtype):
    """rounded to dtype on the CPU (round to nearest even), then uploaded"""
    import torch
    return torch.from_numpy(a).to(dtype).cuda()


def _sha(*tensors):
    import torch
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def conv_digests(L, rows, c, k):
    """{"<kind>_relu<r>": sha256 of y's bytes} of one shape"""
    import torch
    seed = 7100 + rows + 100 * c + k
    x, w, b = _draw(seed, (rows, N, N, c), 2.0), _draw(seed + 1, (k, 3, 3, c), 0.5), _draw(seed + 2, (k,), 1.0)
    out = {}
    for kind in CONV_KINDS:
        t = torch.float16 if kind == "f16" else torch.bfloat16
        xd, wd, bd = _dev(x, torch.bfloat16 if kind == "bf16" else torch.float16), _dev(w, t), _dev(b, t)
        for relu in (0, 1):
            y = torch.full((rows, N, N, k), cc.NAN, device="cuda", dtype=t)
            if kind == "f16":
                rc = L.elfnet_conv3x3_in_f16(cc.ptr(xd), cc.ptr(wd), cc.ptr(bd), cc.ptr(y), rows, N, N, c, k, relu, cc.stream())
            else:
                rc = L.elfnet_conv3x3_in_bf16(cc.ptr(xd), int(kind == "bf16_xf16"), cc.ptr(wd), cc.ptr(bd), cc.ptr(y), rows, N, N, c, k,
                                              relu, cc.stream())
            assert rc == 0
            torch.cuda.synchronize()
            out["%s_relu%d" % (kind, relu)] = _sha(y)
    return out


def heads_digests(L, rows, ch):
    """{"<type>_pi" / "_v" / "_logits" / "_pi_nologits" / "_v_nologits": sha256} of one shape: with a logits buffer and without"""
    import torch
    d, seed = N * N, 9300 + rows + 10 * ch
    a = dict(act=_draw(seed, (rows, N, N, ch), 1.0), pconv_w=_draw(seed + 1, (2, ch), 4.0 / ch ** 0.5), pconv_b=_draw(seed + 2, (2,), 0.5),
             vconv_w=_draw(seed + 3, (1, ch), 4.0 / ch ** 0.5), vconv_b=_draw(seed + 4, (1,), 0.5), pi_w=_draw(seed + 5, (d + 1, 2 * d), 0.25),
             pi_b=_draw(seed + 6, (d + 1,), 0.5), v1_w=_draw(seed + 7, (VH, d), 0.25), v1_b=_draw(seed + 8, (VH,), 0.5),
             v2_w=_draw(seed + 9, (1, VH), 0.125), v2_b=_draw(seed + 10, (1,), 0.25))
    out = {}
    for name, t, entry in (("f16", torch.float16, L.elfnet_heads_f16), ("bf16", torch.bfloat16, L.elfnet_heads_bf16)):
        dev = {nm: _dev(v, t) for nm, v in a.items()}
        hd = cc.heads_struct(dev, ch, VH)
        nb = L.elfnet_heads_workspace(rows, N, N)
        ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)
        for want in (True, False):
            nan = lambda *shape: torch.full(shape, cc.NAN, device="cuda", dtype=torch.float32)
            pi, v, lg = nan(rows, d + 1), nan(rows), nan(rows, d + 1) if want else None
            assert entry(cc.ptr(dev["act"]), C.byref(hd), rows, N, N, cc.ptr(pi), d + 1, cc.ptr(v), cc.ptr(lg), cc.ptr(ws), nb,
                         cc.stream()) == 0
            torch.cuda.synchronize()
            assert not bool(torch.isnan(pi).any()) and not bool(torch.isnan(v).any())
            tag = "" if want else "_nologits"
            out[name + "_pi" + tag], out[name + "_v" + tag] = _sha(pi), _sha(v)
            if want:
                out[name + "_logits"] = _sha(lg)
    return out


def _differing(got, want):
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


@pytest.mark.parametrize("rows,c,k", CONV_SHAPES)
def test_input_conv_bits(elf, rows, c, k):
    import net_io_expected as E
    assert _differing(conv_digests(elf.lib(), rows, c, k), E.CONV[(rows, c, k)]) == []


@pytest.mark.parametrize("rows,ch", HEADS_SHAPES)
def test_heads_bits(elf, rows, ch):
    import net_io_expected as E
    assert _differing(heads_digests(elf.lib(), rows, ch), E.HEADS[(rows, ch)]) == []
