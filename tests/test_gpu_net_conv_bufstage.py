"""GPU: the buffer-addressed staging of the hand-written trunk convolution (algo 1, elf_amd/csrc/net_conv3x3.hip).  The kernel reads
x and w through raw buffer descriptors: a row's 32-bit offset in a vector register, the K tile's offset (tap, 64 channels) in a
scalar, x's descriptor moved back so that no scalar offset is negative, and zeros -- a row at or beyond its item's limit, an
off-board tap in linear order -- from a sentinel offset that the descriptor's range check refuses.

A. The hardware fact all of that rests on: an out-of-range lane of buffer_load_dwordx4 ... lds writes zeros to its 16 bytes of LDS
   (it does not leave them as they were), also for a destination above 64 KiB.
B. Operands cut out of the middle of larger NaN-filled allocations, y out of a NaN-prefilled one: a read outside a tensor is a NaN
   in the output and cannot fault, a write outside y is a missing NaN.  Linear order: 1 row of 2 x 2, 3 x 3 and 9 x 9 (the first
   position's off-board taps, the negative deltas at offset 0), 5 rows of 9 x 9 and 91 of 19 x 19 (a partial last tile).  Board
   order: 256, 257 and 513 rows of 5 x 7 and 9 x 9 (a last block with rows beyond the limit).
C. All-ones operands against the count of taps on the board, both orders, 5 x 37 and 1 x 5: a stale LDS slot where a zero
   belongs changes the count.
D. Chains of at least five items on one workgroup, C = 64 and 192, K = 256 and 512, widths 1, 2, 3, both orders: the next item's
   rows take over in mid-stream and the channel column changes.
E. The largest shape the entry accepts, 11 618 rows of 19 x 19 x 256: vector offsets up to just below 2^31, in linear order
   (a named round width), in board order and through the plain entry.
F. Twenty launches of the headline shape, the same bytes.

Every comparison is exact, against algo 0."""
import ctypes as C

import pytest

import conv_cases as cc
from conv_cases import ALONE, RES_RELU, elf  # noqa: F401  (elf: the fixture)

pytestmark = pytest.mark.gpu

PAD = 16384          # elements of NaN on either side of a cut-out tensor: more than any bias, a multiple of 8 (16-byte alignment)


def _seed(rows, h, wd, c, k):
    return 4099 + rows + 31 * h + 977 * wd + c + 7 * k


def _cut(t):
    """a copy of t in the middle of a NaN-filled allocation; (allocation, view).  Not cc.carve: that one moves the view to an
    address that is 16 modulo 32 and allocates `mod` elements more, and here the view starts exactly PAD elements in, at the
    allocation's own alignment, with exactly PAD behind it."""
    import torch
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device="cuda", dtype=torch.float16)
    v = buf[PAD:PAD + t.numel()].view(t.shape)
    v.copy_(t)
    return buf, v


def _cut_run(elf, x, w, b, r, relu, how, width=0, guard=True):
    """one launch (cc.launch's `how`) into a NaN-prefilled y cut out of a NaN-filled allocation, PAD elements on either side (none
    with guard=False, for the shapes that fill the memory): cc.run_guarded's one guard row behind y is not this"""
    import torch
    rows, h, wd, c = x.shape
    k = w.shape[0]
    n = rows * h * wd * k
    pad = PAD if guard else 0
    buf = torch.full((n + 2 * pad,), float("nan"), device="cuda", dtype=torch.float16)
    y = buf[pad:pad + n].view(rows, h, wd, k)
    rc = cc.launch(elf.lib(), how, x, w, b, r, y, relu, width)
    assert rc == 0
    torch.cuda.synchronize()
    if guard:
        assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + n:]).all()), "written outside y"
    return y


_cases = {}


def _case(elf, rows, h, wd, c, k):
    """random operands of one shape, cut out of NaN, and algo 0's outputs on plain copies of them: made once, not changed.  (Not
    cc.algo0_ref: the reference launch keeps its guard regions on both sides of y.)"""
    import torch
    key = (rows, h, wd, c, k)
    if key not in _cases:
        x, w, b, r = cc.rand_case(_seed(*key), *key)
        t = {"keep": [], "ref": {}}
        for name, v in (("x", x), ("w", w), ("r", r)):
            buf, cut = _cut(v)
            t["keep"].append(buf)
            t[name] = cut
        t["b"] = b
        for use_res, relu in RES_RELU:
            y0 = _cut_run(elf, x, w, b, r if use_res else None, relu, "algo0")
            assert not bool(torch.isnan(y0).any())
            t["ref"][(use_res, relu)] = y0
        _cases[key] = t
    return _cases[key]


# ------------------------------------------------------------------------------------------------ A. the range check's zeros

@pytest.mark.parametrize("lds_offset", [0, 63 * 1024, 97 * 1024, 159 * 1024])
def test_an_out_of_range_lane_writes_zeros_to_lds(elf, lds_offset):
    """One wave, LDS prefilled with 0xFF by ds_write, every second lane at the sentinel offset, a scalar offset that is not zero.
    Lanes in range hold the source bytes, lanes out of range zeros.  Two more lanes pin what the design documents as this chip's
    answer on the scalar offset: it takes part in the range check (a lane whose vector offset is in range and whose sum with the
    scalar offset is not reads zeros; a lane whose sum ends exactly at num_records reads its bytes).  The kernel itself is in range
    under either reading (tests/test_net_conv_bufstage_plan.py)."""
    import torch
    L = elf.lib()
    sen = C.c_uint32()
    assert L.elfnet_conv3x3_f16_bufstage(1, 19, 19, 64, 256, -1, 0, None, None, None, C.byref(sen), None, None) == 0
    records, soff = 4096, 208
    g = torch.Generator(device="cuda").manual_seed(77)
    src = torch.randint(1, 256, (8192,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)   # no zero byte, no 0xFF run
    src[src == 255] = 254
    voff = [(sen.value if l & 1 else 16 * l + 32) for l in range(64)]
    voff[60] = records - 64            # in range by itself, out of range with the scalar offset added
    voff[62] = records - 16 - soff     # the last 16 bytes in range under either reading
    vo = torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in voff], dtype=torch.int32, device="cuda")   # the same 32 bits
    out = torch.full((1024,), 0x55, dtype=torch.uint8, device="cuda")
    assert L.elfnet_conv3x3_f16_bufstage_probe(cc.ptr(src), records, cc.ptr(vo), soff, lds_offset, cc.ptr(out), cc.stream()) == 0
    torch.cuda.synchronize()
    out = out.cpu().view(64, 16)
    srcc = src.cpu()
    for l in range(64):
        if l == 60:
            continue
        if l & 1:
            assert bool((out[l] == 0).all()), "lane %d (sentinel) holds %s, not zeros" % (l, out[l].tolist())
        else:
            at = voff[l] + soff
            assert torch.equal(out[l], srcc[at:at + 16]), "lane %d (in range) does not hold its source bytes" % l
    at = voff[60] + soff
    print("lds_offset %d: a lane whose vector offset is in range and whose sum with the scalar offset is not reads %s"
          % (lds_offset, "zeros (the scalar offset counts)" if bool((out[60] == 0).all()) else
             "memory (the scalar offset does not count)" if torch.equal(out[60], srcc[at:at + 16]) else out[60].tolist()))
    assert bool((out[60] == 0).all()), "lane 60: in range by its vector offset alone, out of range with the scalar offset: %s" % out[60].tolist()


# ------------------------------------------------------------------------------------------------ B. operands cut out of NaN

LINEAR = [(1, 2, 2, 64, 256), (1, 3, 3, 64, 256), (1, 9, 9, 128, 256), (5, 9, 9, 64, 256), (91, 19, 19, 64, 256)]
BOARD = [(256, 5, 7, 64, 256), (257, 5, 7, 64, 256), (513, 5, 7, 128, 256), (256, 9, 9, 64, 256), (257, 9, 9, 64, 512),
         (513, 9, 9, 64, 256)]


@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("width", [1, ALONE])
@pytest.mark.parametrize("shape", LINEAR)
def test_linear_order_reads_nothing_outside_its_tensors(elf, shape, width, use_res, relu):
    import torch
    t = _case(elf, *shape)
    y = _cut_run(elf, t["x"], t["w"], t["b"], t["r"] if use_res else None, relu, "linear", width)
    y0 = t["ref"][(use_res, relu)]
    print("%s width %d: %d NaN, %d of %d differ from algo 0" % (shape, width, int(torch.isnan(y).sum().item()),
                                                               int((cc.bits(y) != cc.bits(y0)).sum().item()), y.numel()))
    assert torch.equal(cc.bits(y), cc.bits(y0))


@pytest.mark.parametrize("use_res,relu", RES_RELU)
@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("shape", BOARD)
def test_board_order_reads_nothing_outside_its_tensors(elf, shape, width, use_res, relu):
    import torch
    t = _case(elf, *shape)
    y = _cut_run(elf, t["x"], t["w"], t["b"], t["r"] if use_res else None, relu, "board", width)
    y0 = t["ref"][(use_res, relu)]
    print("%s width %d: %d NaN, %d of %d differ from algo 0" % (shape, width, int(torch.isnan(y).sum().item()),
                                                               int((cc.bits(y) != cc.bits(y0)).sum().item()), y.numel()))
    assert torch.equal(cc.bits(y), cc.bits(y0))


# ------------------------------------------------------------------------------------------------ C. exact integers

@pytest.mark.parametrize("how,width", [("linear", 1), ("linear", ALONE), ("board", 1), ("board", 3)])
@pytest.mark.parametrize("rows,h,wd,c", [(257, 5, 37, 64), (300, 1, 5, 128)])
def test_all_ones_give_the_count_of_taps_on_the_board(elf, rows, h, wd, c, how, width):
    """x = 1, w = 1 / C: every output is the number of its position's taps that are on the board, 2 to 9"""
    import torch
    k = 256
    x = torch.ones((rows, h, wd, c), device="cuda", dtype=torch.float16)
    w = torch.full((k, 3, 3, c), 1.0 / c, device="cuda", dtype=torch.float16)
    b = torch.zeros((k,), device="cuda", dtype=torch.float16)
    want = torch.zeros((h, wd), dtype=torch.float32)
    for hh in range(h):
        for ww in range(wd):
            want[hh, ww] = sum(1 for ky in range(3) for kx in range(3) if 0 <= hh + ky - 1 < h and 0 <= ww + kx - 1 < wd)
    want = want.cuda()[None, :, :, None].expand(rows, h, wd, k)
    y = _cut_run(elf, x, w, b, None, 0, how, width)
    bad = int((y.float() != want).sum().item())
    print("%s c %d %s width %d: %d of %d differ from the tap counts" % ((rows, h, wd), c, how, width, bad, y.numel()))
    assert bad == 0
    assert torch.equal(cc.bits(y), cc.bits(_cut_run(elf, x, w, b, None, 0, "algo0")))


# ------------------------------------------------------------------------------------------------ D. chains

@pytest.mark.parametrize("use_res,relu", [(False, 0), (True, 1)])
@pytest.mark.parametrize("how", ["linear", "board"])
@pytest.mark.parametrize("width", [1, 2, 3])
@pytest.mark.parametrize("c,k", [(64, 256), (64, 512), (192, 256), (192, 512)])
def test_a_chain_of_items_on_one_workgroup(elf, c, k, width, how, use_res, relu):
    import torch
    L = elf.lib()
    rows, h, wd = 257, 5, 7           # 36 tiles in linear order, 70 items per channel column in board order
    if how == "board":
        assert L.elfnet_conv3x3_f16_boards_deal(rows, h, wd, k, width, 0, 4) >= 0, "fewer than five items on workgroup 0"
    else:
        tiles = (rows * h * wd + 255) // 256
        assert L.elfnet_conv3x3_f16_plan(tiles, k // 256, width, 0, None, None, None) >= 5 * L.elfnet_conv3x3_f16_grid(tiles, k // 256, width)
    t = _case(elf, rows, h, wd, c, k)
    y = _cut_run(elf, t["x"], t["w"], t["b"], t["r"] if use_res else None, relu, how, width)
    assert torch.equal(cc.bits(y), cc.bits(t["ref"][(use_res, relu)]))


# ------------------------------------------------------------------------------------------------ E. offsets up to 2^31

def test_the_largest_shape_the_entry_accepts(elf):
    """11 618 rows of 19 x 19 x 256, just below 2^30 elements: the last rows' vector offsets are just below 2^31 and have to be
    taken as unsigned numbers.  About 6.5 GB: x, algo 0's y and one y of algo 1 at a time.  Linear order is forced by naming the
    round width (the device's CU count: elfnet_conv3x3_f16_width leaves the choice to the shape's rule at width 0, and the rule
    takes board order here); its last tile selects between offsets near 2^31 and the sentinel by the rows' masks."""
    import torch
    rows, h, wd, c, k = 11618, 19, 19, 256, 256
    assert rows * h * wd * c < 1 << 30 <= (rows + 1) * h * wd * c
    g = torch.Generator(device="cuda").manual_seed(11618)
    x = torch.empty((rows, h, wd, c), device="cuda", dtype=torch.float16).normal_(generator=g)
    w = (torch.randn((k, 3, 3, c), device="cuda", generator=g) * (9 * c) ** -0.5).half()
    b = torch.randn((k,), device="cuda", generator=g).half()
    y0 = _cut_run(elf, x, w, b, None, 1, "algo0", guard=False)
    assert not bool(torch.isnan(y0[-1]).any()) and bool((y0[-1] != 0).any())
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus > 0
    for how, width in (("linear", cus), ("linear", ALONE), ("board", 0), ("plain", 0)):
        y = _cut_run(elf, x, w, b, None, 1, how, width, guard=False)
        same = torch.equal(cc.bits(y), cc.bits(y0))
        print("%s width %d: equal to algo 0: %s" % (how, width, same))
        assert same, (how, width)
        del y
    del x, y0
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ F. launch against launch

def test_twenty_launches_of_the_headline_shape(elf):
    import torch
    rows, h, wd, c, k = 2048, 19, 19, 256, 256
    g = torch.Generator(device="cuda").manual_seed(2048)
    x = torch.empty((rows, h, wd, c), device="cuda", dtype=torch.float16).normal_(generator=g)
    w = (torch.randn((k, 3, 3, c), device="cuda", generator=g) * (9 * c) ** -0.5).half()
    b = torch.randn((k,), device="cuda", generator=g).half()
    r = torch.empty((rows, h, wd, k), device="cuda", dtype=torch.float16).normal_(generator=g)
    y0 = _cut_run(elf, x, w, b, r, 1, "algo0", guard=False)
    for i in range(20):
        y = _cut_run(elf, x, w, b, r, 1, "plain", guard=False)
        assert torch.equal(cc.bits(y), cc.bits(y0)), "launch %d differs from algo 0" % i
    torch.cuda.empty_cache()
