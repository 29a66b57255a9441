"""The one copy of what the tests/test_gpu_net*.py files share: the `elf` fixture, pointers and bit views, NaN-guarded buffers,
the nine-tap reference and the header's epilogue in fp32, the seeded operands (random and exact-integer) and the launches of the
trunk convolution's entry points.  A plain helper module beside trained_like.py, imported the same way (`import conv_cases as cc`).

A test file computes its own seed (a one-line `_seed(rows, h, wd, c, k)`); the helpers here own the order of the draws, so two
files that name the same seed and shape see the same bits, and a file's operands change only when its own seed formula does.
Everything drawn or computed once is cached and must be left unchanged: a test that poisons an operand works on a clone.

torch is imported inside the functions, so collecting the GPU files does not import it.  Every function that allocates takes
`device`, so all but the launches run on the CPU too (tests/test_conv_cases_cpu.py)."""
import ctypes as C

import pytest

ALONE = 1 << 30      # a round width above any item count: every item has a workgroup of its own, no split, no chain
RES_RELU = [(False, 0), (False, 1), (True, 0), (True, 1)]
NAN = float("nan")


@pytest.fixture(scope="module")
def elf(built):
    import elf_amd
    return elf_amd


# ------------------------------------------------------------------------------------------------ small helpers

def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    """fp16 as its bit patterns: NaN compares by payload, -0 differs from +0"""
    import torch
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ buffers

def guarded(rows, h, wd, k, device="cuda"):
    """y prefilled with NaN, and one guard row of NaN behind its last row.  -> (buffer [rows h wd + 1, k], y)"""
    import torch
    buf = torch.full((rows * h * wd + 1, k), NAN, device=device, dtype=torch.float16)
    return buf, buf[:rows * h * wd].view(rows, h, wd, k)


def carve(t, guard, mod=32, rem=16):
    """A copy of t inside a larger NaN-filled buffer of t's (floating-point) type and device, at least `guard` elements of NaN in
    front and behind, starting at an address that is `rem` modulo `mod` bytes (the default: 16-byte and not 32-byte aligned, the
    weakest the convolutions' ABI allows).  -> (the copy, front guard, back guard)"""
    import torch
    n, es = t.numel(), t.element_size()
    buf = torch.full((guard + n + guard + mod,), NAN, device=t.device, dtype=t.dtype)
    o = guard
    while (buf.data_ptr() + es * o) % mod != rem:
        o += 1
    v = buf[o:o + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % mod == rem and o >= guard and buf.numel() - (o + n) >= guard
    return v, buf[:o], buf[o + n:]


# ------------------------------------------------------------------------------------------------ numerics

def conv_fp32(x, w):
    """conv2d(x, w, padding=1) for NHWC x [rows,h,w,C] and w [K,3,3,C], written out as its nine taps: one GEMM per tap over the
    zero-padded input, summed in x's dtype -- fp32 for every caller but the fp64 truths of the native net's ends.  (F.conv2d itself
    would either search MIOpen's solvers for an fp32 shape nothing else uses or, with MIOpen off, unfold row by row: 45 s for 2048
    rows.  test_gpu_net_conv._case checks this against it on two rows, tests/test_conv_cases_cpu.py on integers.)"""
    import torch
    rows, h, wd = x.shape[0], x.shape[1], x.shape[2]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((rows, h, wd, w.shape[0]), device=x.device, dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + wd, :] @ w[:, ky, kx, :].t()
    return out


def epilogue_fp32(conv, b, r, relu):
    """the header's sequence on an fp32 convolution result: rounded to fp16, + bias (+ res, unless r is None) in fp32, max(., 0)
    as fmax (a NaN becomes 0), rounded to fp16.  On the integer cases neither rounding changes a value."""
    import torch
    v = conv.half().float() + b.float()
    if r is not None:
        v = v + r.float()
    if relu:
        v = torch.fmax(v, torch.zeros((), device=v.device))
    return v.half()


def differing(y, ref):
    """the number of elements that are neither equal as values (-0 equals +0, Inf equals Inf) nor NaN in both"""
    import torch
    y, ref = y.float(), ref.float()
    return int((~((y == ref) | (torch.isnan(y) & torch.isnan(ref)))).sum().item())


# ------------------------------------------------------------------------------------------------ operands

_rand, _ints, _refs = {}, {}, {}


def rand_case(seed, rows, h, wd, c, k, device="cuda"):
    """(x, w, b, r) in fp16, drawn in that order from one generator: x, b and r standard normal, w scaled by (9 c)^-1/2 so that the
    convolution's output is O(1).  Dense up to and including the border cells: a wrong halo is an O(1) error."""
    import torch
    key = (seed, rows, h, wd, c, k, device)
    if key not in _rand:
        g = torch.Generator(device=device).manual_seed(seed)
        x = torch.randn((rows, h, wd, c), device=device, generator=g).half()
        w = (torch.randn((k, 3, 3, c), device=device, generator=g) * (9 * c) ** -0.5).half()
        b = torch.randn((k,), device=device, generator=g).half()
        r = torch.randn((rows, h, wd, k), device=device, generator=g).half()
        _rand[key] = (x, w, b, r)
    return _rand[key]


def int_case(seed, rows, h, wd, c, k, res=True, limit=1023, not_degenerate=False, device="cuda"):
    """The exact-integer operands, as a dict: x in {-1,0,1}; w in {-1,0,1} with about 3/4 zeros, drawn per element (its sign, then
    its mask) so that it is asymmetric in (k,c) and in (ky,kx); integer bias and, with `res`, integer res in [-8,8]; and conv, the
    nine-tap fp32 form of x and w.  Drawn in the order x, sign of w, mask of w, b, r.  Every partial sum is an integer of
    magnitude at most `limit`, far below 2048: exact in fp32 and in fp16, so any differing element is a wrong halo, layout,
    swizzle or timing, never rounding.  Checked here: |conv| <= limit (conv holds integers, so the default is "below 1024"), and w
    changes under either flip; with `not_degenerate` also that conv is not all zero and that, on a non-square board, the nine-tap
    form of the same memory read as wd x h differs."""
    import torch
    key = (seed, rows, h, wd, c, k, res, limit, not_degenerate, device)
    if key not in _ints:
        g = torch.Generator(device=device).manual_seed(seed)
        ri = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, device=device, generator=g)
        x = ri((rows, h, wd, c), -1, 1).half()
        w = (ri((k, 3, 3, c), -1, 1) * (ri((k, 3, 3, c), 0, 3) == 0)).half()
        d = dict(x=x, w=w, b=ri((k,), -8, 8).half())
        if res:
            d["r"] = ri((rows, h, wd, k), -8, 8).half()
        conv = d["conv"] = conv_fp32(x.float(), w.float())
        assert conv.abs().max().item() <= limit and not torch.equal(w, w.flip(1)) and not torch.equal(w, w.flip(2))
        if not_degenerate:
            assert bool((conv != 0).any())
            if h != wd:
                swapped = conv_fp32(x.float().view(rows, wd, h, c), w.float()).view(rows, h, wd, k)
                assert not torch.equal(swapped, conv)
        _ints[key] = d
    return _ints[key]


# ------------------------------------------------------------------------------------------------ launches

def launch(L, how, x, w, b, r, y, relu, width=0, algo=1, shape=None):
    """One call of a trunk convolution entry of the library L; returns its status.  It neither synchronises nor asserts.  how:
      'algo0'   elfnet_conv3x3_f16 with algo 0
      'plain'   elfnet_conv3x3_f16 with algo 1: order and round width are the library's own choice
      'linear'  elfnet_conv3x3_f16_width with `algo` (1 unless a test of the argument checks says otherwise) at round width `width`
      'board'   elfnet_conv3x3_f16_boards at round width `width`: it takes no algo
      'small'   elfnet_conv3x3_small_f16: the plain entry's arguments but for the algo
    The shape is x's [rows,h,w,C] and w's K unless `shape` = (rows, h, wd, c, k) names another (the refusal tests)."""
    rows, h, wd, c, k = shape if shape is not None else (*x.shape, w.shape[0])
    a = (ptr(x), ptr(w), ptr(b), ptr(r), ptr(y), rows, h, wd, c, k, int(relu))
    if how == "algo0":
        return L.elfnet_conv3x3_f16(*a, 0, stream())
    if how == "plain":
        return L.elfnet_conv3x3_f16(*a, 1, stream())
    if how == "linear":
        return L.elfnet_conv3x3_f16_width(*a, algo, width, stream())
    if how == "board":
        return L.elfnet_conv3x3_f16_boards(*a, width, stream())
    if how == "small":
        return L.elfnet_conv3x3_small_f16(*a, stream())
    raise ValueError(how)


def conv_in(L, x, w, b, y, rows, h, wd, c, k, relu):
    """one call of the native net's input convolution"""
    return L.elfnet_conv3x3_in_f16(ptr(x), ptr(w), ptr(b), ptr(y), rows, h, wd, c, k, int(relu), stream())


HEAD_NAMES = ("pconv_w", "pconv_b", "vconv_w", "vconv_b", "pi_w", "pi_b", "v1_w", "v1_b", "v2_w", "v2_b")


def heads_struct(t, ch, vh):
    """the ElfNetHeads of elfnet_heads_f16 from a dict of device tensors by those names.  (The other heads helpers of
    test_gpu_net_native_io.py and test_gpu_net_native_io_edges.py differ in what they return and accept, and stay in their files.)"""
    from elf_amd._lib import ElfNetHeads
    return ElfNetHeads(*[t[nm].data_ptr() for nm in HEAD_NAMES], ch, vh)


def run_guarded(L, how, x, w, b, r, relu, width=0):
    """one launch into a fresh guarded() y, waited for: the status is 0 and the guard row is still NaN.  -> y"""
    import torch
    buf, y = guarded(x.shape[0], x.shape[1], x.shape[2], w.shape[0])
    assert launch(L, how, x, w, b, r, y, relu, width) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[-1]).all()), "the guard row behind y was written"
    return y


def cached_ref(L, how, seed, shape, use_res, relu, width=0):
    """run_guarded's output on rand_case(seed, *shape), without NaN; computed once per case and left unchanged"""
    import torch
    key = (how, width, seed, shape, use_res, relu)
    if key not in _refs:
        x, w, b, r = rand_case(seed, *shape)
        y = run_guarded(L, how, x, w, b, r if use_res else None, relu, width)
        assert not bool(torch.isnan(y).any())
        _refs[key] = y
    return _refs[key]


def algo0_ref(L, seed, shape, use_res, relu):
    """algo 0's output on rand_case(seed, *shape): the reference wherever bit equality is the claim.  Algo 0 takes neither a round
    width nor an order (net_conv.hip drops both), so this one launch of the plain entry is what every file's reference was."""
    return cached_ref(L, "algo0", seed, tuple(shape), use_res, relu)
