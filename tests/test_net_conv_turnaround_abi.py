"""CPU: elfnet_conv3x3_f16_recip (elf_amd/csrc/net_conv3x3.hip), the multiplier and shift algo 1's kernel decodes a position with.
The host entry makes one pair for H * W and one for W per launch and the kernel computes n / d as
(((n + 1) * mul) >> 32) >> shift (a v_mul_hi_u32 and a shift) for positions n up to tiles * 256 - 1, which the entry's 2^31-byte
limit keeps below 2^31.  A quotient that is off by one anywhere is a tap mask of the wrong board position, so: every divisor
1 .. 4096 against Python's own division, quotient and remainder, at the edges of every multiple and power of two and at 10 000
random positions each, with no exception allowed."""
import ctypes as C

import numpy as np
import pytest

BADARG = -1
# the entry refuses a tensor of 2^31 bytes or more: at C = 64 (128 B per position) x holds at most 2^24 - 1 positions, and the last
# tile's rows run up to 255 positions beyond the last one
LAST_C64 = (1 << 24) - 2


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _recip(L, d):
    mul, shift = C.c_uint32(0xDEADBEEF), C.c_uint32(0xDEADBEEF)
    assert L.elfnet_conv3x3_f16_recip(d, C.byref(mul), C.byref(shift)) == 0, d
    return mul.value, shift.value


def _div(n, mul, shift):
    """the kernel's arithmetic, on Python integers: the high word of a 32 x 32 -> 64 bit product, shifted"""
    assert 0 <= n + 1 < 1 << 32 and 0 <= mul < 1 << 32 and 0 <= shift < 32
    return (((n + 1) * mul) >> 32) >> shift


def test_refusals(L):
    mul, shift = C.c_uint32(7), C.c_uint32(7)
    for d in (0, -1, (1 << 31) + 1, 1 << 40):
        assert L.elfnet_conv3x3_f16_recip(d, C.byref(mul), C.byref(shift)) == BADARG, d
    assert L.elfnet_conv3x3_f16_recip(19, None, C.byref(shift)) == BADARG
    assert L.elfnet_conv3x3_f16_recip(19, C.byref(mul), None) == BADARG
    assert (mul.value, shift.value) == (7, 7)
    assert L.elfnet_conv3x3_f16_recip(1 << 31, C.byref(mul), C.byref(shift)) == 0


def test_every_divisor_up_to_4096_against_divmod(L):
    """p = 0, d - 1, d, d + 1, 2^k - 1, 2^k, 2^k + 1 (below 2^31), the largest positions a C = 64 call can decode, and 10 000
    random p below 2^31 per divisor.  The edge values go through Python's divmod one by one; the random ones through numpy's
    floor division and remainder on int64, which are divmod for non-negative integers."""
    rng = np.random.default_rng(20261019)
    edges = {0, LAST_C64, LAST_C64 + 1, LAST_C64 + 255, (1 << 31) - 1}
    for k in range(0, 31):
        edges.update((max((1 << k) - 1, 0), 1 << k, (1 << k) + 1))
    edges = sorted(e for e in edges if e < 1 << 31)
    bad = []
    for d in range(1, 4097):
        mul, shift = _recip(L, d)
        assert mul < 1 << 32 and shift < 32
        for p in edges + [d - 1, d, d + 1, 2 * d - 1, 2 * d, LAST_C64 // d * d - 1, LAST_C64 // d * d]:
            if p < 0:
                continue
            q, r = divmod(p, d)
            got = _div(p, mul, shift)
            if (got, p - got * d) != (q, r):
                bad.append((d, p, got, q))
        p = rng.integers(0, 1 << 31, 10000, dtype=np.int64).astype(np.uint64)
        got = (((p + np.uint64(1)) * np.uint64(mul)) >> np.uint64(32)) >> np.uint64(shift)   # below 2^63: no wrap
        pi, gi = p.astype(np.int64), got.astype(np.int64)
        wrong = np.nonzero((gi != pi // d) | (pi - gi * d != pi % d))[0]
        bad.extend((d, int(pi[i]), int(gi[i]), int(pi[i]) // d) for i in wrong[:3])
    assert not bad, "divisor, position, got, want: %s" % bad[:10]


def test_board_divisors_and_large_ones(L):
    """the divisors of real launches (H * W and W of the boards the GPU tests use), powers of two up to 2^31 and their neighbours, and
    some large odd divisors: exhaustive at every multiple's edge below 2^31 for the small ones, sampled for the large ones"""
    rng = np.random.default_rng(7)
    ds = [361, 81, 256, 4, 185, 19, 9, 16, 2, 37, 5, 1] + [1 << k for k in range(1, 32)] + [(1 << k) + 1 for k in range(1, 31)] + \
         [(1 << k) - 1 for k in range(2, 32)] + [int(v) for v in rng.integers(4097, 1 << 31, 200)]
    for d in ds:
        mul, shift = _recip(L, d)
        m = np.arange(0, ((1 << 31) - 1) // d + 1, max(1, ((1 << 31) // d) // 20000), dtype=np.int64) * d
        p = np.unique(np.concatenate([m, m - 1, m + 1, rng.integers(0, 1 << 31, 2000, dtype=np.int64)]))
        p = p[(p >= 0) & (p < 1 << 31)]
        got = ((((p.astype(np.uint64) + np.uint64(1)) * np.uint64(mul)) >> np.uint64(32)) >> np.uint64(shift)).astype(np.int64)
        assert np.array_equal(got, p // d), d
        assert np.array_equal(p - got * d, p % d), d
