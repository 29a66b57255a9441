"""CPU: what the net's convolution entries refuse, and what the eight host-arithmetic entries of algo 1's plan return, as literals
recorded from the library before the entries' shared checks moved into elf_amd/csrc/net_common.h (conv_args) and the plan entries
into net_conv3x3_plan.hip.  Nothing here reaches the GPU runtime: the pointers are made-up addresses that are never read, a call
with rows above 0 is made only where it is refused before the pointer is looked up, and every other call has rows = 0, which an
entry accepts (status 0) behind all its argument checks and in front of its first call into the runtime."""
import ctypes as C

import pytest

BADARG = -1
A = 0x10000   # 16-B aligned made-up addresses, all different
PTRS = dict(x=A, w=2 * A, b=3 * A, r=4 * A, y=5 * A)


@pytest.fixture(scope="module")
def L(built):
    import elf_amd
    return elf_amd.lib()


def _p(v):
    return None if v is None else C.c_void_p(v)


# entry -> (its smallest good shape, how it is called); in_f16 has no skip
SHAPES = {
    "f16_algo0": dict(c=64, k=256), "f16_algo1": dict(c=64, k=256), "width": dict(c=64, k=256), "boards": dict(c=64, k=256),
    "small": dict(c=64, k=64), "in": dict(c=18, k=64),
}


def _call(L, entry, a):
    x, w, b, r, y = (_p(a[n]) for n in ("x", "w", "b", "r", "y"))
    s = (a["rows"], a["h"], a["wd"], a["c"], a["k"], 1)
    if entry in ("f16_algo0", "f16_algo1"):
        return L.elfnet_conv3x3_f16(x, w, b, r, y, *s, a.get("algo", int(entry[-1])), None)
    if entry == "width":
        return L.elfnet_conv3x3_f16_width(x, w, b, r, y, *s, a.get("algo", 1), a.get("round_width", 0), None)
    if entry == "boards":
        return L.elfnet_conv3x3_f16_boards(x, w, b, r, y, *s, a.get("round_width", 0), None)
    if entry == "small":
        return L.elfnet_conv3x3_small_f16(x, w, b, r, y, *s, None)
    return L.elfnet_conv3x3_in_f16(x, w, b, y, *s, None)


def _args(entry, **over):
    a = dict(PTRS, rows=0, h=9, wd=9, **SHAPES[entry])
    a.update(over)
    return a


# The table: (label, overrides).  A case without `rows` is run at rows = 0 and, where that is refused, at rows = 2 as well.
# 2^30 elements: 256 positions a row (16 x 16) x rows x max(c, k); k * 9 * c cannot be 2^30 exactly (9 is odd), so the first
# product at or above it and the last below, per entry.
def _table(entry):
    c, k = SHAPES[entry]["c"], SHAPES[entry]["k"]
    t = [("good", {})]
    t += [("null " + n, {n: None}) for n in ("x", "w", "b", "y")]
    t += [("no skip", dict(r=None))]
    t += [("bit 3 of " + n, {n: 9 * A + 8}) for n in ("x", "w", "b", "r", "y")]
    t += [("bit 2 of x", dict(x=9 * A + 4)), ("bit 1 of x", dict(x=9 * A + 2))]
    t += [("y == x", dict(y=PTRS["x"])), ("y == res", dict(y=PTRS["r"]))]
    for n in ("h", "wd", "c", "k", "rows"):
        t += [("%s = %d" % (n, v), {n: v}) for v in (0, -1)]
    t += [("c = %d" % v, dict(c=v)) for v in (1, 2, 8, 12, 18, 32, 34, 36, 72, 96, 128, 192)]
    t += [("k = %d" % v, dict(k=v)) for v in (8, 12, 16, 32, 48, 72, 96, 128, 192, 320, 512)]
    big = max(c, k)
    t += [("2^30 elements of y", dict(rows=(1 << 30) // (256 * big), h=16, wd=16)),
          ("2^30 elements of x", dict(rows=(1 << 30) // (256 * 2 * big), h=16, wd=16, c=2 * big)),
          ("2^31 elements", dict(rows=1 << 22, h=19, wd=19))]
    if entry == "in":
        t += [("w at 2^30", dict(c=32, k=3728288)), ("w below 2^30", dict(c=32, k=3728256))]
    else:
        t += [("w at 2^30", dict(c=1 << 14, k=1 << 13)), ("w below 2^30", dict(c=1 << 13, k=1 << 13))]
    t += [("algo = %d" % v, dict(algo=v)) for v in (-1, 2)]
    t += [("round_width = %d" % v, dict(round_width=v)) for v in (-1, -(1 << 31), 4, 1 << 30)]
    return t


# status at rows = 0 (or at the case's own rows), by entry, in the table's order: recorded from the parent commit's library
Z, B = 0, BADARG
EXPECTED = {
    "f16_algo0": [Z, B, B, B, B, Z, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, Z, B, B, B, Z, B, B, Z, B, B, Z, Z, Z, Z, Z, B, Z, Z,
                  Z, Z, Z, Z, Z, Z, Z, B, B, B, B, Z, B, B, Z, Z, Z, Z],
    "f16_algo1": [Z, B, B, B, B, Z, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, Z, B, B, B, Z, B, B, Z, B, B, Z, Z, Z, Z, Z, B, Z, Z,
                  Z, Z, Z, Z, Z, Z, Z, B, B, B, B, Z, B, B, Z, Z, Z, Z],
    "width": [Z, B, B, B, B, Z, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, Z, B, B, B, Z, B, B, Z, B, B, Z, Z, Z, Z, Z, B, Z, Z,
              Z, Z, Z, Z, Z, Z, Z, B, B, B, B, Z, B, B, B, B, Z, Z],
    "boards": [Z, B, B, B, B, Z, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, Z, B, B, B, Z, B, B, Z, B, B, Z, Z, Z, Z, Z, B, Z, Z,
               Z, Z, Z, Z, Z, Z, Z, B, B, B, B, Z, Z, Z, B, B, Z, Z],
    "small": [Z, B, B, B, B, Z, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, B, Z, B, B, B, B, B, B, B, B, B, B, B, Z, Z, B, B, B, B,
              B, B, B, Z, Z, Z, Z, B, B, B, B, Z, Z, Z, Z, Z, Z, Z],
    "in": [Z, B, B, B, B, Z, Z, B, B, Z, B, Z, B, B, Z, B, B, B, B, B, B, B, B, Z, B, B, Z, Z, Z, Z, Z, B, B, B, B, B, B, B, B, B, Z,
           B, B, Z, Z, Z, Z, Z, B, B, B, B, Z, Z, Z, Z, Z, Z, Z],
}


@pytest.mark.parametrize("entry", list(SHAPES))
def test_the_entries_refuse_what_they_refused(L, entry):
    table = _table(entry)
    got = [_call(L, entry, _args(entry, **over)) for _, over in table]
    assert len(got) == len(EXPECTED[entry])
    wrong = [(label, g, e) for (label, _), g, e in zip(table, got, EXPECTED[entry]) if g != e]
    assert not wrong, wrong
    assert got[0] == 0   # the table's base call is a good one
    # a refusal does not wait for rows: the same call with rows is refused too, before the pointer is looked up
    for (label, over), e in zip(table, EXPECTED[entry]):
        if e == BADARG and "rows" not in over:
            assert _call(L, entry, _args(entry, rows=2, **over)) == BADARG, label


def _ints(n):
    return [C.c_int(-7) for _ in range(n)]


def _u32s(n):
    return [C.c_uint32(7) for _ in range(n)]


def _plan_call(L, name, args):
    """(return value, the values behind the entry's pointers: -7 / 7 where it wrote nothing)"""
    if name == "boards_plan":
        o = _ints(4)
        return (L.elfnet_conv3x3_f16_boards_plan(*args, *map(C.byref, o)),) + tuple(v.value for v in o)
    if name == "plan":
        o = _ints(3)
        return (L.elfnet_conv3x3_f16_plan(*args, *map(C.byref, o)),) + tuple(v.value for v in o)
    if name == "recip":
        o = _u32s(2)
        return (L.elfnet_conv3x3_f16_recip(*args, *map(C.byref, o)),) + tuple(v.value for v in o)
    if name == "bufstage":
        o = _u32s(6)
        return (L.elfnet_conv3x3_f16_bufstage(*args, *map(C.byref, o)),) + tuple(v.value for v in o)
    return (getattr(L, "elfnet_conv3x3_f16_" + name)(*args),)


# rows 1 and 257, boards 1 x 1, 1 x 3, 3 x 3 and 19 x 19, c 64 / 128, k 256 / 512, round widths 1, 2, 7 and 256; good and bad
PLAN_CALLS = {
    # rows, h, wd, k, round_width, id
    "boards_plan": [(1, 1, 1, 256, 1, -1), (1, 1, 3, 256, 2, 2), (257, 3, 3, 512, 7, 35), (257, 3, 3, 512, 7, 36), (257, 19, 19, 256, 256, 721),
                    (1, 19, 19, 512, 256, 0), (257, 1, 3, 256, 1, 5), (0, 3, 3, 256, 2, -1), (1, 0, 3, 256, 2, -1), (1, 3, -1, 256, 2, -1),
                    (1, 3, 3, 128, 2, -1), (1, 3, 3, 0, 2, -1), (1, 3, 3, 256, 0, -1), (1, 3, 3, 256, -1, 0), (1 << 31, 19, 19, 512, 7, -1)],
    # rows, h, wd, k, round_width, g, j
    "boards_deal": [(1, 1, 1, 256, 1, -1, 0), (257, 3, 3, 512, 7, -1, 0), (257, 3, 3, 512, 7, 6, 0), (257, 3, 3, 512, 7, 6, 5), (257, 3, 3, 512, 7, 0, 5),
                    (257, 3, 3, 512, 7, 0, 6), (257, 3, 3, 512, 7, 7, 0), (257, 3, 3, 512, 7, 0, -1), (1, 19, 19, 256, 256, 255, 1),
                    (1, 19, 19, 256, 256, 104, 1), (1, 1, 3, 256, 2, 1, 1), (0, 3, 3, 256, 2, -1, 0), (1, 3, 3, 192, 2, -1, 0), (1, 3, 3, 256, 0, 0, 0)],
    # rows, h, wd, c, k, round_width, g
    "boards_load": [(1, 1, 1, 128, 256, 1, 0), (1, 1, 1, 64, 256, 1, 0), (1, 1, 3, 64, 256, 2, 0), (1, 1, 3, 64, 256, 2, 1), (257, 3, 3, 128, 512, 7, 0),
                    (257, 3, 3, 128, 512, 7, 6), (257, 3, 3, 128, 512, 7, 7), (257, 3, 3, 128, 512, 7, -1), (257, 19, 19, 64, 256, 256, 255),
                    (1, 19, 19, 128, 512, 256, 0), (1, 3, 3, 0, 256, 2, 0), (1, 3, 3, 96, 256, 2, 0), (1, 3, 3, 64, 128, 2, 0), (0, 3, 3, 64, 256, 2, 0)],
    # rows, h, wd, c, k, round_width (above 0: host arithmetic at that width; 0 would ask the device)
    "order": [(1, 19, 19, 64, 256, 256), (257, 19, 19, 64, 256, 256), (257, 19, 19, 128, 512, 7), (257, 3, 3, 64, 256, 2), (257, 1, 1, 64, 256, 1),
              (257, 1, 1, 128, 256, 1), (257, 1, 3, 64, 512, 2), (2048, 19, 19, 128, 256, 256), (1, 3, 3, 64, 256, 1), (0, 3, 3, 64, 256, 1),
              (-1, 3, 3, 64, 256, 1), (257, 3, 3, 96, 256, 1), (257, 3, 3, 64, 128, 1), (257, 3, 3, 64, 256, -1), (1 << 22, 19, 19, 64, 256, 1)],
    # tiles, columns, round_width, id
    "plan": [(1, 1, 1, 0), (2, 1, 7, 1), (2, 2, 7, 3), (2, 2, 7, 4), (9, 1, 7, 8), (9, 1, 7, 10), (9, 1, 7, 11), (258, 2, 256, 519), (258, 2, 256, 520),
             (0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1), (1 << 29, 2, 7, 0)],
    # tiles, columns, round_width
    "grid": [(1, 1, 1), (1, 1, 256), (2, 2, 7), (9, 1, 7), (9, 2, 7), (258, 2, 256), (258, 1, 2), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, -1), (1 << 29, 2, 7)],
    # divisor
    "recip": [(1,), (2,), (3,), (9,), (19,), (361,), (1 << 16,), ((1 << 31) - 1,), (1 << 31,), (0,), (-1,), ((1 << 31) + 1,)],
    # rows, h, wd, c, k, tap, kc
    "bufstage": [(1, 1, 1, 64, 256, -1, 0), (1, 1, 3, 64, 256, 0, 0), (257, 3, 3, 128, 512, 8, 1), (257, 3, 3, 128, 512, 4, 0), (257, 19, 19, 64, 256, 3, 0),
                 (1, 19, 19, 128, 256, 0, 1), (1, 3, 3, 128, 256, 0, 2), (1, 3, 3, 64, 256, 9, 0), (1, 3, 3, 64, 256, 0, -1), (0, 3, 3, 64, 256, -1, 0),
                 (1, 3, 3, 96, 256, -1, 0), (1, 3, 3, 64, 128, -1, 0), (1, 1, 1 << 21, 64, 256, -1, 0), (1, 1, 1 << 21, 256, 256, -1, 0),
                 (1, 3, 3, 1 << 14, 1 << 13, -1, 0)],
}

# (return value, values behind the pointers), in PLAN_CALLS' order: recorded from the parent commit's library
N4, N3, U6 = (-1, -7, -7, -7, -7), (-1, -7, -7, -7), (-1, 7, 7, 7, 7, 7, 7)   # refused, nothing written
PLAN_EXPECTED = {
    "boards_plan": [(1, -7, -7, -7, -7), (3, 0, 2, 0, 24), (36, 1, 8, 1, 27), N4, (722, 1, 360, 0, 27), (722, 0, 20, 0, 511), (6, 1, 2, 0, 24),
                    N4, N4, N4, N4, N4, N4, N4, N4],
    "boards_deal": [(1,), (7,), (6,), (35,), (-1,), (-1,), (-1,), (-1,), (256,), (-1,), (2,), (-1,), (-1,), (-1,)],
    "boards_load": [(2,), (-1,), (2,), (5,), (58,), (56,), (-1,), (-1,), (27,), (36,), (-1,), (-1,), (-1,), (-1,)],
    "order": [(0,), (0,), (0,), (0,), (0,), (1,), (1,), (1,), (0,), (0,), (-1,), (-1,), (-1,), (-1,), (-1,)],
    "plan": [(1, 0, 0, -1), (2, 1, 0, -1), (4, 1, 1, -1), N3, (11, 7, 0, 1), (11, 8, 0, 1), N3, (520, 257, 1, 1), N3, N3, N3, N3, N3, N3],
    "grid": [(1,), (1,), (4,), (7,), (7,), (256,), (2,), (-1,), (-1,), (-1,), (-1,), (-1,)],
    "recip": [(0, 4294967295, 0), (0, 2147483647, 0), (0, 2863311530, 1), (0, 3817748707, 3), (0, 3616814565, 4), (0, 3045738581, 8),
              (0, 2147483647, 15), (0, 2147483649, 30), (0, 2147483647, 30), (-1, 7, 7), (-1, 7, 7), (-1, 7, 7)],
    "bufstage": [(0, 256, 384, 294912, 3221225472, 7, 7), (0, 512, 896, 294912, 3221225472, 0, 0),
                 (0, 1024, 593152, 1179648, 3221225472, 2176, 2176), (0, 1024, 593152, 1179648, 3221225472, 1024, 1024),
                 (0, 2560, 11878016, 294912, 3221225472, 2432, 384), (0, 5120, 97536, 589824, 3221225472, 128, 128),
                 U6, U6, U6, U6, U6, U6, (0, 268435584, 536871040, 294912, 3221225472, 7, 7), U6, U6],
}


@pytest.mark.parametrize("name", list(PLAN_CALLS))
def test_the_plan_entries_return_what_they_returned(L, name):
    got = [_plan_call(L, name, args) for args in PLAN_CALLS[name]]
    assert len(got) == len(PLAN_EXPECTED[name]) >= 12
    wrong = [(args, g, e) for args, g, e in zip(PLAN_CALLS[name], got, PLAN_EXPECTED[name]) if g != e]
    assert not wrong, wrong
