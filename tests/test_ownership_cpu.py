"""CPU: the expected-value helper of the ownership tests is right before anything is compared with it, and the library
surface of elfgo_area_map / elfgo_own_* holds without a GPU."""
import ctypes

import numpy as np
import pytest

import known_answers as ka
import ownership_expected as oe
from adapters import PortState
from pyoracle import Port, Ref, playout_seeds

SUPERKO_CAP = 0.05   # at most this share of the playouts may be exempt from the area / evaluate identity


def engines(n):
    return [Port(n)] + ([Ref(n)] if Ref.available(n) else [])


@pytest.mark.parametrize("n,plies,K", [(9, (20, 40), 32), (19, (60, 200), 16)])
def test_area_map_restatement_equals_evaluate_on_playout_ends(built, n, plies, K):
    """black - white of the restated area map == GoState::evaluate(7.5) + 7.5 on every end position that did not end by
    super-ko (there evaluate answers +-1 by rule), for the C port and, where it was built, the reference itself; both engines
    give the same counts and stats."""
    results = []
    for E in engines(n):
        total = exempt = 0
        res = []
        for seed in playout_seeds(4):
            for pl in plies:
                src, _ = oe.prefix(E, seed, pl)
                ends = []
                res.append(oe.expected(E, src, seed, K, 7.5, ends=ends))
                for c in ends:
                    total += 1
                    if oe.ended_by_superko(E, c):
                        exempt += 1
                    else:
                        assert oe.area_diff(oe.area_map(E.board(c)[0], n)) == E.evaluate(c, 7.5) + 7.5
                    E.free(c)
                E.free(src)
        assert exempt <= SUPERKO_CAP * total, (exempt, total)
        results.append(res)
    for other in results[1:]:
        for (c0, s0), (c1, s1) in zip(results[0], other):
            assert np.array_equal(c0, c1) and np.array_equal(s0, s1)


def test_area_map_restatement_on_the_reference_scoring_positions(built):
    """go_test.cc's two Tromp-Taylor positions (1.5 / 2.5 at komi 6.5), loaded move by move so that E.board shows them"""
    rows = [".XX......", "OOXX.....", "OOOX...X.", "OXX......", "OOXXXXXX.", "OOOXOXOXX", ".O.OOXOOX", ".O.O.OOXX", "......OOO"]
    for E in engines(9):
        for rr, want in ((rows, 1.5), (["X" + rows[0][1:]] + rows[1:], 2.5)):
            b = PortState(E)
            ka.load_board(b, rr)
            assert b.evaluate(6.5) == want
            assert oe.area_diff(oe.area_map(E.board(b.s)[0], 9)) - 6.5 == want


def test_seed_formula():
    assert oe.seed_of(5, 0) == 5 and oe.seed_of(1, 1) == 0x9E3779B97F4A7C16
    assert oe.seed_of(0xFFFFFFFFFFFFFFFF, 2) == (2 * 0x9E3779B97F4A7C15 - 1) & 0xFFFFFFFFFFFFFFFF


def test_ownership_entry_points_without_a_gpu(built):
    """the five entry points are exported with prototypes; null / non-positive arguments are ELFGO_E_BADARG, never a crash"""
    import elf_amd
    from elf_amd import _lib
    L = elf_amd.lib()
    for name in ("elfgo_area_map", "elfgo_own_create", "elfgo_own_destroy", "elfgo_own_scratch_bytes", "elfgo_own_run"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint64 * 64)()
    assert L.elfgo_area_map(None, None, 1, buf, None) == -1
    assert L.elfgo_own_create(None, 0, ctypes.byref(h)) == -1 and not h.value      # no engine (hence no device): a status
    assert L.elfgo_own_destroy(None) == -1
    assert L.elfgo_own_scratch_bytes(None) == 0
    assert L.elfgo_own_run(None, None, buf, 1, 1, 10, ctypes.c_float(7.5), buf, buf, None) == -1
