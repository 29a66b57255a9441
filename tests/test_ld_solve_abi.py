"""CPU: elfgo_ld_solve is exported, declared and bound, a null engine is a status code, and LdSolution derives what it states."""
import ctypes
import os
import re

from conftest import ROOT


def test_symbols_are_exported_declared_and_bound(built):
    from elf_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "elf_amd.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    for name in ("elfgo_ld_solve", "elfgo_ld_solve_max_depth"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert ("int elfgo_ld_solve(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, const uint8_t* attackers, "
            "int max_depth, int max_nodes, int self_atari_thres, int32_t* info, int8_t* value, int32_t* nodes, void* stream);") in flat
    res, args = _lib.SIGNATURES["elfgo_ld_solve"]
    assert res is ctypes.c_int and [i for i, a in enumerate(args) if a is ctypes.c_int] == [2, 5, 6, 7] and len(args) == 12


def test_null_engine_is_a_status_code_and_the_depth_limit_is_positive(built):
    import elf_amd
    L = elf_amd.lib()
    buf = (ctypes.c_uint8 * 4096)()
    assert 0 < L.elfgo_ld_solve_max_depth() <= 64
    assert L.elfgo_ld_solve(None, None, 1, None, None, 3, 16, 3, buf, buf, buf, None) == -1
    assert L.elfgo_ld_solve(None, None, 1, None, None, 3, 16, 3, None, buf, None, None) == -1


def test_solution_on_hand_made_tensors():
    """root_value / best_move / proved: max for the defender, min for the attacker, the smallest action on a tie, the static
    verdict of a terminal root, None where a first move was cut"""
    import torch
    import elf_amd
    from elf_amd.engine import LdSolution
    assert elf_amd.LdSolution is LdSolution and callable(elf_amd.GoEngine.ld_solve)

    def sol(to_move, verdict, cells):
        value = torch.full((1, 82), -1, dtype=torch.int8)
        for a, v in cells.items():
            value[0, a] = v
        info = torch.tensor([[0, 0, 9, 9, 2, 1, to_move, verdict]], dtype=torch.int32)
        return LdSolution(9, info, value, torch.zeros((1, 82), dtype=torch.int32))
    s = sol(1, 1, {5: 1, 7: 2, 9: 2, 81: 0})
    assert (s.root_value(), s.best_move(), s.proved()) == ([2], [7], [True])
    s = sol(2, 1, {5: 1, 7: 2, 9: 1})
    assert (s.root_value(), s.best_move(), s.proved()) == ([1], [5], [False])
    s = sol(2, 0, {})
    assert (s.root_value(), s.best_move(), s.proved()) == ([0], [None], [True])
    s = sol(1, 1, {5: 2, 7: -2})
    assert (s.root_value(), s.best_move(), s.proved()) == ([None], [None], [False])
