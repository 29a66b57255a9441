"""CPU: the region and life-and-death entry points are exported, declared and bound, and the Python surface has the stated
signatures and defaults (no compute calls here)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def test_symbols_are_exported_declared_and_bound(built):
    from elf_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "elf_amd.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())
    for name in ("elfgo_region_moves", "elfgo_ld_run"):
        assert hasattr(L, name), "libelf_amd.so lacks " + name
        assert name in _lib.SIGNATURES
    assert ("int elfgo_region_moves(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, int self_atari_thres, "
            "uint8_t* cand, uint8_t* valid, uint8_t* groups, void* stream);") in flat
    assert ("int elfgo_ld_run(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps, "
            "int self_atari_thres, const int32_t* regions, const uint8_t* attackers, int32_t* info, int64_t* stats, "
            "int32_t* first, void* stream);") in flat
    res, args = _lib.SIGNATURES["elfgo_region_moves"]
    assert res is ctypes.c_int and len(args) == 9
    assert [i for i, a in enumerate(args) if a is ctypes.c_int] == [2, 4] and all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 4))
    res, args = _lib.SIGNATURES["elfgo_ld_run"]
    assert res is ctypes.c_int and len(args) == 13
    assert [i for i, a in enumerate(args) if a is ctypes.c_int] == [3, 4, 5, 6]
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (3, 4, 5, 6))
    # the comments cite the reference's lines, and say what a null region means in each call
    for cite in (":892-947", ":970-1005", ":1183-1196", "THE WHOLE BOARD", "NOT the whole"):
        assert cite in src, cite


def test_null_handles_are_status_codes(built):
    import elf_amd
    L = elf_amd.lib()
    buf = (ctypes.c_uint8 * 4096)()
    assert L.elfgo_region_moves(None, None, 1, None, 1, buf, buf, buf, None) == -1
    assert L.elfgo_region_moves(None, None, 1, None, 1, None, None, None, None) == -1
    assert L.elfgo_ld_run(None, None, buf, 1, 1, 10, 3, None, None, buf, buf, buf, None) == -1


def test_python_surface(built):
    from elf_amd import engine
    from elf_amd.engine import GoEngine, LdReading
    from elf_amd.gtp import GtpEngine
    sig = inspect.signature(GoEngine.region_moves).parameters
    assert list(sig) == ["self", "ids", "n", "regions", "self_atari_thres"]
    assert all(sig[k].default is None for k in ("ids", "n", "regions")) and sig["self_atari_thres"].default == 1
    sig = inspect.signature(GoEngine.ld_read).parameters
    assert list(sig) == ["self", "seeds", "ids", "regions", "playouts", "self_atari_thres", "attackers", "max_steps", "max_lanes"]
    assert (sig["playouts"].default, sig["self_atari_thres"].default, sig["max_steps"].default, sig["max_lanes"].default) == (256, 3, 1 << 20, 0)
    assert all(sig[k].default is None for k in ("ids", "regions", "attackers"))
    assert "track_placed" in GoEngine.ld_read.__doc__
    assert len(engine.LD_INFO_FIELDS) == 8 and len(engine.LD_STAT_FIELDS) == 8
    assert isinstance(LdReading.live_rate, property) and isinstance(LdReading.survive_rate, property) and callable(LdReading.best_move)
    for name in ("on_elf_region_candidates", "on_elf_ld_read"):
        assert callable(getattr(GtpEngine, name))
    sig = inspect.signature(GtpEngine.__init__).parameters
    assert sig["ld_seed"].default == 1 and sig["ld_self_atari_thres"].default == 3


def test_best_move_is_integer_and_breaks_ties_as_stated():
    """LdReading.best_move on hand-made tensors: largest lived / playouts for the defender, smallest for the attacker, compared
    by cross-multiplication; ties by more playouts, then by the smaller action; a pass is an answer; no playout, no answer"""
    import torch
    from elf_amd.engine import LdReading
    n, NA = 9, 82

    def reading(to_move, rows):
        first = torch.zeros((1, 3, NA), dtype=torch.int32)
        for a, (p, l) in rows.items():
            first[0, 0, a], first[0, 1, a] = p, l
        info = torch.tensor([[0, 0, 9, 9, 2, 1, to_move, 0]], dtype=torch.int32)
        return LdReading(n, 64, info, torch.zeros((1, 8), dtype=torch.int64), first)
    assert reading(1, {5: (3, 1), 7: (3, 2), 9: (6, 4)}).best_move() == [9]        # 2/3 == 4/6: more playouts
    assert reading(1, {5: (6, 4), 7: (6, 4)}).best_move() == [5]                    # full tie: smaller action
    assert reading(2, {5: (3, 1), 7: (3, 2), 81: (4, 0)}).best_move() == [81]       # attacker: smallest, the pass
    assert reading(2, {5: (3, 1), 7: (6, 2)}).best_move() == [7]
    assert reading(1, {}).best_move() == [None]
    assert reading(1, {3: (2_000_000_000, 1_000_000_001), 4: (2_000_000_000 - 2, 1_000_000_000)}).best_move() == [4]
