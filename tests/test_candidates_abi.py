"""CPU: the candidate-move entry points are exported, declared and bound, and the Python surface has the stated defaults
(no compute calls here)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT

NEW = ("elfgo_candidates", "elfgo_playout_cand", "elfgo_own_run_cand")


def test_symbols_are_exported_declared_and_bound(built):
    from elf_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "elf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), "libelf_amd.so lacks %s" % name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "include/elf_amd.h lacks %s" % name
        assert name in _lib.SIGNATURES
    # the argument lists, as the header states them
    flat = " ".join(code.split())
    assert ("int elfgo_candidates(ElfGoEngine* e, const int32_t* ids, int n, int self_atari_thres, uint8_t* mask, int16_t* stones, "
            "void* stream);") in flat
    assert ("int elfgo_playout_cand(ElfGoEngine* e, const int32_t* ids, const uint64_t* seeds, int n, int max_steps, "
            "int self_atari_thres, uint32_t* out, void* stream);") in flat
    assert ("int elfgo_own_run_cand(ElfGoOwnership* o, const int32_t* ids, const uint64_t* seeds, int n, int playouts, int max_steps, "
            "float komi, int self_atari_thres, int32_t* counts, int64_t* stats, void* stream);") in flat
    assert len(_lib.SIGNATURES["elfgo_candidates"][1]) == 7
    assert len(_lib.SIGNATURES["elfgo_playout_cand"][1]) == len(_lib.SIGNATURES["elfgo_playout"][1]) + 1
    assert len(_lib.SIGNATURES["elfgo_own_run_cand"][1]) == len(_lib.SIGNATURES["elfgo_own_run"][1]) + 1
    # the comments cite the reference's lines
    assert "board.cc:254-297" in src and "board.cc:850-890" in src


def test_null_handles_are_status_codes(built):
    import elf_amd
    L = elf_amd.lib()
    buf = (ctypes.c_uint8 * 512)()
    assert L.elfgo_candidates(None, None, 1, 1, buf, None, None) == -1
    assert L.elfgo_playout_cand(None, None, buf, 1, 10, 1, buf, None) == -1
    assert L.elfgo_own_run_cand(None, None, buf, 1, 1, 10, ctypes.c_float(7.5), 1, buf, buf, None) == -1


def test_python_surface(built):
    from elf_amd.engine import GoEngine
    from elf_amd.gtp import GtpEngine
    sig = inspect.signature(GoEngine.candidates).parameters
    assert list(sig) == ["self", "ids", "n", "self_atari_thres"]
    assert sig["ids"].default is None and sig["n"].default is None and sig["self_atari_thres"].default == 1
    for f in (GoEngine.playout, GoEngine.ownership):
        p = inspect.signature(f).parameters
        assert p["self_atari_thres"].default is None
    # the existing arguments keep their places and defaults
    assert list(inspect.signature(GoEngine.playout).parameters)[:5] == ["self", "seeds", "ids", "max_steps", "out"]
    assert list(inspect.signature(GoEngine.ownership).parameters)[:7] == ["self", "seeds", "ids", "playouts", "komi", "max_steps", "max_lanes"]
    g = inspect.signature(GtpEngine.__init__).parameters
    assert g["status_self_atari_thres"].default is None
    assert callable(getattr(GtpEngine, "on_elf_candidates"))
