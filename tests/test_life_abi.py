"""CPU: the life-reading entry point is exported, declared and bound, and the Python surface has the stated signatures and defaults
(no compute calls here)."""
import ctypes
import inspect
import os
import re

from conftest import ROOT


def test_symbol_is_exported_declared_and_bound(built):
    from elf_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "elf_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert hasattr(L, "elfgo_life_map"), "libelf_amd.so lacks elfgo_life_map"
    assert "elfgo_life_map" in _lib.SIGNATURES
    flat = " ".join(code.split())
    assert ("int elfgo_life_map(ElfGoEngine* e, const int32_t* ids, int n, const int32_t* regions, uint8_t* eye, int16_t* semi_move, "
            "uint8_t* alive, int32_t* summary, void* stream);") in flat
    res, args = _lib.SIGNATURES["elfgo_life_map"]
    assert res is ctypes.c_int and len(args) == 9 and args[2] is ctypes.c_int
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i != 2)
    # the comments cite the reference's lines
    for cite in ("board.cc:1850-1922", "board.cc:1924-1952", "board.cc:1108-1221", "board.cc:1024-1106"):
        assert cite in src, cite


def test_null_handles_are_status_codes(built):
    import elf_amd
    L = elf_amd.lib()
    buf = (ctypes.c_uint8 * 4096)()
    assert L.elfgo_life_map(None, None, 1, None, buf, buf, buf, buf, None) == -1
    assert L.elfgo_life_map(None, None, 1, None, None, None, None, None, None) == -1
    assert L.elfgo_life_map(None, None, 0, None, buf, None, None, None, None) == -1


def test_python_surface(built):
    from elf_amd import engine
    from elf_amd.engine import GoEngine
    from elf_amd.gtp import GtpEngine
    sig = inspect.signature(GoEngine.life_map).parameters
    assert list(sig) == ["self", "ids", "n", "regions"]
    assert all(sig[k].default is None for k in ("ids", "n", "regions"))
    sig = inspect.signature(GoEngine.fast_score).parameters
    assert list(sig) == ["self", "ids", "n", "rule"]
    assert sig["ids"].default is None and sig["n"].default is None and sig["rule"].default == "chinese"
    assert len(engine.SUMMARY_FIELDS) == 12
    for name in ("eye", "semi_move", "alive", "summary"):
        assert name in inspect.signature(engine.LifeMap.__init__).parameters
    assert isinstance(engine.LifeMap.eye_colour, property)
    for name in ("on_elf_eyes", "on_elf_life", "on_elf_fast_score"):
        assert callable(getattr(GtpEngine, name))
