"""CPU: the C ABI's side of the DarkForest row format of elftrain_extract -- the constant in the header and in _lib, the entry
points that keep refusing it, and the exponent table the store copies at create (no compute calls here)."""
import os
import re

import numpy as np

import df_expected as DE
from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "elf_amd.h")).read()


def test_header_defines_the_format_and_lib_carries_it():
    from elf_amd import _lib
    codes = dict((k, int(v)) for k, v in re.findall(r"#define\s+(ELFGO_FEAT_[A-Z0-9_]+)\s+(\d+)", header()))
    assert codes == {"ELFGO_FEAT_F32_NCHW": 0, "ELFGO_FEAT_F16_NHWC": 1, "ELFGO_FEAT_DF_F32_NCHW": 2}
    assert {k: getattr(_lib, k) for k in codes} == codes


def test_train_batch_layout_is_unchanged():
    import ctypes as C
    from elf_amd.train import TrainBatch
    assert C.sizeof(TrainBatch) == 88 and TrainBatch.s_format.offset == 16 and TrainBatch.offline_a.offset == 24
    body = re.search(r"typedef struct ElfTrainBatch \{(.*?)\} ElfTrainBatch;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+);", body)
    assert names == [f[0] for f in TrainBatch._fields_]
    assert "25" in re.search(r"void\* s;(.*?)int64_t s_stride", header(), re.S).group(1)


def test_loader_knows_three_formats():
    from elf_amd.train import FEATURE_FORMATS
    assert FEATURE_FORMATS == {"f32_nchw": (0, 18), "f16_nhwc": (1, 18), "df_f32_nchw": (2, 25)}


def test_exp_table_is_unchanged(built):
    """elfgo_df_exp_table, whose values the store copies to the device at elftrain_create: still the C library's exp"""
    import elf_amd
    L = elf_amd.lib()
    for n in (9, 19):
        tab = np.full(2 * n * n + 1, np.nan, np.float32)
        assert L.elfgo_df_exp_table(n, tab.ctypes.data) == 0
        assert np.array_equal(DE.bits(tab), DE.bits(DE.libm_exp_table(n)))


def test_other_entry_points_keep_refusing_the_format(built):
    """argument checks that run before any device call: the search and the board extractor take the two AGZ formats only"""
    import elf_amd
    L = elf_amd.lib()
    assert L.elfmcts_set_feature_format(None, 2) == -1
    src = open(os.path.join(ROOT, "elf_amd", "csrc", "mcts_capi.hip")).read() + open(os.path.join(ROOT, "elf_amd", "csrc", "elf_amd.hip")).read()
    assert src.count("fmt != ELFGO_FEAT_F32_NCHW && fmt != ELFGO_FEAT_F16_NHWC") == 2 and "ELFGO_FEAT_DF" not in src
