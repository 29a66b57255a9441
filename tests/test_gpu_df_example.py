"""GPU: examples/df_features.c -- a C11 program linked against libelf_amd.so only (no HIP headers, no torch) -- prints the 25 planes
of a 9x9 ko position; every number it prints is compared with the reference's BoardFeature::extract (df_expected)."""
import os
import subprocess

import numpy as np
import pytest

import df_expected as DE
import ownership_expected as OE
from conftest import ROOT
from pyoracle import Ref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d4", [0, 6])
def test_plain_c_program_prints_the_reference_planes(built, tmp_path, d4):
    assert Ref.available(9)
    exe = str(tmp_path / "df_features")
    lib = os.path.join(ROOT, "elf_amd", "lib")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "df_features.c"), "-o", exe, "-L", lib, "-lelf_amd", "-Wl,-rpath," + lib,
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, str(d4), os.path.join(ROOT, "elf_amd", "data", "zobrist21.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    D = DE.df(9)
    s = OE.states_of(D.E, [OE.ko_moves(9)])[0]
    want = D.planes(s, d4)
    D.E.free(s)
    lines = r.stdout.strip().splitlines()
    sums = {int(w[1]): int(w[3]) for w in (ln.split() for ln in lines) if w[0] == "plane"}
    assert sorted(sums) == list(range(25))
    for p in range(25):
        if p not in (10, 11):
            assert sums[p] == int(want[p].sum(dtype=np.float64)), p
    hist = {(int(w[1]), int(w[3])): int(w[5], 16) for w in (ln.split() for ln in lines) if w[0] == "history"}
    bits = DE.bits(want).reshape(25, -1)
    assert hist == {(p, int(a)): int(bits[p, a]) for p in (10, 11) for a in np.nonzero(bits[p])[0]} and len(hist) == 4
    board = [ln.split("|")[0].strip() for ln in lines if "|" in ln][1:]
    assert len(board) == 9 and sum(row.count("k") for row in board) == 1
