"""GPU: examples/life_and_death.c -- a C11 program linked against libelf_amd.so only (no HIP headers, no torch) -- reads the straight
three by region playouts; every number it prints is compared with the reference driver of region_expected."""
import os
import subprocess

import pytest

import region_expected as RE
from conftest import ROOT
from pyoracle import Ref, RefBoard

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mover", ["b", "w"])
def test_plain_c_program_prints_the_drivers_numbers(built, tmp_path, mover):
    assert Ref.available(9) and RefBoard.available(9)
    n, K = 9, 96
    exe = str(tmp_path / "life_and_death")
    lib = os.path.join(ROOT, "elf_amd", "lib")
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "life_and_death.c"), "-o", exe, "-L", lib, "-lelf_amd", "-Wl,-rpath," + lib,
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe, mover, str(K), os.path.join(ROOT, "elf_amd", "data", "zobrist21.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    src = dict(stones=RE.straight_three(n), mover=1 if mover == "b" else 2)
    info, stats, first = RE.reg(n).ld_row(RE.ref(n), src, 1, K, RE.S3_THRES, RE.S3_BOX, 0)
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "box %d %d %d %d attacker %s defender %s to move %s lives now %d" % (
        info[0], info[1], info[2], info[3], " bw"[info[4]], " bw"[info[5]], " bw"[info[6]], info[7])
    assert lines[1] == "playouts %d lived %d survived %d super-ko endings %d steps %d" % (K, stats[0], stats[1], stats[4], stats[5])
    want = ["%s playouts %d lived %d survived %d" % ("pass" if a == n * n else "(%d,%d)" % (a // n, a % n), first[0, a], first[1, a], first[2, a])
            for a in range(n * n + 1) if first[0, a]]
    assert lines[2:] == want and len(want) >= 3
