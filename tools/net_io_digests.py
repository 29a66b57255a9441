"""Writes tests/net_io_expected.py: the sha256 digests tests/test_gpu_net_io_bits.py compares the outputs of the net's ends with.
The cases and the way an output is digested are that test file's own (conv_digests, heads_digests); this script only runs them on a
library of one's choice and prints the module.  The committed digests were recorded with it on commit b98ed10 ("Add exact
life-and-death search over a box: elfgo_ld_solve"), the last one whose fp16 and bf16 ends were two files, net_io.hip and
net_io_bf16.hip:
    make -C elf_amd/csrc                          # on a checkout of that commit
    python tools/net_io_digests.py --lib <that checkout>/elf_amd/lib/libelf_amd.so --out tests/net_io_expected.py
Never record them from the code under test: then the test says nothing."""
import argparse
import os
import pprint
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HEAD = '''"""Recorded sha256 digests of what elfnet_conv3x3_in_f16 / _bf16 and elfnet_heads_f16 / _bf16 write for the cases of
tests/test_gpu_net_io_bits.py.  Recorded by tools/net_io_digests.py from the library of commit %s.
CONV: (rows, c, k) -> {entry and relu: digest of y}.  HEADS: (rows, channels) -> {type and output: digest}."""
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the libelf_amd.so to record from")
    ap.add_argument("--commit", default="b98ed10", help="the commit that library was built from, for the module's docstring")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "net_io_expected.py"))
    a = ap.parse_args()
    import elf_amd._lib
    elf_amd._lib.LIB_PATH = os.path.abspath(a.lib)
    import test_gpu_net_io_bits as T
    L = elf_amd.lib()
    conv = {s: T.conv_digests(L, *s) for s in T.CONV_SHAPES}
    heads = {s: T.heads_digests(L, *s) for s in T.HEADS_SHAPES}
    with open(a.out, "w") as f:
        f.write(HEAD % a.commit)
        f.write("CONV = " + pprint.pformat(conv, width=130) + "\n\nHEADS = " + pprint.pformat(heads, width=130) + "\n")
    print("wrote %s: %d + %d shapes" % (a.out, len(conv), len(heads)))


if __name__ == "__main__":
    main()
