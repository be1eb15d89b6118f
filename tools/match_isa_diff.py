"""Compares the gfx950 code of the kernels two versions of csrc/match_kernels.hip have in common (build flags of csrc/Makefile,
device code only, no GPU needed).  Comments and label numbers are dropped before the comparison; anything else that differs --
an instruction, a register, an order, a resource count -- is reported.

    python tools/match_isa_diff.py OLD.hip [NEW.hip]     (NEW defaults to the tree's csrc/match_kernels.hip)
    git show REV:cuda-efficient-features_amd/csrc/match_kernels.hip > /tmp/old.hip   # e.g. the parent commit's source

Exit status 0 when every common kernel is identical."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-efficient-features_amd", "csrc")
FLAGS = "-std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math --cuda-device-only -S".split()


def kernels(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + ["-I", CSRC, src, "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
    res = {}
    for m in re.finditer(r"^(_Z\w+):.*?\.end_amdhsa_kernel", text, flags=re.S | re.M):
        lines = []
        for line in m.group(0).splitlines():
            line = line.split(";", 1)[0].rstrip()                      # comments (loop headers name other kernels' blocks)
            if line.strip():
                lines.append(re.sub(r"\.LBB\d+_", ".LBB_", line))      # label numbers follow the kernels before this one
        res[m.group(1)] = lines
    return res


def main():
    old = sys.argv[1]
    new = sys.argv[2] if len(sys.argv) > 2 else os.path.join(CSRC, "match_kernels.hip")
    a, b = kernels(old), kernels(new)
    common = sorted(set(a) & set(b))
    bad = 0
    for k in common:
        same = a[k] == b[k]
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT'}  {len(a[k]):5d} lines  {k}")
    print(f"{len(common)} common kernels, {bad} different; only in the old file: {len(set(a) - set(b))}, only in the new: {len(set(b) - set(a))}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
