"""What the code-generation tests share (test_codegen_invariants.py, test_codegen_montgomery.py, test_codegen_verdict_row.py): the flags of the
cross-compilation to gfx950 assembly (no GPU needed), the compile step, and the two readers of an assembly listing.  Where a function ends is each
test's own rule: they differ on purpose."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc")
FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wno-unused-function -Wno-unused-value -x hip -S --cuda-device-only".split()


def compile_asm(src, dir):
    """The lines of csrc/<src>'s device assembly, written to <dir>/<src>.s; skips the test without hipcc."""
    if not shutil.which("hipcc"):
        pytest.skip("no hipcc")
    out = os.path.join(str(dir), src + ".s")
    subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, src), "-o", out], check=True, capture_output=True, cwd=CSRC)
    return open(out).read().split("\n")


def loops(lines, lo, hi):
    """(first, last) line of every natural loop = backward branch (conditional or not) to a label inside [lo, hi)."""
    labels = {m.group(1): i for i in range(lo, hi) for m in [re.match(r"^(\.LBB\d+_\d+):", lines[i])] if m}
    for i in range(lo, hi):
        m = re.search(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            yield labels[m.group(1)], i


def count(lines, a, b, pat=r"[a-z]"):
    """Instructions of lines [a, b] whose mnemonic starts with `pat` (default: every instruction)."""
    return sum(1 for l in lines[a:b + 1] if re.match(r"^\s+" + pat, l))
