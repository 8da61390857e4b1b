"""The parts of a split select in the device tape (csrc/tapefmt.h SELIND_*, H2W_TRACE_SPLIT_SELECTS), compiled as plain C++ and checked on the host:
tape_check accepts a chain of two and of three parts with a ring's worth of fetches in front of each, and refuses a chain out of shape - an aux byte
above 3, any aux on the narrow select, a "continued" part without its successor, a "continues" part without its predecessor, a "continued" part with a
result slot, more fetched slots in front of one part than the ring holds - by the message that names the part's first word.  A malformed chain would
be a GPU fault or a wrong sum: the interpreter carries the sum between exactly the two ops the checker admits."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tape_check_holds_a_chain_of_parts_to_its_shape(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "tapefmt_chain_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "tapefmt_chain_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    m = re.search(r"^OK tapes: (\d+) refusals: (\d+)$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 4 and int(m.group(2)) >= 24, r.stdout
