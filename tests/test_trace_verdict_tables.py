"""The verdict table of a traced plan (csrc/verdictfmt.h), compiled as plain C++ and checked on the host: verdict_table_check - what stands between a
lowering bug and a wild reference in k_trace_verdict - accepts a hand-built table with every ref kind and width and refuses each single corruption
of it (slot + span one past the end, import / input / pool index out of range, width 3, kind 5 and above, a range site of more than 64 bits on a
one-word ref), by the message that names the entry.  Run once plainly and once under the address and undefined-behaviour sanitizers of the host compiler."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_verdict_table_check_accepts_every_ref_and_refuses_every_corruption(tmp_path, sanitize):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "verdict_table_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "verdict_table_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
    m = re.search(r"^OK tables: (\d+) corruptions: (\d+)$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 3 and int(m.group(2)) >= 40, r.stdout


def test_the_format_header_needs_no_hip():
    src = open(os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc", "verdictfmt.h")).read()
    assert set(re.findall(r'^#include\s+[<"]([^>"]+)[>"]', src, flags=re.M)) <= {"tapefmt.h"}
