"""The device tape format of a traced plan (csrc/tapefmt.h), compiled as plain C++ and checked on the host: the checker every tape passes before
it is uploaded (tape_check: what stands between a lowering bug and a wild reference on the device) accepts hand-built tapes that hold every op, and
refuses each single corruption of them - a length byte, an operand, a result slot, a fetch, a fused permutation's trailing words, the end - by the
message that names the op's first word; operand_span is the descriptor table."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tape_check_accepts_every_op_and_refuses_every_corruption(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "tapefmt_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "tapefmt_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    m = re.search(r"^OK tapes: (\d+) corruptions: (\d+)$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 3 and int(m.group(2)) >= 60, r.stdout


def test_the_format_header_needs_no_hip():
    """tapefmt.h is the part of the traced-plan unit that plain C++ compiles: it includes the record and field headers, nothing of the runtime."""
    src = open(os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc", "tapefmt.h")).read()
    assert set(re.findall(r'^#include\s+[<"]([^>"]+)[>"]', src, flags=re.M)) <= {"cstdint", "string", "vector", "records.h", "field.h"}
