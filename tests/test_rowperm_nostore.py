"""csrc/rowperm.h bn_permute_rows<false> - the row-cooperative PoseidonBN254 permutation of k_verdict_merkle_row, which stores nothing - on the
simulated lanes of tests/cpp/rowperm_nostore_check.cpp: called with a null S-box pointer it gives the state bn_permute_rows<true> and the reference
walk give, on the published and on full-width random tables, from the all-zero state, a state of r - 1 and random states.  The program is plain host
code with its own main: it is also built with the address and undefined-behaviour sanitizers, under which a store through the null pointer - or
an address formed from it - is reported, not merely likely to fault."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rowperm_nostore_check.cpp")
INC = ["-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include")]


def _run(tmp_path, name, extra):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), name)
    subprocess.run(["g++", "-std=c++17", *extra, *INC, SRC, "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK 12 permutations" in r.stdout, r.stdout + r.stderr
    return r


def test_the_store_free_permutation_equals_the_storing_one_and_the_reference(tmp_path):
    _run(tmp_path, "rowperm_nostore_check", ["-O2"])


def test_the_store_free_permutation_under_the_sanitizers(tmp_path):
    r = _run(tmp_path, "rowperm_nostore_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
