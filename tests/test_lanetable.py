"""The lane tables of a traced plan's sharded and verdict calls (csrc/lanetable.h), compiled as plain C++ and checked on the host: what the pure
fill functions put into a table - the root's section (owned proofs, padding to a wavefront, the others marked), the deeper sections (the owned
units' places, ascending), every place emitted by exactly one rank of a world, the quiet table, the 2^31 refusals - and the ownership rule they
share with h2w_plan_shard_block (csrc/shardmap.h shard_owns)."""
import importlib
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path_factory.mktemp("lanetable")), "lanetable_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lanetable_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-4000:] + r.stderr
    return r.stdout


def test_fill_functions_on_a_hand_made_template_set(check_output):
    m = re.search(r"^OK tables: (\d+)$", check_output, flags=re.M)
    assert m and int(m.group(1)) == 4 * (2 + 3) + 4, check_output[-2000:]      # n x every rank of worlds 2 and 3, and the quiet table of every n


def test_the_ownership_helper_agrees_with_shard_block(check_output):
    """shard_owns on the grid the tables were filled on (nq = 2, worlds 2 and 3, every rank, 130 proofs, the root's block and both queries) against
    what h2w_plan_shard_block says of a plan with two queries (host arithmetic, no device)."""
    sys.path.insert(0, ROOT)
    h2w = importlib.import_module("halo2-plonky2-verifier_amd"); api = importlib.import_module("halo2-plonky2-verifier_amd.api")
    rows = [tuple(map(int, l.split()[1:])) for l in check_output.split("\n") if l.startswith("OWNS ")]
    assert len(rows) == (2 + 3) * 130 * 3
    plan = api.Plan(h2w.fibonacci_shape(6, 2, hash_mode=1), h2w.published_consts())
    try:
        for world, rank, proof, q, owned in rows:
            assert (plan.shard_block(rank, world, proof, q) is not None) == bool(owned), (world, rank, proof, q)
    finally:
        plan.close()


def test_the_lane_table_header_needs_no_hip():
    """lanetable.h and the header of the ownership rule are plain C++ (the check above is compiled by g++): the format and field headers, nothing
    of the runtime, no device sink (glcoop.h, bnquad.h)."""
    allowed = {"lanetable.h": {"cstdint", "vector", "tapefmt.h", "shardmap.h"}, "shardmap.h": {"stdint.h", "field.h"}}
    for name, ok in allowed.items():
        src = open(os.path.join(CSRC, name)).read()
        assert set(re.findall(r'^#include\s+[<"]([^>"]+)[>"]', src, flags=re.M)) <= ok, name
