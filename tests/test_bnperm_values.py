"""The per-thread PoseidonBN254 value permutation of a fused traced plan (csrc/bnpval.h: what a lane of the replay interpreter runs for a
DOP_BNPERM op), compiled as plain C++ and checked on the host: the published circomlib vector on the published tables, the oracle's gadget
(orc_bn_poseidon_permute) on random states and on the edge states, with seeded tables as well.  Also: the public surface of the PoseidonBN254
fusing (include/h2w.h, the generated Rust declarations, the library's exports)."""
import ctypes as C
import json
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR_R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def _fr(x):
    return struct.pack("<4Q", *[(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])


def _group(k, cases):
    blob = struct.pack("<Q", len(cases)) + bytes(k)
    for st_in, st_out in cases:
        blob += b"".join(_fr(x) for x in list(st_in) + list(st_out))
    return blob


def _gadget(oracle, k, st):
    """PoseidonBN254PermutationChip::permute of the oracle (hash/poseidon_bn254/permutation.rs:190-203) on the state: its four output values."""
    L = oracle.lib()
    ctx = oracle.Ctx(21, witness_gen_only=True)
    ins = (oracle.AV * 4)(*[L.orc_load_witness(ctx.p, oracle.Fr.from_int(x)) for x in st]); outs = (oracle.AV * 4)()
    L.orc_bn_poseidon_permute(ctx.p, C.byref(k), ins, outs)
    out = [o.v.to_int() for o in outs]; ctx.close()
    return out


EDGES = [[0] * 4, [FR_R - 1] * 4, [0, 1, FR_R - 1, 1 << 253]]


def test_value_permutation_known_answers_and_oracle_parity(tmp_path, oracle):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_published.json")))
    vecs = gold["bn254_t4"]["permutation_vectors"]
    assert vecs[0]["in"] == ["0x0", "0x1", "0x2", "0x3"] and vecs[0]["out"][0] == "0xe7732d89e6939c0ff03d5e58dab6302f3230e269dc5b968f725df34ab36d732"      # circomlib poseidon([1,2,3])
    kp = oracle.published_consts()
    blob = _group(kp, [([int(x, 16) for x in v["in"]], [int(x, 16) for x in v["out"]]) for v in vecs])
    rng = random.Random(20240807)
    n_cases = len(vecs)
    for k in (kp, oracle.synth_consts(0xC0FFEE)):
        states = EDGES + [[rng.randrange(FR_R) for _ in range(4)] for _ in range(20)]
        blob += _group(k, [(st, _gadget(oracle, k, st)) for st in states]); n_cases += len(states)
    path = os.path.join(str(tmp_path), "cases.bin")
    open(path, "wb").write(blob)
    exe = os.path.join(str(tmp_path), "bnperm_values_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "halo2-plonky2-verifier_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "bnperm_values_check.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    assert "groups: 3 cases: %d" % n_cases in r.stdout, r.stdout


def test_header_and_rust_block_declare_the_bn_fusing():
    hdr = open(os.path.join(ROOT, "include", "h2w.h")).read()
    rs = open(os.path.join(ROOT, "rust", "h2w-sys", "src", "lib.rs")).read()
    assert re.search(r"^#define H2W_TRACE_FUSE_BN_PERMUTE 2\s*$", hdr, flags=re.M)
    assert re.search(r"int h2w_plan_trace_info_bn\(const h2w_plan \*, uint64_t out\[3\]\);", hdr)
    assert re.search(r"int h2w_plan_trace_info\(const h2w_plan \*, uint64_t out\[6\]\);", hdr)
    assert "pub const H2W_TRACE_FUSE_BN_PERMUTE: c_int = 2;" in rs
    assert "pub fn h2w_plan_trace_info_bn(a0: *const H2wPlan, out: *mut u64) -> c_int;" in rs


def test_library_exports_the_bn_fusing(h2w):
    lib = h2w.lib()
    assert hasattr(lib, "h2w_plan_trace_info_bn")
    assert h2w.H2W_TRACE_FUSE_BN_PERMUTE == 2 and h2w.H2W_TRACE_FUSE_GL_PERMUTE == 1
